"""PPGN on the host: the numpy restatement of the input tensors on hand-made graphs, the plain-torch restatement of the block
against autograd identities, and the model classes' parameters (names, shapes, creation order, seeding).  No GPU."""
import numpy as np
import pytest
import torch

import _ppgn_ref as R

FACTORIES = {   # factory -> (ninp, C, blocks, bias, readout width factor, hidden, has h2)
    'sr25_ppgn': (3, 32, 3, True, 2, 10, False), 'graph8c_ppgn': (3, 32, 3, True, 2, 10, False),
    'exp_ppgn': (3, 20, 3, False, 2, 10, False), 'exp_classify_ppgn': (3, 20, 3, False, 2, 10, True),
    'zinc_ppgn': (23, 32, 4, False, 2, 64, True), 'counting_ppgn': (3, 40, 5, False, 2, 64, True),
    'mutag_ppgn': (9, 32, 3, True, 1, 32, True)}


def test_inputs_path3():
    from gnn_matlang_amd.ppgn import ppgn_inputs_host
    x = np.array([[2.], [3.], [5.]], dtype=np.float32)
    ei = np.array([[0, 1, 1, 2], [1, 0, 2, 1]])
    X2, M, n = ppgn_inputs_host(x, ei, 4, 1)
    assert n == 3 and X2.shape == (3, 4, 4) and M.shape == (2, 4, 4) and X2.dtype == np.float32
    A = np.zeros((4, 4), np.float32)
    A[0, 1] = A[1, 0] = A[1, 2] = A[2, 1] = 1
    assert np.array_equal(X2[0], A)
    assert np.array_equal(X2[1], np.diag([1, 1, 1, 0]).astype(np.float32))
    assert np.array_equal(X2[2], np.diag([2, 3, 5, 0]).astype(np.float32))
    assert np.array_equal(M[0], np.diag([1, 1, 1, 0]).astype(np.float32))
    off = np.ones((4, 4), np.float32) - np.eye(4, dtype=np.float32)
    off[3, :] = 0
    off[:, 3] = 0
    assert np.array_equal(M[1], off)


def test_inputs_single_node_full_size_and_directed():
    from gnn_matlang_amd.ppgn import ppgn_inputs_host
    X2, M, n = ppgn_inputs_host(np.ones((1, 1), np.float32), np.zeros((2, 0), np.int64), 3, 1)
    assert n == 1 and X2[0].sum() == 0 and X2[1].sum() == 1 and X2[1, 0, 0] == 1 and M[0].sum() == 1 and M[1].sum() == 0
    # n = nmax, directed edges: only (source, target) is set
    ei = np.array([[0, 2, 3], [1, 0, 3]])
    X2, M, n = ppgn_inputs_host(np.arange(4, dtype=np.float32).reshape(4, 1) + 1, ei, 4, 1)
    assert n == 4 and X2[0, 0, 1] == 1 and X2[0, 1, 0] == 0 and X2[0, 2, 0] == 1 and X2[0, 0, 2] == 0 and X2[0, 3, 3] == 1
    assert X2[0].sum() == 3 and M[0].sum() == 4 and M[1].sum() == 12 and np.array_equal(np.diag(X2[2]), [1, 2, 3, 4])
    with pytest.raises(ValueError):
        ppgn_inputs_host(np.ones((5, 1), np.float32), ei, 4, 1)


def test_inputs_degree_column_is_not_placed():
    """nfeat is counted before SpectralDesign appends the degree: x [n, 3] = two features + degree, nfeat = 2 -> 4 channels"""
    from gnn_matlang_amd.ppgn import ppgn_inputs_host
    x = np.array([[1., 7., 100.], [2., 8., 200.]], dtype=np.float32)
    X2, M, n = ppgn_inputs_host(x, np.array([[0], [1]]), 3, 2)
    assert X2.shape == (4, 3, 3)
    assert np.array_equal(np.diag(X2[2]), [1, 2, 0]) and np.array_equal(np.diag(X2[3]), [7, 8, 0])
    assert not (X2 >= 100).any()


@pytest.mark.parametrize('bias', [True, False])
@pytest.mark.parametrize('readout', R.READOUTS)
def test_block_gradcheck(bias, readout):
    torch.manual_seed(3)
    B, nmax, Cin, C = 2, 4, 2, 3
    n = torch.tensor([4, 2], dtype=torch.int32)
    x = torch.randn(B, Cin, nmax, nmax, dtype=torch.float64, requires_grad=True)
    mk = lambda *s: torch.randn(*s, dtype=torch.float64, requires_grad=True)
    w1, w2, w3 = mk(C, Cin), mk(C, Cin), mk(C, C + Cin)
    bs = [mk(C) for _ in range(3)] if bias else []

    def f(x, w1, w2, w3, *b):
        W = dict(w1=w1, w2=w2, w3=w3, b1=b[0] if b else None, b2=b[1] if b else None, b3=b[2] if b else None)
        y, r = R.block_ref(x, n, W, readout)
        return y, r
    assert torch.autograd.gradcheck(f, (x, w1, w2, w3, *bs), eps=1e-6, atol=1e-5)


def test_block_padding_is_ignored_and_zero():
    x, n, W, gy, gr = R.block_case(3, 8, [8, 2, 5], 3, 5, True)
    y, r, dx, gW = R.block_cpu(x, n, W, gy, gr, 'sum', torch.float64)
    m = R.mask(n, 8, torch.float64)
    assert float((y * (1 - m)).abs().max()) == 0 and float((dx * (1 - m)).abs().max()) == 0
    x2 = x * m.float() + 5 * (1 - m.float())
    y2, r2, dx2, gW2 = R.block_cpu(x2, n, W, gy, gr, 'sum', torch.float64)
    assert torch.equal(y, y2) and torch.equal(r, r2) and torch.equal(dx, dx2)
    assert all(torch.equal(gW[k], gW2[k]) for k in gW)


def test_sum_equals_rows_then_columns():
    x, n, W, _, _ = R.block_case(3, 8, [8, 2, 5], 3, 4, True)
    _, _, _, y, m = R.block_parts(x.double(), n, {k: v.double() for k, v in W.items()})
    a, b = R.readout_of(y, m, 'sum'), R.readout_rows_then_cols(y, m)
    assert a.shape == b.shape == (3, 8)
    assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())


def test_mean_at_one_node_is_zero_over_zero():
    x, n, W, _, _ = R.block_case(1, 8, [1], 3, 4, True)
    _, r = R.block_ref(x, n, W, 'mean')
    assert torch.isfinite(r[:, :4]).all() and torch.isnan(r[:, 4:]).all()


@pytest.mark.parametrize('name', sorted(FACTORIES))
def test_state_dict_names_and_shapes(name):
    from gnn_matlang_amd import models
    ninp, C, nb, bias, rf, hidden, h2 = FACTORIES[name]
    m = getattr(models, name)()
    exp, cin = [], ninp
    for b in range(1, nb + 1):
        for i, width in ((1, cin), (2, cin), (3, C + cin)):
            exp.append(('mlp%d_%d.weight' % (b, i), (C, width, 1, 1)))
            if bias:
                exp.append(('mlp%d_%d.bias' % (b, i), (C,)))
        cin = C
    exp += [('h1.weight', (hidden, rf * nb * C)), ('h1.bias', (hidden,))]
    if h2:
        exp += [('h2.weight', (1, hidden)), ('h2.bias', (1,))]
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == exp                                              # names, shapes and the creation order
    assert [k for k, _ in m.named_parameters()] == [k for k, _ in exp]
    assert all(isinstance(getattr(m, 'mlp%d_%d' % (b, i)), torch.nn.Conv2d) for b in range(1, nb + 1) for i in (1, 2, 3))


def test_seeded_construction_equals_the_plain_torch_sequence():
    """torch.manual_seed(s); factory() draws what the script's class draws: the modules in the order mlp1_1, mlp1_2, mlp1_3, mlp2_1,
    ..., h1, each by torch's own initialiser"""
    from gnn_matlang_amd import models
    torch.manual_seed(5)
    a = models.sr25_ppgn().state_dict()
    torch.manual_seed(5)
    b = models.sr25_ppgn().state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    torch.manual_seed(5)
    mods, cin = [], 3
    for blk in range(3):
        mods += [torch.nn.Conv2d(cin, 32, 1), torch.nn.Conv2d(cin, 32, 1), torch.nn.Conv2d(32 + cin, 32, 1)]
        cin = 32
    mods.append(torch.nn.Linear(192, 10))
    flat = [t for mod in mods for t in (mod.weight, mod.bias)]
    assert len(flat) == len(a) and all(torch.equal(t, v) for t, v in zip(flat, a.values()))


def test_cpu_tensors_raise():
    from gnn_matlang_amd import models
    from gnn_matlang_amd.graph import Batch
    m = models.graph8c_ppgn()
    data = Batch(X2=torch.zeros(2, 3, 8, 8), ppgn_n=torch.tensor([8, 3], dtype=torch.int32), ptr=torch.tensor([0, 8, 11]))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m(data)


def test_block_case_margins():
    x, n, W, gy, gr = R.block_case(3, 8, [8, 2, 5], 3, 32, True)
    z1, z2, z3, y, m = R.block_parts(x.double(), n, {k: v.double() for k, v in W.items()})
    for z in (z1, z2, z3):
        v = z[m.bool().expand_as(z)]
        assert float(v.abs().min()) > R.MARGIN * float(v.abs().max())
    assert float((x * (1 - m.float())).abs().min()) >= 0 and float((x * (1 - m.float())).abs().max()) > 0     # padding holds data
    assert not torch.equal(x, x.transpose(2, 3))
