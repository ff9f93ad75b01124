"""ChebNet without a device: the restatement of tests/_cheb_ref.py (its adjoint backward against finite differences of its forward and
against autograd), the torch-op composition functional.cheb_conv_torch against it, the module's parameters and initialisation, every
factory's ordered state_dict against tests/golden/cheb_contract.json (written from the scripts' definitions), the opt-in graph fields
of collate and DeviceDataset, the refusal messages and the kink margins of every case of the GPU layer matrix (tests/test_gpu_cheb.py)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import _cheb_ref as R
from conftest import GOLDEN, rel_err

RAW = os.path.join(GOLDEN, 'raw')
CONTRACT = json.load(open(os.path.join(GOLDEN, 'cheb_contract.json')))


def multigraph():
    """two graphs in one batch: a directed multigraph with self loops (0 -> 0 twice, 3 -> 3), a repeated edge (1 -> 2 twice), one-way
    edges and an isolated node (4) beside a triangle with a pendant; lambda_max differs per graph"""
    src = [0, 0, 1, 1, 2, 3, 3, 0, 2, 5, 6, 6, 7, 5, 7, 8]
    dst = [0, 0, 2, 2, 1, 3, 0, 1, 3, 6, 5, 7, 6, 7, 5, 7]
    ei = np.array([src, dst], np.int64)
    batch = torch.tensor([0] * 5 + [1] * 4)
    return ei, 9, batch, torch.tensor([1.7, 2.0], dtype=torch.float64)


def small_case(shape, act, dtype, seed=0, margin=0.0):
    ei, N, batch, lam = multigraph()
    L = R.laplacian(ei, N, batch, lam, dtype)
    while R.margin(R.draw_case(shape, N, seed), L, act) < margin:
        seed += 1
    c = {k: v.to(dtype) for k, v in R.draw_case(shape, N, seed).items()}
    return c, torch.from_numpy(ei), N, batch, lam, L


def test_laplacian_by_hand():
    """the multigraph's L^ written out: self loops dropped, the repeat counted twice, deg over the SOURCES, the diagonal s - 1 for the
    isolated node too, s per graph"""
    ei, N, batch, lam = multigraph()
    A = R.adjacency(ei, N, torch.float64)
    assert A.diagonal().abs().sum() == 0 and A[2, 1] == 2 and A[1, 2] == 1 and A[0, 3] == 1 and A[3, 0] == 0
    deg = A.sum(0)
    assert deg.tolist() == [1, 2, 2, 1, 0, 2, 2, 2, 1]
    L = R.laplacian(ei, N, batch, lam, torch.float64)
    s0, s1 = 2 / 1.7, 1.0
    assert abs(float(L[2, 1]) + s0 * 2 / math.sqrt(2 * 2)) < 1e-15 and abs(float(L[0, 3]) + s0 / math.sqrt(1 * 1)) < 1e-15
    assert float(L[3, 0]) == 0 and abs(float(L[4, 4]) - (s0 - 1)) < 1e-15 and float(L[4].abs().sum()) == abs(s0 - 1)
    assert abs(float(L[7, 8]) + s1 / math.sqrt(2 * 1)) < 1e-15 and float(L[8, 8]) == 0.0
    assert float(L[:5, 5:].abs().sum() + L[5:, :5].abs().sum()) == 0
    assert torch.equal(R.laplacian(ei, N, None, None, torch.float64), R.laplacian(ei, N, batch, 2.0, torch.float64))


@pytest.mark.parametrize('K', [1, 2, 6])
@pytest.mark.parametrize('act', R.ACTS)
def test_adjoint_backward_against_gradcheck(act, K):
    c, _, _, _, _, L = small_case((3, 4, K), act, torch.float64, seed=3, margin=2e-3)
    assert R.margin(c, L, act) > 1e-3                     # finite differences of 1e-6 stay on one side of every kink
    leaves = [c[k].clone().requires_grad_(True) for k in ('x', 'W', 'b')]
    assert torch.autograd.gradcheck(lambda *a: R.AnalyticCheb.apply(L, act, *a), leaves, eps=1e-6, atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize('K', [1, 2, 3, 6, 8])
@pytest.mark.parametrize('act', R.ACTS)
def test_adjoint_backward_equals_autograd(act, K):
    c, _, _, _, _, L = small_case((5, 6, K), act, torch.float64, seed=4)
    leaves = {k: c[k].clone().requires_grad_(True) for k in ('x', 'W', 'b')}
    R.forward(leaves['x'], L, leaves['W'], leaves['b'], act).backward(c['dy'])
    d = R.backward(c['x'], L, c['W'], c['b'], act, c['dy'])
    for k, g in (('x', 'dx'), ('W', 'dW'), ('b', 'db')):
        assert rel_err(d[g].numpy(), leaves[k].grad.numpy()) <= 1e-12, k


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
@pytest.mark.parametrize('K', [1, 2, 5])
@pytest.mark.parametrize('act', R.ACTS)
def test_cheb_conv_torch_against_restatement(act, K, dtype):
    """self loops, a repeated edge, an isolated node and one-way edges, two graphs with their own lambda_max"""
    from gnn_matlang_amd import functional as Fn
    c, ei, N, batch, lam, L = small_case((7, 9, K), act, dtype, seed=5, margin=1e-4)
    leaves = {k: c[k].clone().requires_grad_(True) for k in ('x', 'W', 'b')}
    y = Fn.cheb_conv_torch(leaves['x'], ei, leaves['W'], leaves['b'], batch, lam.to(dtype), act)
    y.backward(c['dy'])
    d = R.backward(c['x'], L, c['W'], c['b'], act, c['dy'])
    tol = 1e-12 if dtype == torch.float64 else 2e-5
    assert rel_err(y.detach().numpy(), R.forward(c['x'], L, c['W'], c['b'], act).numpy()) <= tol
    for k, g in (('x', 'dx'), ('W', 'dW'), ('b', 'db')):
        assert rel_err(leaves[k].grad.numpy(), d[g].numpy()) <= tol, k


def test_cheb_conv_torch_lambda_forms_and_no_bias():
    from gnn_matlang_amd import functional as Fn
    c, ei, N, batch, lam, _ = small_case((3, 4, 3), None, torch.float64)
    for given, ref in ((None, None), (2.0, None), (1.6, 1.6), (torch.tensor([1.6], dtype=torch.float64), 1.6)):
        want = R.forward(c['x'], R.laplacian(ei, N, batch, ref, torch.float64), c['W'], None, 'tanh')
        for bt in (None, batch):
            assert rel_err(Fn.cheb_conv_torch(c['x'], ei, c['W'], None, bt, given, 'tanh').numpy(), want.numpy()) <= 1e-14
    none = torch.zeros(2, 0, dtype=torch.int64)
    y = Fn.cheb_conv_torch(c['x'], none, c['W'], c['b'], batch, lam)            # no edge: L^ = diag(s - 1)
    s1 = (2 / lam[batch] - 1).unsqueeze(1)
    want = c['x'] @ c['W'][0] + (s1 * c['x']) @ c['W'][1] + ((2 * s1 * s1 - 1) * c['x']) @ c['W'][2] + c['b']
    assert rel_err(y.numpy(), want.numpy()) <= 1e-14
    with pytest.raises(ValueError, match='batch'):
        Fn.cheb_conv_torch(c['x'], ei, c['W'], None, None, lam)
    with pytest.raises(ValueError, match='act'):
        Fn.cheb_conv_torch(c['x'], ei, c['W'], None, None, None, 'elu')


def test_module_parameters_and_glorot():
    from gnn_matlang_amd import ChebConv
    torch.manual_seed(0)
    m = ChebConv(25, 64, 5)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [('weight', (5, 25, 64)), ('bias', (64,))]
    assert [k for k, _ in m.named_parameters()] == ['weight', 'bias']
    a = math.sqrt(6.0 / (25 + 64))                                               # 1.6.1's glorot: the last two dimensions
    assert float(m.weight.detach().abs().max()) <= a and float(m.weight.detach().abs().max()) > 0.98 * a and float(m.bias.detach().abs().max()) == 0.0
    assert abs(float(m.weight.detach().std()) - a / math.sqrt(3)) < 0.02 * a
    w0 = m.weight.detach().clone()
    with torch.no_grad():
        m.bias.fill_(1.0)
    m.reset_parameters()
    assert not torch.equal(m.weight, w0) and float(m.bias.detach().abs().max()) == 0.0
    nb = ChebConv(4, 8, 2, bias=False)
    assert nb.bias is None and list(nb.state_dict()) == ['weight']
    m2 = ChebConv(25, 64, 5)
    m2.load_state_dict(m.state_dict(), strict=True)
    assert torch.equal(m2.weight, m.weight)
    assert 'K=5' in repr(m)


def test_module_on_the_cpu_takes_the_composition():
    from gnn_matlang_amd import ChebConv
    c, ei, N, batch, lam, L = small_case((3, 4, 4), 'relu', torch.float64, seed=2, margin=1e-4)
    m = ChebConv(3, 4, 4).double()
    with torch.no_grad():
        m.weight.copy_(c['W']); m.bias.copy_(c['b'])
    y = m(c['x'], ei, batch=batch, lambda_max=lam, act='relu')
    assert rel_err(y.detach().numpy(), R.forward(c['x'], L, c['W'], c['b'], 'relu').numpy()) <= 1e-13


def test_refusals():
    from gnn_matlang_amd import ChebConv, collate, models
    with pytest.raises(NotImplementedError, match="normalization='rw'"):
        ChebConv(4, 8, 3, normalization='rw')
    with pytest.raises(NotImplementedError, match='normalization=None'):
        ChebConv(4, 8, 3, normalization=None)
    with pytest.raises(ValueError, match='K >= 1'):
        ChebConv(4, 8, 0)
    with pytest.raises(ValueError):
        models.Cheb(2, (32, 64), 4, act='elu')
    with pytest.raises(ValueError):
        models.Cheb(2, (), 4)
    with pytest.raises(ValueError):
        models.Cheb(2, (32,), 4, pool=None, head='mlp', hidden=4)
    with pytest.raises(ValueError):
        models.Cheb(2, (32,), 4, head='bn_mlp', hidden=4, nbn=1)
    # a batch without lmax: the model names the way to carry it (before anything touches a device)
    g = dict(x=np.ones((3, 2), np.float32), edge_index=np.array([[0, 1], [1, 0]], np.int64), y=0.0)
    with pytest.raises(ValueError, match=r"graph_fields=\('lmax',\)"):
        models.sr25_cheb().forward(_with_csr(collate([g])))


def _with_csr(b):
    b._csr['edge_index'] = object()                       # (the model asks for the adjacency first; the refusal comes before any kernel)
    return b


# ------------------------------------------------------------------------------------------------------------------ factories
@pytest.mark.parametrize('name', R.FACTORIES)
def test_factory_state_dict(name):
    from gnn_matlang_amd import models
    assert sorted(CONTRACT) == sorted(R.FACTORIES) and len(R.FACTORIES) == 14
    spec = CONTRACT[name]
    keys = [(k, tuple(s)) for k, s in spec['keys']]
    torch.manual_seed(1)
    m = getattr(models, name)()
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == keys
    assert m.K == spec['K'] and m.lmax == spec['lmax'] and m.conv1.in_channels == spec['ninp']
    g = torch.Generator().manual_seed(2)
    sd = {k: (torch.randn(s, generator=g) if k.split('.')[-1] != 'num_batches_tracked' else torch.tensor(7)) for k, s in keys}
    m.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    wide = any(max(s[1:]) > 64 for k, s in keys if k.startswith('conv') and k.endswith('weight'))
    assert wide == (name in R.WIDE)


def test_script_details():
    from gnn_matlang_amd import models
    assert models.zinc_cheb().K == 2                                  # Zinc12k.py:197 overrides its S = 5 default
    assert models.ptc_cheb().bn_after == frozenset() and hasattr(models.ptc_cheb(), 'bn2')        # declared, never called
    assert models.proteins_cheb().bn_after == {1, 2} and models.enzymes_contfeat_cheb().bn_after == {1, 2}
    assert models.filtering_cheb().pool is None and models.enzymes_cheb().pool == ('mean', 'max')
    assert models.sr25_cheb().act == 'tanh' and models.exp_classify_cheb().act == 'relu'
    assert models.freqclass_cheb().dropout == 0.2 and models.mnist75_cheb().dropout == 0.1 and models.ptc_cheb().dropout == 0.2
    assert models.enzymes_cheb().dropout == 0.1 and models.zinc_cheb().dropout == 0.0


# ------------------------------------------------------------------------------------------------------------------ graph fields
def _mutag_dicts(n, lmax=True):
    from gnn_matlang_amd import readers
    raw = readers.load_mutag(os.path.join(RAW, 'mutag.mat'))[:n]
    gs = [dict(x=x, edge_index=ei, y=np.float32(y)) for x, ei, y in raw]
    if lmax:
        for g, l in zip(gs, R.graph_lambdas(gs)):
            g['lmax'] = l
    return gs


def test_collate_graph_fields_are_opt_in():
    from gnn_matlang_amd import collate
    gs = _mutag_dicts(3)
    fields = lambda b: sorted(k for k in b.__dict__ if not k.startswith('_'))
    plain = collate(gs)
    assert fields(plain) == ['batch', 'edge_index', 'ptr', 'x', 'y']              # lmax in the dicts: not carried unless named
    b = collate(gs, graph_fields=('lmax',))
    assert fields(b) == ['batch', 'edge_index', 'lmax', 'ptr', 'x', 'y']
    assert b.lmax.dtype == torch.float32 and tuple(b.lmax.shape) == (3,) and b.lmax.tolist() == [float(g['lmax']) for g in gs]
    for k in ('x', 'edge_index', 'batch', 'ptr', 'y'):
        assert torch.equal(getattr(b, k), getattr(plain, k))
    with pytest.raises(KeyError):
        collate(_mutag_dicts(2, lmax=False), graph_fields=('lmax',))


def test_device_dataset_graph_fields_on_the_host():
    """from_graphs / tiled / batch / batch_padded with torch indexing only: on CPU tensors here"""
    from gnn_matlang_amd import SpectralDesign
    from gnn_matlang_amd.dataset import DeviceDataset
    from gnn_matlang_amd import readers
    raw = readers.load_mutag(os.path.join(RAW, 'mutag.mat'))[:6]
    gs = SpectralDesign(recfield=1, dv=2, nfreq=2).design_many(raw)
    for g in gs:
        g['w'] = float(g['x'].shape[0])
    plain = DeviceDataset.from_graphs(gs, 'cpu')
    assert plain.graph_fields == {} and not hasattr(plain.batch(torch.tensor([1, 0])), 'lmax')
    dd = DeviceDataset.from_graphs(gs, 'cpu', graph_fields=('lmax', 'w'))
    lm = [float(np.float32(g['lmax'])) for g in gs]
    assert sorted(dd.graph_fields) == ['lmax', 'w'] and dd.graph_fields['lmax'].tolist() == lm
    b = dd.batch(torch.tensor([4, 1, 5]))
    assert b.lmax.tolist() == [lm[4], lm[1], lm[5]] and b.w.tolist() == [float(gs[i]['x'].shape[0]) for i in (4, 1, 5)]
    t = dd.tiled(2)
    assert t.graph_fields['lmax'].tolist() == lm + lm
    G = len(dd)
    ids = torch.tensor([2, G, 0, G])
    p = dd.batch_padded(ids, dd.bounds(4), adjacency=True)
    assert p.lmax.tolist() == [lm[2], 2.0, lm[0], 2.0, 2.0] and p.w.tolist() == [gs[2]['x'].shape[0], 0.0, gs[0]['x'].shape[0], 0.0, 0.0]
    assert p.lmax.numel() == p.y.numel() and int(p.batch.max()) == 4               # padding nodes index the last entry
    q = plain.batch_padded(ids, plain.bounds(4))
    assert not hasattr(q, 'lmax')


# ------------------------------------------------------------------------------------------------------------------ GPU matrix
def test_matrix_cases_keep_the_kink_margin():
    """every relu case of the GPU layer matrix: all pre-activations of the float64 restatement lie at least MARGIN x max-abs away from
    0, so no relu decision can differ between fp32 and float64 -- no element is ever excluded from a comparison.  The float32
    restatement's own error on the pre-activations is printed: the margin must stay 3 x above it."""
    worst, worst_e32, seeds = float('inf'), 0.0, set()
    for si in range(len(R.SHAPES)):
        for g in sorted(R.GRAPHS):
            case, gr, L, seed = R.layer_case(si, 'relu', g)
            worst = min(worst, R.margin(case, L, 'relu'))
            seeds.add(seed - (1000 * si + 100 * R.ACTS.index('relu') + 10 * sorted(R.GRAPHS).index(g)))
            if g in ('hand', 'rand67', 'mutag16'):
                ei, N, batch, lam = gr
                d32, d64 = {k: v.float() for k, v in case.items()}, {k: v.double() for k, v in case.items()}
                L32 = R.laplacian(ei, N, batch, None if lam is None else lam.float(), torch.float32)
                p32 = R.forward(d32['x'], L32, d32['W'], d32['b'], 'relu', parts=True)[2]
                p64 = R.forward(d64['x'], L, d64['W'], d64['b'], 'relu', parts=True)[2]
                worst_e32 = max(worst_e32, float((p32.double() - p64).abs().max() / p64.abs().max()))
    print('smallest pre-activation margin %.2e, float32 pre-activation error %.2e, seed offsets used %s' % (worst, worst_e32, sorted(seeds)))
    assert worst >= R.MARGIN
    assert 3 * worst_e32 < R.MARGIN


def test_case_graphs_have_their_features():
    ei, N, batch, lam = R.get_graph('mutag16')
    assert lam.numel() == 16 and len(set(lam.tolist())) >= 4 and int(batch.max()) == 15 and N > 4 * 32
    assert R.get_graph('hand')[3] is None and R.NO_LAMBDA == 'hand'               # the lambda_max=None case
    ei, N, batch, lam = R.get_graph('star')
    assert lam.numel() == 2 and N == 204
    ei, N, batch, lam = R.get_graph('rand129')
    assert N == 129 and (ei[0] == ei[1]).any()                                      # self loops to drop; five tiles of 32 rows
    ei, N, _, _ = R.get_graph('loops')
    assert ((ei[1] == 7) & (ei[0] != 7)).sum() == 0 and ((ei[1] == 7) & (ei[0] == 7)).sum() == 1     # a row holding only a self loop
