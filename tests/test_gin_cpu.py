"""GIN without a device: the restatement of tests/_gin_ref.py (its analytic backward against finite differences of its forward and
against autograd), the torch-op composition functional.gin_conv_torch against it, the module's parameters, every factory's
state_dict written out by hand, the scripts' eps draws, the kink margins of every case of the GPU layer matrix
(tests/test_gpu_gin.py) and the EXP claim (no pair is ever separated) in float64."""
import os

import numpy as np
import pytest
import torch

import _gin_ref as R
from conftest import GOLDEN, rel_err

RAW = os.path.join(GOLDEN, 'raw')
LEAVES = {1: ('x', 'eps', 'W1', 'b1'), 2: ('x', 'eps', 'W1', 'b1', 'W2', 'b2')}
GRAD = dict(x='dx', eps='deps', W1='dW1', b1='db1', W2='dW2', b2='db2')


def small_case(shape, act, dtype, seed=0, margin=0.0, graph='loops'):
    """a small graph with the first seed from `seed` upwards whose kink margins reach `margin`"""
    ei, N = R.get_graph(graph)
    A = R.adjacency(ei, N, dtype)
    while min(R.margins(R.draw_case(shape, N, seed), A, act)) < margin:
        seed += 1
    c = {k: v.to(dtype) for k, v in R.draw_case(shape, N, seed).items()}
    return c, torch.from_numpy(ei), N, A


def test_self_loop_graph_has_its_features():
    ei, N = R.self_loops()
    pairs = list(zip(ei[0].tolist(), ei[1].tolist()))
    A = R.adjacency(ei, N, torch.float64)
    assert N == 9 and pairs.count((2, 2)) == 2 and pairs.count((1, 0)) == 2 and 8 not in ei
    assert A.diagonal().tolist() == [1, 0, 2, 0, 0, 1, 0, 1, 0]              # self loops are counted, as often as they occur
    assert A[7].sum() == 1 and A[7, 7] == 1 and A[8].sum() == 0 and A[:, 8].sum() == 0
    assert A[0, 1] == 2


@pytest.mark.parametrize('depth', [1, 2])
@pytest.mark.parametrize('act', R.ACTS)
def test_analytic_backward_against_gradcheck(act, depth):
    c, _, _, A = small_case((3, 5, 4, depth), act, torch.float64, seed=3, margin=2e-3)
    assert min(R.margins(c, A, act)) > 1e-3              # finite differences of 1e-6 stay on one side of every kink
    leaves = [c[k].clone().requires_grad_(True) for k in LEAVES[depth]]
    assert torch.autograd.gradcheck(lambda *a: R.AnalyticGIN.apply(A, act, *a), leaves, eps=1e-6, atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize('depth', [1, 2])
@pytest.mark.parametrize('act', R.ACTS)
def test_analytic_backward_equals_autograd(act, depth):
    c, _, _, A = small_case((5, 8, 6, depth), act, torch.float64, seed=4)
    leaves = {k: c[k].clone().requires_grad_(True) for k in LEAVES[depth]}
    y = R.forward(leaves['x'], A, leaves['eps'], R.lins_of(leaves), act)
    y.backward(c['dy'])
    d = R.backward(c['x'], A, c['eps'], R.lins_of(c), act, c['dy'])
    for k in LEAVES[depth]:
        assert rel_err(d[GRAD[k]].numpy(), leaves[k].grad.numpy()) <= 1e-12, k
    assert float(d['teps']) >= abs(float(d['deps']))


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
@pytest.mark.parametrize('depth', [1, 2])
@pytest.mark.parametrize('act', R.ACTS)
def test_gin_conv_torch_against_restatement(act, depth, dtype):
    from gnn_matlang_amd import functional as Fn
    c, ei, N, A = small_case((7, 12, 9, depth), act, dtype, seed=5, margin=1e-4)
    leaves = {k: c[k].clone().requires_grad_(True) for k in LEAVES[depth]}
    y = Fn.gin_conv_torch(leaves['x'], ei, leaves['eps'], R.lins_of(leaves), act)
    y.backward(c['dy'])
    d = R.backward(c['x'], A, c['eps'], R.lins_of(c), act, c['dy'])
    tol = 1e-12 if dtype == torch.float64 else 2e-5
    assert rel_err(y.detach().numpy(), R.forward(c['x'], A, c['eps'], R.lins_of(c), act).numpy()) <= tol
    for k in LEAVES[depth]:
        assert rel_err(leaves[k].grad.numpy(), d[GRAD[k]].numpy()) <= tol, k


def test_gin_conv_torch_without_edges_and_without_bias():
    from gnn_matlang_amd import functional as Fn
    c = {k: v.double() for k, v in R.draw_case((3, 4, 5, 2), 2, 0).items()}
    none = torch.zeros(2, 0, dtype=torch.int64)
    y = Fn.gin_conv_torch(c['x'], none, c['eps'], [(c['W1'], None), (c['W2'], None)], 'tanh')
    want = torch.tanh(torch.relu(((1 + c['eps']) * c['x']) @ c['W1'].t()) @ c['W2'].t())
    assert rel_err(y.numpy(), want.numpy()) <= 1e-15
    y1 = Fn.gin_conv_torch(c['x'], none, c['eps'], [(c['W1'], c['b1'])], None)
    assert rel_err(y1.numpy(), (((1 + c['eps']) * c['x']) @ c['W1'].t() + c['b1']).numpy()) <= 1e-15


def test_a_self_loop_edge_is_counted():
    """one node, one edge 0 -> 0: h = x + (1 + eps) x = (2 + eps) x, in the composition and in the restatement"""
    from gnn_matlang_amd import functional as Fn
    c = {k: v.double() for k, v in R.draw_case((3, 4, 0, 1), 1, 1).items()}
    ei = torch.zeros(2, 1, dtype=torch.int64)
    want = ((2 + c['eps']) * c['x']) @ c['W1'].t() + c['b1']
    assert rel_err(Fn.gin_conv_torch(c['x'], ei, c['eps'], R.lins_of(c)).numpy(), want.numpy()) <= 1e-15
    assert rel_err(R.forward(c['x'], R.adjacency(ei, 1, torch.float64), c['eps'], R.lins_of(c), None).numpy(), want.numpy()) <= 1e-15


def test_module_parameters_and_reset():
    from gnn_matlang_amd import GINConv
    from torch.nn import Linear, ReLU, Sequential
    torch.manual_seed(0)
    m = GINConv(Sequential(Linear(25, 64), ReLU(), Linear(64, 64)), eps=0.25, train_eps=True)
    assert {k: tuple(v.shape) for k, v in m.named_parameters()} == {'eps': (1,), 'nn.0.weight': (64, 25), 'nn.0.bias': (64,),
                                                                    'nn.2.weight': (64, 64), 'nn.2.bias': (64,)}
    assert list(m.state_dict()) == ['eps', 'nn.0.weight', 'nn.0.bias', 'nn.2.weight', 'nn.2.bias']
    assert isinstance(m.eps, torch.nn.Parameter) and m.initial_eps == 0.25 and m.eps.item() == 0.25
    w0 = m.nn[0].weight.detach().clone()
    with torch.no_grad():
        m.eps.fill_(3.0)
    m.reset_parameters()
    assert m.eps.item() == 0.25 and not torch.equal(m.nn[0].weight, w0)           # the Linears are redrawn, eps is refilled
    b = GINConv(Sequential(Linear(4, 8)))                                          # eps=0., train_eps=False: a buffer under the same key
    assert not isinstance(b.eps, torch.nn.Parameter) and 'eps' in dict(b.named_buffers()) and float(b.eps) == 0.0
    assert list(b.state_dict()) == ['eps', 'nn.0.weight', 'nn.0.bias'] and [k for k, _ in b.named_parameters()] == ['nn.0.weight', 'nn.0.bias']
    m2 = GINConv(Sequential(Linear(25, 64), ReLU(), Linear(64, 64)), train_eps=True)
    m2.load_state_dict(m.state_dict(), strict=True)
    assert torch.equal(m2.nn[2].weight, m.nn[2].weight) and m2.eps.item() == 0.25


def test_tuple_inputs_raise():
    from gnn_matlang_amd import GINConv
    m = GINConv(torch.nn.Sequential(torch.nn.Linear(4, 8)))
    with pytest.raises(NotImplementedError, match='tuple'):
        m((torch.zeros(2, 4), torch.zeros(2, 4)), torch.zeros(2, 0, dtype=torch.int64))


def test_other_nn_takes_the_composition_on_the_cpu():
    """an nn that is neither Linear nor Linear-ReLU-Linear: aggregate, then nn -- on any device"""
    from gnn_matlang_amd import GINConv
    torch.manual_seed(2)
    nn = torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.Tanh(), torch.nn.Linear(5, 2)).double()
    m = GINConv(nn, eps=0.5, train_eps=True).double()
    ei, N = R.self_loops()
    x = torch.randn(N, 3, dtype=torch.float64)
    y = m(x, torch.from_numpy(ei), act='relu')
    h = R.adjacency(ei, N, torch.float64) @ x + 1.5 * x
    assert rel_err(y.detach().numpy(), torch.relu(nn(h)).detach().numpy()) <= 1e-14


# ------------------------------------------------------------------------------------------------------------------ factories
def _conv(i, fin, w, depth):
    k = [('conv%d.eps' % i, (1,)), ('conv%d.nn.0.weight' % i, (w, fin)), ('conv%d.nn.0.bias' % i, (w,))]
    return k + ([('conv%d.nn.2.weight' % i, (w, w)), ('conv%d.nn.2.bias' % i, (w,))] if depth == 2 else [])


def _bn(i, w):
    return [('bn%d.weight' % i, (w,)), ('bn%d.bias' % i, (w,)), ('bn%d.running_mean' % i, (w,)), ('bn%d.running_var' % i, (w,)),
            ('bn%d.num_batches_tracked' % i, ())]


def _fc(n, out, fin):
    return [(n + '.weight', (out, fin)), (n + '.bias', (out,))]


_ISO = _conv(1, 2, 64, 1) + _conv(2, 64, 64, 1) + _conv(3, 64, 64, 1)
# the scripts' GinNet attributes in their declaration order (convI, bnI, ..., fc1, fc2), shapes by hand
KEYS = {
    'sr25_gin': _ISO + _fc('fc1', 10, 64),
    'graph8c_gin': _ISO + _fc('fc1', 10, 64),
    'exp_gin': _ISO + _fc('fc1', 10, 64),
    'exp_classify_gin': _ISO + _fc('fc1', 10, 64) + _fc('fc2', 1, 10),
    'zinc_gin': _conv(1, 25, 64, 2) + _bn(1, 64) + _conv(2, 64, 64, 2) + _bn(2, 64) + _conv(3, 64, 64, 2) + _bn(3, 64) + _conv(4, 64, 64, 2)
                + _bn(4, 64) + _fc('fc1', 32, 64) + _fc('fc2', 1, 32),
    'counting_gin': _conv(1, 2, 64, 2) + _conv(2, 64, 64, 2) + _conv(3, 64, 64, 2) + _conv(4, 64, 64, 2) + _conv(5, 64, 64, 2)
                    + _fc('fc1', 32, 64) + _fc('fc2', 1, 32),
    'mutag_gin': _conv(1, 8, 64, 2) + _bn(1, 64) + _conv(2, 64, 64, 2) + _bn(2, 64) + _conv(3, 64, 64, 2) + _bn(3, 64) + _fc('fc1', 10, 64)
                 + _fc('fc2', 1, 10),
    'freqclass_gin': _conv(1, 1, 64, 2) + _bn(1, 64) + _conv(2, 64, 64, 2) + _bn(2, 64) + _conv(3, 64, 64, 2) + _bn(3, 64) + _fc('fc1', 32, 64)
                     + _fc('fc2', 1, 32),
    'filtering_gin': _conv(1, 1, 64, 2) + _conv(2, 64, 64, 2) + _conv(3, 64, 64, 2) + _fc('fc2', 1, 64),
    'enzymes_gin': _conv(1, 4, 64, 2) + _bn(1, 64) + _conv(2, 64, 64, 2) + _bn(2, 64) + _conv(3, 64, 64, 2) + _bn(3, 64) + _conv(4, 64, 64, 2)
                   + _bn(4, 64) + _fc('fc2', 6, 128),
    'ptc_gin': _conv(1, 20, 200, 2) + _bn(1, 200) + _conv(2, 200, 200, 2) + _bn(2, 200) + _fc('fc2', 2, 400),
    'proteins_gin': _conv(1, 4, 200, 2) + _bn(1, 200) + _conv(2, 200, 200, 2) + _bn(2, 200) + _fc('fc2', 2, 400),
    'enzymes_contfeat_gin': _conv(1, 22, 200, 2) + _bn(1, 200) + _conv(2, 200, 200, 2) + _bn(2, 200) + _fc('fc2', 6, 400),
}


@pytest.mark.parametrize('name', R.FACTORIES)
def test_factory_state_dict(name):
    from gnn_matlang_amd import models
    assert sorted(KEYS) == sorted(R.FACTORIES) and len(R.FACTORIES) == 13
    torch.manual_seed(1)
    m = getattr(models, name)()
    own = m.state_dict()
    assert [(k, tuple(v.shape)) for k, v in own.items()] == KEYS[name]
    g = torch.Generator().manual_seed(2)
    sd = {k: (torch.randn(s, generator=g) if k.split('.')[-1] != 'num_batches_tracked' else torch.tensor(7)) for k, s in KEYS[name]}
    if name == 'enzymes_gin':                                # conv4 was built on nn3: a checkpoint holds the same tensors under both key sets
        for k in list(sd):
            if k.startswith('conv4.nn.'):
                sd[k] = sd[k.replace('conv4', 'conv3')]
    m.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    assert all(isinstance(getattr(m, 'conv%d' % i).eps, torch.nn.Parameter) for i in range(1, m.nlayers + 1))       # train_eps=True


def test_enzymes_shares_nn3():
    from gnn_matlang_amd import models
    m = models.enzymes_gin()
    assert m.conv4.nn is m.conv3.nn and m.conv3.nn[0].weight is m.conv4.nn[0].weight and m.conv4.eps is not m.conv3.eps
    sd = m.state_dict()
    assert sd['conv3.nn.2.weight'].data_ptr() == sd['conv4.nn.2.weight'].data_ptr()
    names = [k for k, _ in m.named_parameters()]
    assert 'conv4.eps' in names and not any(k.startswith('conv4.nn') for k in names)           # one tensor, listed once
    assert models.zinc_gin().conv4.nn is not models.zinc_gin().conv3.nn


@pytest.mark.parametrize('name', ['sr25_gin', 'graph8c_gin', 'exp_gin', 'exp_classify_gin'])
@pytest.mark.parametrize('k', [0, 5])
def test_uniform_eps_are_the_scripts_draws(name, k):
    """sr25.py:78-80: r1, r2, r3 = np.random.uniform() three times, before any Linear is built"""
    from gnn_matlang_amd import models
    np.random.seed(k)
    want = [np.random.uniform() for _ in range(3)]
    np.random.seed(k)
    m = getattr(models, name)()
    got = [getattr(m, 'conv%d' % i).eps.item() for i in (1, 2, 3)]
    assert got == [float(np.float32(w)) for w in want]
    assert [getattr(m, 'conv%d' % i).initial_eps for i in (1, 2, 3)] == want
    assert models.zinc_gin().conv1.eps.item() == 0.0


def test_arguments_that_raise():
    from gnn_matlang_amd import models
    with pytest.raises(ValueError):
        models.GIN(2, 64, 3, act='elu')
    with pytest.raises(ValueError):
        models.GIN(2, 64, 3, depth=3)
    with pytest.raises(ValueError):
        models.GIN(2, 64, 3, share_nn={2: 3})
    with pytest.raises(ValueError):
        models.GIN(2, 64, 3, head='bn_mlp', hidden=4)
    assert not hasattr(models, 'mnist75_gin')                 # out of scope: its head normalises the pooled rows with a BatchNorm named bn3


# ------------------------------------------------------------------------------------------------------------------ GPU matrix, EXP
def test_matrix_cases_keep_the_kink_margin():
    """every case of the GPU layer matrix: all hidden pre-activations (and, for relu, all outer ones) of the float64 restatement lie at
    least MARGIN x max-abs away from 0, so no relu decision can differ between fp32 and float64 -- no element is ever excluded from a
    comparison.  The float32 restatement's own error on the pre-activations is printed: the margin must stay 3 x above it."""
    worst, worst_e32, seeds = float('inf'), 0.0, set()
    for si in range(len(R.SHAPES)):
        for act in R.ACTS:
            for g in sorted(R.GRAPHS):
                case, ei, N, A, seed = R.layer_case(si, act, g)
                worst = min(worst, *R.margins(case, A, act))
                seeds.add(seed - (1000 * si + 100 * R.ACTS.index(act) + 10 * sorted(R.GRAPHS).index(g)))
                if g in ('hand', 'rand67'):
                    d32, d64 = {k: v.float() for k, v in case.items()}, {k: v.double() for k, v in case.items()}
                    p32 = R.forward(d32['x'], A.float(), d32['eps'], R.lins_of(d32), act, parts=True)
                    p64 = R.forward(d64['x'], A, d64['eps'], R.lins_of(d64), act, parts=True)
                    for j in (2, 4):
                        if p64[j] is not None:
                            worst_e32 = max(worst_e32, float((p32[j].double() - p64[j]).abs().max() / p64[j].abs().max()))
    print('smallest pre-activation margin %.2e, float32 pre-activation error %.2e, seed offsets used %s' % (worst, worst_e32, sorted(seeds)))
    assert worst >= R.MARGIN
    assert 3 * worst_e32 < R.MARGIN


def _as_batch(gs):
    x = np.concatenate([g[0] for g in gs])
    off = np.cumsum([0] + [g[0].shape[0] for g in gs])
    ei = np.concatenate([np.asarray(g[1], np.int64) + off[i] for i, g in enumerate(gs)], 1)
    batch = np.repeat(np.arange(len(gs)), [g[0].shape[0] for g in gs])
    return x, ei, batch, off


def test_embed_sparse_equals_the_dense_restatement():
    from gnn_matlang_amd import models, readers
    gs = readers.load_exp(os.path.join(RAW, 'exp.npz'))[:6]
    x, ei, batch, off = _as_batch(gs)
    for name in ('exp_gin', 'exp_classify_gin'):
        torch.manual_seed(0)
        m = getattr(models, name)(x.shape[1])
        p = {k: v.detach().double() for k, v in m.state_dict().items()}
        a = R.embed_sparse(p, m, x, ei, batch, len(gs))
        b = R.ginnet_ref(p, m, x, ei, off.tolist())
        assert rel_err(a.numpy(), b.numpy()) <= 1e-13


def test_exp_pairs_stay_similar_in_float64():
    """exp_iso.py:284-304 with GinNet: a 1-WL bounded model separates none of the 600 EXP pairs.  In float64 the largest pair distance
    over seeds 0-2 is rounding noise (4.6e-15 when this was written) against the tolerance 1e-3: no pair hangs on the tolerance."""
    from gnn_matlang_amd import expressivity, models, readers
    gs = readers.load_exp(os.path.join(RAW, 'exp.npz'))
    x, ei, batch, _ = _as_batch(gs)
    pairs = expressivity.exp_pairs(len(gs))
    assert pairs.shape == (600, 2)
    dmax = 0.0
    for s in (0, 1, 2):
        torch.manual_seed(s)
        np.random.seed(s)
        m = models.exp_gin(x.shape[1])
        p = {k: v.detach().double() for k, v in m.state_dict().items()}
        E = R.embed_sparse(p, m, x, ei, batch, len(gs)).numpy()
        assert np.abs(E).max() > 0.1                                              # (not a constant-zero embedding)
        dmax = max(dmax, float(np.abs(E[pairs[:, 0]] - E[pairs[:, 1]]).sum(1).max()))
    print('largest EXP pair distance in float64: %.2e' % dmax)
    assert dmax < 1e-3 / 2 and dmax < 1e-9
