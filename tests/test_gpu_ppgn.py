"""PPGN on the MI355X (csrc/gml_ppgn.hip, gnn_matlang_amd/ppgn.py, functional.PPGNBlockFunction, models.PPGN): the input tensors
bit-equal to the numpy restatement, the fused block against the float64 restatement over the shape matrix (tests/_ppgn_ref.py), the
padding, the three readouts, the roads, reproducibility and capture, every factory against float64 and the expressivity counts."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _ppgn_ref as R
from _gnnml1_ref import check
from conftest import GOLDEN, rel_err

pytestmark = pytest.mark.gpu

RAW = os.path.join(GOLDEN, 'raw')
MODEL_TOL = 1e-4

# (B, nmax, n list, Cin, C)
MATRIX = [(1, 8, [1], 3, 32), (3, 8, [8, 2, 5], 3, 32), (70, 8, 'random', 3, 20), (3, 25, [25, 15, 17], 32, 32),
          (2, 37, [16, 33], 23, 32), (2, 30, [30, 9], 40, 40), (3, 64, [64, 63, 1], 20, 20), (2, 64, [37, 64], 64, 64)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


def as_dicts(graphs):
    return [dict(x=x, edge_index=ei, y=y) for x, ei, y in graphs]


@pytest.fixture(scope='module')
def sr25():
    from gnn_matlang_amd import readers
    return as_dicts(readers.load_sr(os.path.join(RAW, 'sr251256.g6')))


@pytest.fixture(scope='module')
def graph8c():
    from gnn_matlang_amd import readers
    return as_dicts(readers.load_graph8c(os.path.join(RAW, 'graph8c.g6'))[:1000])


@pytest.fixture(scope='module')
def exp():
    from gnn_matlang_amd import readers
    return as_dicts(readers.load_exp(os.path.join(RAW, 'exp.npz'))[:50])


def device_batch(graphs, dev, nmax, nfeat):
    from gnn_matlang_amd import collate, ppgn
    return ppgn.attach(collate(graphs).to(dev), nmax, nfeat)


# ------------------------------------------------------------------------------------------------------------------ 1. inputs
def check_inputs(graphs, dev, nmax, nfeat):
    b = device_batch(graphs, dev, nmax, nfeat)
    X2, M, n = R.inputs_ref(graphs, nmax, nfeat)
    assert b.X2.is_contiguous() and b.M.is_contiguous() and b.ppgn_n.dtype == torch.int32
    assert np.array_equal(b.X2.cpu().numpy(), X2) and np.array_equal(b.M.cpu().numpy(), M) and np.array_equal(b.ppgn_n.cpu().numpy(), n)


def test_inputs_sr25(dev, sr25):
    assert len(sr25) == 15 and all(g['x'].shape[0] == 25 for g in sr25)
    check_inputs(sr25, dev, 25, 1)


def test_inputs_exp(dev, exp):
    assert len(set(g['x'].shape[0] for g in exp)) > 1
    check_inputs(exp, dev, 64, 1)


def test_inputs_hand_made(dev):
    """n = 1 beside n = nmax, directed edges, a self loop, a repeated edge, two features + a degree column that is not placed"""
    rng = np.random.default_rng(0)
    full = np.array([[0, 1, 2, 5, 5, 3, 3], [1, 2, 0, 4, 5, 0, 0]])
    gs = [dict(x=rng.standard_normal((1, 3)).astype(np.float32), edge_index=np.zeros((2, 0), np.int64), y=0),
          dict(x=rng.standard_normal((6, 3)).astype(np.float32), edge_index=full, y=0),
          dict(x=rng.standard_normal((3, 3)).astype(np.float32), edge_index=np.array([[0, 1], [1, 2]]), y=0)]
    check_inputs(gs, dev, 6, 2)
    check_inputs(gs, dev, 9, 0)


def test_inputs_graph_above_nmax_raises(dev, sr25):
    from gnn_matlang_amd import collate, ppgn
    with pytest.raises(ValueError, match='nmax'):
        ppgn.ppgn_inputs(collate(sr25[:2]).to(dev), 24, 1)


# ------------------------------------------------------------------------------------------------------------------ 2. block
_CPU = {}


def cpu_ref(key, case, readout, need_dx=True):
    """float64 and float32 restatements, computed once per case and shared"""
    k = (key, readout, need_dx)
    if k not in _CPU:
        x, n, W, gy, gr = case
        _CPU[k] = (R.block_cpu(x, n, W, gy, gr, readout, torch.float64, need_dx), R.block_cpu(x, n, W, gy, gr, readout, torch.float32, need_dx))
    return _CPU[k]


_CASES = {}


def get_case(idx, bias):
    if (idx, bias) not in _CASES:
        B, nmax, nl, Cin, C = MATRIX[idx]
        _CASES[(idx, bias)] = R.block_case(B, nmax, nl, Cin, C, bias, seed=idx)
    return _CASES[(idx, bias)]


def block_gpu(dev, case, readout='sum', need_dx=True, view=False, dy=True):
    from gnn_matlang_amd import functional as Fn
    x, n, W, gy, gr = case
    B, Cin, nmax = x.shape[:3]
    C = W['w1'].size(0)
    if view:                                           # channels 2 .. 2 + Cin of a wider tensor: not contiguous
        leaf = torch.randn(B, Cin + 3, nmax, nmax, device=dev)
        leaf[:, 2:2 + Cin] = x.to(dev)
        leaf.requires_grad_(need_dx)
        xd = leaf[:, 2:2 + Cin]
        assert not xd.is_contiguous()
    else:
        leaf = xd = x.to(dev).requires_grad_(need_dx)
    Wd = {k: (None if v is None else v.to(dev).requires_grad_(True)) for k, v in W.items()}
    assert Fn.ppgn_block_supported(xd, nmax, Cin, C)
    y, r = Fn.PPGNBlockFunction.apply(xd, n.to(dev), Wd['w1'], Wd['b1'], Wd['w2'], Wd['b2'], Wd['w3'], Wd['b3'], readout)
    grd = gr.to(dev)[:, :r.size(1)]
    if dy:
        torch.autograd.backward((y, r), (gy.to(dev), grd))
    else:
        r.backward(grd)
    dx = None if leaf.grad is None else (leaf.grad[:, 2:2 + Cin] if view else leaf.grad)
    if view and need_dx:
        assert float(leaf.grad[:, :2].abs().max()) == 0 and float(leaf.grad[:, 2 + Cin:].abs().max()) == 0
    return y.detach(), r.detach(), dx, {k: (None if v is None else v.grad) for k, v in Wd.items()}


def check_block(got, ref64, ref32, what, need_dx=True):
    y, r, dx, gW = got
    check(y, ref64[0], ref32[0], 'y', what, computed=True)
    check(r, ref64[1], ref32[1], 'readout', what, computed=True)
    if need_dx:
        check(dx, ref64[2], ref32[2], 'dx', what, computed=True)
    else:
        assert dx is None
    for k in sorted(gW):
        if ref64[3][k] is None:
            assert gW[k] is None
        else:
            check(gW[k], ref64[3][k], ref32[3][k], 'd' + k, what, computed=True)


@pytest.mark.parametrize('need_dx', [True, False])
@pytest.mark.parametrize('bias', [True, False])
@pytest.mark.parametrize('idx', range(len(MATRIX)))
def test_block_against_float64(dev, idx, bias, need_dx):
    case = get_case(idx, bias)
    ref64, ref32 = cpu_ref((idx, bias), case, 'sum', need_dx)
    check_block(block_gpu(dev, case, need_dx=need_dx), ref64, ref32, 'case %s bias=%s dx=%s' % (MATRIX[idx], bias, need_dx), need_dx)


def test_block_non_contiguous_view(dev):
    case = get_case(4, True)
    ref64, ref32 = cpu_ref((4, True), case, 'sum', True)
    check_block(block_gpu(dev, case, view=True), ref64, ref32, 'case %s view' % (MATRIX[4],))


# ------------------------------------------------------------------------------------------------------------------ 3. padding
@pytest.mark.parametrize('idx', [1, 4, 6])
def test_padding_is_zero_and_ignored(dev, idx):
    case = get_case(idx, True)
    x, n, W, gy, gr = case
    y, r, dx, gW = block_gpu(dev, case)
    out = (1 - R.mask(n, x.size(-1), torch.float32)).bool().to(dev)
    assert out.any()
    assert float(y[out.expand_as(y)].abs().max()) == 0 and float(dx[out.expand_as(dx)].abs().max()) == 0
    x2 = torch.where(out.cpu().expand_as(x), x * 3 + 7, x)
    assert not torch.equal(x2, x)
    y2, r2, dx2, gW2 = block_gpu(dev, (x2, n, W, gy, gr))
    assert torch.equal(y, y2) and torch.equal(r, r2) and torch.equal(dx, dx2)
    assert all(torch.equal(gW[k], gW2[k]) for k in gW)


# ------------------------------------------------------------------------------------------------------------------ 4. readouts
@pytest.mark.parametrize('dy', [True, False])
@pytest.mark.parametrize('readout', R.READOUTS)
def test_readouts(dev, readout, dy):
    case = get_case(3, True)
    x, n, W, gy, gr = case
    c = case if dy else (x, n, W, torch.zeros_like(gy), gr)              # dy = False: the block's output feeds the readout only
    ref64, ref32 = R.block_cpu(*c, readout, torch.float64), R.block_cpu(*c, readout, torch.float32)
    got = block_gpu(dev, c, readout=readout, dy=dy)
    assert got[1].shape == (3, 32 if readout == 'diag' else 64)
    check_block(got, ref64, ref32, 'readout %s dy=%s' % (readout, dy))


def test_mean_at_one_node(dev):
    from gnn_matlang_amd import functional as Fn
    x, n, W, gy, gr = get_case(6, True)                                 # n = [64, 63, 1]
    _, r32 = R.block_ref(x, n, W, 'mean')
    with torch.no_grad():
        _, r = Fn.PPGNBlockFunction.apply(x.to(dev), n.to(dev), *(W[k].to(dev) for k in ('w1', 'b1', 'w2', 'b2', 'w3', 'b3')), 'mean')
    r = r.cpu()
    assert torch.isnan(r32[2, 20:]).all() and torch.equal(torch.isnan(r), torch.isnan(r32))
    ok = ~torch.isnan(r32)
    assert rel_err(r[ok].numpy(), r32[ok].numpy()) <= 2e-5


# ------------------------------------------------------------------------------------------------------------------ 5. roads
@pytest.mark.parametrize('nmax,C', [(65, 4), (8, 65)])
def test_outside_the_range(dev, nmax, C):
    from gnn_matlang_amd import functional as Fn, models, _lib
    from gnn_matlang_amd.graph import Batch, _ptr, _stream
    B, Cin = 2, 3
    x = torch.randn(B, Cin, nmax, nmax, device=dev)
    assert not Fn.ppgn_block_supported(x, nmax, Cin, C)
    assert Fn.ppgn_block_supported(x[:, :, :8, :8].contiguous(), 8, Cin, 4)
    n = torch.tensor([nmax, 3], dtype=torch.int32, device=dev)
    w1, w2, w3 = torch.randn(C, Cin, device=dev), torch.randn(C, Cin, device=dev), torch.randn(C, C + Cin, device=dev)
    a12 = torch.full((B, 2 * C, nmax, nmax), 7.0, device=dev)
    p, y, r = torch.full((B, C, nmax, nmax), 7.0, device=dev), torch.full((B, C, nmax, nmax), 7.0, device=dev), torch.full((B, 2 * C), 7.0, device=dev)
    L = _lib.lib()
    rc = L.gml_ppgn_fwd(_ptr(x), _ptr(n), B, nmax, Cin, C, _ptr(w1), None, _ptr(w2), None, _ptr(w3), None, 0, _ptr(a12), _ptr(p), _ptr(y),
                        _ptr(r), _stream(dev))
    assert rc == _lib.GML_E_UNSUPPORTED
    flat = torch.full((int(L.gml_ppgn_dw_floats(Cin, C)),), 7.0, device=dev)
    ws = torch.zeros(16, device=dev)
    rc = L.gml_ppgn_bwd(_ptr(x), _ptr(n), B, nmax, Cin, C, _ptr(w1), _ptr(w2), _ptr(w3), _ptr(a12), _ptr(p), _ptr(y), _ptr(y), None, 0, None,
                        _ptr(flat), _ptr(ws), 64, _stream(dev))
    assert rc == _lib.GML_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (a12, p, y, r, flat))          # nothing was launched
    # the module takes the composition and gives the restatement's result
    torch.manual_seed(1)
    m = models.PPGN(Cin, C, 2, bias=True, readout='sum', hidden=10, head_act='tanh', nmax=nmax)
    params = {k: v.detach().double() for k, v in m.state_dict().items()}
    pooled64, out64 = R.model_ref(params, 2, x.cpu(), n.cpu(), 'sum', 'tanh', torch.float64)
    m = m.to(dev)
    data = Batch(X2=x, ppgn_n=n, ptr=torch.tensor([0, nmax, nmax + 3]))
    with torch.no_grad():
        assert rel_err(m.features(data).cpu().numpy(), pooled64.numpy()) <= MODEL_TOL
        assert rel_err(m(data).cpu().numpy(), out64.numpy()) <= MODEL_TOL


# ------------------------------------------------------------------------------------------------------------------ 6. reproducibility, capture
def test_bit_reproducible(dev):
    case = get_case(2, True)                           # 70 graphs: several partials per weight gradient
    a = block_gpu(dev, case)
    b = block_gpu(dev, case)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert all(torch.equal(a[3][k], b[3][k]) for k in a[3])


def test_captured_block_equals_eager(dev):
    from gnn_matlang_amd import functional as Fn
    c0, c1 = get_case(1, True), get_case(1, False)
    x0, n0, W, gy0, gr0 = c0
    x1, n1, gy1, gr1 = c1[0], torch.tensor([3, 8, 1], dtype=torch.int32), c1[3], c1[4]
    keys = ('w1', 'b1', 'w2', 'b2', 'w3', 'b3')
    sx, sn = x0.to(dev).requires_grad_(True), n0.to(dev)
    sW = [W[k].to(dev).requires_grad_(True) for k in keys]
    sgy, sgr = gy0.to(dev), gr0.to(dev)

    def step():
        y, r = Fn.PPGNBlockFunction.apply(sx, sn, *sW, 'sum')
        return (y, r) + torch.autograd.grad((y, r), [sx] + sW, (sgy, sgr))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                          # warm-up outside the capture
        step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = step()
    with torch.no_grad():
        sx.copy_(x1.to(dev)); sn.copy_(n1.to(dev)); sgy.copy_(gy1.to(dev)); sgr.copy_(gr1.to(dev))
    g.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in outs]
    y, r, dx, gW = block_gpu(dev, (x1, n1, W, gy1, gr1))
    want = [y, r, dx] + [gW[k] for k in keys]
    assert all(torch.equal(a, b) for a, b in zip(got, want))


# ------------------------------------------------------------------------------------------------------------------ 7. models
def model_case(name, dev, sr25, graph8c, exp):
    from gnn_matlang_amd import models, readers, synthetic
    if name == 'sr25_ppgn':
        gs, nmax, nfeat, loss = sr25, 25, 1, None
    elif name == 'graph8c_ppgn':
        gs, nmax, nfeat, loss = graph8c[:200], 8, 1, None
    elif name in ('exp_ppgn', 'exp_classify_ppgn'):
        gs, nmax, nfeat, loss = exp[:40], 64, 1, (models.exp_classify_loss if name == 'exp_classify_ppgn' else None)
    elif name == 'zinc_ppgn':
        gs, nmax, nfeat, loss = as_dicts(synthetic.make_graphs('zinc', 16, seed=5)), 37, 21, models.zinc_loss
    elif name == 'counting_ppgn':
        gs, nmax, nfeat, loss = as_dicts(synthetic.make_graphs('counting', 16, seed=5)), 30, 1, models.counting_loss
    else:
        gs, nmax, nfeat, loss = as_dicts(readers.load_mutag(os.path.join(RAW, 'mutag.mat'))[:16]), 28, 7, models.mutag_loss
    return gs, nmax, nfeat, loss


@pytest.mark.parametrize('name', ['sr25_ppgn', 'graph8c_ppgn', 'exp_ppgn', 'exp_classify_ppgn', 'zinc_ppgn', 'counting_ppgn', 'mutag_ppgn'])
def test_models_against_float64(dev, sr25, graph8c, exp, name):
    from gnn_matlang_amd import models
    gs, nmax, nfeat, loss = model_case(name, dev, sr25, graph8c, exp)
    b = device_batch(gs, dev, nmax, nfeat)
    torch.manual_seed(11)
    m = getattr(models, name)()
    assert m.mlp1_1.weight.size(1) == nfeat + 2 and m.nmax == nmax
    p64 = {k: v.detach().double().clone().requires_grad_(True) for k, v in m.named_parameters()}
    X2, _, n = R.inputs_ref(gs, nmax, nfeat)
    pooled64, out64 = R.model_ref(p64, m.nblocks, X2, torch.from_numpy(n), m.readout, m.head_act, torch.float64)
    y = b.y
    wsum = torch.randn(out64.shape, generator=torch.Generator().manual_seed(3))
    l64 = loss(out64, y.cpu().to(torch.float64 if y.is_floating_point() else y.dtype)) if loss is not None else (out64 * wsum.double()).sum()
    l64.backward()
    m = m.to(dev)
    pooled = m.features(b)
    out = m(b)
    l = loss(out, y) if loss is not None else (out * wsum.to(dev)).sum()
    l.backward()
    e = {'pooled': rel_err(pooled.detach().cpu().numpy(), pooled64.detach().numpy()),
         'out': rel_err(out.detach().cpu().numpy(), out64.detach().numpy())}
    for k, v in m.named_parameters():
        e[k] = rel_err(v.grad.cpu().numpy(), p64[k].grad.numpy())
    print(name, {k: '%.2e' % v for k, v in e.items()})
    assert float(pooled64.abs().max()) > 0
    assert max(e.values()) <= MODEL_TOL, e


def test_reference_shaped_state_dict_loads(dev):
    from gnn_matlang_amd import models
    torch.manual_seed(2)
    ref = torch.nn.Module()
    cin = 3
    for blk in (1, 2, 3):                               # the script's class: Conv2d(., ., 1) modules and one Linear
        for i, w in ((1, cin), (2, cin), (3, 32 + cin)):
            setattr(ref, 'mlp%d_%d' % (blk, i), torch.nn.Conv2d(w, 32, 1))
        cin = 32
    ref.h1 = torch.nn.Linear(192, 10)
    sd = ref.state_dict()
    assert sd['mlp1_3.weight'].shape == (32, 35, 1, 1)
    m = models.sr25_ppgn()
    m.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())


# ------------------------------------------------------------------------------------------------------------------ 8. expressivity
def reference_counts(factory, graphs, nmax, seeds, tol=1e-3):
    """the float64 restatement with numpy distances; asserts that no pair's decision hangs on the tolerance"""
    X2, _, n = R.inputs_ref(graphs, nmax, 1)
    G = len(graphs)
    iu = np.triu_indices(G, 1)
    dmax = np.zeros(iu[0].size)
    sep = np.zeros(iu[0].size, dtype=bool)
    counts = []
    for s in seeds:
        torch.manual_seed(int(s))
        m = factory()
        p = {k: v.detach().double() for k, v in m.state_dict().items()}
        with torch.no_grad():
            E = R.model_ref(p, m.nblocks, X2, torch.from_numpy(n), m.readout, m.head_act, torch.float64)[1].numpy()
        d = np.zeros(iu[0].size)
        for k in range(E.shape[1]):
            d += np.abs(E[iu[0], k] - E[iu[1], k])
        dmax = np.maximum(dmax, d)
        sep |= d > tol
        counts.append(int((~sep).sum()))
    band = ~((dmax > 2 * tol) | (dmax < tol / 2))
    assert not band.any(), 'pairs whose decision hangs on the tolerance: %d' % int(band.sum())
    return counts


@pytest.mark.parametrize('which', ['sr25', 'graph8c'])
def test_count_similar_equals_float64(dev, sr25, graph8c, which):
    from gnn_matlang_amd import expressivity, models
    gs, nmax, factory = (sr25, 25, models.sr25_ppgn) if which == 'sr25' else (graph8c, 8, models.graph8c_ppgn)
    seeds = [0, 1, 2]
    want = reference_counts(factory, gs, nmax, seeds)
    got = expressivity.count_similar(factory, device_batch(gs, dev, nmax, 1), seeds=seeds)
    print(which, got, want)
    assert got == want
