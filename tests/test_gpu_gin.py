"""GIN on the MI355X (csrc/gml_gin.hip, functional.GINConvFunction, gin.GINConv, models.GIN): the layer against the float64 restatement
of tests/_gin_ref.py over the shape / activation / graph matrix -- through the module and through the raw ABI with sentinel-framed
buffers --, the refusals, the order and edge cases, reproducibility and capture (eps included), every factory against the float64
GinNet restatement, the two roads, the padded static batch and the expressivity counts."""
import copy
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import _conv_ref as CR
import _gin_ref as R
from _gnnml1_ref import TOL, check
from conftest import GOLDEN, rel_err

pytestmark = pytest.mark.gpu

RAW = os.path.join(GOLDEN, 'raw')
MODEL_TOL = 1e-4
# deps is ONE scalar: the signed sum of N Fin terms dh[i, c] x[i, c].  An fp32 evaluation's error scales with the TERM sum
# teps = sum |dh| |x|, not with the result.  Where the signed sum keeps at least 1 / 100 of its term sum it is held like every other
# gradient (check(computed=True): TOL of |float64|, or 4 x the float32 restatement's own error).  Below that ("tiny": the terms have
# cancelled two digits or more, so TOL of the result would ask for 2e-7 of the term sum -- a few ulp of a sum of thousands of terms)
# it is held to TOL x teps, as check_att of tests/test_gpu_gat.py holds attention gradients that cancel.
EPS_CANCEL = 1e-2


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


_CSR = {}


def csr_of(gname, dev):
    from gnn_matlang_amd.graph import GraphCSR
    if gname not in _CSR:
        ei, N = R.get_graph(gname)
        _CSR[gname] = GraphCSR.from_edge_index(torch.from_numpy(ei).to(dev), N)
    return _CSR[gname]


def grad_keys(case):
    return ('dx', 'deps', 'dW1', 'db1') + (('dW2', 'db2') if 'W2' in case else ())


def make_module(dev, case):
    from gnn_matlang_amd import GINConv
    from torch.nn import Linear, ReLU, Sequential
    Fh, Fin = case['W1'].shape
    nn = Sequential(Linear(Fin, Fh), ReLU(), Linear(Fh, case['W2'].size(0))) if 'W2' in case else Sequential(Linear(Fin, Fh))
    m = GINConv(nn, eps=0.0, train_eps=True).to(dev)
    with torch.no_grad():
        m.eps.copy_(case['eps']); m.nn[0].weight.copy_(case['W1']); m.nn[0].bias.copy_(case['b1'])
        if 'W2' in case:
            m.nn[2].weight.copy_(case['W2']); m.nn[2].bias.copy_(case['b2'])
    return m


def layer_gpu(dev, case, csr, act, need_dx=True):
    """the module on the fused road: (y, {dx, deps, dW1, db1[, dW2, db2]})"""
    from gnn_matlang_amd import functional as Fn
    m = make_module(dev, case)
    x = case['x'].to(dev).requires_grad_(need_dx)
    assert Fn.gin_conv_supported(x, case['W1'].size(0), case['W2'].size(0) if 'W2' in case else None)
    y = m(x, csr, act=act)
    y.backward(case['dy'].to(dev))
    g = dict(dx=x.grad, deps=m.eps.grad, dW1=m.nn[0].weight.grad, db1=m.nn[0].bias.grad)
    if 'W2' in case:
        g.update(dW2=m.nn[2].weight.grad, db2=m.nn[2].bias.grad)
    return y.detach(), g


def check_eps(got, ref64, ref32, what):
    d64, t = float(ref64['deps']), float(ref64['teps'])
    g = float(got.detach().cpu().double().reshape(-1)[0])
    print('%s deps: got %.6e, float64 %.6e, float32 restatement %.6e, term sum %.3e' % (what, g, d64, float(ref32['deps']), t))
    assert np.isfinite(g)
    if t == 0:                                            # every term is zero (one node whose only relu output is off): exactly 0
        assert g == 0.0 and d64 == 0.0
        return
    if abs(d64) >= EPS_CANCEL * t:
        return check(got.reshape(1), ref64['deps'], ref32['deps'], 'deps', what, computed=True)
    assert abs(g - d64) <= TOL * t, '%s deps: |got - float64| %.3e > %.1e x term sum %.3e' % (what, abs(g - d64), TOL, t)


def check_layer(got, ref64, ref32, what, need_dx=True):
    y, g = got
    check(y, ref64['y'], ref32['y'], 'y', what, computed=True)
    for k in g:
        if k == 'dx' and not need_dx:
            assert g[k] is None
        elif k == 'deps':
            check_eps(g[k], ref64, ref32, what)
        else:
            check(g[k], ref64[k], ref32[k], k, what, computed=True)


def assert_margin(case, A, act, what):
    """kinks: asserted on the float64 restatement before any result is compared; no element is excluded"""
    mh, mo = R.margins(case, A, act)
    assert mh >= R.MARGIN and mo >= R.MARGIN, '%s: kink margin %.2e / %.2e below %.0e' % (what, mh, mo, R.MARGIN)


# ------------------------------------------------------------------------------------------------------------------ 1. layer matrix
MATRIX = [(si, act, g) for si in range(len(R.SHAPES)) for act in R.ACTS for g in sorted(R.GRAPHS)]


@pytest.mark.parametrize('need_dx', [True, False])
@pytest.mark.parametrize('si,act,gname', MATRIX)
def test_module_against_float64(dev, si, act, gname, need_dx):
    case, ei, N, A, seed = R.layer_case(si, act, gname)
    what = 'shape %s act=%s graph=%s seed=%d dx=%s' % (R.SHAPES[si], act, gname, seed, need_dx)
    assert_margin(case, A, act, what)
    ref64, ref32 = R.layer_ref((si, act, gname), case, A, act)
    check_layer(layer_gpu(dev, case, csr_of(gname, dev), act, need_dx), ref64, ref32, what, need_dx)


def _dev_buf(buf, dev):
    return torch.from_numpy(buf).to(dev)


def _at(t, off):
    return ctypes.c_void_p(t.data_ptr() + 4 * int(off))


def abi_run(dev, case, csr, act, depth=None, need_dx=True, ws_short=0, bias=True):
    """gml_gin_fwd / _bwd on sentinel-framed buffers with padded leading dimensions (ldx = Fin + 3, ...); the shape is the case's own
    (depth: an override for the refusal test).  Returns the return codes, the host copies of every buffer, their layouts and the
    workspace tail."""
    from gnn_matlang_amd import _lib
    from gnn_matlang_amd.graph import _ptr, _stream
    L = _lib.lib()
    two = 'W2' in case
    N, Fin, Fh = case['x'].size(0), case['x'].size(1), case['W1'].size(0)
    Fout = case['W2'].size(0) if two else 0
    depth = depth if depth is not None else (2 if two else 1)
    Fo, E = (Fout if two else Fh), csr.E
    ldx, lddy = Fin + 3, Fo + 1
    x = torch.zeros(N, ldx, device=dev)
    x[:, :Fin] = case['x'].to(dev)
    dy = torch.zeros(N, lddy, device=dev)
    dy[:, :Fo] = case['dy'].to(dev)
    d = lambda k: case[k].to(dev).contiguous() if k in case and (bias or k[0] != 'b') else None
    eps, w1, b1, w2, b2 = d('eps'), d('W1'), d('b1'), d('W2'), d('b2')
    P = Fh * Fin + Fh + (Fout * Fh + Fout if two else 0) + 1
    lay = dict(h=(N, Fin, Fin + 1), t=(N, Fh, Fh + 2), y=(N, Fo, Fo + 3), dx=(N, Fin, Fin + 5), dflat=(1, P, P))
    bufs, offs = {}, {}
    for k, (n, nc, l) in lay.items():
        hb, offs[k] = CR.alloc(n, nc, l, head=k in ('y', 'dx'))
        bufs[k] = _dev_buf(hb, dev)
    nws = int(L.gml_gin_bwd_workspace_bytes(N, Fin, Fh, Fout, depth)) // 4
    assert P == int(L.gml_gin_dflat_floats(Fin, Fh, Fout, depth)) or nws == 0
    wsn = max(nws, 4) if nws else 4096
    hb, _ = CR.alloc(1, wsn, wsn + 64, guard_rows=0)
    ws = _dev_buf(hb, dev)
    st = _stream(dev)
    p = lambda k: _at(bufs[k], offs[k])
    a = R.ACTS.index(act)
    rc = [L.gml_gin_fwd(_ptr(csr.rowptr), _ptr(csr.col), _ptr(x), ldx, N, E, Fin, _ptr(eps), _ptr(w1), _ptr(b1), Fh, _ptr(w2), _ptr(b2), Fout,
                        depth, a, p('h'), lay['h'][2], p('t'), lay['t'][2], p('y'), lay['y'][2], st)]
    rc.append(L.gml_gin_bwd(_ptr(csr.rowptr_t), _ptr(csr.col_t), _ptr(x), ldx, p('h'), lay['h'][2], p('t'), lay['t'][2], p('y'), lay['y'][2],
                            _ptr(dy), lddy, N, E, Fin, _ptr(eps), _ptr(w1), Fh, _ptr(w2), Fout, depth, a, p('dx') if need_dx else None,
                            lay['dx'][2], p('dflat'), _ptr(ws), (wsn - ws_short) * 4, st))
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in bufs.items()}
    return rc, host, lay, ws.cpu().numpy()[wsn:]


def abi_values(host, lay, untouched=()):
    """{name: values}, asserting that every guard word of every buffer is still the sentinel (and, for `untouched`, every word)"""
    out = {}
    for k, (n, nc, l) in lay.items():
        if k in untouched:
            assert (host[k].view(np.int32) == CR.SENTINEL).all(), '%s was written' % k
            continue
        v, guards = CR.split(host[k], n, nc, l)
        assert (guards == CR.SENTINEL).all(), '%s: %d guard words overwritten' % (k, int((guards != CR.SENTINEL).sum()))
        out[k] = torch.from_numpy(np.array(v))
    return out


def dflat_parts(v, case):
    Fh, Fin = case['W1'].shape
    f = v.reshape(-1)
    o1, o2 = Fh * Fin, Fh * Fin + Fh
    out = dict(dW1=f[:o1].reshape(Fh, Fin), db1=f[o1:o2], deps=f[-1:])
    if 'W2' in case:
        Fout = case['W2'].size(0)
        out.update(dW2=f[o2:o2 + Fout * Fh].reshape(Fout, Fh), db2=f[o2 + Fout * Fh:o2 + Fout * Fh + Fout])
    return out


@pytest.mark.parametrize('need_dx', [True, False])
@pytest.mark.parametrize('si,act,gname', MATRIX)
def test_abi_against_float64(dev, si, act, gname, need_dx):
    from gnn_matlang_amd import _lib
    case, ei, N, A, seed = R.layer_case(si, act, gname)
    what = 'ABI shape %s act=%s graph=%s seed=%d dx=%s' % (R.SHAPES[si], act, gname, seed, need_dx)
    assert_margin(case, A, act, what)
    ref64, ref32 = R.layer_ref((si, act, gname), case, A, act)
    rc, host, lay, tail = abi_run(dev, case, csr_of(gname, dev), act, need_dx=need_dx)
    assert rc == [_lib.GML_OK] * 2
    assert (tail.view(np.int32) == CR.SENTINEL).all(), 'the workspace tail was written'
    depth1 = 'W2' not in case
    v = abi_values(host, lay, untouched=(('t',) if depth1 else ()) + (() if need_dx else ('dx',)))
    for k in ('y', 'h') + (() if depth1 else ('t',)) + (('dx',) if need_dx else ()):
        check(v[k], ref64[k], ref32[k], k, what, computed=True)
    for k, g in dflat_parts(v['dflat'], case).items():
        if k == 'deps':
            check_eps(g, ref64, ref32, what)
        else:
            check(g, ref64[k], ref32[k], k, what, computed=True)


def test_abi_without_biases(dev):
    from gnn_matlang_amd import _lib
    case, ei, N, A, seed = R.layer_case(2, 'tanh', 'rand67')
    nb = dict(case, b1=torch.zeros_like(case['b1']), b2=torch.zeros_like(case['b2']))
    ref64, ref32 = R.layer_ref('nobias', nb, A, 'tanh')
    rc, host, lay, tail = abi_run(dev, case, csr_of('rand67', dev), 'tanh', bias=False)
    assert rc == [_lib.GML_OK] * 2
    v = abi_values(host, lay)
    for k in ('y', 'dx'):
        check(v[k], ref64[k], ref32[k], k, 'b1 = b2 = NULL', computed=True)


# ------------------------------------------------------------------------------------------------------------------ 2. refusals
@pytest.mark.parametrize('shape,depth', [((65, 64, 64, 2), None), ((64, 65, 64, 2), None), ((64, 64, 200, 2), None), ((8, 16, 16, 2), 3),
                                         ((65, 64, 0, 1), None)])
def test_unsupported_shapes_are_refused(dev, shape, depth):
    from gnn_matlang_amd import functional as Fn, _lib
    ei, N = R.get_graph('hand')
    case = R.draw_case(shape, N, 1)
    Fin, Fh, Fout, d = shape
    L = _lib.lib()
    assert not L.gml_gin_supported(Fin, Fh, Fout, depth or d)
    assert L.gml_gin_dflat_floats(Fin, Fh, Fout, depth or d) == 0 and L.gml_gin_bwd_workspace_bytes(N, Fin, Fh, Fout, depth or d) == 0
    rc, host, lay, tail = abi_run(dev, case, csr_of('hand', dev), None, depth=depth)
    assert rc == [_lib.GML_E_UNSUPPORTED] * 2
    for k in host:
        assert (host[k].view(np.int32) == CR.SENTINEL).all(), k       # nothing was launched
    if depth is None:
        assert not Fn.gin_conv_supported(case['x'].to(dev), Fh, Fout if d == 2 else None)
        # the module takes the composition and gives the restatement's result
        y = make_module(dev, case)(case['x'].to(dev), csr_of('hand', dev), act='tanh')
        c64 = {k: v.double() for k, v in case.items()}
        y64 = R.forward(c64['x'], R.adjacency(ei, N, torch.float64), c64['eps'], R.lins_of(c64), 'tanh')
        assert rel_err(y.detach().cpu().numpy(), y64.numpy()) <= 2e-5


def test_supported_agrees_with_the_library(dev, monkeypatch):
    from gnn_matlang_amd import functional as Fn, _lib
    L = _lib.lib()
    for Fin in (1, 3, 64, 65):
        x = torch.zeros(2, Fin, device=dev)
        for Fh in (1, 33, 64, 65, 200):
            assert Fn.gin_conv_supported(x, Fh) == bool(L.gml_gin_supported(Fin, Fh, 0, 1))
            for Fout in (1, 64, 65, 200):
                assert Fn.gin_conv_supported(x, Fh, Fout) == bool(L.gml_gin_supported(Fin, Fh, Fout, 2))
    assert Fn.gin_conv_supported(torch.zeros(2, 25, device=dev), 64, 64)
    assert not Fn.gin_conv_supported(torch.zeros(2, 25), 64, 64) and not Fn.gin_conv_supported(torch.zeros(0, 25, device=dev), 64, 64)
    assert not Fn.gin_conv_supported(torch.zeros(2, 25, device=dev, dtype=torch.float64), 64, 64)
    monkeypatch.setenv('GML_NO_GIN_FUSED', '1')
    assert not Fn.gin_conv_supported(torch.zeros(2, 25, device=dev), 64, 64)


def test_small_workspace_is_refused(dev):
    from gnn_matlang_amd import _lib
    case, ei, N, A, seed = R.layer_case(3, None, 'hand')
    rc, host, lay, tail = abi_run(dev, case, csr_of('hand', dev), None, ws_short=1)
    assert rc == [_lib.GML_OK, _lib.GML_E_WORKSPACE]
    for k in ('dx', 'dflat'):
        assert (host[k].view(np.int32) == CR.SENTINEL).all(), k


# ------------------------------------------------------------------------------------------------------------------ 3. order, edge cases
@pytest.mark.parametrize('si', [2, 4])
@pytest.mark.parametrize('act', R.ACTS)
def test_self_loop_only_and_isolated_rows(dev, si, act):
    """node 7 of the self-loop graph: its row holds only its own self loop, h = x + (1 + eps) x; node 8 (and node 5 of the hand-made
    graph, and the single node): no edge at all, h = (1 + eps) x.  Held to the layer tolerance against act(nn(.)) in float64."""
    for gname, rows, loops in (('loops', [7], 1), ('loops', [8], 0), ('hand', [5], 0), ('one', [0], 0)):
        case, ei, N, A, seed = R.layer_case(si, act, gname)
        y, _ = layer_gpu(dev, case, csr_of(gname, dev), act)
        c = {k: v.double() for k, v in case.items()}
        h = (loops + 1 + c['eps']) * c['x'][rows]
        want = R.forward(h, torch.zeros(len(rows), len(rows), dtype=torch.float64), torch.zeros(1, dtype=torch.float64), R.lins_of(c), act)
        assert rel_err(y[rows].cpu().numpy(), want.numpy()) <= TOL, (gname, rows)


def test_unsorted_source_rows(dev):
    """the same edges in shuffled order: GraphCSR's general construction (source keys not sorted), the same layer result"""
    from gnn_matlang_amd.graph import GraphCSR
    case, ei, N, A, seed = R.layer_case(3, 'relu', 'rand67')
    order = np.lexsort((ei[1], ei[0]))
    srt = ei[:, order]
    shuf = srt[:, np.random.default_rng(3).permutation(ei.shape[1])]
    assert (np.diff(shuf[0]) < 0).any() and (np.diff(srt[0]) >= 0).all()
    ref64, ref32 = R.layer_ref((3, 'relu', 'rand67'), case, A, 'relu')
    outs = []
    for e in (srt, shuf):
        csr = GraphCSR.from_edge_index(torch.from_numpy(np.ascontiguousarray(e)).to(dev), N)
        outs.append(layer_gpu(dev, case, csr, 'relu'))
        check_layer(outs[-1], ref64, ref32, 'unsorted' if e is shuf else 'sorted')
    assert not csr.src_sorted
    assert rel_err(outs[1][0].cpu().numpy(), outs[0][0].cpu().numpy()) <= 2e-6


def test_edge_index_and_no_bias_and_empty_edge_list(dev):
    from gnn_matlang_amd import GINConv
    g = torch.Generator().manual_seed(2)
    x = torch.randn(5, 4, generator=g).to(dev).requires_grad_(True)
    m = GINConv(torch.nn.Sequential(torch.nn.Linear(4, 8, bias=False)), eps=0.5, train_eps=True).to(dev)
    y = m(x, torch.zeros(2, 0, dtype=torch.int64, device=dev), act='relu')            # an edge_index, not a GraphCSR
    assert rel_err(y.detach().cpu().numpy(), torch.relu((1.5 * x) @ m.nn[0].weight.t()).detach().cpu().numpy()) <= TOL
    y.sum().backward()
    assert m.nn[0].bias is None and x.grad is not None and torch.isfinite(x.grad).all() and torch.isfinite(m.eps.grad).all()


def test_eps_as_a_buffer(dev):
    """train_eps=False: eps is a buffer; the fused road reads it from device memory all the same and returns no gradient for it"""
    from gnn_matlang_amd import GINConv
    case, ei, N, A, seed = R.layer_case(2, None, 'loops')
    m = GINConv(torch.nn.Sequential(torch.nn.Linear(3, 20), torch.nn.ReLU(), torch.nn.Linear(20, 36)), eps=float(case['eps'])).to(dev)
    with torch.no_grad():
        m.nn[0].weight.copy_(case['W1']); m.nn[0].bias.copy_(case['b1']); m.nn[2].weight.copy_(case['W2']); m.nn[2].bias.copy_(case['b2'])
    y = m(case['x'].to(dev), csr_of('loops', dev))
    y.backward(case['dy'].to(dev))
    ref64, ref32 = R.layer_ref((2, None, 'loops'), case, A, None)
    check(y.detach(), ref64['y'], ref32['y'], 'y', 'eps buffer', computed=True)
    assert not m.eps.requires_grad and m.eps.grad is None


# ------------------------------------------------------------------------------------------------------------------ 4. reproducibility, capture
def test_bit_reproducible(dev):
    case, ei, N, A, seed = R.layer_case(5, 'tanh', 'mutag16')          # 280 rows: nine partials of the row pass
    assert N > 4 * 32
    a = layer_gpu(dev, case, csr_of('mutag16', dev), 'tanh')
    b = layer_gpu(dev, case, csr_of('mutag16', dev), 'tanh')
    assert torch.equal(a[0], b[0]) and all(torch.equal(a[1][k], b[1][k]) for k in grad_keys(case))


def test_captured_layer_equals_eager(dev):
    """a captured forward + backward replayed after x, the weights, EPS and dy were overwritten in place equals the eager result bit
    for bit: eps is read from device memory by the kernels (passed by value, the replay would keep the captured one)"""
    from gnn_matlang_amd import functional as Fn
    c0 = R.layer_case(3, 'tanh', 'star')[0]
    c1 = R.draw_case(R.SHAPES[3], c0['x'].size(0), 77)
    assert abs(float(c1['eps']) - float(c0['eps'])) > 0.05
    csr = csr_of('star', dev)
    keys = ('x', 'eps', 'W1', 'b1', 'W2', 'b2')
    s = {k: c0[k].to(dev).requires_grad_(True) for k in keys}
    sdy = c0['dy'].to(dev)

    def step():
        y = Fn.GINConvFunction.apply(s['x'], csr, s['eps'], s['W1'], s['b1'], s['W2'], s['b2'], 'tanh')
        return (y,) + torch.autograd.grad(y, [s[k] for k in keys], sdy)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up outside the capture
        step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = step()
    with torch.no_grad():
        for k in keys:
            s[k].copy_(c1[k].to(dev))
        sdy.copy_(c1['dy'].to(dev))
    g.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in outs]
    y, gr = layer_gpu(dev, c1, csr, 'tanh')
    want = [y] + [gr[k] for k in grad_keys(c1)]
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    y0, _ = layer_gpu(dev, dict(c1, eps=c0['eps']), csr, 'tanh')
    assert not torch.equal(y0, y)                       # (the two eps give different bits: the comparison above can tell)


# ------------------------------------------------------------------------------------------------------------------ 5. models
def _rand_graphs(count, ninp, seed, y, nmin=5, nmax=14):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.integers(nmin, nmax + 1))
        A = np.triu(rng.random((n, n)) < 0.3, 1)
        A[np.arange(n - 1), np.arange(1, n)] = True       # connected
        A = A | A.T
        r, c = np.where(A)
        out.append(dict(x=rng.standard_normal((n, ninp)).astype(np.float32), edge_index=np.vstack((r, c)).astype(np.int64), y=y(rng, n)))
    return out


_BIN = lambda rng, n: np.float32(rng.integers(0, 2))
_REAL = lambda rng, n: np.float32(rng.standard_normal())


def model_case(name):
    """(graphs as dicts, ninp, loss kind, node fields)"""
    from gnn_matlang_amd import readers
    cls = lambda k: (lambda rng, n: np.int64(rng.integers(0, k)))
    if name == 'mutag_gin':
        gs = [dict(x=x, edge_index=ei, y=np.float32(y)) for x, ei, y in readers.load_mutag(os.path.join(RAW, 'mutag.mat'))[:16]]
        return gs, gs[0]['x'].shape[1], 'mutag', ()
    if name == 'filtering_gin':
        gs = _rand_graphs(3, 1, 5, _REAL, 20, 30)
        rng = np.random.default_rng(6)
        for g in gs:
            n = g['x'].shape[0]
            g['y'] = rng.standard_normal((n, 3)).astype(np.float32)
            g['mask'] = (rng.random((n, 1)) < 0.7).astype(np.float32)
        return gs, 1, 'filtering', ('y', 'mask')
    table = {'sr25_gin': (2, _REAL, None), 'graph8c_gin': (2, _REAL, None), 'exp_gin': (2, _REAL, None),
             'exp_classify_gin': (2, _BIN, 'bce'), 'zinc_gin': (25, _REAL, 'zinc'), 'counting_gin': (2, _REAL, 'counting'),
             'ptc_gin': (20, cls(2), 'tu'), 'enzymes_gin': (4, cls(6), 'tu'), 'proteins_gin': (4, cls(2), 'tu'),
             'enzymes_contfeat_gin': (22, cls(6), 'tu'), 'freqclass_gin': (1, _BIN, 'bce')}
    ninp, y, kind = table[name]
    return _rand_graphs(12, ninp, 7, y), ninp, kind, ()


def losses(kind, models, wsum):
    """(loss of the model on a device batch, the same loss of the float64 output)"""
    if kind is None:
        return (lambda m, b: (m(b) * wsum.to(b.x.device)).sum()), (lambda o, b: (o * wsum.double()).sum())
    if kind == 'zinc':
        return models.zinc_step_loss, (lambda o, b: models.zinc_loss(o, b.y.double()))
    if kind == 'mutag':
        return models.mutag_step_loss, (lambda o, b: models.mutag_loss(o, b.y.double()))
    if kind == 'counting':
        return (lambda m, b: models.counting_loss(m(b), b.y)), (lambda o, b: models.counting_loss(o, b.y.double()))
    if kind == 'bce':
        return models.exp_classify_step_loss, (lambda o, b: models.exp_classify_loss(o, b.y.double()))
    if kind == 'tu':
        return models.tu_step_loss, (lambda o, b: models.tu_loss(o, b.y))
    return models.filtering_step_loss, (lambda o, b: models.filtering_loss(o, b.y.double(), b.mask.double()))


@pytest.mark.parametrize('name', R.FACTORIES)
def test_models_against_float64(dev, name, monkeypatch):
    """output, loss and every parameter gradient within MODEL_TOL of the float64 GinNet.  An eps gradient that is tiny against its term
    sum (the rule at EPS_CANCEL) is held to TOL x that term sum, taken from the float64 restatement: behind a BatchNorm the signed sum
    cancels (mutag_gin: |deps| = 5e-3 of its term sum in all three layers), and the error of the upstream gradient -- the BatchNorm
    backward's, not this layer's -- is amplified by that factor: conv1.eps of mutag_gin came out 5.4e-4 off on the fused road and
    4.3e-4 on the torch-op composition (3e-6 of the term sum), 3.2e-5 and 1.4e-4 with torch's own BatchNorm."""
    from gnn_matlang_amd import collate, models, functional as Fn
    gs, ninp, kind, fields = model_case(name)
    cpu = collate(gs, node_fields=fields)
    b = cpu.to(dev)
    factory = getattr(models, name)
    kw = dict(dropout=0.0) if 'dropout' in inspect.signature(factory).parameters else {}      # (the masks are not part of the restatement)
    torch.manual_seed(11)
    np.random.seed(11)
    m = factory(ninp, **kw)
    with torch.no_grad():
        for n, v in m.named_parameters():                      # biases and BatchNorm parameters off their constant initial values
            if n.endswith('bias') or n.startswith('bn'):
                v.add_(0.1 * torch.randn(v.shape))
    p64 = {k: v.detach().double().clone().requires_grad_(True) for k, v in m.named_parameters()}
    taps = []
    out64 = R.ginnet_ref(p64, m, cpu.x, cpu.edge_index, cpu.ptr.tolist(), taps=taps)
    wsum = torch.randn(out64.shape, generator=torch.Generator().manual_seed(3))
    loss_dev, loss_ref = losses(kind, models, wsum)
    l64 = loss_ref(out64, cpu)
    l64.backward()
    m2 = factory(ninp, **kw)
    m2.load_state_dict(m.state_dict(), strict=True)
    m, m2 = m.to(dev).train(), m2.to(dev).train()
    monkeypatch.setattr(Fn, 'VERBOSE', True)
    monkeypatch.setattr(Fn, 'PATHS', {})
    out = m2(b)
    l = loss_dev(m, b)
    l.backward()
    roads = {k: v for k, v in Fn.PATHS.items() if k.startswith('gin:')}
    if name in R.WIDE:                                         # 200 wide: both layers of both forwards on the composition
        assert sum(roads.values()) == 2 * m.nlayers and all('torch ops (outside the fused layer)' in k for k in roads), roads
    else:
        assert not roads, roads
    e = {'out': rel_err(out.detach().cpu().numpy(), out64.detach().numpy()), 'loss': abs(float(l.detach()) - float(l64.detach())) / abs(float(l64.detach()))}
    neps = 0
    for k, v in m.named_parameters():
        assert p64[k].grad is not None and v.grad is not None, k
        err = rel_err(v.grad.cpu().numpy(), p64[k].grad.numpy())
        if k.endswith('.eps'):
            xin, h = taps[int(k[4:-4]) - 1]
            d64, t = float(p64[k].grad), float((h.grad.abs() * xin.abs()).sum())
            print('%s %s: float64 %.4e, term sum %.4e (ratio %.1e), rel err %.2e, err / term sum %.2e' % (name, k, d64, t, abs(d64) / t, err, err * abs(d64) / t))
            neps += 1
            if abs(d64) < EPS_CANCEL * t:                      # tiny against its terms: held to the term sum (the rule at EPS_CANCEL)
                assert err * abs(d64) <= TOL * t, (k, err, d64, t)
                continue
        e[k] = err
    print(name, {k: '%.2e' % v for k, v in e.items()})
    assert float(out64.detach().abs().max()) > 0 and neps == m.nlayers
    assert max(e.values()) <= MODEL_TOL, e


def test_fused_road_and_composition_agree(dev):
    from gnn_matlang_amd import collate, models
    gs, ninp, _, _ = model_case('zinc_gin')
    b = collate(gs).to(dev)
    torch.manual_seed(5)
    m = models.zinc_gin(ninp).to(dev)
    grads = []
    for road in (None, 'torch'):
        m.zero_grad()
        out = m(b, _road=road)
        models.zinc_loss(out, b.y).backward()
        grads.append((out.detach(), {k: v.grad.clone() for k, v in m.named_parameters()}))
    assert rel_err(grads[0][0].cpu().numpy(), grads[1][0].cpu().numpy()) <= MODEL_TOL
    for k in grads[0][1]:
        assert rel_err(grads[0][1][k].cpu().numpy(), grads[1][1][k].cpu().numpy()) <= MODEL_TOL, k


def test_padded_static_batch_equals_the_plain_batch(dev):
    """padded static batches work.  A padding node carries only self loops, which count like any edge, so it reaches itself alone; the
    pool skips the padding graph and the bnI get the row validity.  Same graphs plain and padded (absent slots included): logits of
    the real graphs, the masked loss and every parameter gradient."""
    from gnn_matlang_amd import SpectralDesign, models, readers
    from gnn_matlang_amd.dataset import DeviceDataset
    raw = readers.load_mutag(os.path.join(RAW, 'mutag.mat'))[:20]
    dd = DeviceDataset.from_graphs(SpectralDesign(recfield=1, dv=4, nfreq=3, adddegree=True).design_many(raw), dev)
    dd.y = dd.y.float()
    G = len(dd)
    torch.manual_seed(3)
    mp = models.mutag_gin(int(dd.x.size(1))).to(dev).train()
    ms = copy.deepcopy(mp)
    sl = [11, 0, G, 7, 3, G, 14, 2, 9, 1, 5, G, 12, 4, 8, 6]
    ids = torch.tensor(sl, device=dev)
    real = torch.tensor([i for i in sl if i < G], device=dev)
    keep = torch.tensor([k for k, i in enumerate(sl) if i < G], device=dev)
    bs = dd.batch_padded(ids, dd.bounds(16), adjacency=True)
    bpl = dd.batch(real)
    lp, ls = models.mutag_step_loss(mp, bpl), models.mutag_step_loss(ms, bs)
    with torch.no_grad():
        pre_p, pre_s = mp(bpl), ms(bs)
    assert rel_err(pre_s[keep].cpu().numpy(), pre_p.cpu().numpy()) <= 2e-5
    assert abs(ls.item() - lp.item()) <= 2e-5 * abs(lp.item())
    lp.backward()
    ls.backward()
    sp = dict(ms.named_parameters())
    for n, p in mp.named_parameters():
        err = rel_err(sp[n].grad.cpu().numpy(), p.grad.cpu().numpy())
        assert err <= 2e-5, (n, err)


# ------------------------------------------------------------------------------------------------------------------ 6. expressivity
def _seeded(factory, ninp, seeds):
    """the factory count_similar calls after torch.manual_seed(s): the scripts' eps come from numpy's generator, seeded alongside"""
    it = iter(seeds)

    def make():
        np.random.seed(next(it))
        return factory(ninp)
    return make


def _float64_embeddings(factory, ninp, seeds, gs):
    x = np.concatenate([g['x'] for g in gs])
    off = np.cumsum([0] + [g['x'].shape[0] for g in gs])
    ei = np.concatenate([np.asarray(g['edge_index'], np.int64) + off[i] for i, g in enumerate(gs)], 1)
    batch = np.repeat(np.arange(len(gs)), [g['x'].shape[0] for g in gs])
    out = []
    for s in seeds:
        torch.manual_seed(s)
        np.random.seed(s)
        m = factory(ninp)
        p = {k: v.detach().double() for k, v in m.state_dict().items()}
        with torch.no_grad():
            out.append(R.embed_sparse(p, m, x, ei, batch, len(gs)).numpy())
    return out


def _as_dicts(raw):
    return [dict(x=x, edge_index=ei, y=y) for x, ei, y in raw]


def test_sr25_pairs_stay_similar(dev):
    """sr25.py:281-300 with GinNet: a 1-WL bounded model on regular graphs with constant features gives every node the same row, so
    all 105 pairs stay similar for every seed -- in float64 with no pair near the tolerance, and on the device"""
    from gnn_matlang_amd import collate, expressivity, models, readers
    gs = _as_dicts(readers.load_sr(os.path.join(RAW, 'sr251256.g6')))
    ninp, seeds, tol = gs[0]['x'].shape[1], [0, 1, 2], 1e-3
    iu = np.triu_indices(len(gs), 1)
    assert iu[0].size == 105
    for E in _float64_embeddings(models.sr25_gin, ninp, seeds, gs):
        assert np.abs(E).max() > 0.1 and np.abs(E[iu[0]] - E[iu[1]]).sum(1).max() < tol / 2
    b = collate(gs).to(dev)
    assert expressivity.count_similar(_seeded(models.sr25_gin, ninp, seeds), b, seeds=seeds) == [105, 105, 105]
    torch.manual_seed(0)
    np.random.seed(0)
    m = models.sr25_gin(ninp).to(dev).eval()
    with torch.no_grad():
        rows = m(b, _features=True)                       # pooled; the node rows of one graph: through the first layer's module
        x1 = m.conv1(b.x, b.csr('edge_index'), act='tanh')
    assert float((x1 - x1[0]).abs().max()) <= 1e-6 and rows.shape == (15, 64)


def test_exp_pairs_stay_similar(dev):
    """exp_iso.py:284-304 with GinNet: 600 of 600 pairs stay similar for seeds 0-2 (float64: tests/test_gin_cpu.py, largest pair
    distance 8e-15 against the tolerance 1e-3, so no pair hangs on the tolerance)"""
    from gnn_matlang_amd import collate, expressivity, models, readers
    gs = _as_dicts(readers.load_exp(os.path.join(RAW, 'exp.npz')))
    seeds = [0, 1, 2]
    b = collate(gs).to(dev)
    got = expressivity.count_similar(_seeded(models.exp_gin, gs[0]['x'].shape[1], seeds), b, seeds=seeds, pairs=expressivity.exp_pairs(1200))
    assert got == [600, 600, 600]


def test_graph8c_decisions_equal_float64(dev):
    """the discriminating case (a constant output cannot pass): graphs [1000:1500] of graph8c, graph8c_gin(ninp=1), seeds 0-2.  Every
    pair whose float64 distance (maximum over the seeds) is above 2 tol must be separated on the device, every pair below tol / 2 must
    stay similar; pairs in between are left out, and they must be at most 0.1 % of the 124,750 pairs."""
    from gnn_matlang_amd import collate, expressivity, models, readers
    gs = _as_dicts(readers.load_graph8c(os.path.join(RAW, 'graph8c.g6'))[1000:1500])
    seeds, tol = [0, 1, 2], 1e-3
    iu = np.triu_indices(len(gs), 1)
    assert iu[0].size == 124750
    dmax = np.zeros(iu[0].size)
    for E in _float64_embeddings(models.graph8c_gin, 1, seeds, gs):
        dmax = np.maximum(dmax, np.abs(E[iu[0]] - E[iu[1]]).sum(1))
    must_sep, must_sim = dmax > 2 * tol, dmax < tol / 2
    band = ~(must_sep | must_sim)
    b = collate(gs).to(dev)
    tr = expressivity.PairTracker(len(gs), tol=tol, device=dev)
    counts = expressivity.count_similar(_seeded(models.graph8c_gin, 1, seeds), b, seeds=seeds, tracker=tr)
    sim = np.zeros((len(gs), len(gs)), dtype=bool)
    sp = tr.similar_pairs().cpu().numpy().reshape(-1, 2)
    sim[sp[:, 0], sp[:, 1]] = True
    got_sim = sim[iu[0], iu[1]]
    print('graph8c[1000:1500]: float64 separates %d, never separates %d, left out %d (%.3f %%); device counts %s'
          % (int(must_sep.sum()), int(must_sim.sum()), int(band.sum()), 100.0 * band.sum() / band.size, counts))
    assert band.sum() <= 0.001 * band.size
    assert must_sep.sum() > 100000 and must_sim.sum() > 0
    assert not got_sim[must_sep].any(), '%d pairs the float64 model separates stayed similar' % int(got_sim[must_sep].sum())
    assert got_sim[must_sim].all(), '%d pairs the float64 model cannot separate were separated' % int((~got_sim[must_sim]).sum())
    assert counts[-1] == int(got_sim.sum())


# ------------------------------------------------------------------------------------------------------------------ 7. many tiles
MAXWG = 768              # the workgroups of a tile-walking launch and of a row pass (csrc/gml_rowtile64.h)
COPIES = 367             # of rand67: 24,589 rows = 769 tiles of 32 rows, the fewest copies with more than MAXWG tiles


def many_tiles_case(si, act):
    """(case, edge_index, N) of rand67 as COPIES block-diagonal copies: x repeated per copy, the weights of the small case, dy fresh
    for every row; the kink margin is asserted on the small case, whose pre-activations are the only values the big one takes"""
    case, ei, N, A, seed = R.layer_case(si, act, 'rand67')
    assert_margin(case, A, act, 'many tiles: the small case, seed %d' % seed)
    big = dict(case, x=case['x'].repeat(COPIES, 1))
    big['dy'] = torch.randn(COPIES * N, case['dy'].size(1), generator=torch.Generator().manual_seed(seed + 1))
    eib = (ei[:, None, :] + N * np.arange(COPIES, dtype=np.int64)[None, :, None]).reshape(2, -1)
    return big, eib, COPIES * N


@pytest.mark.parametrize('need_dx', [True, False])
def test_many_tiles(dev, need_dx):
    """769 tiles: the forward's workgroups make a second trip of their tile loop, the row pass gets two tiles per workgroup and a last
    workgroup that owns one.  Reference: backward() / forward() of tests/_gin_ref.py, the float64 restatement and its float32 twin, fed
    a SPARSE adjacency (torch.sparse_coo_tensor, coalesced: repeats summed, self loops kept) in place of the dense [N, N] one."""
    from gnn_matlang_amd import _lib
    from gnn_matlang_amd.graph import GraphCSR
    si, act = 2, 'relu'
    assert R.SHAPES[si] == (3, 20, 36, 2)
    big, eib, N = many_tiles_case(si, act)
    Fin, Fh, Fout, depth = R.SHAPES[si]
    tiles = -(-N // 32)
    L = _lib.lib()
    P = int(L.gml_gin_dflat_floats(Fin, Fh, Fout, depth))
    nwg, rest = divmod(int(L.gml_gin_bwd_workspace_bytes(N, Fin, Fh, Fout, depth)) // 4 - N * Fin, P)
    tpw = -(-tiles // nwg)
    print('many tiles: N %d, tiles %d, row-pass workgroups %d of %d tiles (the last: %d)' % (N, tiles, nwg, tpw, tiles - (nwg - 1) * tpw))
    assert N == 24589 and tiles == MAXWG + 1                   # the forward: a second trip for workgroup 0 alone
    assert rest == 0 and 1 < nwg < tiles and tpw == 2 and tiles - (nwg - 1) * tpw == 1
    t = torch.from_numpy(eib)
    A = torch.sparse_coo_tensor(torch.stack([t[1], t[0]]), torch.ones(t.size(1), dtype=torch.float64), (N, N)).coalesce()
    ref64, ref32 = R.layer_ref('many tiles', big, A, act)
    csr = GraphCSR.from_edge_index(t.to(dev), N)
    check_layer(layer_gpu(dev, big, csr, act, need_dx), ref64, ref32, 'many tiles dx=%s' % need_dx, need_dx)
