"""ChebNet on the MI355X (csrc/gml_cheb.hip, functional.ChebConvFunction, cheb.ChebConv, models.Cheb): the layer against the float64
restatement of tests/_cheb_ref.py over the shape / activation / graph matrix -- through the module and through the raw ABI with
sentinel-framed, odd-stride buffers --, the refusals, the edge cases, reproducibility and capture (the norm launch and lambda_max
included), every fused-range factory against the float64 ChebNet restatement, the two roads, the padded static batch with lmax carried
and the expressivity decisions."""
import copy
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import _cheb_ref as R
import _conv_ref as CR
from _gnnml1_ref import TOL, check
from conftest import GOLDEN, rel_err

pytestmark = pytest.mark.gpu

RAW = os.path.join(GOLDEN, 'raw')
MODEL_TOL = 1e-4


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


_CSR = {}


def csr_of(gname, dev):
    from gnn_matlang_amd.graph import GraphCSR
    if gname not in _CSR:
        ei, N, _, _ = R.get_graph(gname)
        _CSR[gname] = GraphCSR.from_edge_index(torch.from_numpy(ei).to(dev), N)
    return _CSR[gname]


def lam_dev(gr, dev):
    """(batch, lambda_max) as the module takes them: the device copies, or (None, None) for the lambda_max=None graph"""
    _, _, batch, lam = gr
    return (None, None) if lam is None else (batch.to(dev), lam.float().to(dev))


def make_module(dev, case, bias=True):
    from gnn_matlang_amd import ChebConv
    K, Fin, Fout = case['W'].shape
    m = ChebConv(Fin, Fout, K, bias=bias).to(dev)
    with torch.no_grad():
        m.weight.copy_(case['W'])
        if bias:
            m.bias.copy_(case['b'])
    return m


def layer_gpu(dev, case, gr, graph, act, need_dx=True, bias=True):
    """the module on the fused road: (y, {dx, dW, db})"""
    from gnn_matlang_amd import functional as Fn
    m = make_module(dev, case, bias)
    x = case['x'].to(dev).requires_grad_(need_dx)
    assert Fn.cheb_conv_supported(x, case['W'].size(2), case['W'].size(0))
    batch, lam = lam_dev(gr, dev)
    y = m(x, graph, batch=batch, lambda_max=lam, act=act)
    y.backward(case['dy'].to(dev))
    return y.detach(), dict(dx=x.grad, dW=m.weight.grad, db=m.bias.grad if bias else None)


def check_layer(got, ref64, ref32, what, need_dx=True):
    y, g = got
    check(y, ref64['y'], ref32['y'], 'y', what, computed=True)
    assert (g['dx'] is None) == (not need_dx)                  # need_dx=False: dx is None, not a tensor of zeros
    for k in ('dx', 'dW', 'db'):
        if g[k] is not None:
            check(g[k], ref64[k], ref32[k], k, what, computed=True)


def assert_margin(case, L, act, what):
    """kinks: asserted on the float64 restatement before any result is compared; no element is excluded"""
    m = R.margin(case, L, act)
    assert m >= R.MARGIN, '%s: kink margin %.2e below %.0e' % (what, m, R.MARGIN)


# ------------------------------------------------------------------------------------------------------------------ 1. layer matrix
MATRIX = [(si, act, g) for si in range(len(R.SHAPES)) for act in R.ACTS for g in sorted(R.GRAPHS)]


@pytest.mark.parametrize('need_dx', [True, False])
@pytest.mark.parametrize('si,act,gname', MATRIX)
def test_module_against_float64(dev, si, act, gname, need_dx):
    case, gr, L, seed = R.layer_case(si, act, gname)
    what = 'shape %s act=%s graph=%s seed=%d dx=%s' % (R.SHAPES[si], act, gname, seed, need_dx)
    assert_margin(case, L, act, what)
    ref64, ref32 = R.layer_ref((si, act, gname), case, gr, act)
    check_layer(layer_gpu(dev, case, gr, csr_of(gname, dev), act, need_dx), ref64, ref32, what, need_dx)


def _dev_buf(buf, dev):
    return torch.from_numpy(buf).to(dev)


def _at(t, off):
    return ctypes.c_void_p(t.data_ptr() + 4 * int(off))


def abi_run(dev, case, gr, csr, act, K=None, need_dx=True, ws_short=0, bias=True, widths=None):
    """gml_cheb_norm / _fwd / _bwd on sentinel-framed buffers with padded, odd leading dimensions (ldx = Fin + 3, ...); the shape is the
    case's own (K, widths: overrides for the refusal tests).  Returns the return codes, the host copies of every buffer, their layouts
    and the workspace tail."""
    from gnn_matlang_amd import _lib
    from gnn_matlang_amd.graph import _ptr, _stream
    L = _lib.lib()
    N, Fin = case['x'].shape
    Kc, _, Fout = case['W'].shape
    K = Kc if K is None else K
    if widths is not None:
        Fin, Fout = widths
    E = csr.E
    ldx, lddy = case['x'].size(1) + 3, case['W'].size(2) + 1
    x = torch.zeros(N, ldx, device=dev)
    x[:, :case['x'].size(1)] = case['x'].to(dev)
    dy = torch.zeros(N, lddy, device=dev)
    dy[:, :case['W'].size(2)] = case['dy'].to(dev)
    w = case['W'].to(dev).contiguous()
    b = case['b'].to(dev).contiguous() if bias else None
    _, _, batch, lam = gr
    bt = None if lam is None else batch.to(dev).to(torch.int32)
    lm = None if lam is None else lam.float().to(dev)
    KT = max(Kc - 1, 0) * case['x'].size(1)
    P = Kc * case['x'].size(1) * case['W'].size(2) + case['W'].size(2)
    lay = dict(norm=(N, 2, 2), T=(N, KT, KT + 1), y=(N, case['W'].size(2), case['W'].size(2) + 3),
               dx=(N, case['x'].size(1), case['x'].size(1) + 5), dflat=(1, P, P))
    bufs, offs = {}, {}
    for k, (n, nc, l) in lay.items():
        hb, offs[k] = CR.alloc(n, nc, l, head=k in ('y', 'dx', 'norm'))
        bufs[k] = _dev_buf(hb, dev)
    nws = int(L.gml_cheb_bwd_workspace_bytes(N, Fin, Fout, K)) // 4
    assert nws == 0 or P == int(L.gml_cheb_dflat_floats(Fin, Fout, K))
    wsn = max(nws, 4) if nws else 4096
    hb, _ = CR.alloc(1, wsn, wsn + 64, guard_rows=0)
    ws = _dev_buf(hb, dev)
    st = _stream(dev)
    p = lambda k: _at(bufs[k], offs[k])
    a = R.ACTS.index(act)
    rc = [L.gml_cheb_norm(_ptr(csr.rowptr_t), _ptr(csr.col_t), _ptr(bt), _ptr(lm), 0 if lm is None else lm.numel(), 2.0, N, E, p('norm'), st)]
    rc.append(L.gml_cheb_fwd(_ptr(csr.rowptr), _ptr(csr.col), p('norm'), _ptr(x), ldx, N, E, Fin, _ptr(w), _ptr(b), Fout, K, a, p('T'),
                             lay['T'][2], p('y'), lay['y'][2], st))
    rc.append(L.gml_cheb_bwd(_ptr(csr.rowptr_t), _ptr(csr.col_t), p('norm'), _ptr(x), ldx, p('T'), lay['T'][2], p('y'), lay['y'][2],
                             _ptr(dy), lddy, N, E, Fin, _ptr(w), Fout, K, a, p('dx') if need_dx else None, lay['dx'][2], p('dflat'),
                             _ptr(ws), (wsn - ws_short) * 4, st))
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


def norm_ref(gr):
    ei, N, batch, lam = gr
    A = R.adjacency(ei, N, torch.float64)
    deg = A.sum(0)
    dis = torch.where(deg > 0, deg.clamp(min=1).pow(-0.5), torch.zeros_like(deg))
    s = torch.ones(N, dtype=torch.float64) if lam is None else 2.0 / lam[batch]
    return torch.stack([dis, s], 1)


@pytest.mark.parametrize('need_dx', [True, False])
@pytest.mark.parametrize('si,act,gname', MATRIX)
def test_abi_against_float64(dev, si, act, gname, need_dx):
    from gnn_matlang_amd import _lib
    case, gr, L, seed = R.layer_case(si, act, gname)
    what = 'ABI shape %s act=%s graph=%s seed=%d dx=%s' % (R.SHAPES[si], act, gname, seed, need_dx)
    assert_margin(case, L, act, what)
    ref64, ref32 = R.layer_ref((si, act, gname), case, gr, act)
    rc, host, lay, tail = abi_run(dev, case, gr, csr_of(gname, dev), act, need_dx=need_dx)
    assert rc == [_lib.GML_OK] * 3
    assert (tail.view(np.int32) == CR.SENTINEL).all(), 'the workspace tail was written'
    K1 = case['W'].size(0) == 1
    v = abi_values(host, lay, untouched=(('T',) if K1 else ()) + (() if need_dx else ('dx',)))
    nr = norm_ref(gr)
    check(v['norm'], nr, nr.float(), 'norm', what, computed=True)
    for k in ('y',) + (() if K1 else ('T',)) + (('dx',) if need_dx else ()):
        check(v[k], ref64[k], ref32[k], k, what, computed=True)
    f = v['dflat'].reshape(-1)
    nw = case['W'].numel()
    check(f[:nw].reshape(case['W'].shape), ref64['dW'], ref32['dW'], 'dW', what, computed=True)
    check(f[nw:], ref64['db'], ref32['db'], 'db', what, computed=True)


# ------------------------------------------------------------------------------------------------------------------ 2. refusals
@pytest.mark.parametrize('K,widths', [(9, None), (0, None), (None, (65, 8)), (None, (8, 65))])
def test_unsupported_shapes_are_refused(dev, K, widths):
    """K = 9, K = 0, a width of 65: GML_E_UNSUPPORTED from the forward and the backward, nothing written (the buffers hold a supported
    shape: the refusal comes before any pointer is read)"""
    from gnn_matlang_amd import _lib
    gr = R.get_graph('hand')
    case = R.draw_case((8, 8, 3), gr[1], 1)
    L = _lib.lib()
    Fin, Fout = widths or (8, 8)
    Kk = 3 if K is None else K
    assert not L.gml_cheb_supported(Fin, Fout, Kk)
    assert L.gml_cheb_dflat_floats(Fin, Fout, Kk) == 0 and L.gml_cheb_bwd_workspace_bytes(gr[1], Fin, Fout, Kk) == 0
    rc, host, lay, tail = abi_run(dev, case, gr, csr_of('hand', dev), None, K=K, widths=widths)
    assert rc == [_lib.GML_OK, _lib.GML_E_UNSUPPORTED, _lib.GML_E_UNSUPPORTED]
    for k in host:
        if k != 'norm':
            assert (host[k].view(np.int32) == CR.SENTINEL).all(), k      # nothing was launched


def test_wide_module_takes_the_composition(dev):
    from gnn_matlang_amd import functional as Fn
    gr = R.get_graph('rand67')
    for shape in ((65, 8, 3), (8, 65, 3), (8, 8, 9)):
        case = R.draw_case(shape, gr[1], 2)
        x = case['x'].to(dev)
        assert not Fn.cheb_conv_supported(x, shape[1], shape[2])
        batch, lam = lam_dev(gr, dev)
        y = make_module(dev, case)(x, csr_of('rand67', dev), batch=batch, lambda_max=lam, act='tanh')
        c64 = {k: v.double() for k, v in case.items()}
        y64 = R.forward(c64['x'], R.laplacian(*gr, torch.float64), c64['W'], c64['b'], 'tanh')
        assert rel_err(y.detach().cpu().numpy(), y64.numpy()) <= 2e-5


def test_supported_agrees_with_the_library(dev, monkeypatch):
    from gnn_matlang_amd import functional as Fn, _lib
    L = _lib.lib()
    for Fin in (1, 3, 64, 65):
        x = torch.zeros(2, Fin, device=dev)
        for Fout in (1, 33, 64, 65, 200):
            for K in (0, 1, 2, 8, 9):
                assert Fn.cheb_conv_supported(x, Fout, K) == bool(L.gml_cheb_supported(Fin, Fout, K))
                assert Fn.cheb_conv_supported(torch.zeros(2, 7, device=dev), Fout, K, Fin=Fin) == bool(L.gml_cheb_supported(Fin, Fout, K))
    assert Fn.cheb_conv_supported(torch.zeros(2, 25, device=dev), 64, 2)
    assert not Fn.cheb_conv_supported(torch.zeros(2, 25), 64, 2) and not Fn.cheb_conv_supported(torch.zeros(0, 25, device=dev), 64, 2)
    assert not Fn.cheb_conv_supported(torch.zeros(2, 25, device=dev, dtype=torch.float64), 64, 2)
    monkeypatch.setenv('GML_NO_CHEB_FUSED', '1')
    assert not Fn.cheb_conv_supported(torch.zeros(2, 25, device=dev), 64, 2)


@pytest.mark.parametrize('si', [0, 4])
def test_small_workspace_is_refused(dev, si):
    from gnn_matlang_amd import _lib
    case, gr, L, seed = R.layer_case(si, None, 'hand')
    rc, host, lay, tail = abi_run(dev, case, gr, csr_of('hand', dev), None, ws_short=1)
    assert rc == [_lib.GML_OK, _lib.GML_OK, _lib.GML_E_WORKSPACE]
    for k in ('dx', 'dflat'):
        assert (host[k].view(np.int32) == CR.SENTINEL).all(), k


# ------------------------------------------------------------------------------------------------------------------ 3. edge cases
@pytest.mark.parametrize('si', [2, 6])
@pytest.mark.parametrize('act', R.ACTS)
def test_self_loop_only_and_isolated_rows(dev, si, act):
    """node 7 of the self-loop graph: its row holds only its own self loop, which is dropped; node 8, node 5 of the hand-made graph and
    the single node have no edge at all.  Such a row sees L^ = s - 1 alone: Tx_k = T_k(s - 1) x with the Chebyshev polynomials T_k."""
    for gname, row in (('loops', 7), ('loops', 8), ('hand', 5), ('one', 0)):
        case, gr, L, seed = R.layer_case(si, act, gname)
        y, _ = layer_gpu(dev, case, gr, csr_of(gname, dev), act)
        c = {k: v.double() for k, v in case.items()}
        lam = gr[3]
        t = (1.0 if lam is None else 2.0 / float(lam[gr[2][row]])) - 1.0
        poly = [1.0, t]
        for _ in range(2, c['W'].size(0)):
            poly.append(2 * t * poly[-1] - poly[-2])
        want = R.act_fn(sum(poly[k] * (c['x'][row:row + 1] @ c['W'][k]) for k in range(c['W'].size(0))) + c['b'], act)
        assert rel_err(y[row:row + 1].cpu().numpy(), want.numpy()) <= TOL, (gname, row)


def test_unsorted_source_rows(dev):
    """the same edges in shuffled order: GraphCSR's general construction (source keys not sorted), the same layer result"""
    from gnn_matlang_amd.graph import GraphCSR
    case, gr, L, seed = R.layer_case(4, 'relu', 'rand67')
    ei, N = gr[0], gr[1]
    order = np.lexsort((ei[1], ei[0]))
    srt = ei[:, order]
    shuf = srt[:, np.random.default_rng(3).permutation(ei.shape[1])]
    assert (np.diff(shuf[0]) < 0).any() and (np.diff(srt[0]) >= 0).all()
    ref64, ref32 = R.layer_ref((4, 'relu', 'rand67'), case, gr, 'relu')
    outs = []
    for e in (srt, shuf):
        csr = GraphCSR.from_edge_index(torch.from_numpy(np.ascontiguousarray(e)).to(dev), N)
        outs.append(layer_gpu(dev, case, gr, csr, 'relu'))
        check_layer(outs[-1], ref64, ref32, 'unsorted' if e is shuf else 'sorted')
    assert not csr.src_sorted
    assert rel_err(outs[1][0].cpu().numpy(), outs[0][0].cpu().numpy()) <= 2e-6


def test_edge_index_instead_of_a_csr_and_no_bias(dev):
    case, gr, L, seed = R.layer_case(2, 'tanh', 'rand67')
    ref64, ref32 = R.layer_ref('nobias', case, gr, 'tanh', bias=False)
    ei = torch.from_numpy(gr[0]).to(dev)
    assert ei.dtype == torch.int64
    y, g = layer_gpu(dev, case, gr, ei, 'tanh', bias=False)
    assert g['db'] is None
    check_layer((y, g), ref64, ref32, 'int64 edge_index, bias=None')


def test_empty_edge_list(dev):
    from gnn_matlang_amd import ChebConv
    g = torch.Generator().manual_seed(2)
    x = torch.randn(5, 4, generator=g).to(dev).requires_grad_(True)
    m = ChebConv(4, 8, 3).to(dev)
    lam = torch.tensor([1.5], device=dev)
    y = m(x, torch.zeros(2, 0, dtype=torch.int64, device=dev), batch=torch.zeros(5, dtype=torch.int64, device=dev), lambda_max=lam, act='relu')
    t = 2 / 1.5 - 1
    xd, W = x.detach().double().cpu(), m.weight.detach().double().cpu()
    want = torch.relu(xd @ W[0] + t * (xd @ W[1]) + (2 * t * t - 1) * (xd @ W[2]) + m.bias.detach().double().cpu())
    assert rel_err(y.detach().cpu().numpy(), want.numpy()) <= TOL
    y.sum().backward()
    assert torch.isfinite(x.grad).all() and torch.isfinite(m.weight.grad).all()


# ------------------------------------------------------------------------------------------------------------------ 4. reproducibility, capture
def test_bit_reproducible(dev):
    case, gr, L, seed = R.layer_case(7, 'tanh', 'mutag16')             # 279 rows: nine partials of the row pass, K = 8
    assert gr[1] > 4 * 32
    a = layer_gpu(dev, case, gr, csr_of('mutag16', dev), 'tanh')
    b = layer_gpu(dev, case, gr, csr_of('mutag16', dev), 'tanh')
    assert torch.equal(a[0], b[0]) and all(torch.equal(a[1][k], b[1][k]) for k in ('dx', 'dW', 'db'))


def test_captured_layer_equals_eager(dev):
    """a captured norm + forward + backward replayed after x, the weights, dy AND lambda_max were overwritten in place equals the eager
    result bit for bit: the norm launch is inside the capture and reads lambda_max from device memory"""
    from gnn_matlang_amd import functional as Fn
    c0, gr, _, _ = R.layer_case(4, 'tanh', 'mutag16')
    c1 = R.draw_case(R.SHAPES[4], c0['x'].size(0), 77)
    csr = csr_of('mutag16', dev)
    batch = gr[2].to(dev)
    lam0 = gr[3].float().to(dev)
    lam1 = (gr[3].float() * torch.linspace(0.8, 1.1, gr[3].numel())).to(dev)
    keys = ('x', 'W', 'b')
    s = {k: c0[k].to(dev).requires_grad_(True) for k in keys}
    sdy, slam = c0['dy'].to(dev), lam0.clone()

    def step(lam):
        norm = Fn.cheb_norm(csr, batch, lam)
        y = Fn.ChebConvFunction.apply(s['x'], csr, norm, s['W'], s['b'], 'tanh')
        return (y,) + torch.autograd.grad(y, [s[k] for k in keys], sdy)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up outside the capture
        step(slam)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = step(slam)
    g.replay()
    torch.cuda.synchronize()
    eager0 = step(lam0)
    assert all(torch.equal(a, b) for a, b in zip(outs, eager0))
    first = outs[0].clone()
    with torch.no_grad():
        for k in keys:
            s[k].copy_(c1[k].to(dev))
        sdy.copy_(c1['dy'].to(dev))
        slam.copy_(lam1)
    g.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in outs]
    want = step(lam1)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert not torch.equal(step(lam0)[0], want[0]) and not torch.equal(first, got[0])      # (lambda_max changes the bits: the test can tell)


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
    for g, l in zip(out, R.graph_lambdas(out)):
        g['lmax'] = l
    return out


_BIN = lambda rng, n: np.float32(rng.integers(0, 2))
_REAL = lambda rng, n: np.float32(rng.standard_normal())
FUSED = [n for n in R.FACTORIES if n not in R.WIDE]


def model_case(name):
    """(graphs as dicts with lmax, ninp, loss kind, node fields)"""
    cls = lambda k: (lambda rng, n: np.int64(rng.integers(0, k)))
    if name == 'filtering_cheb':
        gs = _rand_graphs(3, 1, 5, _REAL, 20, 30)
        rng = np.random.default_rng(6)
        for g in gs:
            n = g['x'].shape[0]
            g['y'] = rng.standard_normal((n, 3)).astype(np.float32)
            g['mask'] = (rng.random((n, 1)) < 0.7).astype(np.float32)
        return gs, 1, 'filtering', ('y', 'mask')
    table = {'sr25_cheb': (2, _REAL, None), 'graph8c_cheb': (2, _REAL, None), 'exp_cheb': (2, _REAL, None),
             'exp_classify_cheb': (2, _BIN, 'bce'), 'zinc_cheb': (25, _REAL, 'zinc'), 'counting_cheb': (2, _REAL, 'counting'),
             'mutag_cheb': (8, _BIN, 'mutag'), 'freqclass_cheb': (1, _BIN, 'bce'), 'mnist75_cheb': (3, cls(10), 'tu'),
             'enzymes_cheb': (4, cls(6), 'tu'), 'ptc_cheb': (20, cls(2), 'tu'), 'proteins_cheb': (4, cls(2), 'tu'),
             'enzymes_contfeat_cheb': (22, cls(6), 'tu')}
    ninp, y, kind = table[name]
    return _rand_graphs(8, ninp, 7, y), ninp, kind, ()


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
    """output, loss and every parameter gradient within MODEL_TOL of the float64 ChebNet on 8 random graphs of 5-14 nodes (filtering:
    3 of 20-30) with each graph's own lambda_max; the fused-range factories launch no composition layer, the wide ones only those"""
    from gnn_matlang_amd import collate, models, functional as Fn
    gs, ninp, kind, fields = model_case(name)
    cpu = collate(gs, node_fields=fields, graph_fields=('lmax',))
    b = cpu.to(dev)
    factory = getattr(models, name)
    kw = dict(dropout=0.0) if 'dropout' in inspect.signature(factory).parameters else {}      # (the masks are not part of the restatement)
    torch.manual_seed(11)
    m = factory(ninp, **kw)
    with torch.no_grad():
        for n, v in m.named_parameters():                      # biases and BatchNorm parameters off their constant initial values
            if n.endswith('bias') or n.startswith('bn'):
                v.add_(0.1 * torch.randn(v.shape))
    p64 = {k: v.detach().double().clone().requires_grad_(True) for k, v in m.named_parameters()}
    out64 = R.chebnet_ref(p64, m, cpu.x, cpu.edge_index, cpu.ptr.tolist(), cpu.lmax)
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
    roads = {k: v for k, v in Fn.PATHS.items() if k.startswith('cheb:')}
    if name in R.WIDE:                                         # 128 / 200 wide: every layer of both forwards on the composition
        assert sum(roads.values()) == 2 * m.nlayers and all('torch ops (outside the fused layer)' in k for k in roads), roads
    else:
        assert not roads, roads
    e = {'out': rel_err(out.detach().cpu().numpy(), out64.detach().numpy()), 'loss': abs(float(l.detach()) - float(l64.detach())) / abs(float(l64.detach()))}
    for k, v in m.named_parameters():
        if k in ('bn1.weight', 'bn1.bias', 'bn2.weight', 'bn2.bias') and int(k[2]) not in m.bn_after and m.head != 'bn_mlp':
            assert v.grad is None and p64[k].grad is None, k   # declared, never called (ptc.py:203-204)
            continue
        assert p64[k].grad is not None and v.grad is not None, k
        e[k] = rel_err(v.grad.cpu().numpy(), p64[k].grad.numpy())
    print(name, {k: '%.2e' % v for k, v in e.items()})
    assert float(out64.detach().abs().max()) > 0
    assert max(e.values()) <= MODEL_TOL, e


def test_fused_road_and_composition_agree(dev):
    from gnn_matlang_amd import collate, models
    gs, ninp, _, _ = model_case('zinc_cheb')
    b = collate(gs, graph_fields=('lmax',)).to(dev)
    torch.manual_seed(5)
    m = models.zinc_cheb(ninp).to(dev)
    grads = []
    for road in (None, 'torch'):
        m.zero_grad()
        out = m(b, _road=road)
        models.zinc_loss(out, b.y).backward()
        grads.append((out.detach(), {k: v.grad.clone() for k, v in m.named_parameters()}))
    assert rel_err(grads[0][0].cpu().numpy(), grads[1][0].cpu().numpy()) <= MODEL_TOL
    for k in grads[0][1]:
        assert rel_err(grads[0][1][k].cpu().numpy(), grads[1][1][k].cpu().numpy()) <= MODEL_TOL, k


def test_missing_lmax_is_named(dev):
    from gnn_matlang_amd import collate, models
    gs, ninp, _, _ = model_case('zinc_cheb')
    b = collate(gs).to(dev)
    with pytest.raises(ValueError, match=r"graph_fields=\('lmax',\)"):
        models.zinc_cheb(ninp).to(dev)(b)
    models.mutag_cheb(ninp).to(dev)(b)                         # lambda_max = None in the script: no lmax needed


def test_padded_static_batch_equals_the_plain_batch(dev):
    """padded static batches work with lmax carried.  A padding node carries only self loops, which are dropped, so it is isolated; the
    padding graph and absent slots read lambda_max = 2.0; the pool skips the padding graph.  Same graphs plain and padded (absent slots
    included): logits of the real graphs, the masked loss and every parameter gradient."""
    from gnn_matlang_amd import SpectralDesign, models, readers
    from gnn_matlang_amd.dataset import DeviceDataset
    raw = readers.load_mutag(os.path.join(RAW, 'mutag.mat'))[:20]
    dd = DeviceDataset.from_graphs(SpectralDesign(recfield=1, dv=4, nfreq=3, adddegree=True).design_many(raw), dev, graph_fields=('lmax',))
    dd.y = dd.y.float()
    G = len(dd)
    torch.manual_seed(3)
    mp = models.Cheb(int(dd.x.size(1)), (32, 32, 32), 3, act='relu', pool='mean', head='mlp', hidden=32).to(dev).train()
    assert mp.lmax
    ms = copy.deepcopy(mp)
    sl = [11, 0, G, 7, 3, G, 14, 2, 9, 1, 5, G, 12, 4, 8, 6]
    ids = torch.tensor(sl, device=dev)
    real = torch.tensor([i for i in sl if i < G], device=dev)
    keep = torch.tensor([k for k, i in enumerate(sl) if i < G], device=dev)
    bs = dd.batch_padded(ids, dd.bounds(16), adjacency=True)
    bpl = dd.batch(real)
    assert bs.lmax.numel() == 17 and torch.equal(bs.lmax[keep], bpl.lmax) and float(bs.lmax[-1]) == 2.0 and float(bs.lmax[2]) == 2.0
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
    ba = dd.batch_assembled(ids, dd.bounds(16), adjacency=True)          # the one-launch assembly carries the same values
    assert torch.equal(ba.lmax, bs.lmax)
    with torch.no_grad():
        assert rel_err(ms(ba)[keep].cpu().numpy(), pre_p.cpu().numpy()) <= 2e-5


# ------------------------------------------------------------------------------------------------------------------ 6. expressivity
def _as_dicts(raw):
    gs = [dict(x=x, edge_index=ei, y=y) for x, ei, y in raw]
    for g, l in zip(gs, R.graph_lambdas(gs)):
        g['lmax'] = l
    return gs


def _float64_distances(factory, ninp, seeds, gs, iu):
    """per seed, the L1 distance of every pair of iu between the float64 ChebNet's graph rows"""
    from gnn_matlang_amd import collate
    cpu = collate(gs, graph_fields=('lmax',))
    out = []
    for s in seeds:
        torch.manual_seed(s)
        m = factory(ninp)
        p = {k: v.detach().double() for k, v in m.state_dict().items()}
        with torch.no_grad():
            E = R.chebnet_ref(p, m, cpu.x, cpu.edge_index, cpu.ptr.tolist(), cpu.lmax).numpy()
        assert np.abs(E).max() > 0.1
        out.append(np.abs(E[iu[0]] - E[iu[1]]).sum(1))
    return out


def _decisions(dev, factory, ninp, seeds, gs, tol, what):
    """the rule of test_graph8c_decisions_equal_float64 (tests/test_gpu_gin.py): every pair whose float64 distance (maximum over the
    seeds) is above 2 tol must be separated on the device, every pair below tol / 2 must stay similar; first, on the CPU, no pair
    may lie in between.  The counts are printed."""
    from gnn_matlang_amd import collate, expressivity
    iu = np.triu_indices(len(gs), 1)
    dmax = np.zeros(iu[0].size)
    for d in _float64_distances(factory, ninp, seeds, gs, iu):
        dmax = np.maximum(dmax, d)
    must_sep, must_sim = dmax > 2 * tol, dmax < tol / 2
    assert (must_sep | must_sim).all(), '%s: %d pairs between tol / 2 and 2 tol: pick other seeds' % (what, int((~(must_sep | must_sim)).sum()))
    b = collate(gs, graph_fields=('lmax',)).to(dev)
    tr = expressivity.PairTracker(len(gs), tol=tol, device=dev)
    counts = expressivity.count_similar(lambda: factory(ninp), b, seeds=seeds, tracker=tr)
    sim = np.zeros((len(gs), len(gs)), dtype=bool)
    sp = tr.similar_pairs().cpu().numpy().reshape(-1, 2)
    sim[sp[:, 0], sp[:, 1]] = True
    got_sim = sim[iu[0], iu[1]]
    print('%s: float64 separates %d, never separates %d of %d pairs; device counts %s' % (what, int(must_sep.sum()), int(must_sim.sum()), iu[0].size, counts))
    assert not got_sim[must_sep].any(), '%d pairs the float64 model separates stayed similar' % int(got_sim[must_sep].sum())
    assert got_sim[must_sim].all(), '%d pairs the float64 model cannot separate were separated' % int((~got_sim[must_sim]).sum())
    assert counts[-1] == int(got_sim.sum())
    return must_sep, must_sim


def test_sr25_decisions_equal_float64(dev):
    """sr25.py:281-300 with ChebNet over seeds 0-2: count_similar(models.sr25_cheb, ...) runs and decides every pair as float64 does"""
    from gnn_matlang_amd import models, readers
    gs = _as_dicts(readers.load_sr(os.path.join(RAW, 'sr251256.g6')))
    must_sep, must_sim = _decisions(dev, models.sr25_cheb, gs[0]['x'].shape[1], [0, 1, 2], gs, 1e-3, 'sr25')
    assert must_sep.size == 105


def test_graph8c_decisions_equal_float64(dev):
    """graphs [1000:1300] of graph8c with graph8c_cheb over seeds 0-2: the discriminating case (a constant output cannot pass)"""
    from gnn_matlang_amd import models, readers
    gs = _as_dicts(readers.load_graph8c(os.path.join(RAW, 'graph8c.g6'))[1000:1300])
    must_sep, must_sim = _decisions(dev, models.graph8c_cheb, gs[0]['x'].shape[1], [0, 1, 2], gs, 1e-3, 'graph8c[1000:1300]')
    assert must_sep.size == 44850 and must_sep.sum() > 40000


# ------------------------------------------------------------------------------------------------------------------ 7. many tiles
MAXWG = 768              # the workgroups of a tile-walking launch and of a row pass (csrc/gml_rowtile64.h)
COPIES = 367             # of rand67: 24,589 rows = 769 tiles of 32 rows, the fewest copies with more than MAXWG tiles


def sparse_laplacian(ei, N, batch, lam, dtype):
    """R.laplacian as a sparse [N, N] matrix, every step in `dtype`: the same entries, repeats summed"""
    ei = torch.as_tensor(ei, dtype=torch.int64)
    ei = ei[:, ei[0] != ei[1]]
    A = torch.sparse_coo_tensor(torch.stack([ei[1], ei[0]]), torch.ones(ei.size(1), dtype=dtype), (N, N)).coalesce()
    deg = torch.sparse.sum(A, 0).to_dense()
    dis = torch.where(deg > 0, deg.clamp(min=1).pow(-0.5), torch.zeros_like(deg))
    s = 2.0 / lam.to(dtype)[batch]
    i, j = A.indices()
    d = torch.arange(N)
    return torch.sparse_coo_tensor(torch.cat([A.indices(), torch.stack([d, d])], 1), torch.cat([-(s * dis)[i] * A.values() * dis[j], s - 1]),
                                   (N, N)).coalesce()


_MANY = {}


def many_tiles_case(si, act):
    """(case, graph tuple, (float64, float32) references) of rand67 as COPIES block-diagonal copies, each a graph of the batch with the
    small graph's lambda_max: x repeated per copy, the weights of the small case, dy fresh for every row; the kink margin is asserted
    on the small case, whose pre-activations are the only values the big one takes.  Computed once."""
    if not _MANY:
        case, (ei, n, batch, lam), L, seed = R.layer_case(si, act, 'rand67')
        assert_margin(case, L, act, 'many tiles: the small case, seed %d' % seed)
        N = COPIES * n
        big = dict(case, x=case['x'].repeat(COPIES, 1))
        big['dy'] = torch.randn(N, case['dy'].size(1), generator=torch.Generator().manual_seed(seed + 1))
        eib = (ei[:, None, :] + n * np.arange(COPIES, dtype=np.int64)[None, :, None]).reshape(2, -1)
        gr = (eib, N, torch.arange(COPIES).repeat_interleave(n), lam.repeat(COPIES))
        refs = []
        for dt in (torch.float64, torch.float32):
            d = {k: v.to(dt) for k, v in big.items()}
            Ls = sparse_laplacian(eib, N, gr[2], gr[3], dt)
            r = R.backward(d['x'], Ls, d['W'], d['b'], act, d['dy'])
            r['y'] = R.forward(d['x'], Ls, d['W'], d['b'], act)
            refs.append(r)
        _MANY.update(case=big, gr=gr, refs=tuple(refs))
    return _MANY['case'], _MANY['gr'], _MANY['refs']


@pytest.mark.parametrize('need_dx', [True, False])
def test_many_tiles(dev, need_dx):
    """769 tiles at K = 3 (the smallest K whose adjoint runs one step without G_{k+2} and one with it): the forward's and the adjoint's
    workgroups make a second trip of their tile loop, the row pass gets two tiles per workgroup and a last workgroup that owns one.
    Reference: backward() / forward() of tests/_cheb_ref.py, the float64 restatement and its float32 twin, fed a SPARSE L^
    (sparse_laplacian above, built from the big edge list in the reference's own dtype) in place of the dense [N, N] one."""
    from gnn_matlang_amd import _lib
    from gnn_matlang_amd.graph import GraphCSR
    si, act = 2, 'relu'
    Fin, Fout, K = R.SHAPES[si]
    assert K == 3 and Fin != Fout and max(Fin, Fout) < 64
    big, gr, (ref64, ref32) = many_tiles_case(si, act)
    N = gr[1]
    tiles = -(-N // 32)
    L = _lib.lib()
    P = int(L.gml_cheb_dflat_floats(Fin, Fout, K))
    nwg, rest = divmod(int(L.gml_cheb_bwd_workspace_bytes(N, Fin, Fout, K)) // 4 - 3 * N * Fin, P)
    tpw = -(-tiles // nwg)
    print('many tiles: N %d, tiles %d, row-pass workgroups %d of %d tiles (the last: %d)' % (N, tiles, nwg, tpw, tiles - (nwg - 1) * tpw))
    assert N == 24589 and tiles == MAXWG + 1                   # the forward and the adjoint: a second trip for workgroup 0 alone
    assert rest == 0 and 1 < nwg < tiles and tpw == 2 and tiles - (nwg - 1) * tpw == 1
    csr = GraphCSR.from_edge_index(torch.from_numpy(gr[0]).to(dev), N)
    check_layer(layer_gpu(dev, big, gr, csr, act, need_dx), ref64, ref32, 'many tiles dx=%s' % need_dx, need_dx)
