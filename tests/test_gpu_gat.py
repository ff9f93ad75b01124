"""GAT on the MI355X (csrc/gml_gat.hip, functional.GATConvFunction, gat.GATConv, models.GAT): the layer against the float64 restatement
of tests/_gat_ref.py over the shape / activation / graph matrix -- through the module and through the raw ABI with sentinel-framed
buffers --, the softmax range, the kink margins, the bit-level edge cases, reproducibility and capture, every factory against the
float64 GatNet restatement, the expressivity count, the two roads and the padded static batch."""
import copy
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import _conv_ref as CR
import _gat_ref as R
from _gnnml1_ref import TOL, check
from conftest import GOLDEN, rel_err

pytestmark = pytest.mark.gpu

RAW = os.path.join(GOLDEN, 'raw')
MODEL_TOL = 1e-4
H = R.H
GRADS = ('dx', 'dW', 'datt_l', 'datt_r', 'dbias')


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


def layer_gpu(dev, case, csr, act, need_dx=True):
    """the module: (y, {dx, dW, datt_l, datt_r, dbias})"""
    from gnn_matlang_amd import GATConv, functional as Fn
    Fin, C = case['x'].size(1), case['att_l'].size(2)
    m = GATConv(Fin, C, heads=H).to(dev)
    with torch.no_grad():
        m.lin_l.weight.copy_(case['W']); m.att_l.copy_(case['att_l']); m.att_r.copy_(case['att_r']); m.bias.copy_(case['bias'])
    x = case['x'].to(dev).requires_grad_(need_dx)
    assert Fn.gat_conv_supported(x, H, C)
    y = m(x, csr, act=act)
    y.backward(case['dy'].to(dev))
    return y.detach(), dict(dx=x.grad, dW=m.lin_l.weight.grad, datt_l=m.att_l.grad, datt_r=m.att_r.grad, dbias=m.bias.grad)


def check_att(got, ref64, ref32, k, what, self_only):
    """datt_l / datt_r.  On a graph whose rows hold their self edge only, de = alpha (dalpha - <g, out>) is exactly zero: the float64
    restatement gives rounding noise, and an error relative to it measures nothing.  There the result is held to the project's
    tolerance for exact fp32 products against the gradient's TERM SUM (tests/_gat_ref.py backward(): tl, tr), as the conv ABI tests
    hold elements whose terms cancel; everywhere else to check(computed=True)."""
    if not self_only:
        return check(got, ref64[k], ref32[k], k, what, computed=True)
    t = float(ref64['tl' if k == 'datt_l' else 'tr'].max())
    e = float(got.detach().cpu().double().abs().max())
    print('%s %s: |got| %.3e, |float64| %.3e, term sum %.3e' % (what, k, e, float(ref64[k].abs().max()), t))
    assert t > 0 and float(ref64[k].abs().max()) <= 1e-12 * t and e <= TOL * t


def check_layer(got, ref64, ref32, what, need_dx=True, self_only=False):
    y, g = got
    check(y, ref64['y'], ref32['y'], 'y', what, computed=True)
    for k in GRADS:
        if k == 'dx' and not need_dx:
            assert g[k] is None
        elif k in ('datt_l', 'datt_r'):
            check_att(g[k], ref64, ref32, k, what, self_only)
        else:
            check(g[k], ref64[k], ref32[k], k, what, computed=True)


# ------------------------------------------------------------------------------------------------------------------ 1. layer matrix
MATRIX = [(si, act, g) for si in range(len(R.SHAPES)) for act in R.ACTS for g in sorted(R.GRAPHS)]


def assert_margin(case, A, act, what):
    """3. kinks: asserted on the float64 restatement before any result is compared; no element is excluded"""
    ms, mp = R.margins(case, A, act)
    assert ms >= R.MARGIN and mp >= R.MARGIN, '%s: kink margin %.2e / %.2e below %.0e' % (what, ms, mp, R.MARGIN)


@pytest.mark.parametrize('need_dx', [True, False])
@pytest.mark.parametrize('si,act,gname', MATRIX)
def test_module_against_float64(dev, si, act, gname, need_dx):
    case, ei, N, A, seed = R.layer_case(si, act, gname)
    what = 'Fin, C = %s act=%s graph=%s seed=%d dx=%s' % (R.SHAPES[si], act, gname, seed, need_dx)
    assert_margin(case, A, act, what)
    ref64, ref32 = R.layer_ref((si, act, gname), case, A, act)
    check_layer(layer_gpu(dev, case, csr_of(gname, dev), act, need_dx), ref64, ref32, what, need_dx, self_only=gname == 'one')


@pytest.mark.parametrize('gname', ['hand', 'rand67', 'star'])
@pytest.mark.parametrize('C', [4, 32])
def test_widths_beside_the_scripts(dev, C, gname):
    """C = 4 (eight rows per wave) and C = 32 (one row per wave, eight lanes per head): served, used by no script"""
    ei, N = R.get_graph(gname)
    A = R.adjacency(ei, N, torch.float64)
    seed = 7000 + C
    while min(R.margins(R.draw_case(5, C, N, seed), A, 'elu')) < R.MARGIN:
        seed += 1
    case = R.draw_case(5, C, N, seed)
    assert_margin(case, A, 'elu', 'C=%d' % C)
    ref64, ref32 = R.layer_ref(('width', C, gname), case, A, 'elu')
    check_layer(layer_gpu(dev, case, csr_of(gname, dev), 'elu'), ref64, ref32, 'C=%d graph=%s seed=%d' % (C, gname, seed))


def _dev_buf(buf, dev):
    return torch.from_numpy(buf).to(dev)


def _at(t, off):
    return ctypes.c_void_p(t.data_ptr() + 4 * int(off))


def abi_run(dev, case, csr, act, C, H_=H, pad=4, bias=True):
    """gml_gat_logits / _fwd / _bwd on sentinel-framed buffers with leading dimensions HC + pad; returns the return codes, the host
    copies of every buffer and their layouts"""
    from gnn_matlang_amd import _lib
    from gnn_matlang_amd.graph import _ptr, _stream
    L = _lib.lib()
    N, HC, E = case['x'].size(0), H_ * C, csr.E
    ld = HC + pad
    xl = torch.zeros(N, ld, device=dev)
    xl[:, :HC] = case['x'].to(dev) @ case['W'].to(dev).t()
    dy = torch.zeros(N, ld, device=dev)
    dy[:, :HC] = case['dy'].to(dev)
    attl, attr = case['att_l'].reshape(-1).to(dev).contiguous(), case['att_r'].reshape(-1).to(dev).contiguous()
    b = case['bias'].to(dev) if bias else None
    lay = dict(al=(N, H_, H_), ar=(N, H_, H_), m=(N, H_, H_), z=(N, H_, H_), y=(N, HC, ld), dxl=(N, HC, ld), datt_l=(1, HC, HC), datt_r=(1, HC, HC),
               dbias=(1, HC, HC))
    nws = int(L.gml_gat_bwd_workspace_bytes(N, E, H_, C)) // 4
    bufs, offs = {}, {}
    for k, (n, nc, l) in lay.items():
        hb, offs[k] = CR.alloc(n, nc, l, head=k in ('y', 'dxl'))
        bufs[k] = _dev_buf(hb, dev)
    wsn = max(nws, 4)
    hb, _ = CR.alloc(1, wsn, wsn + 64, guard_rows=0)
    ws = _dev_buf(hb, dev)
    st = _stream(dev)
    p = lambda k: _at(bufs[k], offs[k])
    rc = [L.gml_gat_logits(_ptr(xl), ld, _ptr(attl), _ptr(attr), N, H_, C, p('al'), p('ar'), st)]
    rc.append(L.gml_gat_fwd(_ptr(csr.rowptr), _ptr(csr.col), _ptr(xl), ld, p('al'), p('ar'), _ptr(b), N, E, H_, C, R.ACTS.index(act), p('y'), ld,
                            p('m'), p('z'), st))
    rc.append(L.gml_gat_bwd(_ptr(csr.rowptr), _ptr(csr.col), _ptr(csr.rowptr_t), _ptr(csr.col_t), _ptr(csr.pos_t), _ptr(xl), ld, p('al'), p('ar'),
                            p('m'), p('z'), p('y'), ld, _ptr(dy), ld, _ptr(attl), _ptr(attr), N, E, H_, C, R.ACTS.index(act), p('dxl'), ld,
                            p('datt_l'), p('datt_r'), p('dbias') if bias else None, _ptr(ws), wsn * 4, st))
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in bufs.items()}
    return rc, host, lay, ws.cpu().numpy()[wsn:]


def abi_values(host, lay):
    """{name: values}, asserting that every guard word of every buffer is still the sentinel"""
    out = {}
    for k, (n, nc, l) in lay.items():
        v, guards = CR.split(host[k], n, nc, l)
        assert (guards == CR.SENTINEL).all(), '%s: %d guard words overwritten' % (k, int((guards != CR.SENTINEL).sum()))
        out[k] = torch.from_numpy(np.array(v))
    return out


@pytest.mark.parametrize('si,act,gname', MATRIX)
def test_abi_against_float64(dev, si, act, gname):
    from gnn_matlang_amd import _lib
    case, ei, N, A, seed = R.layer_case(si, act, gname)
    what = 'ABI Fin, C = %s act=%s graph=%s seed=%d' % (R.SHAPES[si], act, gname, seed)
    assert_margin(case, A, act, what)
    ref64, ref32 = R.layer_ref((si, act, gname), case, A, act)
    C = R.SHAPES[si][1]
    rc, host, lay, tail = abi_run(dev, case, csr_of(gname, dev), act, C)
    assert rc == [_lib.GML_OK] * 3
    assert (tail.view(np.int32) == CR.SENTINEL).all(), 'the workspace tail was written'
    v = abi_values(host, lay)
    check(v['y'], ref64['y'], ref32['y'], 'y', what, computed=True)
    check(v['dxl'], ref64['dxl'], ref32['dxl'], 'dxl', what, computed=True)
    for k in ('datt_l', 'datt_r'):
        check_att(v[k].reshape(ref64[k].shape), ref64, ref32, k, what, self_only=gname == 'one')
    check(v['dbias'].reshape(ref64['dbias'].shape), ref64['dbias'], ref32['dbias'], 'dbias', what, computed=True)
    assert float(v['z'].min()) >= 1.0                     # the row maximum contributes exp(0)


# ------------------------------------------------------------------------------------------------------------------ 2. softmax range
def test_softmax_range(dev):
    case, A = R.range_case()
    d = {k: v.double() for k, v in case.items()}
    s = R.forward(d['x'], A, d['W'], d['att_l'], d['att_r'], d['bias'], None, parts=True)[2]
    row = torch.where(A[0] > 0)[0]
    assert float(s[0, row].max()) >= 80 and float(s[0, row].min()) <= -80        # exp() of the raw logit overflows fp32 from 88.8
    assert_margin(case, A, None, 'range')
    ref64, ref32 = R.layer_ref('range', case, A, None)
    check_layer(layer_gpu(dev, case, csr_of('star', dev), None), ref64, ref32, 'softmax range')


# ------------------------------------------------------------------------------------------------------------------ 4. edge cases
@pytest.mark.parametrize('act', R.ACTS)
def test_self_edge_only_rows_are_act_of_their_own_row(dev, act):
    """rows without neighbours (the isolated node of the hand-made graph, the single node): exp(0) = 1, z = 1, 1 / (1 + 1e-16) = 1,
    so the pre-activation is xl + b in one fmaf with a unit factor: bit-exact.  relu and none are compared bit for bit with torch;
    tanh and elu against torch's own tanh / elu of those bits within 2 ulp (two implementations of one function)."""
    for gname, rows in (('hand', [5]), ('one', [0])):
        case, ei, N, A, seed = R.layer_case(2, act, gname)
        y, _ = layer_gpu(dev, case, csr_of(gname, dev), act)
        pre = (case['x'].to(dev) @ case['W'].to(dev).t() + case['bias'].to(dev))[rows]
        if act in (None, 'relu'):
            assert torch.equal(y[rows], pre if act is None else torch.relu(pre))
        else:
            want = torch.tanh(pre) if act == 'tanh' else torch.nn.functional.elu(pre)
            assert float(((y[rows] - want).abs() / want.abs().clamp(min=1e-30)).max()) <= 2 * 2.0 ** -23


@pytest.mark.parametrize('Hh,C', [(4, 16), (8, 5), (8, 64), (1, 8)])
def test_unsupported_shapes(dev, Hh, C):
    from gnn_matlang_amd import GATConv, functional as Fn, _lib
    ei, N = R.get_graph('hand')
    g = torch.Generator().manual_seed(1)
    case = dict(x=torch.randn(N, 3, generator=g), W=torch.randn(Hh * C, 3, generator=g), att_l=torch.randn(1, Hh, C, generator=g),
                att_r=torch.randn(1, Hh, C, generator=g), bias=torch.randn(Hh * C, generator=g), dy=torch.randn(N, Hh * C, generator=g))
    assert not Fn.gat_conv_supported(case['x'].to(dev), Hh, C)
    pad = (-Hh * C) % 4 + 4                              # (rows stay float4 addressable: the refusal is about H and C)
    rc, host, lay, tail = abi_run(dev, case, csr_of('hand', dev), None, C, H_=Hh, pad=pad)
    assert rc == [_lib.GML_E_UNSUPPORTED] * 3
    for k in host:
        assert (host[k].view(np.int32) == CR.SENTINEL).all(), k       # nothing was launched
    # the module takes the composition and gives the restatement's result
    m = GATConv(3, C, heads=Hh).to(dev)
    with torch.no_grad():
        m.lin_l.weight.copy_(case['W']); m.att_l.copy_(case['att_l']); m.att_r.copy_(case['att_r']); m.bias.copy_(case['bias'])
    y = m(case['x'].to(dev), csr_of('hand', dev), act='elu')
    d = {k: v.double() for k, v in case.items()}
    y64 = R.forward(d['x'], R.adjacency(ei, N, torch.float64), d['W'], d['att_l'], d['att_r'], d['bias'], 'elu')
    assert rel_err(y.detach().cpu().numpy(), y64.numpy()) <= 2e-5


def test_misaligned_rows_are_refused(dev):
    from gnn_matlang_amd import _lib
    case, ei, N, A, seed = R.layer_case(2, None, 'hand')
    rc, host, lay, tail = abi_run(dev, case, csr_of('hand', dev), None, 8, pad=3)
    assert rc[1:] == [_lib.GML_E_UNSUPPORTED] * 2
    for k in ('y', 'm', 'z', 'dxl', 'datt_l', 'datt_r', 'dbias'):
        assert (host[k].view(np.int32) == CR.SENTINEL).all(), k


def test_unsorted_source_rows(dev):
    """the same edges in shuffled order: GraphCSR's general construction (source keys not sorted), the same layer result"""
    from gnn_matlang_amd.graph import GraphCSR
    case, ei, N, A, seed = R.layer_case(3, 'elu', 'rand67')
    order = np.lexsort((ei[1], ei[0]))
    srt = ei[:, order]
    shuf = srt[:, np.random.default_rng(3).permutation(ei.shape[1])]
    assert (np.diff(shuf[0]) < 0).any() and (np.diff(srt[0]) >= 0).all()
    ref64, ref32 = R.layer_ref((3, 'elu', 'rand67'), case, A, 'elu')
    outs = []
    for e in (srt, shuf):
        csr = GraphCSR.from_edge_index(torch.from_numpy(np.ascontiguousarray(e)).to(dev), N)
        outs.append(layer_gpu(dev, case, csr, 'elu'))
        check_layer(outs[-1], ref64, ref32, 'unsorted' if e is shuf else 'sorted')
    assert not csr.src_sorted
    assert rel_err(outs[1][0].cpu().numpy(), outs[0][0].cpu().numpy()) <= 2e-6


def test_no_bias_and_empty_edge_list(dev):
    from gnn_matlang_amd import GATConv
    from gnn_matlang_amd.graph import GraphCSR
    g = torch.Generator().manual_seed(2)
    x = torch.randn(5, 4, generator=g).to(dev).requires_grad_(True)
    m = GATConv(4, 8, heads=8, bias=False).to(dev)
    csr = GraphCSR.from_edge_index(torch.zeros(2, 0, dtype=torch.int64, device=dev), 5)
    y = m(x, csr, act='relu')
    assert torch.equal(y, torch.relu(x @ m.lin_l.weight.t()))
    y.sum().backward()
    assert m.bias is None and x.grad is not None and torch.isfinite(x.grad).all()


# ------------------------------------------------------------------------------------------------------------------ 5. reproducibility, capture
def test_bit_reproducible(dev):
    case, ei, N, A, seed = R.layer_case(5, 'tanh', 'mutag16')          # several partials of the reduction
    a = layer_gpu(dev, case, csr_of('mutag16', dev), 'tanh')
    b = layer_gpu(dev, case, csr_of('mutag16', dev), 'tanh')
    assert torch.equal(a[0], b[0]) and all(torch.equal(a[1][k], b[1][k]) for k in GRADS)


def test_captured_layer_equals_eager(dev):
    from gnn_matlang_amd import functional as Fn
    c0 = R.layer_case(3, 'elu', 'star')[0]
    c1 = R.draw_case(64, 12, c0['x'].size(0), 77)
    csr = csr_of('star', dev)
    keys = ('x', 'W', 'att_l', 'att_r', 'bias')
    s = {k: c0[k].to(dev).requires_grad_(True) for k in keys}
    sdy = c0['dy'].to(dev)

    def step():
        y = Fn.GATConvFunction.apply(s['x'], csr, s['W'], s['att_l'], s['att_r'], s['bias'], 'elu')
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
    y, gr = layer_gpu(dev, c1, csr, 'elu')
    want = [y] + [gr[k] for k in GRADS]
    assert all(torch.equal(a, b) for a, b in zip(got, want))


# ------------------------------------------------------------------------------------------------------------------ 6. models
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
    if name == 'sr25_real':                               # (the expressivity count; as a model case its attention gradients are
        gs = [dict(x=x, edge_index=ei, y=y) for x, ei, y in readers.load_sr(os.path.join(RAW, 'sr251256.g6'))]       # exactly zero:
        return gs, gs[0]['x'].shape[1], None, ()          # constant features on regular graphs make every logit of a row equal)
    if name == 'mutag_gat':
        gs = [dict(x=x, edge_index=ei, y=np.float32(y)) for x, ei, y in readers.load_mutag(os.path.join(RAW, 'mutag.mat'))[:16]]
        return gs, gs[0]['x'].shape[1], 'mutag', ()
    if name == 'filtering_gat':
        gs = _rand_graphs(3, 1, 5, _REAL, 20, 30)
        rng = np.random.default_rng(6)
        for g in gs:
            n = g['x'].shape[0]
            g['y'] = rng.standard_normal((n, 3)).astype(np.float32)
            g['mask'] = (rng.random((n, 1)) < 0.7).astype(np.float32)
        return gs, 1, 'filtering', ('y', 'mask')
    table = {'sr25_gat': (2, _REAL, None), 'graph8c_gat': (2, _REAL, None), 'exp_gat': (2, _REAL, None),
             'exp_classify_gat': (2, _BIN, 'bce'), 'zinc_gat': (25, _REAL, 'zinc'),
             'counting_gat': (2, _REAL, 'counting'), 'ptc_gat': (20, cls(2), 'tu'), 'enzymes_gat': (4, cls(6), 'tu'),
             'proteins_gat': (4, cls(2), 'tu'), 'enzymes_contfeat_gat': (22, cls(6), 'tu'), 'freqclass_gat': (1, _BIN, 'bce'),
             'mnist75_gat': (3, cls(10), 'tu')}
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
def test_models_against_float64(dev, name):
    from gnn_matlang_amd import collate, models
    gs, ninp, kind, fields = model_case(name)
    cpu = collate(gs, node_fields=fields)
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
    out64 = R.gatnet_ref(p64, m, cpu.x, cpu.edge_index, cpu.ptr.tolist())
    wsum = torch.randn(out64.shape, generator=torch.Generator().manual_seed(3))
    loss_dev, loss_ref = losses(kind, models, wsum)
    l64 = loss_ref(out64, cpu)
    l64.backward()
    m2 = factory(ninp, **kw)
    m2.load_state_dict(m.state_dict(), strict=True)
    m, m2 = m.to(dev).train(), m2.to(dev).train()
    out = m2(b)
    l = loss_dev(m, b)
    l.backward()
    e = {'out': rel_err(out.detach().cpu().numpy(), out64.detach().numpy()), 'loss': abs(float(l.detach()) - float(l64.detach())) / abs(float(l64.detach()))}
    for k, v in m.named_parameters():
        if p64[k].grad is None:                                # a BatchNorm the script declares and never calls
            assert v.grad is None and k.startswith('bn')
        else:
            e[k] = rel_err(v.grad.cpu().numpy(), p64[k].grad.numpy())
    print(name, {k: '%.2e' % v for k, v in e.items()})
    assert float(out64.detach().abs().max()) > 0
    assert max(e.values()) <= MODEL_TOL, e


def test_count_similar_equals_float64(dev):
    """sr25: GAT cannot tell the strongly regular graphs apart (a 1-WL bounded model on regular graphs with constant features), so
    every one of the 105 pairs stays similar -- in float64 with no pair inside the tolerance band, and on the device"""
    from gnn_matlang_amd import collate, expressivity, models
    gs, ninp, _, _ = model_case('sr25_real')
    cpu = collate(gs)
    seeds, tol = [0, 1, 2], 1e-3
    iu = np.triu_indices(len(gs), 1)
    dmax, sep, want = np.zeros(iu[0].size), np.zeros(iu[0].size, dtype=bool), []
    for s in seeds:
        torch.manual_seed(s)
        m = models.sr25_gat(ninp)
        p = {k: v.detach().double() for k, v in m.state_dict().items()}
        with torch.no_grad():
            E = R.gatnet_ref(p, m, cpu.x, cpu.edge_index, cpu.ptr.tolist()).numpy()
        d = np.abs(E[iu[0]] - E[iu[1]]).sum(1)
        dmax = np.maximum(dmax, d)
        sep |= d > tol
        want.append(int((~sep).sum()))
    band = ~((dmax > 2 * tol) | (dmax < tol / 2))
    assert not band.any(), 'pairs whose decision hangs on the tolerance: %d' % int(band.sum())
    got = expressivity.count_similar(lambda: models.sr25_gat(ninp), cpu.to(dev), seeds=seeds)
    print(got, want)
    assert got == want


def test_fused_road_and_composition_agree(dev):
    from gnn_matlang_amd import collate, models
    gs, ninp, _, _ = model_case('zinc_gat')
    b = collate(gs).to(dev)
    torch.manual_seed(5)
    m = models.zinc_gat(ninp).to(dev)
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
    """the decision for padded static batches: they work.  A padding node carries only self loops, which are dropped and re-added
    like any other, so it sees itself alone; the pool skips the padding graph.  Same graphs plain and padded (absent slots included):
    logits of the real graphs, the masked loss and every parameter gradient."""
    from gnn_matlang_amd import SpectralDesign, models, readers
    from gnn_matlang_amd.dataset import DeviceDataset
    raw = readers.load_mutag(os.path.join(RAW, 'mutag.mat'))[:20]
    dd = DeviceDataset.from_graphs(SpectralDesign(recfield=1, dv=4, nfreq=3, adddegree=True).design_many(raw), dev)
    dd.y = dd.y.float()
    G = len(dd)
    torch.manual_seed(3)
    mp = models.mutag_gat(int(dd.x.size(1))).to(dev).train()
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
