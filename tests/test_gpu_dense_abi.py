"""The dense-block family for equal-size graphs of n <= 96 nodes (csrc/gml_dense.hip, and gml_xty_wide) at the level of its C ABI
(include/gml.h): every entry point by name through _lib.lib(), one launch and one numpy reference per case, against the float64
restatement of tests/_dense_ref.py -- which also holds the case tables, shared with the CPU companion tests/test_dense_ref_cpu.py.

What dense_block.py never passes: leading dimensions beyond the width and off the float4 grid, operands and outputs 4 bytes past a
16-byte boundary, sa / so other than 0 and F, a KP larger than 32 ceil(n / 32), relu, no bias, dw == NULL, images and workspaces of
exactly the queried size, and every error answer.

Conventions (those of the other ABI matrices):
  * an output sits in a buffer of _conv_ref.alloc(): its padding columns, 8 rows behind it and 4 floats in front of an offset output
    hold a NaN sentinel and must still hold it afterwards;
  * a packed image, a weight image and a workspace have exactly the queried size, 16-byte aligned, sentinel words behind;
  * inputs carry 7.0 in their padding columns and NaN in the rows behind row B n - 1 (8 of them, or KP - n where that is more: the
    rows a staging loop without its `k < n` guard would read): no NaN may reach an output;
  * after an error answer every output and workspace is bit-unchanged;
  * two launches of a case agree bit for bit; so do the float4 and the scalar road, and a larger KP, on the same data;
  * the road a launch takes is the one the case names: gml_dense_plan, the launchers' own decision, is asked with the very pointers
    of the launch (a misaligned float4 access gave the same bits where it was tried, DESIGN.md s4.7a: the values need not show a wrong decision).
Values: TOL = 1e-4 on the max-norm and on every element's own term sum (_dense_ref).  The last test prints the roads that ran and
the worst figures (pytest -rP; recorded in DESIGN.md s4.7a) and asserts that everything the tables below list did run."""
import ctypes

import numpy as np
import pytest
import torch

import _conv_ref as R
import _dense_ref as Q
from gnn_matlang_amd import _lib as G
from test_gpu_conv_fwd_abi import _Out, _done, _f32, _p, _rng, _up
from test_gpu_readout_abi import _flat, _written

pytestmark = pytest.mark.gpu

OK, BAD, UNS, WSP = G.GML_OK, G.GML_E_BADARG, G.GML_E_UNSUPPORTED, G.GML_E_WORKSPACE
TOL = Q.TOL
V, SC = 'vec', 'scalar'

# (kernel, NFT, NOT, road) that must have run.  NFT: feature tiles of the template (from F / Fin), NOT: output tiles (from Fout; the
# weight gradient: its number of 64-column blocks); road: 'vec' or 'scalar' per operand, in the order named by the kernel's row.
TEMPLATES = set(
    # support product, plain and summed over s (in, out)
    [(k, nft, '-', r) for k in ('support_mm', 'support_mm_sum') for nft in (1, 2, 4, 8) for r in ((V, V), (SC, SC))] +
    [(k, 2, '-', r) for k in ('support_mm', 'support_mm_sum') for r in ((SC, V), (V, SC))] +
    # chained forward without Hcat (x, out2) and with it (x, hcat, out2)
    [('conv_fwd', a, b, r) for a, b, r in ((1, 4, (SC, SC)), (1, 8, (SC, SC)), (1, 4, (V, SC)), (1, 8, (V, V)), (2, 4, (SC, V)), (2, 8, (V, SC)),
                                           (4, 4, (SC, V)), (4, 8, (V, V)), (8, 4, (SC, SC)), (8, 8, (V, V)), (2, 4, (V, V)), (2, 4, (V, SC)),
                                           (4, 8, (V, SC)))] +
    [('conv_fwd_hcat', a, b, r) for a, b, r in ((1, 4, (SC, SC, SC)), (1, 8, (SC, SC, SC)), (1, 4, (V, V, SC)), (1, 8, (V, V, V)), (2, 4, (SC, SC, V)),
                                                (2, 8, (V, V, SC)), (4, 4, (SC, SC, V)), (4, 8, (V, V, V)), (8, 4, (SC, SC, SC)), (8, 8, (V, V, V)),
                                                (2, 4, (V, V, V)), (2, 4, (SC, V, V)), (2, 4, (V, SC, V)), (2, 4, (V, V, SC)), (4, 8, (V, V, SC)))] +
    # chained backward for dx (dx); NFT = 8 is the FQ = 2 variant
    [('conv_bwd_x', a, b, (r,)) for a, b, r in ((1, 4, SC), (1, 8, SC), (1, 4, V), (1, 8, V), (2, 4, SC), (2, 8, V), (4, 4, SC), (4, 8, V), (8, 4, SC),
                                                (8, 8, V), (2, 4, V), (8, 8, SC))] +
    # weight gradient (x); NOT = column blocks
    [('conv_bwd_w', a, b, (r,)) for a, b, r in ((1, 1, SC), (1, 2, SC), (1, 1, V), (1, 2, V), (2, 1, SC), (2, 2, V), (4, 1, SC), (4, 2, V), (8, 1, SC),
                                                (8, 2, V), (1, 3, V), (4, 3, SC), (2, 1, V))])
# (kernel, operand, condition) that must have put an operand on the scalar road on its own
CONDITIONS = set(
    [(k, 'in', c) for k in ('support_mm', 'support_mm_sum') for c in ('F', 'ld', 'ptr')] + [('support_mm_sum', 'in', 'sa')] +
    [(k, 'out', c) for k in ('support_mm', 'support_mm_sum') for c in ('F', 'ld', 'ptr')] + [('support_mm', 'out', 'so')] +
    [('conv_fwd_hcat', 'x', c) for c in ('F', 'ld', 'ptr')] + [('conv_fwd_hcat', 'hcat', c) for c in ('F', 'ptr')] +
    [(k, 'out2', c) for k in ('conv_fwd', 'conv_fwd_hcat') for c in ('F', 'ld', 'ptr')] +
    [('conv_bwd_x', 'dx', c) for c in ('F', 'ld', 'ptr')] + [('conv_bwd_w', 'x', c) for c in ('F', 'ld', 'ptr')])

RAN, COND_RAN = set(), set()
WORST = {}                                                   # (kernel, road, output) -> [cases, worst max-norm, worst term-sum figure]
BITS = {}                                                    # what was compared bit for bit -> comparisons
_VALS = {}                                                   # (kernel, case name) -> output values, for the bitwise comparisons
_IMGS = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    assert G.lib().gml_version() >= 1
    return torch.device('cuda:0')


def _st(dev):
    from gnn_matlang_amd.graph import _stream
    return _stream(dev)


def _coarse(*roads):
    return tuple(r.split(':')[0] for r in roads)


def _ran(kern, nft, no, roads, names):
    RAN.add((kern, nft, no, _coarse(*roads)))
    for r, name in zip(roads, names):
        if r.startswith('scalar:') and '+' not in r:
            COND_RAN.add((kern, name, r[7:]))


def _note(kern, road, out, e):
    w = WORST.setdefault((kern, '/'.join(road), out), [0, 0.0, 0.0])
    w[0] += 1
    w[1], w[2] = max(w[1], e[0]), max(w[2], e[1])


def _bit(what, a, b, msg):
    a, b = np.ascontiguousarray(a, np.float32).view(np.int32), np.ascontiguousarray(b, np.float32).view(np.int32)
    assert a.shape == b.shape and np.array_equal(a, b), '%s: %s: %d elements differ' % (msg, what, int((a != b).sum()))
    BITS[what] = BITS.get(what, 0) + 1


def _vals(o):
    return R.split(o.get(), o.n, o.ncols, o.ldo, o.guard_rows)[0].copy()


def _in(a, ld, dev, lead=0, tail=R.GUARD_ROWS):
    """a [N, w] -> device float32 [N + tail, ld]: 7.0 in the padding columns, the NaN sentinel in the rows behind; `lead`: the
    array starts 4 bytes past a 16-byte boundary"""
    a = np.asarray(a, np.float32)
    h = np.full((a.shape[0] + tail, ld), 7.0, np.float32)
    h[a.shape[0]:] = np.array([R.SENTINEL], np.int32).view(np.float32)[0]
    h[:a.shape[0], :a.shape[1]] = a
    t = _up(h, dev, lead)
    assert (t.data_ptr() + 4 * lead) % 16 == (4 if lead else 0)
    return t


def _vec(a, dev):
    """a vector input (or None) with 8 junk floats behind it"""
    return None if a is None else _up(np.concatenate([np.asarray(a, np.float32).ravel(), np.full(8, 7.0, np.float32)]), dev)


class _Words(object):
    """`n` 16-bit words on the device at exactly that size, 16-byte aligned, Q.IMG_TAIL sentinel words behind"""

    def __init__(self, dev, n, fill=0xA5A5):
        self.n, self.fill = n, fill
        self.t = torch.from_numpy(np.full(n + Q.IMG_TAIL, fill, np.uint16).view(np.int16)).to(dev)
        assert self.t.data_ptr() % 16 == 0

    def ptr(self):
        return _p(self.t)

    def get(self):
        return self.t.cpu().numpy().view(np.uint16)

    def inside(self, what):
        w = self.get()
        assert (w[self.n:] == self.fill).all(), what + ': wrote behind the image'
        return w[:self.n]

    def unchanged(self):
        return bool((self.get() == self.fill).all())


def _image(dev, B, S, n, KP, transpose):
    """the packed supports of a case (cached per shape), through gml_dense_pack into exactly nblocks * 2 * n * KP words, and held
    to the reference bit for bit on the way"""
    key = (B, S, n, KP, transpose)
    if key not in _IMGS:
        D = Q.blocks(B, S, n)
        img = _Words(dev, B * S * 2 * n * KP)
        src = _up(D, dev)
        assert _done(G.lib().gml_dense_pack(_p(src), img.ptr(), B * S, n, KP, transpose, _st(dev))) == OK
        want = Q.pack_ref(D.reshape(B * S, n, n), KP, transpose)
        assert np.array_equal(img.inside('pack %r' % (key,)), want.ravel()), 'pack %r: image differs from the reference' % (key,)
        _IMGS[key] = img
    return _IMGS[key]


def _hold(o, ref, what, key, written=None):
    """the output buffer against the reference: guards, finiteness, both bars; columns no support owns must still be sentinel"""
    buf = o.get().copy()
    if written is not None and not written.all():
        rows = buf[buf.size - (o.n + o.guard_rows) * o.ldo:].reshape(o.n + o.guard_rows, o.ldo)
        gap = rows[:o.n, :o.ncols][:, ~written]
        assert (gap.view(np.int32) == R.SENTINEL).all(), what + ': a column between the supports\' slices was written'
        rows[:o.n, np.flatnonzero(~written)] = 0.0
    e = R.check(buf, ref.v, ref.t, o.n, o.ncols, o.ldo, TOL, what, o.guard_rows)
    _note(key[0], key[1], key[2], e)
    return e


def _tail(c):
    return max(R.GUARD_ROWS, c['KP'] - c['n'])


def _plan(kind, c, p_in=None, p_out=None, p_out2=None, with_h=True):
    a = [0 if p is None else (p.value or 0) for p in (p_in, p_out, p_out2)]
    got, want = Q.plan_ask(G.lib(), kind, c, *a), Q.plan_want(kind, c, with_h)
    assert got == want, 'plan of %s: %#x, the case names %#x' % (c['name'], got, want)
    BITS['plan against the case\'s roads'] = BITS.get('plan against the case\'s roads', 0) + 1


def _case_of(table, name):
    return next(c for c in table if c['name'] == name)


# ------------------------------------------------------------------------------------------------------------------ support product
def launch_mm(dev, c, i=None):
    i = i or Q.inputs(c['B'], c['S'], c['n'], c['F'], act_cols=c['acols'])
    B, S, n = c['B'], c['S'], c['n']
    img = _image(dev, B, S, n, c['KP'], 1 if c['form'] == 'a' else 0)
    act = _in(i['act'], c['lda'], dev, c['alead'], _tail(c))
    out = _Out(dev, B * n, c['width'], c['ldo'], c['off4'])
    _plan(Q.MM, c, _p(act, c['alead']), out.ptr())
    rc = G.lib().gml_dense_support_mm(img.ptr(), _p(act, c['alead']), c['lda'], c['sa'], out.ptr(), c['ldo'], c['so'], c['sum_s'], B, S, n,
                                      c['KP'], c['F'], _st(dev))
    assert _done(rc) == OK, (c['name'], rc)
    return out


def run_mm(dev, c):
    key = ('mm', c['name'])
    if key in _VALS:
        return _VALS[key]
    i = Q.inputs(c['B'], c['S'], c['n'], c['F'], act_cols=c['acols'])
    out = launch_mm(dev, c, i)
    D = i['D'].transpose(0, 1, 3, 2) if c['form'] == 'a' else i['D']
    ref, written = Q.support_mm_ref(D, i['act'], c['sa'], c['so'], c['sum_s'], c['F'])
    kern = 'support_mm_sum' if c['sum_s'] else 'support_mm'
    roads = (c['road_in'], c['road_out'])
    _hold(out, ref, 'support_mm ' + c['name'], (kern, _coarse(*roads), 'out'), written)
    _ran(kern, Q.nft_of(c['F']), '-', roads, ('in', 'out'))
    v = _vals(out)
    _bit('two launches', v[:, written], _vals(launch_mm(dev, c, i))[:, written], 'support_mm ' + c['name'])
    _VALS[key] = v[:, written]
    return _VALS[key]


@pytest.mark.parametrize('c', Q.MM_CASES, ids=lambda c: c['name'])
def test_support_mm(dev, c):
    v = run_mm(dev, c)
    if c['same']:
        _bit('road or KP against its twin', v, run_mm(dev, _case_of(Q.MM_CASES, c['same'])), 'support_mm %s vs %s' % (c['name'], c['same']))


# ------------------------------------------------------------------------------------------------------------------ chained forward
def _wimg(dev, w, S, Fin, Fout, transposed):
    L = G.lib()
    elems = int((L.gml_dense_wimgt_elems if transposed else L.gml_dense_wimg_elems)(S, Fin, Fout))
    img = _Words(dev, elems)
    wd = _up(w, dev)
    assert _done((L.gml_dense_pack_wt if transposed else L.gml_dense_pack_w)(_p(wd), img.ptr(), S, Fin, Fout, _st(dev))) == OK
    img.inside('weight image S=%d Fin=%d Fout=%d' % (S, Fin, Fout))
    return img


def launch_cf(dev, c, i, x, wimg, bias, with_h):
    B, S, n, Fin, Fout = c['B'], c['S'], c['n'], c['Fin'], c['Fout']
    out2 = _Out(dev, B * n, Fout, c['ldo2'], c['off4'])
    hcat = _Out(dev, B * n, S * Fin, S * Fin, c['hoff4']) if with_h else None
    _plan(Q.CF, c, _p(x, c['xlead']), hcat.ptr() if with_h else None, out2.ptr(), with_h)
    rc = G.lib().gml_dense_conv_fwd(_image(dev, B, S, n, c['KP'], 0).ptr(), _p(x, c['xlead']), c['ldx'], wimg.ptr(), _p(bias), out2.ptr(),
                                    c['ldo2'], hcat.ptr() if with_h else None, B, S, n, c['KP'], Fin, Fout, 1 if c['relu'] else 0, _st(dev))
    assert _done(rc) == OK, (c['name'], rc)
    return out2, hcat


def run_cf(dev, c):
    key = ('cf', c['name'])
    if key in _VALS:
        return _VALS[key]
    B, S, n, Fin, Fout = c['B'], c['S'], c['n'], c['Fin'], c['Fout']
    i = Q.inputs(B, S, n, Fin, Fout)
    x = _in(i['x'], c['ldx'], dev, c['xlead'], _tail(c))
    wimg = _wimg(dev, i['w'], S, Fin, Fout, False)
    bias = _vec(i['bias'], dev) if c['bias'] else None
    ref = Q.conv_fwd_ref(i['D'], i['x'], i['w'], i['bias'] if c['bias'] else None, c['relu'])
    what = 'conv_fwd ' + c['name']
    o_h, hcat = launch_cf(dev, c, i, x, wimg, bias, True)
    o_n, _ = launch_cf(dev, c, i, x, wimg, bias, False)
    nft, no = Q.nft_of(Fin), Q.not_of(Fout)
    _hold(o_h, ref['out2'], what + ' (hcat)', ('conv_fwd_hcat', _coarse(c['road_x'], c['road_h'], c['road_o']), 'out2'))
    _hold(o_n, ref['out2'], what, ('conv_fwd', _coarse(c['road_x'], c['road_o']), 'out2'))
    _hold(hcat, ref['hcat'], what + ' hcat', ('conv_fwd_hcat', _coarse(c['road_x'], c['road_h'], c['road_o']), 'hcat'))
    _ran('conv_fwd_hcat', nft, no, (c['road_x'], c['road_h'], c['road_o']), ('x', 'hcat', 'out2'))
    _ran('conv_fwd', nft, no, (c['road_x'], c['road_o']), ('x', 'out2'))
    v = _vals(o_h)
    _bit('out2 with and without hcat', v, _vals(o_n), what)
    _bit('two launches', v, _vals(launch_cf(dev, c, i, x, wimg, bias, False)[0]), what)
    if c['relu']:                                            # a zero the activation selects is +0.0; elements near zero may fall either side
        off = (ref['pre'] < 0) & ~ref['near']
        assert off.any() and (v.view(np.int32)[off] == 0).all(), what + ': a deselected element is not +0.0'
        on = (ref['pre'] > 0) & ~ref['near']
        assert (v[on] > 0).all(), what + ': a selected element is not positive'
    # hcat is, bit for bit, what gml_dense_support_mm(sum_s = 0) writes for the same inputs
    mm = _Out(dev, B * n, S * Fin, S * Fin)
    rc = G.lib().gml_dense_support_mm(_image(dev, B, S, n, c['KP'], 0).ptr(), _p(x, c['xlead']), c['ldx'], 0, mm.ptr(), S * Fin, Fin, 0, B, S, n,
                                      c['KP'], Fin, _st(dev))
    assert _done(rc) == OK
    _bit('hcat against gml_dense_support_mm', _vals(hcat), _vals(mm), what)
    _VALS[key] = v
    return v


@pytest.mark.parametrize('c', Q.CF_CASES, ids=lambda c: c['name'])
def test_conv_fwd(dev, c):
    v = run_cf(dev, c)
    if c['same']:
        _bit('road or KP against its twin', v, run_cf(dev, _case_of(Q.CF_CASES, c['same'])), 'conv_fwd %s vs %s' % (c['name'], c['same']))


# ------------------------------------------------------------------------------------------------------------------ chained backward, dx
def run_bx(dev, c):
    key = ('bx', c['name'])
    if key in _VALS:
        return _VALS[key]
    B, S, n, Fin, Fout = c['B'], c['S'], c['n'], c['Fin'], c['Fout']
    i = Q.inputs(B, S, n, Fin, Fout)
    g = _in(i['g'], c['ldg'], dev, 0, _tail(c))
    wimgT = _wimg(dev, i['w'], S, Fin, Fout, True)
    img = _image(dev, B, S, n, c['KP'], 1)

    def launch():
        dx = _Out(dev, B * n, Fin, c['lddx'], c['off4'])
        _plan(Q.BX, c, None, dx.ptr())
        rc = G.lib().gml_dense_conv_bwd_x(img.ptr(), _p(g), c['ldg'], wimgT.ptr(), dx.ptr(), c['lddx'], B, S, n, c['KP'], Fin, Fout,
                                          _st(dev))
        assert _done(rc) == OK, (c['name'], rc)
        return dx
    dx = launch()
    what = 'conv_bwd_x ' + c['name']
    _hold(dx, Q.conv_bwd_x_ref(i['D'], i['g'], i['w']), what, ('conv_bwd_x', _coarse(c['road_o']), 'dx'))
    _ran('conv_bwd_x', Q.nft_of(Fin), Q.not_of(Fout), (c['road_o'],), ('dx',))
    v = _vals(dx)
    _bit('two launches', v, _vals(launch()), what)
    _VALS[key] = v
    return v


@pytest.mark.parametrize('c', Q.BX_CASES, ids=lambda c: c['name'])
def test_conv_bwd_x(dev, c):
    v = run_bx(dev, c)
    if c['same']:
        _bit('road or KP against its twin', v, run_bx(dev, _case_of(Q.BX_CASES, c['same'])), 'conv_bwd_x %s vs %s' % (c['name'], c['same']))


# ------------------------------------------------------------------------------------------------------------------ weight gradient
def run_bw(dev, c):
    key = ('bw', c['name'])
    if key in _VALS:
        return _VALS[key]
    L = G.lib()
    B, S, n, Fin, Fout = c['B'], c['S'], c['n'], c['Fin'], c['Fout']
    i = Q.inputs(B, S, n, Fin, Fout)
    x = _in(i['x'], c['ldx'], dev, c['xlead'], _tail(c))
    g = _in(i['g'], c['ldg'], dev)
    img = _image(dev, B, S, n, c['KP'], 0)
    slices = int(L.gml_dense_dw_slices(B))
    nw = S * Fin * Fout
    nbytes = int(L.gml_dense_dw_workspace_bytes(B, S, Fin, Fout))
    assert slices == Q.dw_slices(B) and nbytes == 4 * slices * nw

    def launch(with_dw):
        ws = _flat(dev, slices * nw)
        assert ws.t.data_ptr() % 16 == 0
        dw = _Out(dev, S * Fin, Fout, Fout) if with_dw else None
        _plan(Q.BW, c, _p(x, c['xlead']))
        rc = L.gml_dense_conv_bwd_w(img.ptr(), _p(x, c['xlead']), c['ldx'], _p(g), c['ldg'], dw.ptr() if with_dw else None, B, S, n, c['KP'], Fin,
                                    Fout, ws.ptr(), nbytes, _st(dev))
        assert _done(rc) == OK, (c['name'], rc)
        return ws, dw
    ws, dw = launch(True)
    ref = Q.conv_bwd_w_ref(i['D'], i['x'], i['g'])
    what = 'conv_bwd_w ' + c['name']
    road = _coarse(c['road_x'])
    _hold(dw, Ref2(ref['dw']), what, ('conv_bwd_w', road, 'dw'))
    _written(ws, slices * nw, np.ones(slices * nw, bool), what)
    P = ref['partials']
    e = R.check(ws.get(), P.v.reshape(1, -1), P.t.reshape(1, -1), 1, slices * nw, slices * nw + 16, TOL, what + ' partials', 0)
    _note('conv_bwd_w', road, 'partials', e)
    used = -(-B // ref['per'])
    part = R.split(ws.get(), 1, slices * nw, slices * nw + 16, 0)[0].reshape(slices, nw)
    assert (part[used:].view(np.int32) == 0).all(), what + ': a slice without a graph is not +0.0'
    if used < slices:
        BITS['empty slices held at +0.0'] = BITS.get('empty slices held at +0.0', 0) + slices - used
    _ran('conv_bwd_w', Q.nft_of(Fin), -(-Fout // 64), (c['road_x'],), ('x',))
    v = _vals(dw)
    ws2, dw2 = launch(True)
    _bit('two launches', v, _vals(dw2), what)
    # dw == NULL: the partials stay, in the same layout, and gml_fold_many on them gives the folding call's dw bit for bit
    ws3, _ = launch(False)
    _bit('partials with and without the fold', part, R.split(ws3.get(), 1, slices * nw, slices * nw + 16, 0)[0].reshape(slices, nw), what)
    out = _Out(dev, S * Fin, Fout, Fout)
    job = G.FoldJob()
    job.partial, job.nparts, job.n = ws3.ptr().value, slices, nw
    job.dst[0], job.ndst[0] = out.ptr().value, nw
    assert _done(L.gml_fold_many(ctypes.addressof(job), 1, _st(dev))) == OK
    _bit('gml_fold_many on the partials against the folding call', _vals(out), v, what)
    _VALS[key] = v
    return v


def Ref2(r):
    """a [S, Fin, Fout] reference as the [S Fin, Fout] matrix the output buffer is"""
    return R.Ref(r.v.reshape(-1, r.v.shape[-1]), r.t.reshape(-1, r.t.shape[-1]), r.n)


@pytest.mark.parametrize('c', Q.BW_CASES, ids=lambda c: c['name'])
def test_conv_bwd_w(dev, c):
    v = run_bw(dev, c)
    if c['same']:
        _bit('road or KP against its twin', v, run_bw(dev, _case_of(Q.BW_CASES, c['same'])), 'conv_bwd_w %s vs %s' % (c['name'], c['same']))


def test_conv_bwd_w_no_graphs_and_short_workspace(dev):
    """B = 0 with dw zero-fills it and needs no workspace; a workspace one byte short, or NULL, answers GML_E_WORKSPACE and writes
    nothing"""
    L = G.lib()
    c = _case_of(Q.BW_CASES, 'base')
    B, S, n, Fin, Fout = c['B'], c['S'], c['n'], c['Fin'], c['Fout']
    i = Q.inputs(B, S, n, Fin, Fout)
    x, g, img = _in(i['x'], c['ldx'], dev), _in(i['g'], c['ldg'], dev), _image(dev, B, S, n, c['KP'], 0)
    nw, nbytes = S * Fin * Fout, int(L.gml_dense_dw_workspace_bytes(B, S, Fin, Fout))
    assert int(L.gml_dense_dw_workspace_bytes(0, S, Fin, Fout)) == 0
    dw = _Out(dev, S * Fin, Fout, Fout)
    assert _done(L.gml_dense_conv_bwd_w(img.ptr(), _p(x), c['ldx'], _p(g), c['ldg'], dw.ptr(), 0, S, n, c['KP'], Fin, Fout, None, 0, _st(dev))) == OK
    got, guards = R.split(dw.get(), S * Fin, Fout, Fout)
    assert (got.view(np.int32) == 0).all() and (guards == R.SENTINEL).all()
    assert _done(L.gml_dense_conv_bwd_w(img.ptr(), _p(x), c['ldx'], _p(g), c['ldg'], None, 0, S, n, c['KP'], Fin, Fout, None, 0, _st(dev))) == OK
    ws, dw = _flat(dev, 2 * nw), _Out(dev, S * Fin, Fout, Fout)
    for wsp, nb in ((ws.ptr(), nbytes - 1), (None, nbytes), (None, 0)):
        assert _done(L.gml_dense_conv_bwd_w(img.ptr(), _p(x), c['ldx'], _p(g), c['ldg'], dw.ptr(), B, S, n, c['KP'], Fin, Fout, wsp, nb, _st(dev))) == WSP
        assert ws.unchanged() and dw.unchanged()


# ------------------------------------------------------------------------------------------------------------------ the packers
@pytest.mark.parametrize('n,KP,nblocks', ((1, 32, 3), (15, 32, 2), (16, 32, 1), (17, 64, 2), (17, 96, 1), (32, 32, 2), (33, 96, 2), (64, 64, 1),
                                          (65, 96, 1), (75, 96, 2), (96, 96, 1)))
def test_pack_is_bit_exact(dev, n, KP, nblocks):
    L = G.lib()
    b = Q.pack_blocks(nblocks, n)
    src = _up(np.concatenate([b.ravel(), np.array([R.SENTINEL] * 8, np.int32).view(np.float32)]), dev)
    for tr in (0, 1):
        img = _Words(dev, nblocks * 2 * n * KP)
        assert _done(L.gml_dense_pack(_p(src), img.ptr(), nblocks, n, KP, tr, _st(dev))) == OK
        got, want = img.inside('pack'), Q.pack_ref(b, KP, tr).ravel()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, 'pack n=%d KP=%d transpose=%d: %d words differ, first at %d: got %#x want %#x' % (
            n, KP, tr, bad.size, bad[0], got[bad[0]], want[bad[0]])
        BITS['gml_dense_pack against the reference'] = BITS.get('gml_dense_pack against the reference', 0) + 1
    empty = _Words(dev, 64)
    assert _done(L.gml_dense_pack(_p(src), empty.ptr(), 0, n, KP, 0, _st(dev))) == OK and empty.unchanged()


def test_pack_beyond_the_grid_cap(dev):
    """the smallest nblocks at n = KP = 96 whose elements exceed the 64 GML_NUM_CU workgroups of 256 threads: the grid-stride loop runs
    a second time"""
    L = G.lib()
    n = KP = 96
    cap = 64 * Q.NUM_CU * 256
    nblocks = cap // (n * KP) + 1
    assert (nblocks - 1) * n * KP <= cap < nblocks * n * KP and nblocks == 456
    b = Q.pack_blocks(nblocks, n)
    src = _up(b, dev)
    img = _Words(dev, nblocks * 2 * n * KP)
    assert _done(L.gml_dense_pack(_p(src), img.ptr(), nblocks, n, KP, 1, _st(dev))) == OK
    assert np.array_equal(img.inside('pack'), Q.pack_ref(b, KP, 1).ravel())
    RAN.add(('pack', 'grid-stride'))


@pytest.mark.parametrize('S,Fin,Fout', ((1, 1, 1), (3, 16, 64), (1, 16, 65), (2, 32, 64), (2, 17, 65), (2, 33, 128), (1, 64, 63), (2, 65, 4), (1, 80, 128), (2, 96, 64), (1, 97, 65),
                                        (3, 128, 128)))
def test_weight_packers_fill_exactly_the_queried_size(dev, S, Fin, Fout):
    """the fragment order is private to the kernels and held through the consumers; here: the queried size is the one the kernels
    address (S x K steps x output tiles x (hi, lo) x 64 lanes x 8), every word of it is written (two fills of different sentinels
    agree on every word) and none behind, and packing is repeatable"""
    L = G.lib()
    w = _up(_f32(_rng('w', S, Fin, Fout).standard_normal((S, Fin, Fout))), dev)
    nft, no = Q.nft_of(Fin), Q.not_of(Fout)
    for tr, query, pack, want in ((False, L.gml_dense_wimg_elems, L.gml_dense_pack_w, S * ((nft + 1) // 2) * no * 2 * 64 * 8),
                                  (True, L.gml_dense_wimgt_elems, L.gml_dense_pack_wt, S * nft * (no // 2) * 2 * 64 * 8)):
        elems = int(query(S, Fin, Fout))
        assert elems == want, ('the query disagrees with the template the launcher runs', tr, elems, want)
        a, b = _Words(dev, elems, 0xA5A5), _Words(dev, elems, 0x5A5A)
        for img in (a, b):
            assert _done(pack(_p(w), img.ptr(), S, Fin, Fout, _st(dev))) == OK
        assert np.array_equal(a.inside('weight image'), b.inside('weight image')), 'a word of the weight image is never written'
    RAN.add(('pack_w', nft, no))


# ------------------------------------------------------------------------------------------------------------------ gml_xty_wide
@pytest.mark.parametrize('c', Q.XW_CASES, ids=lambda c: c['name'])
def test_xty_wide_at_the_queried_size(dev, c):
    L = G.lib()
    A, Bm = Q.xw_inputs(c)
    n, a, b = c['n'], c['a'], c['b']
    assert L.gml_xty_wide_supported(n, a, b) == 1
    nbytes = int(L.gml_xty_wide_workspace_bytes(n, a, b))
    assert nbytes > 0 and nbytes % (4 * a * b) == 0
    Ad, Bd = _in(A, c['lda'], dev), _in(Bm, c['ldb'], dev)

    def launch():
        ws, out = _flat(dev, nbytes // 4), _Out(dev, a, b, b)
        assert _done(L.gml_xty_wide(_p(Ad), c['lda'], _p(Bd), c['ldb'], out.ptr(), n, a, b, ws.ptr(), nbytes, _st(dev))) == OK
        return ws, out
    ws, out = launch()
    _written(ws, nbytes // 4, np.ones(nbytes // 4, bool), 'xty_wide ' + c['name'])
    _hold(out, Q.xty_ref(A, Bm), 'xty_wide ' + c['name'], ('xty_wide', ('-',), 'out'))
    _bit('two launches', _vals(out), _vals(launch()[1]), 'xty_wide ' + c['name'])
    RAN.add(('xty_wide', c['name']))


def test_xty_wide_error_answers(dev):
    L = G.lib()
    c = Q.XW_CASES[0]
    A, Bm = Q.xw_inputs(c)
    n, a, b = c['n'], c['a'], c['b']
    Ad, Bd = _in(A, c['lda'], dev), _in(Bm, c['ldb'], dev)
    nbytes = int(L.gml_xty_wide_workspace_bytes(n, a, b))
    ws, out = _flat(dev, nbytes // 4), _Out(dev, a, b, b)
    base = dict(A=_p(Ad), lda=c['lda'], B=_p(Bd), ldb=c['ldb'], out=out.ptr(), n=n, a=a, b=b, ws=ws.ptr(), nb=nbytes)

    def call(**kw):
        k = dict(base, **kw)
        return _done(L.gml_xty_wide(k['A'], k['lda'], k['B'], k['ldb'], k['out'], k['n'], k['a'], k['b'], k['ws'], k['nb'], _st(dev)))
    for kw, want in ((dict(a=0), UNS), (dict(a=4097, lda=4100), UNS), (dict(b=0), UNS), (dict(b=129, ldb=132), UNS), (dict(n=-1), UNS),
                     (dict(out=None), BAD), (dict(lda=a - 1), BAD), (dict(ldb=b - 1), BAD), (dict(A=None), BAD), (dict(B=None), BAD),
                     (dict(ws=None), WSP), (dict(nb=nbytes - 1), WSP), (dict(nb=0), WSP),
                     (dict(a=4097, out=None), UNS)):                             # the shape is looked at first (include/gml.h)
        assert call(**kw) == want, (kw, want)
        assert ws.unchanged() and out.unchanged(), kw
    for kw in (dict(a=0), dict(b=129), dict(n=-1)):
        k = dict(base, **kw)
        assert L.gml_xty_wide_supported(k['n'], k['a'], k['b']) == 0 and L.gml_xty_wide_workspace_bytes(k['n'], k['a'], k['b']) == 0
    # no rows: out is zero-filled, nothing else is touched and nothing else is needed
    assert L.gml_xty_wide_workspace_bytes(0, a, b) == 0
    assert call(n=0, A=None, B=None, ws=None, nb=0) == OK
    got, guards = R.split(out.get(), a, b, b)
    assert (got.view(np.int32) == 0).all() and (guards == R.SENTINEL).all() and ws.unchanged()


# ------------------------------------------------------------------------------------------------------------------ error answers
def _answers(call, base, outs, variants):
    for kw, want in variants:
        assert call(**dict(base, **kw)) == want, (kw, want)
        for o in outs:
            assert o.unchanged(), ('written after an error answer', kw)


_SHAPE_ERRORS = ((dict(n=0), UNS), (dict(n=97, KP=128), UNS), (dict(n=97, KP=96), UNS), (dict(KP=48), UNS), (dict(KP=16), UNS), (dict(KP=128), UNS),
                 (dict(KP=32), UNS), (dict(KP=0), UNS), (dict(S=0), UNS), (dict(B=-1), UNS), (dict(B=0), OK))


def test_pack_error_answers(dev):
    L = G.lib()
    src, img = _up(Q.pack_blocks(2, 17), dev), _Words(dev, 2 * 2 * 17 * 32)
    base = dict(src=_p(src), img=img.ptr(), nb=2, n=17, KP=32, tr=0)
    call = lambda **k: _done(L.gml_dense_pack(k['src'], k['img'], k['nb'], k['n'], k['KP'], k['tr'], _st(dev)))
    _answers(call, base, (img,), ((dict(src=None), BAD), (dict(img=None), BAD), (dict(n=0), UNS), (dict(n=97, KP=128), UNS), (dict(KP=48), UNS),
                                  (dict(KP=16), UNS), (dict(KP=128), UNS), (dict(n=33), UNS), (dict(nb=-1), UNS), (dict(nb=0), OK),
                                  (dict(src=None, n=0), BAD)))            # NULL is looked at first (include/gml.h)
    w, wi = _up(_f32(np.ones((2, 16, 16))), dev), _Words(dev, int(L.gml_dense_wimg_elems(2, 16, 16)))
    for pack in (L.gml_dense_pack_w, L.gml_dense_pack_wt):
        base = dict(w=_p(w), img=wi.ptr(), S=2, Fin=16, Fout=16)
        call = lambda **k: _done(pack(k['w'], k['img'], k['S'], k['Fin'], k['Fout'], _st(dev)))
        _answers(call, base, (wi,), ((dict(w=None), BAD), (dict(img=None), BAD), (dict(S=0), UNS), (dict(Fin=0), UNS), (dict(Fin=129), UNS),
                                     (dict(Fout=0), UNS), (dict(Fout=129), UNS), (dict(w=None, S=0), BAD)))


def test_support_mm_error_answers(dev):
    L = G.lib()
    c = _case_of(Q.MM_CASES, 'f-n33-F32')
    i = Q.inputs(c['B'], c['S'], c['n'], c['F'], act_cols=c['acols'])
    act, out = _in(i['act'], c['lda'], dev), _Out(dev, c['B'] * c['n'], c['width'], c['ldo'])
    base = dict(img=_image(dev, c['B'], c['S'], c['n'], c['KP'], 0).ptr(), act=_p(act), lda=c['lda'], sa=0, out=out.ptr(), ldo=c['ldo'], so=c['so'],
                sum_s=0, B=c['B'], S=c['S'], n=c['n'], KP=c['KP'], F=c['F'])
    call = lambda **k: _done(L.gml_dense_support_mm(k['img'], k['act'], k['lda'], k['sa'], k['out'], k['ldo'], k['so'], k['sum_s'], k['B'], k['S'],
                                                    k['n'], k['KP'], k['F'], _st(dev)))
    _answers(call, base, (out,), ((dict(img=None), BAD), (dict(act=None), BAD), (dict(out=None), BAD), (dict(lda=c['F'] - 1), BAD),
                                  (dict(ldo=c['F'] - 1), BAD), (dict(ldo=c['width'] - 1), BAD),
                                  (dict(sa=c['F'], lda=3 * c['F'] - 1), BAD), (dict(sa=-1), BAD), (dict(so=-1), BAD), (dict(F=0), UNS), (dict(F=129, lda=132, ldo=196), UNS),
                                  (dict(F=129), BAD)) + _SHAPE_ERRORS)      # a short ld is looked at before the range (include/gml.h)


def test_conv_fwd_error_answers(dev):
    L = G.lib()
    c = _case_of(Q.CF_CASES, 'base')
    B, S, n, Fin, Fout = c['B'], c['S'], c['n'], c['Fin'], c['Fout']
    i = Q.inputs(B, S, n, Fin, Fout)
    x, wimg, bias = _in(i['x'], c['ldx'], dev), _wimg(dev, i['w'], S, Fin, Fout, False), _vec(i['bias'], dev)
    out2, hcat = _Out(dev, B * n, Fout, c['ldo2']), _Out(dev, B * n, S * Fin, S * Fin)
    base = dict(img=_image(dev, B, S, n, c['KP'], 0).ptr(), x=_p(x), ldx=c['ldx'], w=wimg.ptr(), bias=_p(bias), out2=out2.ptr(), ldo2=c['ldo2'],
                hcat=hcat.ptr(), B=B, S=S, n=n, KP=c['KP'], Fin=Fin, Fout=Fout)
    call = lambda **k: _done(L.gml_dense_conv_fwd(k['img'], k['x'], k['ldx'], k['w'], k['bias'], k['out2'], k['ldo2'], k['hcat'], k['B'], k['S'], k['n'],
                                                  k['KP'], k['Fin'], k['Fout'], 0, _st(dev)))
    _answers(call, base, (out2, hcat), ((dict(img=None), BAD), (dict(x=None), BAD), (dict(w=None), BAD), (dict(out2=None), BAD),
                                        (dict(ldx=Fin - 1), BAD), (dict(ldo2=Fout - 1), BAD), (dict(Fin=0), UNS), (dict(Fin=129, ldx=132), UNS),
                                        (dict(Fout=0), UNS), (dict(Fout=129, ldo2=132), UNS), (dict(Fout=129), BAD)) + _SHAPE_ERRORS)


def test_conv_bwd_x_error_answers(dev):
    L = G.lib()
    c = _case_of(Q.BX_CASES, 'base')
    B, S, n, Fin, Fout = c['B'], c['S'], c['n'], c['Fin'], c['Fout']
    i = Q.inputs(B, S, n, Fin, Fout)
    g, wimgT, dx = _in(i['g'], c['ldg'], dev), _wimg(dev, i['w'], S, Fin, Fout, True), _Out(dev, B * n, Fin, c['lddx'])
    base = dict(img=_image(dev, B, S, n, c['KP'], 1).ptr(), g=_p(g), ldg=c['ldg'], w=wimgT.ptr(), dx=dx.ptr(), lddx=c['lddx'], B=B, S=S, n=n,
                KP=c['KP'], Fin=Fin, Fout=Fout)
    call = lambda **k: _done(L.gml_dense_conv_bwd_x(k['img'], k['g'], k['ldg'], k['w'], k['dx'], k['lddx'], k['B'], k['S'], k['n'], k['KP'], k['Fin'],
                                                    k['Fout'], _st(dev)))
    _answers(call, base, (dx,), ((dict(img=None), BAD), (dict(g=None), BAD), (dict(w=None), BAD), (dict(dx=None), BAD), (dict(ldg=Fout - 1), BAD),
                                 (dict(lddx=Fin - 1), BAD), (dict(Fin=0), UNS), (dict(Fin=129, lddx=132), UNS), (dict(Fout=0), UNS),
                                 (dict(Fout=129, ldg=132), UNS), (dict(Fin=129), BAD)) + _SHAPE_ERRORS)


def test_conv_bwd_w_error_answers(dev):
    L = G.lib()
    c = _case_of(Q.BW_CASES, 'base')
    B, S, n, Fin, Fout = c['B'], c['S'], c['n'], c['Fin'], c['Fout']
    i = Q.inputs(B, S, n, Fin, Fout)
    x, g = _in(i['x'], c['ldx'], dev), _in(i['g'], c['ldg'], dev)
    nbytes = int(L.gml_dense_dw_workspace_bytes(B, S, Fin, Fout))
    ws, dw = _flat(dev, nbytes // 4), _Out(dev, S * Fin, Fout, Fout)
    base = dict(img=_image(dev, B, S, n, c['KP'], 0).ptr(), x=_p(x), ldx=c['ldx'], g=_p(g), ldg=c['ldg'], dw=dw.ptr(), B=B, S=S, n=n, KP=c['KP'],
                Fin=Fin, Fout=Fout, ws=ws.ptr(), nb=nbytes)
    call = lambda **k: _done(L.gml_dense_conv_bwd_w(k['img'], k['x'], k['ldx'], k['g'], k['ldg'], k['dw'], k['B'], k['S'], k['n'], k['KP'], k['Fin'],
                                                    k['Fout'], k['ws'], k['nb'], _st(dev)))
    shape = tuple(v for v in _SHAPE_ERRORS if v[0] != dict(B=0))              # (B = 0 zero-fills dw: its own test)
    _answers(call, base, (dw, ws), ((dict(img=None), BAD), (dict(x=None), BAD), (dict(g=None), BAD), (dict(ldx=Fin - 1), BAD),
                                    (dict(ldg=Fout - 1), BAD), (dict(Fin=0), UNS), (dict(Fin=129, ldx=132), UNS), (dict(Fout=0), UNS),
                                    (dict(Fout=16321, ldg=16324), UNS), (dict(Fout=16384, ldg=16384), UNS), (dict(Fout=16385, ldg=16388), UNS),
                                    (dict(Fin=129), BAD), (dict(ws=None), WSP), (dict(nb=nbytes - 1), WSP)) + shape)
    for q in ((0, S, Fin, Fout), (B, 0, Fin, Fout), (B, S, 0, Fout), (B, S, Fin, 0), (-1, S, Fin, Fout)):
        assert L.gml_dense_dw_workspace_bytes(*q) == 0
    assert [int(L.gml_dense_dw_slices(b)) for b in (-1, 0, 1, 2, 63, 64, 65, 129, 4096)] == [1, 1, 1, 2, 63, 64, 64, 64, 64]


# ------------------------------------------------------------------------------------------------------------------ the report
def test_every_road_ran_and_worst_figures_report():
    """LAST: every (kernel, template, road) and every single road condition of the tables at the top ran; prints the table DESIGN.md
    s4.7a records (pytest -rP)"""
    missing = sorted(TEMPLATES - RAN, key=repr)
    assert not missing, 'templates / roads of the table that never ran: %r' % (missing,)
    missing = sorted(CONDITIONS - COND_RAN, key=repr)
    assert not missing, 'road conditions that never ran on their own: %r' % (missing,)
    assert ('pack', 'grid-stride') in RAN and {r[1:] for r in RAN if r[0] == 'pack_w'} >= {(a, b) for a in (1, 2, 4, 8) for b in (4, 8)}
    assert {r[1] for r in RAN if r[0] == 'xty_wide'} == {c['name'] for c in Q.XW_CASES}
    print('kernel           NFT NOT  road')
    for r in sorted((r for r in RAN if len(r) == 4), key=repr):
        print('%-16s %3s %3s  %s' % (r[0], r[1], r[2], '/'.join(r[3])))
    print('road conditions on their own: ' + ', '.join('%s %s %s' % r for r in sorted(COND_RAN)))
    print('%-16s %-22s %-9s %5s  %-10s %-10s' % ('kernel', 'road', 'output', 'cases', 'max-norm', 'term sum'))
    for k in sorted(WORST):
        w = WORST[k]
        assert w[1] <= TOL and w[2] <= TOL
        print('%-16s %-22s %-9s %5d  %.3e  %.3e' % (k[0], k[1], k[2], w[0], w[1], w[2]))
    for k in sorted(BITS):
        print('bit for bit: %-60s %4d' % (k, BITS[k]))
