"""The readout side at the level of its C ABI (include/gml.h): the heads with their losses -- gml_head_l1_fwd / _fwd_acc / _bwd (one
workgroup), gml_head_l1_big_workspace_floats / _big_fwd / _big_bwd (any rows), gml_head_bce_workspace_floats / _fwd / _bwd --, the node
head gml_node_head_fwd / _bwd, and BatchNorm: gml_bn_workspace_bytes / _stats / _apply / _bwd_sums / _bwd_apply and
gml_bn_masked_workspace_bytes / _stats / _apply / _bwd_sums / _bwd_apply / _running_update.  22 entry points, each called by name
through _lib.lib() against the float64 restatement of tests/_readout_ref.py: one launch and one numpy reference per case, so that a
case decides what functional.py and models.py never vary -- widths other than 32, a leading dimension beyond the width, NULL
optionals, rows_loss = 0, the LDS edge where the forward is served and the backward is not, the grid cap and the first row past it,
the layout of the partials left in a workspace of the exact size, a column slice of a wider buffer, the 2048-row block boundary,
every legal BatchNorm width, blocks without a valid row, and the error answers.

Every output sits in a buffer of _conv_ref.alloc(): 8 guard rows behind it, and the columns between its width and its leading
dimension, hold a NaN sentinel and must still hold it; scalars sit in a one-row buffer with sentinel floats behind them.  Every
workspace is passed at exactly the size its query returns, 16-byte aligned, with 16 sentinel floats behind: every float the launch
is documented to write was written, none behind.  Inputs carry 8 readable rows behind the last row and finite junk (7.0) in their
padding columns -- the heads READ the rows >= rows_loss (gml.h), so they hold finite junk too; masked BatchNorm's invalid rows hold
the NaN sentinel, and no NaN may reach an output.  After an error answer every output is bit-unchanged.  No pointer that a launcher
does not check is ever misaligned: a case exists to be answered.

Values: _readout_ref.hold() -- TOL_F32 = 2e-5 on the max-norm AND on each element's own term sum; the sums (loss, dw*, db*, the
column sums, var) also within _conv_ref.f32_bound; selects bit-exact (+0.0); the BCE head at the 1e-4 of tests/test_gpu_exp_classify.py
(exp / log1p are the device library's), ok and n as integers.  Two departures, both derived in _readout_ref.py and shown on the CPU:
dx of BatchNorm over exactly two rows is zero but for eps and is held on its term sums only (bn_dx_bar); a single valid row sits
on multiples of 1/8 so that var is exactly 0 (bn_inputs).  tests/test_readout_ref_cpu.py shows that plain fp32 meets every figure on
the same arrays.

The worst figures per (kernel, road, output) are printed by the last test (pytest -rP) and recorded in DESIGN.md s4.4b.  That test
reads what the tests before it recorded in this module: run the file whole -- under -k or --lf it reports roads as "not run" that
merely were not selected."""
import ctypes

import numpy as np
import pytest
import torch

import _conv_ref as R
import _readout_ref as Q
from gnn_matlang_amd import _lib as G
from test_gpu_conv_fwd_abi import _Out, _done, _f32, _p, _rng, _up

pytestmark = pytest.mark.gpu

OK, BAD, UNS, WSP = G.GML_OK, G.GML_E_BADARG, G.GML_E_UNSUPPORTED, G.GML_E_WORKSPACE
PAD = R.GUARD_ROWS
NPART = 32 * 32 + 32 + 32 + 1                                # HB_NPART, csrc/gml_head_big.hip:18: dw1 | db1 | dw2 | db2
CAP_ROWS = Q.SLAB * Q.NCU                                    # hb_grid :228-231, hbce_grid csrc/gml_head_bce.hip:287-290: 256 workgroups of 256 rows
WORST = {}                                                   # (kernel, road, output) -> [cases, worst max-norm, worst term-sum figure]
ROADS = set()                                                # (kernel class, road) that ran
WIDTHS = set()                                               # BatchNorm widths that ran
BITS = {'masked all valid: cases': 0, 'masked all valid: bit-equal to the unmasked kernels': 0}
COND = []                                                    # the conditioning table's lines


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    assert G.lib().gml_version() >= 1
    return torch.device('cuda:0')


def _st(dev):
    from gnn_matlang_amd.graph import _stream
    return _stream(dev)


def _note(kern, road, out, e):
    w = WORST.setdefault((kern, road, out), [0, 0.0, 0.0])
    w[0] += 1
    w[1], w[2] = max(w[1], e[0]), max(w[2], e[1])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _vals(o):
    return R.split(o.get(), o.n, o.ncols, o.ldo, o.guard_rows)[0]


def _flat(dev, n, tail=16):
    """a workspace of n floats with `tail` sentinel floats behind it"""
    return _Out(dev, 1, n, n + tail, guard_rows=0)


def _written(ws, n, idx, what):
    """of the n floats of a workspace exactly those at `idx` (a boolean mask) were written, and nothing behind the n"""
    w = ws.get().view(np.int32)
    assert (w[n:] == R.SENTINEL).all(), what + ': wrote behind the workspace'
    left = np.flatnonzero((w[:n] == R.SENTINEL) & idx)
    assert left.size == 0, '%s: %d workspace floats never written, first at %d of %d' % (what, left.size, left[0], n)
    hit = np.flatnonzero((w[:n] != R.SENTINEL) & ~idx)
    assert hit.size == 0, '%s: %d workspace floats written that are not the launch\'s, first at %d of %d' % (what, hit.size, hit[0], n)


def _wide(a, ld, rows=None, col0=0):
    """a [n, w] -> float32 [rows or n + PAD, ld] with finite junk in the padding columns and rows; col0: the first column used"""
    a = np.asarray(a, np.float32)
    a = a[:, None] if a.ndim == 1 else a
    out = np.full((a.shape[0] + PAD if rows is None else rows, ld), 7.0, np.float32)
    out[:a.shape[0], col0:col0 + a.shape[1]] = a
    return out


def _vec(a, dev, lead=0):
    """a vector input (or None) with 8 junk floats behind it"""
    return None if a is None else _up(np.concatenate([np.asarray(a, np.float32).ravel(), np.full(PAD, 7.0, np.float32)]), dev, lead)


def _hold(o, ref, what, key, tol=Q.TOL_F32, bound=None, **kw):
    e = Q.hold(o.get(), ref, o.n, o.ncols, o.ldo, what, tol=tol, bound=(key[2] in Q.SUMS and tol == Q.TOL_F32) if bound is None else bound,
               guard_rows=o.guard_rows, **kw)
    _note(key[0], key[1], key[2], e)


def _exact(o, want, what):
    got, guards = R.split(o.get(), o.n, o.ncols, o.ldo, o.guard_rows)
    assert (guards == R.SENTINEL).all(), what + ': guard words overwritten'
    want = np.asarray(want, np.float32).reshape(o.n, o.ncols)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, '%s: %d elements differ, first at %s: got %r want %r' % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def _zero_rows(o, rows, what):
    """rows of an output that are a select: bitwise +0.0"""
    got = _vals(o)
    assert (_bits(got[rows]) == 0).all(), what + ': a row outside the sum is not +0.0'


# ------------------------------------------------------------------------------------------------------------------------ the heads
class _Head(object):
    """a head case on the device: the eight operand arguments every head entry point starts with, and the outputs"""

    def __init__(self, dev, c, ref, ldp=None, ldgp=None, lead_p=0):
        self.dev, self.c, self.ref = dev, c, ref
        self.rows, self.nin = c['p'].shape
        self.nh = c['w1'].shape[0]
        self.ldp, self.ldgp = ldp or self.nin, ldgp or self.nin
        self.lead_p = lead_p
        self.p = _up(_wide(c['p'], self.ldp), dev, lead_p)
        self.y, self.valid = _vec(c['y'], dev), _vec(c['valid'], dev)
        self.w1, self.b1, self.w2, self.b2 = _up(c['w1'], dev), _vec(c['b1'], dev), _vec(c['w2'], dev), _vec(c['b2'], dev)
        self.gs = None if c['gscale'] is None else _up(np.array([c['gscale'], 7.0], np.float32), dev)
        self.Rl = c['rows_loss']

    def ops(self, **over):
        a = dict(p=_p(self.p, self.lead_p), ldp=self.ldp, y=_p(self.y), valid=_p(self.valid), w1=_p(self.w1), b1=_p(self.b1), w2=_p(self.w2),
                 b2=_p(self.b2), rows=self.rows, rows_loss=self.Rl, nin=self.nin, nh=self.nh)
        a.update({k: v for k, v in over.items() if k in a})
        return list(a.values())

    def grads(self, null=()):
        o = {'gp': _Out(self.dev, self.rows, self.nin, self.ldgp), 'dw1': _Out(self.dev, self.nh, self.nin, self.nin),
             'db1': _Out(self.dev, 1, self.nh, self.nh), 'dw2': _Out(self.dev, 1, self.nh, self.nh), 'db2': _Out(self.dev, 1, 1, 1)}
        return {k: v for k, v in o.items() if k not in null}

    def check_grads(self, o, what, kern, road, tol=Q.TOL_F32, dyadic=False):
        for k, b in o.items():
            _hold(b, self.ref[k], what + ' ' + k, (kern, road, k), tol=tol)
        _zero_rows(o['gp'], self.ref['gp_zero'], what + ' gp')
        if self.Rl == 0:
            for k, b in o.items():
                assert (_bits(_vals(b)) == 0).all(), what + ': %s is not +0.0 without a row of the loss' % k
        if dyadic and 'db2' in o:
            _exact(o['db2'], self.ref['db2'].v, what + ' db2 of the dyadic family')


def _scalar(dev, out0=None):
    return _Out(dev, 1, 1, 1, out0=None if out0 is None else np.array([[out0]], np.float32))


def _ptr(o, k):
    return o[k].ptr() if k in o else _p(None)


def run_l1(dev, rows, nin, nh, family, kw, i=0, null=(), bwd=True, acc=True):
    """gml_head_l1_fwd_acc (acc = False: gml_head_l1_fwd) and gml_head_l1_bwd on one case; i rotates ldp and ldgp"""
    c, ref = Q.l1_case(rows, nin, nh, family, **kw)
    ldp = sorted({nin, nin + 4, 64})[i % 3 % len({nin, nin + 4, 64})]
    h = _Head(dev, c, ref, ldp, (nin, nin + 4)[i % 2])
    what = 'head_l1 rows=%d %d->%d %s %s ldp=%d ldgp=%d' % (rows, nin, nh, family, kw, h.ldp, h.ldgp)
    L, st = G.lib(), _st(dev)
    loss, pre = _scalar(dev), (None if 'pre' in null else _Out(dev, rows, 1, 1))
    lsum = None if 'loss_sum' in null or not acc else _scalar(dev, 3.25)
    if acc:
        rc = _done(L.gml_head_l1_fwd_acc(*h.ops(), loss.ptr(), lsum.ptr() if lsum else _p(None), pre.ptr() if pre else _p(None), st))
    else:
        rc = _done(L.gml_head_l1_fwd(*h.ops(), loss.ptr(), pre.ptr() if pre else _p(None), st))
    assert rc == OK, what
    _hold(loss, ref['loss'], what + ' loss', ('head_l1', 'fwd', 'loss'))
    if pre:
        _hold(pre, ref['pre'], what + ' pre', ('head_l1', 'fwd', 'pre'))
        if family == 'dyadic':
            _exact(pre, ref['pre'].v, what + ' pre of the dyadic family')
    if lsum:
        _exact(lsum, np.float32(3.25) + _vals(loss), what + ': loss_sum is not its prior value + loss')
    if h.Rl == 0:
        assert _bits(_vals(loss))[0, 0] == 0, what + ': the loss without a row is not +0.0'
    out = {'loss': _bits(loss.get()).copy(), 'pre': _bits(pre.get()).copy() if pre else None}
    ROADS.add(('head_l1', 'fwd'))
    if bwd:
        o = h.grads(null)
        rc = _done(L.gml_head_l1_bwd(*h.ops(), _p(h.gs), o['gp'].ptr(), h.ldgp, o['dw1'].ptr(), _ptr(o, 'db1'), o['dw2'].ptr(), _ptr(o, 'db2'), st))
        assert rc == OK, what
        h.check_grads(o, what, 'head_l1', 'bwd', dyadic=family == 'dyadic')
        out.update({k: _bits(b.get()).copy() for k, b in o.items()})
        ROADS.add(('head_l1', 'bwd'))
    return out


@pytest.mark.parametrize('rows', Q.L1_ROWS)
def test_head_l1_shapes(dev, rows):
    """every width pair at this row count where the LDS allows, ldp in {nin, nin + 4, 64} and ldgp in {nin, nin + 4} rotating"""
    for i, (nin, nh) in enumerate(Q.L1_WIDTHS):
        if Q.l1_fwd_fits(rows, nin, nh):
            for j in (0, 1):
                run_l1(dev, rows, nin, nh, 'drawn', Q.l1_args(rows, {}), i=i + 3 * j + Q.L1_ROWS.index(rows), bwd=Q.l1_bwd_fits(rows, nin, nh))


@pytest.mark.parametrize('variant', sorted(Q.L1_VARIANTS))
def test_head_l1_variants(dev, variant):
    for rows, nin, nh in Q.L1_VARIANT_SHAPES:
        for i in range(6):
            run_l1(dev, rows, nin, nh, 'drawn', Q.l1_args(rows, Q.L1_VARIANTS[variant]), i=i)


@pytest.mark.parametrize('null', (('db1',), ('db2',), ('pre',), ('loss_sum',), ('db1', 'db2', 'pre', 'loss_sum')))
def test_head_l1_null_outputs(dev, null):
    for rows, nin, nh in Q.L1_VARIANT_SHAPES:
        a = run_l1(dev, rows, nin, nh, 'drawn', Q.l1_args(rows, {}), null=null)
        b = run_l1(dev, rows, nin, nh, 'drawn', Q.l1_args(rows, {}))
        assert all(np.array_equal(a[k], b[k]) for k in a if a[k] is not None), 'head_l1: an output changes with %s NULL' % (null,)


def test_head_l1_fwd_leaves_no_running_sum(dev):
    """gml_head_l1_fwd is gml_head_l1_fwd_acc without the accumulator: the same bits"""
    for rows, nin, nh in Q.L1_VARIANT_SHAPES:
        a = run_l1(dev, rows, nin, nh, 'drawn', Q.l1_args(rows, {}), acc=False, bwd=False)
        b = run_l1(dev, rows, nin, nh, 'drawn', Q.l1_args(rows, {}), acc=True, bwd=False)
        assert np.array_equal(a['loss'], b['loss']) and np.array_equal(a['pre'], b['pre'])


def test_head_l1_dyadic_family(dev):
    for rows, nin, nh, family, kw in Q.l1_value_cases():
        if family == 'dyadic':
            for i in range(3):
                run_l1(dev, rows, nin, nh, family, kw, i=i)


def test_head_l1_lds_edge(dev):
    """64 -> 64: the backward runs at 188 (functional.head_l1_supported's last) and 189 (its own last) and answers 190; the forward
    runs at 190 and at 256.  The largest case of each is launched twice: the same bits"""
    (r188, r189, r256) = (c[0] for c in Q.L1_EDGE)
    run_l1(dev, r188, 64, 64, 'drawn', Q.l1_args(r188, {}))
    a = run_l1(dev, r189, 64, 64, 'drawn', Q.l1_args(r189, {}), i=1)
    b = run_l1(dev, r189, 64, 64, 'drawn', Q.l1_args(r189, {}), i=1)
    assert all(np.array_equal(a[k], b[k]) for k in a), 'head_l1: two launches differ'
    a = run_l1(dev, r256, 64, 64, 'drawn', Q.l1_args(r256, {}), bwd=False)
    b = run_l1(dev, r256, 64, 64, 'drawn', Q.l1_args(r256, {}), bwd=False)
    assert np.array_equal(a['loss'], b['loss']) and np.array_equal(a['pre'], b['pre']), 'head_l1: two launches differ'
    c = Q.head_inputs(190, 64, 64, ('edge',), 189)[0]
    h = _Head(dev, c, None)
    loss, o, L, st = _scalar(dev), h.grads(), G.lib(), _st(dev)
    assert _done(L.gml_head_l1_fwd(*h.ops(), loss.ptr(), _p(None), st)) == OK and not loss.unchanged()
    rc = _done(L.gml_head_l1_bwd(*h.ops(), _p(h.gs), o['gp'].ptr(), 64, o['dw1'].ptr(), o['db1'].ptr(), o['dw2'].ptr(), o['db2'].ptr(), st))
    assert rc == UNS and all(b.unchanged() for b in o.values()), 'head_l1_bwd at 190 rows of 64 -> 64'


def test_head_l1_error_answers(dev):
    rows, nin, nh = 65, 32, 32
    c, ref = Q.l1_case(rows, nin, nh, 'drawn', **Q.l1_args(rows, {}))
    h = _Head(dev, c, ref, 36, 36)
    hoff = _Head(dev, c, ref, 36, 36, lead_p=1)               # p 4 bytes off a 16-byte boundary
    w1off, w2off = _up(c['w1'], dev, 1), _up(c['w2'], dev, 1)
    loss, lsum, pre, o = _scalar(dev), _scalar(dev, 3.25), _Out(dev, rows, 1, 1), h.grads()
    gpoff, dw1off = _Out(dev, rows, nin, 36, off4=True), _Out(dev, nh, nin, nin, off4=True)
    L, st = G.lib(), _st(dev)
    outs = [loss, lsum, pre, gpoff, dw1off] + list(o.values())

    def refused(want, why, hh=h, gp=None, ldgp=36, dw1=None, dw2=None, lossp=None, fwd=True, bwd=True, **over):
        rcs = []
        if fwd:
            rcs.append(_done(L.gml_head_l1_fwd_acc(*hh.ops(**over), loss.ptr() if lossp is None else lossp, lsum.ptr(), pre.ptr(), st)))
            rcs.append(_done(L.gml_head_l1_fwd(*hh.ops(**over), loss.ptr() if lossp is None else lossp, pre.ptr(), st)))
        if bwd:
            rcs.append(_done(L.gml_head_l1_bwd(*hh.ops(**over), _p(h.gs), o['gp'].ptr() if gp is None else gp, ldgp, o['dw1'].ptr() if dw1 is None else dw1,
                                               o['db1'].ptr(), o['dw2'].ptr() if dw2 is None else dw2, o['db2'].ptr(), st)))
        assert rcs and all(rc == want for rc in rcs), 'head_l1: %s answered %s, not %d' % (why, rcs, want)
        assert all(b.unchanged() for b in outs), 'head_l1: an output changed under the error answer for ' + why

    refused(UNS, 'rows = 257', rows=257, rows_loss=257)
    refused(UNS, 'nin = 68', nin=68, ldp=68, ldgp=68)
    refused(UNS, 'nh = 68', nh=68)
    refused(UNS, 'nin % 4', nin=30)
    refused(UNS, 'nh % 4', nh=30)
    refused(UNS, 'ldp % 4', ldp=35)
    refused(UNS, 'p off alignment', hh=hoff)
    refused(UNS, 'w1 off alignment', w1=_p(w1off, 1))
    refused(UNS, 'w2 off alignment', w2=_p(w2off, 1))
    refused(UNS, 'gp off alignment', gp=gpoff.ptr(), fwd=False)
    refused(UNS, 'dw1 off alignment', dw1=dw1off.ptr(), fwd=False)
    refused(UNS, 'ldgp % 4', ldgp=35, fwd=False)
    for k in ('p', 'y', 'w1', 'w2'):
        refused(BAD, k + ' NULL', **{k: _p(None)})
    refused(BAD, 'loss NULL', lossp=_p(None), bwd=False)
    refused(BAD, 'gp NULL', gp=_p(None), fwd=False)
    refused(BAD, 'dw1 NULL', dw1=_p(None), fwd=False)
    refused(BAD, 'dw2 NULL', dw2=_p(None), fwd=False)
    refused(BAD, 'rows_loss > rows', rows_loss=rows + 1)
    refused(BAD, 'rows_loss < 0', rows_loss=-1)
    refused(BAD, 'rows = 0', rows=0, rows_loss=0)
    refused(BAD, 'ldp < nin', ldp=nin - 4)
    refused(BAD, 'ldgp < nin', ldgp=nin - 4, fwd=False)
    # nothing above left a trace: the same buffers now take the calls
    assert _done(L.gml_head_l1_fwd_acc(*h.ops(), loss.ptr(), lsum.ptr(), pre.ptr(), st)) == OK
    assert _done(L.gml_head_l1_bwd(*h.ops(), _p(h.gs), o['gp'].ptr(), 36, o['dw1'].ptr(), o['db1'].ptr(), o['dw2'].ptr(), o['db2'].ptr(), st)) == OK
    _hold(loss, ref['loss'], 'head_l1 after the error answers: loss', ('head_l1', 'fwd', 'loss'))
    h.check_grads(o, 'head_l1 after the error answers', 'head_l1', 'bwd')


# ------------------------------------------------------------------------------------------------------------ gml_head_l1_big_*
def _parts(rows):
    need = int(G.lib().gml_head_l1_big_workspace_floats(rows, 32, 32))
    assert need % NPART == 0 and need // NPART == min(-(-rows // Q.SLAB), Q.NCU), 'the size query no longer follows hb_grid'
    return need, need // NPART


def run_big(dev, rows, family, kw, i=0, null=(), partials=False):
    c, ref = Q.l1_case(rows, 32, 32, family, sums='slabs', **kw)
    h = _Head(dev, c, ref, (32, 36, 64)[i % 3], (32, 36)[i % 2])
    road = Q.road(rows)
    what = 'head_l1_big rows=%d %s %s ldp=%d ldgp=%d null=%s partials=%d (%s)' % (rows, family, kw, h.ldp, h.ldgp, null, partials, road)
    L, st = G.lib(), _st(dev)
    need, parts = _parts(rows)
    loss, lsum, ws = _scalar(dev), (None if 'loss_sum' in null else _scalar(dev, 3.25)), _flat(dev, need)
    rc = _done(L.gml_head_l1_big_fwd(*h.ops(), loss.ptr(), lsum.ptr() if lsum else _p(None), ws.ptr(), need, st))
    assert rc == OK, what
    _hold(loss, ref['loss'], what + ' loss', ('head_l1_big', road, 'loss'))
    if lsum:
        _exact(lsum, np.float32(3.25) + _vals(loss), what + ': loss_sum is not its prior value + loss')
    if h.Rl == 0:
        assert _bits(_vals(loss))[0, 0] == 0, what + ': the loss without a row is not +0.0'
    _written(ws, need, np.arange(need) < parts, what + ' forward: one loss partial per workgroup')
    o = h.grads(('dw1', 'db1', 'dw2', 'db2') if partials else null)
    ws = _flat(dev, need)
    rc = _done(L.gml_head_l1_big_bwd(*h.ops(), _p(h.gs), o['gp'].ptr(), h.ldgp, _ptr(o, 'dw1'), _ptr(o, 'db1'), _ptr(o, 'dw2'), _ptr(o, 'db2'),
                                     ws.ptr(), need, st))
    assert rc == OK, what
    _written(ws, need, np.ones(need, bool), what + ' backward: parts records of 1089')
    h.check_grads(o, what, 'head_l1_big', road, dyadic=family == 'dyadic')
    rec = R.split(ws.get(), 1, need, need + 16, 0)[0].reshape(parts, NPART).astype(np.float64).sum(0)       # the records, summed in double
    for k, (a, b) in (('dw1', (0, 1024)), ('db1', (1024, 1056)), ('dw2', (1056, 1088)), ('db2', (1088, 1089))):
        e = Q.hold_values(rec[a:b].reshape(ref[k].v.shape), ref[k], what + ' records: ' + k, bound=True)
        _note('head_l1_big', road + ', records', k, e)
    ROADS.add(('head_l1_big', road))
    return {k: _bits(b.get()).copy() for k, b in list(o.items()) + [('loss', loss)]}


@pytest.mark.parametrize('rows', Q.BIG_ROWS)
def test_head_l1_big_rows(dev, rows):
    """one tile, several, the cap and the first row past it (workgroup 0 takes a second trip over a one-row tile); at each the folded
    form and the partials form (dw1 = dw2 = NULL), the largest twice"""
    q = lambda n: int(G.lib().gml_head_l1_big_workspace_floats(n, 32, 32)) // NPART
    assert [q(n) for n in (CAP_ROWS - 256, CAP_ROWS - 255, CAP_ROWS, CAP_ROWS + 1, 4 * CAP_ROWS)] == [255, 256, 256, 256, 256]
    kw = Q.l1_args(rows, {})
    for i in ((0, 1, 2, 3, 4, 5) if rows <= 1000 else (Q.BIG_ROWS.index(rows),)):
        a = run_big(dev, rows, 'drawn', kw, i=i)
    run_big(dev, rows, 'drawn', kw, i=1, partials=True)
    if rows == Q.BIG_ROWS[-1]:
        b = run_big(dev, rows, 'drawn', kw, i=Q.BIG_ROWS.index(rows))
        assert all(np.array_equal(a[k], b[k]) for k in a), 'head_l1_big: two launches differ'
    Q._l1_large.cache_clear()


@pytest.mark.parametrize('variant', sorted(Q.BIG_VARIANTS))
def test_head_l1_big_variants(dev, variant):
    for rows in (257, 1000):
        for i in range(3):
            run_big(dev, rows, 'drawn', Q.l1_args(rows, Q.BIG_VARIANTS[variant]), i=i)


@pytest.mark.parametrize('null', (('db1',), ('db2',), ('loss_sum',), ('db1', 'db2', 'loss_sum')))
def test_head_l1_big_null_outputs(dev, null):
    a = run_big(dev, 1000, 'drawn', Q.l1_args(1000, {}), null=null)
    b = run_big(dev, 1000, 'drawn', Q.l1_args(1000, {}))
    assert all(np.array_equal(a[k], b[k]) for k in a), 'head_l1_big: an output changes with %s NULL' % (null,)


def test_head_l1_big_dyadic_family(dev):
    for rows, family, kw in Q.big_value_cases():
        if family == 'dyadic':
            run_big(dev, rows, family, kw, i=rows % 6)
    Q._l1_large.cache_clear()


def test_head_l1_big_error_answers(dev):
    rows = 1000
    c, ref = Q.l1_case(rows, 32, 32, 'drawn', sums='slabs', **Q.l1_args(rows, {}))
    h, hoff = _Head(dev, c, ref, 36, 36), _Head(dev, c, ref, 36, 36, lead_p=1)
    w1off = _up(c['w1'], dev, 1)
    need, parts = _parts(rows)
    loss, lsum, o, ws = _scalar(dev), _scalar(dev, 3.25), h.grads(), _flat(dev, need)
    gpoff = _Out(dev, rows, 32, 36, off4=True)
    L, st = G.lib(), _st(dev)
    outs = [loss, lsum, ws, gpoff] + list(o.values())

    def refused(want, why, hh=h, gp=None, ldgp=36, dw1=False, dw2=False, lossp=None, wsp=None, nf=parts, nb=need, fwd=True, bwd=True, **over):
        rcs = []
        if fwd:
            rcs.append(_done(L.gml_head_l1_big_fwd(*hh.ops(**over), loss.ptr() if lossp is None else lossp, lsum.ptr(), ws.ptr() if wsp is None else wsp, nf, st)))
        if bwd:
            rcs.append(_done(L.gml_head_l1_big_bwd(*hh.ops(**over), _p(h.gs), o['gp'].ptr() if gp is None else gp, ldgp, _p(None) if dw1 else o['dw1'].ptr(),
                                                   o['db1'].ptr(), _p(None) if dw2 else o['dw2'].ptr(), o['db2'].ptr(), ws.ptr() if wsp is None else wsp, nb, st)))
        assert rcs and all(rc == want for rc in rcs), 'head_l1_big: %s answered %s, not %d' % (why, rcs, want)
        assert all(b.unchanged() for b in outs), 'head_l1_big: an output changed under the error answer for ' + why

    for nin, nh in ((28, 32), (32, 28), (64, 64), (36, 36)):
        assert L.gml_head_l1_big_workspace_floats(rows, nin, nh) == 0
        refused(UNS, 'widths %d -> %d' % (nin, nh), nin=nin, nh=nh, ldp=max(36, nin), ldgp=max(36, nin))
    assert L.gml_head_l1_big_workspace_floats(0, 32, 32) == 0
    refused(UNS, 'ldp % 4', ldp=35)
    refused(UNS, 'p off alignment', hh=hoff)
    refused(UNS, 'w1 off alignment', w1=_p(w1off, 1))
    refused(UNS, 'gp off alignment', gp=gpoff.ptr(), fwd=False)
    refused(UNS, 'ldgp % 4', ldgp=35, fwd=False)
    refused(BAD, 'dw1 NULL, dw2 given', dw1=True, fwd=False)
    refused(BAD, 'dw2 NULL, dw1 given', dw2=True, fwd=False)
    for k in ('p', 'y', 'w1', 'w2'):
        refused(BAD, k + ' NULL', **{k: _p(None)})
    refused(BAD, 'loss NULL', lossp=_p(None), bwd=False)
    refused(BAD, 'gp NULL', gp=_p(None), fwd=False)
    refused(BAD, 'rows_loss > rows', rows_loss=rows + 1)
    refused(BAD, 'rows = 0', rows=0, rows_loss=0)
    refused(BAD, 'ldp < nin', ldp=28)
    refused(BAD, 'ldgp < nin', ldgp=28, fwd=False)
    refused(WSP, 'a workspace one float short', nf=parts - 1, nb=need - 1)
    refused(WSP, 'ws NULL', wsp=_p(None))


# ---------------------------------------------------------------------------------------------------------------- gml_head_bce_*
def _bce_parts(rows, nin, nh):
    need = int(G.lib().gml_head_bce_workspace_floats(rows, nin, nh))
    np_ = nh * nin + 2 * nh + 4                               # hbce_npart, csrc/gml_head_bce.hip:34: dw1 | db1 | dw2 | db2 | loss | ok | n
    assert need % np_ == 0 and need // np_ == (0 if rows <= Q.SLAB else min(-(-rows // Q.SLAB), Q.NCU)), 'the size query no longer follows hbce_grid'
    return need, need // np_, np_


def run_bce(dev, rows, nin, nh, act, ldp=None, ldgp=None):
    c, ref = Q.bce_case(rows, nin, nh, act, rows - 1)
    h = _Head(dev, c, ref, ldp, ldgp)
    road = Q.road(rows)
    what = 'head_bce rows=%d %d->%d act=%d ldp=%d ldgp=%d (%s)' % (rows, nin, nh, act, h.ldp, h.ldgp, road)
    L, st = G.lib(), _st(dev)
    need, parts, np_ = _bce_parts(rows, nin, nh)
    prior = np.array([[0.5, 3.0, 7.0]], np.float32)
    loss, pre, stats, ws = _scalar(dev), _Out(dev, rows, 1, 1), _Out(dev, 1, 3, 3, out0=prior), _flat(dev, need)
    rc = _done(L.gml_head_bce_fwd(*h.ops(), act, loss.ptr(), pre.ptr(), stats.ptr(), ws.ptr(), need, st))
    assert rc == OK, what
    key = lambda k: ('head_bce', road, k)
    _hold(loss, ref['loss'], what + ' loss', key('loss'), tol=Q.TOL_BCE)
    _hold(pre, ref['pre'], what + ' pre', key('pre'), tol=Q.TOL_BCE)
    got = _vals(stats)[0]
    assert _same(got[0], np.float32(0.5) + _vals(loss)[0, 0]), what + ': stats[0] is not its prior value + loss'
    assert (got[1] - 3.0, got[2] - 7.0) == (ref['ok'], ref['n']), what + ': ok / n %s, reference %s' % (got[1:] - prior[0, 1:], (ref['ok'], ref['n']))
    rec = np.arange(need) % np_
    _written(ws, need, rec >= np_ - 3, what + ' forward: the last three floats of each record')
    o, ws = h.grads(), _flat(dev, need)
    rc = _done(L.gml_head_bce_bwd(*h.ops(), act, _p(h.gs), o['gp'].ptr(), h.ldgp, o['dw1'].ptr(), o['db1'].ptr(), o['dw2'].ptr(), o['db2'].ptr(),
                                  ws.ptr(), need, st))
    assert rc == OK, what
    _written(ws, need, rec < np_ - 3, what + ' backward: every float of a record but the last three')
    h.check_grads(o, what, 'head_bce', road, tol=Q.TOL_BCE)
    ROADS.add(('head_bce', road))
    return {k: _bits(b.get()).copy() for k, b in list(o.items()) + [('loss', loss), ('pre', pre)]}


@pytest.mark.parametrize('rows,nin,nh,act', Q.BCE_BIG)
def test_head_bce_grid_cap_and_the_first_row_past_it(dev, rows, nin, nh, act):
    """65,536 rows fill 256 workgroups with one slab each; at 65,537 workgroup 0 takes a second slab and adds it into its record"""
    q = lambda n: _bce_parts(n, nin, nh)[1]
    assert [q(n) for n in (256, 257, CAP_ROWS - 256, CAP_ROWS - 255, CAP_ROWS, CAP_ROWS + 1, 4 * CAP_ROWS)] == [0, 2, 255, 256, 256, 256, 256]
    a = run_bce(dev, rows, nin, nh, act, ldp=64 if rows % 2 else None)
    if rows > CAP_ROWS:
        b = run_bce(dev, rows, nin, nh, act, ldp=64)
        assert all(np.array_equal(a[k], b[k]) for k in a), 'head_bce: two launches differ'
    Q.bce_case.cache_clear()


def test_head_bce_one_slab(dev):
    run_bce(dev, *Q.BCE_ONE)
    run_bce(dev, *Q.BCE_ONE, ldp=52, ldgp=49)


def test_head_bce_odd_leading_dimensions(dev):
    rows, nin, nh, act = Q.BCE_ODD
    run_bce(dev, rows, nin, nh, act, ldp=7, ldgp=7)
    run_bce(dev, rows, nin, nh, act, ldp=5, ldgp=9)


def test_head_bce_error_answers(dev):
    rows, nin, nh, act = Q.BCE_ODD
    c, ref = Q.bce_case(rows, nin, nh, act, rows - 1)
    h = _Head(dev, c, ref, 7, 7)
    need, parts, np_ = _bce_parts(rows, nin, nh)
    loss, pre, stats, o, ws = _scalar(dev), _Out(dev, rows, 1, 1), _Out(dev, 1, 3, 3, out0=np.ones((1, 3), np.float32)), h.grads(), _flat(dev, need)
    L, st = G.lib(), _st(dev)
    outs = [loss, pre, stats, ws] + list(o.values())

    def refused(want, why, act=act, gp=None, ldgp=7, dw1=None, lossp=None, wsp=None, n=need, fwd=True, bwd=True, **over):
        rcs = []
        if fwd:
            rcs.append(_done(L.gml_head_bce_fwd(*h.ops(**over), act, loss.ptr() if lossp is None else lossp, pre.ptr(), stats.ptr(),
                                                ws.ptr() if wsp is None else wsp, n, st)))
        if bwd:
            rcs.append(_done(L.gml_head_bce_bwd(*h.ops(**over), act, _p(h.gs), o['gp'].ptr() if gp is None else gp, ldgp, o['dw1'].ptr() if dw1 is None else dw1,
                                                o['db1'].ptr(), o['dw2'].ptr(), o['db2'].ptr(), ws.ptr() if wsp is None else wsp, n, st)))
        assert rcs and all(rc == want for rc in rcs), 'head_bce: %s answered %s, not %d' % (why, rcs, want)
        assert all(b.unchanged() for b in outs), 'head_bce: an output changed under the error answer for ' + why

    refused(UNS, 'nin = 65', nin=65, ldp=65, ldgp=65)
    refused(UNS, 'nh = 65', nh=65)
    refused(UNS, 'act = 2', act=2)
    assert L.gml_head_bce_workspace_floats(rows, 65, nh) == 0 and L.gml_head_bce_workspace_floats(rows, nin, 65) == 0
    for k in ('p', 'y', 'w1', 'w2'):
        refused(BAD, k + ' NULL', **{k: _p(None)})
    refused(BAD, 'loss NULL', lossp=_p(None), bwd=False)
    refused(BAD, 'gp NULL', gp=_p(None), fwd=False)
    refused(BAD, 'dw1 NULL', dw1=_p(None), fwd=False)
    refused(BAD, 'rows_loss > rows', rows_loss=rows + 1)
    refused(BAD, 'rows = 0', rows=0, rows_loss=0)
    refused(BAD, 'ldp < nin', ldp=nin - 1)
    refused(BAD, 'ldgp < nin', ldgp=nin - 1, fwd=False)
    refused(WSP, 'a workspace one float short', n=need - 1)
    refused(WSP, 'ws NULL', wsp=_p(None))


# ------------------------------------------------------------------------------------------------------------- gml_node_head_*
def run_node(dev, N, F, mask, bias, i=0, null=()):
    """gml_node_head_fwd and gml_node_head_bwd (handed the reference's pre); i rotates ldx, ldy, ldm, lddx"""
    c, ref = Q.node_case(N, F, mask, bias)
    ldx, ldy, ldm, lddx = (F, F + 3)[i % 2], (1, 3)[i // 2 % 2], (1, 2)[i // 4 % 2], (F + 3, F)[i % 2 ^ (i // 8 % 2)]
    what = 'node_head N=%d F=%d mask=%s bias=%d ldx=%d ldy=%d ldm=%d lddx=%d null=%s' % (N, F, mask, bias, ldx, ldy, ldm, lddx, null)
    x, y, m = _up(_wide(c['x'], ldx), dev), _up(_wide(c['y'], ldy), dev), _up(_wide(c['mask'], ldm), dev)
    w, b, g = _vec(c['w'], dev), _vec(c['b'], dev), _up(np.array([c['g'], 7.0], np.float32), dev)
    pre, loss, stats = _Out(dev, N, 1, 1), _scalar(dev), (None if 'stats' in null else _Out(dev, 1, 4, 4))
    L, st = G.lib(), _st(dev)
    rc = _done(L.gml_node_head_fwd(_p(x), ldx, _p(w), _p(b), _p(y), ldy, _p(m), ldm, N, F, pre.ptr(), loss.ptr(), stats.ptr() if stats else _p(None), st))
    assert rc == OK, what
    road = 'N <= 1024' if N <= 1024 else 'strided'
    _hold(pre, ref['pre'], what + ' pre', ('node_head', road, 'pre'))
    _hold(loss, ref['loss'], what + ' loss', ('node_head', road, 'loss'))
    if stats:
        _hold(stats, ref['stats'], what + ' stats', ('node_head', road, 'stats'))
        got = _vals(stats)[0]
        assert got[3] == ref['count'] and _same(got[0], _vals(loss)[0, 0]), what + ': count or stats[0]'
        if ref['count'] == 0:
            assert _bits(got[1:])[0:3].tolist() == [0, 0, 0], what + ': no row with mask == 1, yet ss_res / ss_tot / count are not +0.0'
    pre_in = _vec(Q.f32(ref['pre'].v[:, 0]), dev)
    o = {'dx': _Out(dev, N, F, lddx), 'dw': _Out(dev, 1, F, F), 'db': _scalar(dev)}
    o = {k: v for k, v in o.items() if k not in null}
    rc = _done(L.gml_node_head_bwd(_p(g), _p(x), ldx, _p(w), _p(pre_in), _p(y), ldy, _p(m), ldm, N, F, _ptr(o, 'dx'), lddx, _ptr(o, 'dw'), _ptr(o, 'db'), st))
    assert rc == OK, what
    for k, buf in o.items():
        _hold(buf, ref[k], what + ' ' + k, ('node_head', road, k))
    if 'dx' in o and N:
        assert not _vals(o['dx'])[c['mask'] == 0].any(), what + ': dx of a row with mask 0 is not zero'
    ROADS.add(('node_head', road))
    return {k: _bits(buf.get()).copy() for k, buf in list(o.items()) + [('pre', pre), ('loss', loss)]}


@pytest.mark.parametrize('N', Q.NODE_N)
def test_node_head_shapes(dev, N):
    for j, F in enumerate(Q.NODE_F):
        mask = Q.NODE_MASKS[(Q.NODE_N.index(N) + j) % 4]
        for i in range(16):
            a = run_node(dev, N, F, mask, True, i=i)
    b = run_node(dev, N, F, mask, True, i=15)
    assert all(np.array_equal(a[k], b[k]) for k in a), 'node_head: two launches differ'


@pytest.mark.parametrize('mask', Q.NODE_MASKS)
@pytest.mark.parametrize('bias', (True, False))
def test_node_head_masks_and_null_operands(dev, mask, bias):
    for N, F in ((17, 2), (1025, 63)):
        full = run_node(dev, N, F, mask, bias, i=5)
        for null in (('stats',), ('dx',), ('dw',), ('db',), ('dx', 'dw', 'db')):
            a = run_node(dev, N, F, mask, bias, i=5, null=null)
            assert all(np.array_equal(a[k], full[k]) for k in a), 'node_head: an output changes with %s NULL' % (null,)


def test_node_head_error_answers(dev):
    N, F = 17, 2
    c, ref = Q.node_case(N, F, '01', True)
    x, y, m = _up(_wide(c['x'], 5), dev), _up(_wide(c['y'], 3), dev), _up(_wide(c['mask'], 2), dev)
    w, b, g, pre_in = _vec(c['w'], dev), _vec(c['b'], dev), _up(np.array([0.75, 7.0], np.float32), dev), _vec(Q.f32(ref['pre'].v[:, 0]), dev)
    pre, loss, stats = _Out(dev, N, 1, 1), _scalar(dev), _Out(dev, 1, 4, 4)
    o = {'dx': _Out(dev, N, F, 5), 'dw': _Out(dev, 1, F, F), 'db': _scalar(dev)}
    L, st = G.lib(), _st(dev)
    outs = [pre, loss, stats] + list(o.values())

    def refused(want, why, fwd=True, bwd=True, **over):
        a = dict(g=_p(g), x=_p(x), ldx=5, w=_p(w), b=_p(b), pre_in=_p(pre_in), y=_p(y), ldy=3, mask=_p(m), ldm=2, N=N, F=F, pre=pre.ptr(), loss=loss.ptr(),
                 dx=o['dx'].ptr(), lddx=5)
        a.update(over)
        rcs = []
        if fwd:
            rcs.append(_done(L.gml_node_head_fwd(a['x'], a['ldx'], a['w'], a['b'], a['y'], a['ldy'], a['mask'], a['ldm'], a['N'], a['F'], a['pre'], a['loss'],
                                                 stats.ptr(), st)))
        if bwd:
            rcs.append(_done(L.gml_node_head_bwd(a['g'], a['x'], a['ldx'], a['w'], a['pre_in'], a['y'], a['ldy'], a['mask'], a['ldm'], a['N'], a['F'], a['dx'],
                                                 a['lddx'], o['dw'].ptr(), o['db'].ptr(), st)))
        assert rcs and all(rc == want for rc in rcs), 'node_head: %s answered %s, not %d' % (why, rcs, want)
        assert all(buf.unchanged() for buf in outs), 'node_head: an output changed under the error answer for ' + why

    refused(UNS, 'F = 0', F=0)
    refused(UNS, 'F = 65', F=65, ldx=65, lddx=65)
    refused(BAD, 'ldx < F', ldx=F - 1)
    refused(BAD, 'ldy = 0', ldy=0)
    refused(BAD, 'ldm = 0', ldm=0)
    refused(BAD, 'lddx < F with dx given', lddx=F - 1, fwd=False)
    refused(BAD, 'N < 0', N=-1)
    for k in ('x', 'w', 'y', 'mask'):
        refused(BAD, k + ' NULL', **{k: _p(None)})
    refused(BAD, 'pre NULL', pre=_p(None), bwd=False)
    refused(BAD, 'loss NULL', loss=_p(None), bwd=False)
    refused(BAD, 'g NULL', g=_p(None), fwd=False)
    refused(BAD, 'pre (input) NULL', pre_in=_p(None), fwd=False)


# ----------------------------------------------------------------------------------------------------------------------- BatchNorm
LDS = ('C', 'C+4', '64', 'slice')                            # leading dimensions of x, dy, y, dx: tight, padded, 64 wide, a column slice of 64


def _ld(C, kind):
    """(leading dimension, first column): 'slice' starts at the last 16-byte-aligned column a 64-wide row leaves room for"""
    return {'C': (C, 0), 'C+4': (C + 4, 0), '64': (64, 0), 'slice': (64, min(8, 64 - C))}[kind]


class _Mat(object):
    """an output [N, C] in rows of ld starting at column col0 of its buffer: the columns around it are guards too"""

    def __init__(self, dev, N, C, kind):
        self.N, self.C, (self.ld, self.col0) = N, C, _ld(C, kind)
        self.o = _Out(dev, N, self.ld, self.ld)

    def ptr(self):
        return ctypes.c_void_p(self.o.ptr().value + 4 * self.col0)

    def hold(self, ref, what, key, **kw):
        full, guards = R.split(self.o.get(), self.N, self.ld, self.ld)
        assert (guards == R.SENTINEL).all(), what + ': guard rows overwritten'
        side = np.delete(_bits(full), np.s_[self.col0:self.col0 + self.C], axis=1)
        assert (side == R.SENTINEL).all(), what + ': wrote beside its columns'
        got = full[:, self.col0:self.col0 + self.C]
        assert np.isfinite(got).all(), what + ': a value is not finite'
        if self.N:
            _note(key[0], key[1], key[2], Q.hold_values(got, ref, what, **kw))
        return got

    def unchanged(self):
        return self.o.unchanged()


def _bn_in(a, C, kind, dev, valid=None):
    """an input [N, C] in the layout `kind`; the invalid rows hold the NaN sentinel"""
    ld, col0 = _ld(C, kind)
    a = np.array(a, np.float32)
    if valid is not None:
        a.view(np.int32)[valid == 0] = R.SENTINEL
    t = _up(_wide(a, ld, col0=col0), dev)
    return t, ctypes.c_void_p(t.data_ptr() + 4 * col0), ld


def run_bn(dev, N, C, pattern=None, i=0, affine=True):
    """the four launches, each on its own, fed the REFERENCE's statistics / sums; i rotates the four leading dimensions"""
    c, r = Q.bn_case(N, C, pattern)
    valid = c.get('valid')
    masked = pattern is not None
    kx, kdy, ky, kdx = LDS[i % 4], LDS[(i // 4 + i) % 4], LDS[(i + 1) % 4], LDS[(i + 2) % 4]
    road = ('masked, ' if masked else '') + Q.bn_road(N)
    kern = 'bn_masked' if masked else 'bn'
    what = '%s N=%d C=%d pattern=%s x:%s dy:%s y:%s dx:%s affine=%d (%s)' % (kern, N, C, pattern, kx, kdy, ky, kdx, affine, road)
    L, st = G.lib(), _st(dev)
    x, xp, ldx = _bn_in(c['x'], C, kx, dev, valid)
    dy, dyp, lddy = _bn_in(c['dy'], C, kdy, dev, valid)
    rv = _vec(valid, dev)
    w, b = (_vec(c['weight'], dev), _vec(c['bias'], dev)) if affine else (None, None)
    if not affine:
        r = dict(r)
        r['y'] = Q.bn_apply_ref(c['x'], r['mean32'], r['rstd32'], None, None, valid)
        r['dx'] = Q.bn_bwd_apply_ref(c['dy'], c['x'], r['mean32'], r['rstd32'], None, r['sdy32'], r['sdx32'], N if not masked else r['stats']['count'], valid)
    mean_in, rstd_in, sdy_in, sdx_in = (_vec(r[k], dev) for k in ('mean32', 'rstd32', 'sdy32', 'sdx32'))
    n = r['stats']['count']
    cnt_in = _up(np.array([n, 7.0], np.float32), dev)
    need = int((L.gml_bn_masked_workspace_bytes if masked else L.gml_bn_workspace_bytes)(N))
    nblk = -(-N // Q.BN_ROWS)
    assert need == 4 * nblk * (129 if masked else 128), 'the size query no longer follows GML_BN_ROWS'
    key = lambda k: (kern, road, k)
    out = {}
    # --- stats
    mean, var, rstd, cnt, ws = _Out(dev, 1, C, C), _Out(dev, 1, C, C), _Out(dev, 1, C, C), _scalar(dev), _flat(dev, need // 4)
    if masked:
        rc = L.gml_bn_masked_stats(xp, ldx, _p(rv), N, C, Q.EPS, mean.ptr(), var.ptr(), rstd.ptr(), cnt.ptr(), ws.ptr(), need, st)
    else:
        rc = L.gml_bn_stats(xp, ldx, N, C, Q.EPS, mean.ptr(), var.ptr(), rstd.ptr(), ws.ptr(), need, st)
    assert _done(rc) == OK, what
    for k, o in (('mean', mean), ('var', var), ('rstd', rstd)):
        _hold(o, r['stats'][k], what + ' ' + k, key(k), bound=True)
        out[k] = _bits(o.get()).copy()
    _written(ws, need // 4, np.ones(need // 4, bool), what + ' stats')
    if masked:
        assert _vals(cnt)[0, 0] == n, what + ': count %r, %d rows are valid' % (_vals(cnt)[0, 0], n)
    else:
        assert cnt.unchanged()
    if n <= 1:
        assert not _vals(var).any() and np.allclose(_vals(rstd), Q.EPS ** -0.5, rtol=1e-6), what + ': var = 0 and rstd = eps^-1/2 at %d rows' % n
        if n == 0:
            assert (_bits(_vals(mean)) == 0).all() and (_bits(_vals(var)) == 0).all(), what + ': mean and var without a valid row are not +0.0'
    # --- apply
    y = _Mat(dev, N, C, ky)
    if masked:
        rc = L.gml_bn_masked_apply(xp, ldx, _p(rv), N, C, _p(mean_in), _p(rstd_in), _p(w), _p(b), y.ptr(), y.ld, st)
    else:
        rc = L.gml_bn_apply(xp, ldx, N, C, _p(mean_in), _p(rstd_in), _p(w), _p(b), y.ptr(), y.ld, st)
    assert _done(rc) == OK, what
    got = y.hold(r['y'][0], what + ' y', key('y'))
    assert (_bits(got[r['y'][1]]) == 0).all(), what + ': y of an invalid row is not +0.0'
    out['y'] = _bits(got).copy()
    # --- bwd_sums
    sdy, sdx, ws = _Out(dev, 1, C, C), _Out(dev, 1, C, C), _flat(dev, need // 4)
    if masked:
        rc = L.gml_bn_masked_bwd_sums(dyp, lddy, xp, ldx, _p(rv), N, C, _p(mean_in), _p(rstd_in), sdy.ptr(), sdx.ptr(), ws.ptr(), need, st)
    else:
        rc = L.gml_bn_bwd_sums(dyp, lddy, xp, ldx, N, C, _p(mean_in), _p(rstd_in), sdy.ptr(), sdx.ptr(), ws.ptr(), need, st)
    assert _done(rc) == OK, what
    _hold(sdy, r['sums']['sum_dy'], what + ' sum_dy', key('sum_dy'), bound=True)
    _hold(sdx, r['sums']['sum_dyxhat'], what + ' sum_dyxhat', key('sum_dyxhat'), bound=True)
    out['sum_dy'], out['sum_dyxhat'] = _bits(sdy.get()).copy(), _bits(sdx.get()).copy()
    _written(ws, need // 4, np.arange(need // 4) < nblk * 128, what + ' bwd_sums: the column partials (the row counts are the statistics pass\'s)')
    # --- bwd_apply
    dx = _Mat(dev, N, C, kdx)
    if masked:
        rc = L.gml_bn_masked_bwd_apply(dyp, lddy, xp, ldx, _p(rv), N, C, _p(mean_in), _p(rstd_in), _p(w), _p(sdy_in), _p(sdx_in), _p(cnt_in), dx.ptr(), dx.ld, st)
    else:
        rc = L.gml_bn_bwd_apply(dyp, lddy, xp, ldx, N, C, _p(mean_in), _p(rstd_in), _p(w), _p(sdy_in), _p(sdx_in), dx.ptr(), dx.ld, st)
    assert _done(rc) == OK, what
    bar = Q.bn_dx_bar(n if masked else N)
    got = dx.hold(r['dx'][0], what + ' dx', key('dx, 2 rows' if bar else 'dx'), **bar)
    assert (_bits(got[r['dx'][1]]) == 0).all(), what + ': dx of an invalid row is not +0.0'
    if N == 1:
        assert not got.any(), what + ': dx of a single row is not 0'
    out['dx'] = _bits(got).copy()
    ROADS.add((kern, Q.bn_road(N)))
    WIDTHS.add((kern, C))
    return out


def test_batchnorm_every_width(dev):
    """C = 4, 8, ..., 64 at N = 257, with and without the affine pair"""
    for i, C in enumerate(Q.BN_WIDTHS):
        run_bn(dev, 257, C, i=i)
        run_bn(dev, 257, C, i=i + 5, affine=False)


@pytest.mark.parametrize('N', Q.BN_N_LIST)
def test_batchnorm_rows(dev, N):
    """the 16-row sweep, the 64-row step, the 2048-row block boundary and 17 blocks (a thread group of the finish kernel takes a second
    partial) at C = 4, 48, 64; the four leading dimensions vary independently"""
    for j, C in enumerate(Q.BN_N_WIDTHS):
        for i in (range(0, 16, 3) if N <= 4097 else (Q.BN_N_LIST.index(N) + j,)):
            a = run_bn(dev, N, C, i=i + j)
    b = run_bn(dev, N, C, i=i + j)
    assert all(np.array_equal(a[k], b[k]) for k in a), 'bn: two launches differ'


@pytest.mark.parametrize('N', sorted({n for n, _, _ in Q.bn_masked_cases()}))
def test_masked_batchnorm(dev, N):
    """the validity patterns; x and dy hold NaN on the invalid rows; all valid: the unmasked kernels' figures, bit-equality recorded;
    at N = 257 (every width) also without the affine pair"""
    last = None
    for i, (n, C, pattern) in enumerate(Q.bn_masked_cases()):
        if n == N:
            last = (run_bn(dev, N, C, pattern, i=i), C, pattern, i)
            if N == 257:
                run_bn(dev, N, C, pattern, i=i + 1, affine=False)
            if pattern == 'all':
                plain = run_bn(dev, N, C, None, i=i)
                BITS['masked all valid: cases'] += 1
                BITS['masked all valid: bit-equal to the unmasked kernels'] += int(all(np.array_equal(plain[k], last[0][k]) for k in plain))
    a, C, pattern, i = last
    b = run_bn(dev, N, C, pattern, i=i)
    assert all(np.array_equal(a[k], b[k]) for k in a), 'bn_masked: two launches differ'


@pytest.mark.parametrize('C', Q.BN_N_WIDTHS)
def test_batchnorm_chain_against_torch_in_double(dev, C):
    """stats -> apply -> bwd_sums -> bwd_apply on the kernels' OWN intermediates, against torch.nn.BatchNorm1d(C).double()"""
    N = 2049
    c = Q.bn_inputs(N, C, ('chain',))
    bn = torch.nn.BatchNorm1d(C, eps=Q.EPS).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(c['weight'].astype(np.float64)))
        bn.bias.copy_(torch.from_numpy(c['bias'].astype(np.float64)))
    xt = torch.tensor(c['x'].astype(np.float64), requires_grad=True)
    yt = bn(xt)
    (yt * torch.from_numpy(c['dy'].astype(np.float64))).sum().backward()
    L, st = G.lib(), _st(dev)
    x, xp, ldx = _bn_in(c['x'], C, 'C+4', dev)
    dy, dyp, lddy = _bn_in(c['dy'], C, 'slice', dev)
    w, b = _vec(c['weight'], dev), _vec(c['bias'], dev)
    need = int(L.gml_bn_workspace_bytes(N))
    mean, var, rstd, sdy, sdx, ws = tuple(_Out(dev, 1, C, C) for _ in range(5)) + (_flat(dev, need // 4),)
    y, dx = _Mat(dev, N, C, '64'), _Mat(dev, N, C, 'C')
    assert _done(L.gml_bn_stats(xp, ldx, N, C, Q.EPS, mean.ptr(), var.ptr(), rstd.ptr(), ws.ptr(), need, st)) == OK
    assert _done(L.gml_bn_apply(xp, ldx, N, C, mean.ptr(), rstd.ptr(), _p(w), _p(b), y.ptr(), y.ld, st)) == OK
    assert _done(L.gml_bn_bwd_sums(dyp, lddy, xp, ldx, N, C, mean.ptr(), rstd.ptr(), sdy.ptr(), sdx.ptr(), ws.ptr(), need, st)) == OK
    assert _done(L.gml_bn_bwd_apply(dyp, lddy, xp, ldx, N, C, mean.ptr(), rstd.ptr(), _p(w), sdy.ptr(), sdx.ptr(), dx.ptr(), dx.ld, st)) == OK
    s = Q.bn_stats_ref(c['x'])
    yr = Q.bn_apply_ref(c['x'], s['mean'].v, s['rstd'].v, c['weight'], c['bias'])[0]
    sm = Q.bn_bwd_sums_ref(c['dy'], c['x'], s['mean'].v, s['rstd'].v)
    dxr = Q.bn_bwd_apply_ref(c['dy'], c['x'], s['mean'].v, s['rstd'].v, c['weight'], sm['sum_dy'].v, sm['sum_dyxhat'].v, N)[0]
    tor = {'y': yt.detach().numpy(), 'dx': xt.grad.numpy(), 'sum_dy': bn.bias.grad.numpy()[None], 'sum_dyxhat': bn.weight.grad.numpy()[None]}
    for k, ref in (('y', yr), ('dx', dxr), ('sum_dy', sm['sum_dy']), ('sum_dyxhat', sm['sum_dyxhat'])):
        assert np.abs(ref.v - tor[k]).max() <= 1e-9 * np.abs(tor[k]).max(), 'the reference left torch: ' + k
    y.hold(yr, 'bn chain C=%d y' % C, ('bn', 'chain', 'y'))
    dx.hold(dxr, 'bn chain C=%d dx' % C, ('bn', 'chain', 'dx'))
    _hold(sdy, sm['sum_dy'], 'bn chain sum_dy', ('bn', 'chain', 'sum_dy'), bound=False)
    _hold(sdx, sm['sum_dyxhat'], 'bn chain sum_dyxhat', ('bn', 'chain', 'sum_dyxhat'), bound=False)
    _hold(var, s['var'], 'bn chain var', ('bn', 'chain', 'var'), bound=True)


def test_batchnorm_error_answers(dev):
    N, C = 65, 8
    for masked in (False, True):
        c, r = Q.bn_case(N, C, 'tail' if masked else None)
        L, st = G.lib(), _st(dev)
        name = 'bn_masked' if masked else 'bn'
        rv = _vec(c.get('valid'), dev)
        x, dy = _up(_wide(c['x'], 12), dev), _up(_wide(c['dy'], 12), dev)
        x1, dy1 = _up(_wide(c['x'], 12), dev, 1), _up(_wide(c['dy'], 12), dev, 1)
        vec = {k: _vec(v, dev) for k, v in (('mean', r['mean32']), ('rstd', r['rstd32']), ('weight', c['weight']), ('bias', c['bias']), ('sum_dy', r['sdy32']),
                                             ('sum_dyxhat', r['sdx32']))}
        off = {k: _vec(v, dev, 1) for k, v in (('mean', r['mean32']), ('rstd', r['rstd32']), ('weight', c['weight']), ('bias', c['bias']),
                                                ('sum_dy', r['sdy32']), ('sum_dyxhat', r['sdx32']))}
        cnt_in = _up(np.array([r['stats']['count'], 7.0], np.float32), dev)
        need = int((L.gml_bn_masked_workspace_bytes if masked else L.gml_bn_workspace_bytes)(N))
        assert (L.gml_bn_masked_workspace_bytes if masked else L.gml_bn_workspace_bytes)(0) == 0
        o = {k: _Out(dev, 1, C, C) for k in ('mean', 'var', 'rstd', 'sum_dy', 'sum_dyxhat')}
        o.update(count=_scalar(dev), y=_Out(dev, N, C, 12), dx=_Out(dev, N, C, 12), ws=_flat(dev, need // 4), ws4=_Out(dev, 1, need // 4, need // 4 + 16, off4=True, guard_rows=0),
                 y4=_Out(dev, N, C, 12, off4=True), dx4=_Out(dev, N, C, 12, off4=True))

        def refused(want, why, which=('stats', 'apply', 'sums', 'bwd'), **over):
            a = dict(x=_p(x), ldx=12, dy=_p(dy), lddy=12, N=N, C=C, y=o['y'].ptr(), ldy=12, dx=o['dx'].ptr(), lddx=12, ws=o['ws'].ptr(), wsb=need, rv=_p(rv),
                     count=_p(cnt_in), mean_out=o['mean'].ptr(), sdy_out=o['sum_dy'].ptr())
            a.update({k: _p(v) for k, v in vec.items()})
            a.update(over)
            m = (a['rv'],) if masked else ()
            rcs = {}
            if 'stats' in which:
                f = L.gml_bn_masked_stats if masked else L.gml_bn_stats
                rcs['stats'] = f(a['x'], a['ldx'], *m, a['N'], a['C'], Q.EPS, a['mean_out'], o['var'].ptr(), o['rstd'].ptr(),
                                 *((o['count'].ptr(),) if masked else ()), a['ws'], a['wsb'], st)
            if 'apply' in which:
                f = L.gml_bn_masked_apply if masked else L.gml_bn_apply
                rcs['apply'] = f(a['x'], a['ldx'], *m, a['N'], a['C'], a['mean'], a['rstd'], a['weight'], a['bias'], a['y'], a['ldy'], st)
            if 'sums' in which:
                f = L.gml_bn_masked_bwd_sums if masked else L.gml_bn_bwd_sums
                rcs['sums'] = f(a['dy'], a['lddy'], a['x'], a['ldx'], *m, a['N'], a['C'], a['mean'], a['rstd'], a['sdy_out'], o['sum_dyxhat'].ptr(), a['ws'], a['wsb'], st)
            if 'bwd' in which:
                f = L.gml_bn_masked_bwd_apply if masked else L.gml_bn_bwd_apply
                rcs['bwd'] = f(a['dy'], a['lddy'], a['x'], a['ldx'], *m, a['N'], a['C'], a['mean'], a['rstd'], a['weight'], a['sum_dy'], a['sum_dyxhat'],
                               *((a['count'],) if masked else ()), a['dx'], a['lddx'], st)
            _done(max(rcs.values()))
            assert rcs and all(rc == want for rc in rcs.values()), '%s: %s answered %s, not %d' % (name, why, rcs, want)
            assert all(b.unchanged() for b in o.values()), '%s: an output changed under the error answer for %s' % (name, why)

        for Cbad in (0, 3, 68):
            refused(UNS, 'C = %d' % Cbad, C=Cbad, ldx=max(12, Cbad + 4 - Cbad % 4), lddy=72, ldy=72, lddx=72)
        refused(UNS, 'ldx % 4', ldx=13)
        refused(UNS, 'ldx < C', ldx=4)
        refused(UNS, 'lddy % 4', lddy=13, which=('sums', 'bwd'))
        refused(UNS, 'lddy < C', lddy=4, which=('sums', 'bwd'))
        refused(UNS, 'ldy % 4', ldy=13, which=('apply',))
        refused(UNS, 'ldy < C', ldy=4, which=('apply',))
        refused(UNS, 'lddx % 4', lddx=13, which=('bwd',))
        refused(UNS, 'lddx < C', lddx=4, which=('bwd',))
        refused(UNS, 'x off alignment', x=_p(x1, 1))
        refused(UNS, 'dy off alignment', dy=_p(dy1, 1), which=('sums', 'bwd'))
        refused(UNS, 'y off alignment', y=o['y4'].ptr(), which=('apply',))
        refused(UNS, 'dx off alignment', dx=o['dx4'].ptr(), which=('bwd',))
        # the vectors a kernel reads as f32x4, and the workspace whose partials it stores as f32x4 (gml.h): host checks, nothing launches
        refused(UNS, 'mean off alignment', mean=_p(off['mean'], 1), which=('apply', 'sums', 'bwd'))
        refused(UNS, 'rstd off alignment', rstd=_p(off['rstd'], 1), which=('apply', 'sums', 'bwd'))
        refused(UNS, 'weight off alignment', weight=_p(off['weight'], 1), which=('apply', 'bwd'))
        refused(UNS, 'bias off alignment', bias=_p(off['bias'], 1), which=('apply',))
        refused(UNS, 'sum_dy off alignment', sum_dy=_p(off['sum_dy'], 1), which=('bwd',))
        refused(UNS, 'sum_dyxhat off alignment', sum_dyxhat=_p(off['sum_dyxhat'], 1), which=('bwd',))
        refused(UNS, 'ws off alignment', ws=o['ws4'].ptr(), which=('stats', 'sums'))
        refused(WSP, 'a workspace 4 bytes short', wsb=need - 4, which=('stats', 'sums'))
        refused(WSP, 'ws NULL', ws=_p(None), which=('stats', 'sums'))
        refused(BAD, 'num_rows = 0', N=0)
        refused(BAD, 'x NULL', x=_p(None))
        refused(BAD, 'dy NULL', dy=_p(None), which=('sums', 'bwd'))
        refused(BAD, 'mean NULL', mean=_p(None), which=('apply', 'sums', 'bwd'))
        refused(BAD, 'rstd NULL', rstd=_p(None), which=('apply', 'sums', 'bwd'))
        refused(BAD, 'mean (output) NULL', mean_out=_p(None), which=('stats',))
        refused(BAD, 'sum_dy (output) NULL', sdy_out=_p(None), which=('sums',))
        refused(BAD, 'sum_dy NULL', sum_dy=_p(None), which=('bwd',))
        refused(BAD, 'y NULL', y=_p(None), which=('apply',))
        refused(BAD, 'dx NULL', dx=_p(None), which=('bwd',))
        if masked:
            refused(BAD, 'row_valid NULL', rv=_p(None))
            refused(BAD, 'count NULL', count=_p(None), which=('bwd',))


@pytest.mark.parametrize('C', (4, 64))
def test_masked_batchnorm_running_update(dev, C):
    g = _rng('running', C)
    mean, var, rm, rv = (_f32(g.standard_normal(C)), _f32(g.random(C) + 0.5), _f32(g.standard_normal(C)), _f32(g.random(C) + 0.5))
    L, st = G.lib(), _st(dev)
    m_d, v_d = _vec(mean, dev), _vec(var, dev)
    for n in (0, 1, 2, 3, 1000):
        cnt = _up(np.array([n, 7.0], np.float32), dev)
        orm, orv = _Out(dev, 1, C, C, out0=rm[None]), _Out(dev, 1, C, C, out0=rv[None])
        assert _done(L.gml_bn_masked_running_update(_p(cnt), _p(m_d), _p(v_d), C, 0.1, orm.ptr(), orv.ptr(), st)) == OK
        ref = Q.bn_running_ref(rm, rv, mean, var, n, np.float64(np.float32(0.1)))
        if ref is None:
            assert orm.unchanged() and orv.unchanged(), 'running_update at n = %d changed a buffer' % n
        else:
            _hold(orm, ref[0], 'running_mean C=%d n=%d' % (C, n), ('bn_masked', 'running', 'running_mean'))
            _hold(orv, ref[1], 'running_var C=%d n=%d' % (C, n), ('bn_masked', 'running', 'running_var'))
    cnt = _up(np.array([5.0, 7.0], np.float32), dev)
    for a in (dict(C=0), dict(C=65), dict(count=_p(None)), dict(mean=_p(None)), dict(var=_p(None)), dict(rm=_p(None)), dict(rv=_p(None))):
        k = dict(count=_p(cnt), mean=_p(m_d), var=_p(v_d), C=C, rm=orm.ptr(), rv=orv.ptr())
        before = (_bits(orm.get()).copy(), _bits(orv.get()).copy())
        k.update(a)
        assert _done(L.gml_bn_masked_running_update(k['count'], k['mean'], k['var'], k['C'], 0.1, k['rm'], k['rv'], st)) == BAD, a
        assert np.array_equal(before[0], _bits(orm.get())) and np.array_equal(before[1], _bits(orv.get()))


@pytest.mark.parametrize('N', Q.COND_N)
def test_batchnorm_conditioning(dev, N):
    """gml_bn.hip: E[x^2] - mean^2 is "fine for activations whose mean is of the order of their spread".  x ~ N(r, 1), C = 4: var is held
    to its f32_bound (n = 144 on T = E[x^2] + mean^2) and to TOL_F32 of T -- NOT to the max-norm bar: its relative error grows like
    r^2, a property of the formula.  Recorded beside float32 torch.nn.BatchNorm1d on the CPU, both against float64."""
    L, st = G.lib(), _st(dev)
    need = int(L.gml_bn_workspace_bytes(N))
    for r in Q.COND_R:
        x = Q.bn_cond_inputs(N, r)
        s = Q.bn_stats_ref(x)
        x_d = _up(_wide(x, 4), dev)
        mean, var, rstd, ws = _Out(dev, 1, 4, 4), _Out(dev, 1, 4, 4), _Out(dev, 1, 4, 4), _flat(dev, need // 4)
        assert _done(L.gml_bn_stats(_p(x_d), 4, N, 4, Q.EPS, mean.ptr(), var.ptr(), rstd.ptr(), ws.ptr(), need, st)) == OK
        _hold(mean, s['mean'], 'cond mean r=%d' % r, ('bn', 'conditioning r=%d' % r, 'mean'), bound=True)
        _hold(var, s['var'], 'cond var r=%d' % r, ('bn', 'conditioning r=%d' % r, 'var'), bound=True, maxnorm=False)
        _hold(rstd, s['rstd'], 'cond rstd r=%d' % r, ('bn', 'conditioning r=%d' % r, 'rstd'), bound=True, maxnorm=False)
        bn = torch.nn.BatchNorm1d(4, eps=Q.EPS, momentum=1.0, affine=False)
        bn(torch.from_numpy(x))
        tv = bn.running_var.numpy().astype(np.float64) * (N - 1) / N
        rel = lambda got, ref: float((np.abs(np.asarray(got, np.float64) - ref) / np.abs(ref)).max())
        COND.append('N = %5d  r = %3d   kernel: var %.1e  rstd %.1e    torch fp32 (CPU): var %.1e  rstd %.1e' % (
            N, r, rel(_vals(var)[0], s['var'].v[0]), rel(_vals(rstd)[0], s['rstd'].v[0]), rel(tv, s['var'].v[0]),
            rel(1.0 / np.sqrt(tv + Q.EPS), s['rstd'].v[0])))


# ------------------------------------------------------------------------------------------------------------------------ coverage
def test_every_road_ran_and_worst_figures_report():
    """runs last (file order)"""
    print('roads run: %s' % sorted(ROADS))
    print('BatchNorm widths run: %s' % sorted(c for k, c in WIDTHS if k == 'bn'))
    for k, v in BITS.items():
        print('%s: %d' % (k, v))
    print('conditioning of E[x^2] - mean^2 (relative error against float64):')
    for line in COND:
        print('  ' + line)
    print('%-12s %-34s %-12s %6s %12s %12s' % ('kernel', 'road', 'output', 'cases', 'max-norm', 'term sum'))
    for (kern, road, out), (n, a, b) in sorted(WORST.items()):
        print('%-12s %-34s %-12s %6d %12.3e %12.3e' % (kern, road, out, n, a, b))
    want = {('head_l1', 'fwd'), ('head_l1', 'bwd'), ('node_head', 'N <= 1024'), ('node_head', 'strided')}
    want |= {(k, r) for k in ('head_l1_big', 'head_bce') for r in ('one slab', 'several slabs', 'second trip')}
    want |= {(k, r) for k in ('bn', 'bn_masked') for r in ('one block', 'several blocks', '17 blocks')}
    assert want <= ROADS, 'not run: %s' % sorted(want - ROADS)
    for k in ('bn', 'bn_masked'):
        assert {c for kk, c in WIDTHS if kk == k} == set(Q.BN_WIDTHS), 'BatchNorm widths not run (%s): %s' % (k, sorted(set(Q.BN_WIDTHS) - {c for kk, c in WIDTHS if kk == k}))
    assert len(COND) == len(Q.COND_N) * len(Q.COND_R) and BITS['masked all valid: cases'] > 0
