"""float64 restatement of the readout side of include/gml.h -- the heads with their losses (gml_head_l1_*, gml_head_l1_big_*,
gml_head_bce_*), the node-level head (gml_node_head_*) and BatchNorm (gml_bn_*, gml_bn_masked_*) -- with the TERM SUM and the number of
terms of every output, and the input generators the CPU test and the GPU matrix share, so that both judge the same arrays.  Plain
numpy, no device, nothing imported from the package: tests/test_readout_ref_cpu.py holds it to float64 autograd.

    a = W1 p + b1,  h = act(a),  z = w2 . h + b2                                          (_head_core)
    L1 :  loss = sum_{r < rows_loss} valid |z - y|,   s = gscale valid sign(z - y)        (head_l1_ref)
    BCE:  loss = sum valid (y sp(-z) + (1 - y) sp(z)), s = gscale valid (sigmoid(z) - y)  (head_bce_ref; sp capped at 100)
    dh = s w2 [a > 0],  gp = dh W1,  dw1 = dh^T p,  db1 = dh^T 1,  dw2 = s^T h,  db2 = s^T 1
    node: pre = x . w + b, loss = sum (m (pre - y))^2, dpre = 2 g m^2 (pre - y)           (node_head_ref)
    bn  : mean, var = E[x^2] - mean^2 (biased), rstd = (var + eps)^-1/2, y = (x - mean) rstd w + b,
          sum_dy, sum_dyxhat, dx = (dy - sum_dy / n - xhat sum_dyxhat / n) rstd w          (bn_*_ref, over the valid rows)

Every value comes as _conv_ref.Ref(v, t, n): t the sum of |terms| (an error of an input that is itself computed enters with its own
term sum times the derivative's bound), n the length of the longest fp32 chain the KERNEL sums it in, read off the kernels: nin and
nh for the dot products; `rows` for the row sums of the one-workgroup kernels; 256 per slab + slabs per workgroup + workgroups for
the others (rowsum_n); 128 + 16 for BatchNorm's column sums (128 sequential rows per thread of a 2048-row block, the 16-way fold;
blocks are combined in double).  Selects (rows of gp outside the loss, masked BatchNorm's invalid rows) are returned as row masks:
those rows are exactly +0.0.

The relu and the sign are jumps: head_inputs REDRAWS every row with a unit or a residual inside the margin until none is left
(no row is ever left out of a comparison); head_inputs_dyadic puts everything on multiples of 1/8, where fp32 is exact in any
order and the jumps -- sign(0) = 0 and relu'(0) = 0 among them -- are decided exactly."""
import functools
import math
import zlib

import numpy as np

import _conv_ref as R
from _conv_ref import Ref

MARGIN = 1e-3                                                # |a| of every unit and |pre - y| of every loss row (L1 heads)
BCE_Z = (1e-3, 12.0)                                         # |z| window of tests/test_gpu_exp_classify.py, on every loss row
BCE_RELU = 2e-6                                              # its relu margin
SLAB = 256                                                   # rows per slab / tile (HB_ROWS, HBCE_ROWS)
NCU = 256                                                    # workgroups at the cap (GML_NUM_CU)
BN_ROWS = 2048                                               # GML_BN_ROWS
BN_N = 128 + 16
EPS = 1e-5
SEEDS = {}                                                   # case key -> seed override; empty: the redraw makes every key serve


def rng(*key):
    return np.random.default_rng(SEEDS.get(key, zlib.crc32(repr(key).encode())))


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def f64(a):
    return np.asarray(a, np.float64)


def rowsum_n(rows, road):
    """terms of the longest fp32 chain of a sum over `rows` rows: 'one' workgroup walks them all; 'slabs': 256 per slab, the slabs
    of a workgroup, the workgroups"""
    if road == 'one' or rows <= SLAB:
        return float(rows)
    slabs = -(-rows // SLAB)
    wgs = min(slabs, NCU)
    return float(SLAB + -(-slabs // wgs) + wgs)


def road(rows):
    """'one slab', 'several slabs' (one per workgroup), 'second trip' (a workgroup takes a second slab)"""
    slabs = -(-rows // SLAB)
    return 'one slab' if slabs == 1 else ('several slabs' if slabs <= NCU else 'second trip')


TOL_F32 = 2e-5                                               # the default bar: max-norm AND each element on its own term sum
TOL_BCE = 1e-4                                               # tests/test_gpu_exp_classify.py's: exp / log1p are the device library's
SUMS = ('loss', 'dw1', 'db1', 'dw2', 'db2', 'dw', 'db', 'stats', 'mean', 'var', 'sum_dy', 'sum_dyxhat')      # also within f32_bound


def hold(buf, ref, n, ncols, ldo, what, tol=TOL_F32, bound=False, guard_rows=R.GUARD_ROWS, maxnorm=True):
    """THE criterion of the matrix, for a device buffer and for the CPU test's plain-fp32 values alike: buf a buffer of
    _conv_ref.alloc() holding [n, ncols] in rows of ldo; tol on the max-norm (maxnorm = False: not asked -- the conditioning test
    only) and on each element's own term sum, f32_bound for the sums, guards intact.  Returns (max-norm figure, term-sum figure)."""
    v, t = f64(ref.v).reshape(n, ncols), f64(ref.t).reshape(n, ncols)
    b = np.broadcast_to(R.f32_bound(ref), np.asarray(ref.v).shape).reshape(n, ncols) if bound else None
    if maxnorm:
        return R.check(buf, v, t, n, ncols, ldo, tol, what, guard_rows, bound=b)
    got, guards = R.split(buf, n, ncols, ldo, guard_rows)
    assert (guards == R.SENTINEL).all() and np.isfinite(got).all(), what
    d = np.abs(f64(got) - v)
    assert (d <= tol * t + 1e-30).all() and (d <= b + 1e-30).all(), '%s: beyond its term sum / derived bound: %s' % (what, (d / np.maximum(t, 1e-300)).max())
    return R.errors(got, v, t)


def hold_values(values, ref, what, **kw):
    """hold() for an array of plain values (the CPU test's fp32 evaluation)"""
    a = f32(values)
    a = a.reshape(-1, a.shape[-1]) if a.ndim > 1 else a.reshape(1, -1)
    return hold(R.alloc(a.shape[0], a.shape[1], a.shape[1], out0=a)[0], ref, a.shape[0], a.shape[1], a.shape[1], what, **kw)


# ------------------------------------------------------------------------------------------------------------------------ the heads
def _head_core(c, relu=True):
    p, w1, w2 = f64(c['p']), f64(c['w1']), f64(c['w2']).ravel()
    b1 = np.zeros(w1.shape[0]) if c['b1'] is None else f64(c['b1'])
    b2 = 0.0 if c['b2'] is None else float(f64(c['b2']).ravel()[0])
    a, at = p @ w1.T + b1, np.abs(p) @ np.abs(w1).T + np.abs(b1)
    on = a > 0 if relu else np.ones(a.shape, bool)
    h, ht = np.where(on, a, 0.0), np.where(on, at, 0.0)
    return p, w1, w2, a, at, on, h, ht, h @ w2 + b2, ht @ np.abs(w2) + abs(b2)


def _weights(c):
    rows = c['p'].shape[0]
    v = np.ones(rows) if c['valid'] is None else f64(c['valid'])
    inl = np.arange(rows) < c['rows_loss']
    return np.where(inl, v, 0.0), inl, 1.0 if c['gscale'] is None else float(c['gscale'])


def _head_grads(p, w1, w2, on, h, ht, s, st, nin, nh, ns):
    """the five gradients from the per-row factor s (st: its error basis, |s| where s is exact)"""
    dh, dht = on * s[:, None] * w2[None, :], on * st[:, None] * np.abs(w2)[None, :]
    one = lambda v: np.asarray(v, np.float64).reshape(1, -1)
    return {'gp': Ref(dh @ w1, dht @ np.abs(w1), nh + 3.0), 'gp_zero': s == 0,
            'dw1': Ref(dh.T @ p, dht.T @ np.abs(p), ns + 3.0), 'db1': Ref(one(dh.sum(0)), one(dht.sum(0)), ns + 3.0),
            'dw2': Ref(one(s @ h), one(st @ ht), ns + nin + 3.0), 'db2': Ref(one(s.sum()), one(st.sum()), ns + 2.0)}


def head_l1_ref(c, sums='one'):
    """c: p [rows, nin], w1 [nh, nin], b1 [nh] / None, w2 [nh], b2 [1] / None, y [rows], valid [rows] / None, rows_loss, gscale / None.
    {'a', 'pre' [rows, 1], 'loss' [1, 1], 'gp' [rows, nin], 'gp_zero' (rows that are exactly +0.0), 'dw1', 'db1', 'dw2', 'db2'}"""
    p, w1, w2, a, at, on, h, ht, z, zt = _head_core(c)
    (rows, nin), nh = p.shape, w1.shape[0]
    vv, inl, gs = _weights(c)
    ns = rowsum_n(rows, sums)
    d = z - f64(c['y'])
    r = {'a': Ref(a, at, nin + 1.0), 'pre': Ref(z[:, None], zt[:, None], nin + nh + 2.0),
         'loss': Ref(np.array([[np.sum(vv * np.abs(d))]]), np.array([[np.sum(np.abs(vv) * (zt + np.abs(f64(c['y']))))]]), nin + nh + 3.0 + ns),
         'margin': (float(np.abs(a).min()), float(np.abs(d[inl]).min()) if inl.any() else np.inf)}
    s = np.sign(d) * vv * gs
    r.update(_head_grads(p, w1, w2, on, h, ht, s, np.abs(s), nin, nh, ns))
    return r


def _softplus(t):
    return np.minimum(np.logaddexp(0.0, t), 100.0)


def head_bce_ref(c):
    """as head_l1_ref with c['act'] (1 relu, 0 identity); also 'ok' and 'n' as exact integers.  A logit's error moves a loss term by at
    most as much (|l'| <= 1) and sigmoid by a quarter of it: the bases of the loss and of s carry the logit's term sum"""
    p, w1, w2, a, at, on, h, ht, z, zt = _head_core(c, relu=bool(c['act']))
    (rows, nin), nh = p.shape, w1.shape[0]
    vv, inl, gs = _weights(c)
    ns = rowsum_n(rows, 'slabs')
    y = f64(c['y'])
    l = y * _softplus(-z) + (1.0 - y) * _softplus(z)
    e = np.exp(-np.abs(z))
    sigmoid = lambda t: np.where(t >= 0, 1.0, e) / (1.0 + e)                     # of t = z or -z: e serves both
    dz = np.where(y == 1.0, -sigmoid(-z), sigmoid(z) - y)                        # (1 - sigmoid(z) = sigmoid(-z): no cancellation)
    s, st = gs * vv * dz, np.abs(gs * vv) * (np.abs(dz) + 0.25 * zt)
    r = {'a': Ref(a, at, nin + 1.0), 'pre': Ref(z[:, None], zt[:, None], nin + nh + 2.0),
         'loss': Ref(np.array([[np.sum(vv * l)]]), np.array([[np.sum(np.abs(vv) * (l + zt))]]), nin + nh + 8.0 + ns),
         'ok': int(round(float(np.sum(vv * ((z > 0) == (y == 1.0)))))), 'n': int(np.sum((vv != 0) & inl)),
         'ok_f': float(np.sum(vv * ((z > 0) == (y == 1.0)))),
         'margin': (float(np.abs(a).min()) if c['act'] else np.inf, float(np.abs(z[inl]).min()) if inl.any() else np.inf,
                    float(np.abs(z[inl]).max()) if inl.any() else 0.0)}
    r.update(_head_grads(p, w1, w2, on, h, ht, s, st, nin, nh, ns))
    r['gp_zero'] = vv == 0
    return r


def _valid(g, rows, kind):
    if kind is None:
        return None
    if kind == '01':
        return f32(g.random(rows) < 0.7)
    assert kind == 'w', kind
    return f32(g.choice(np.array([0.0, 0.5, 1.0, 2.0]), rows))


def head_inputs(rows, nin, nh, key=(), rows_loss=None, valid='01', bias=True, gscale=1.5, act=None):
    """Row-resampled inputs of a head (bias: True, False, or 'b1' / 'b2' for that one alone).  act None: the L1 heads (relu; y ~ N(0, 1)); act 0 / 1: the BCE head (labels 0 / 1, w2 scaled
    to logits of rms 2.5).  Every row with a unit inside the relu margin, or -- on a row of the loss -- a residual inside MARGIN
    (L1) / a logit outside BCE_Z (BCE), is drawn again until none is left; the margin is asserted.  Returns the case dict and the
    number of rounds."""
    g = rng('head', rows, nin, nh, key, rows_loss, valid, bias, gscale, act)
    bce = act is not None
    c = {'p': f32(g.standard_normal((rows, nin))), 'w1': f32(g.standard_normal((nh, nin)) * ((2.0 if bce else 1.5) / math.sqrt(nin))),
         'b1': f32(g.standard_normal(nh) * 0.5) if bias in (True, 'b1') else None,
         'w2': f32(g.standard_normal(nh) * (1.0 if bce else 1.5 / math.sqrt(nh))), 'b2': f32(g.standard_normal(1) * 0.5) if bias in (True, 'b2') else None,
         'y': f32(g.random(rows) < 0.5) if bce else f32(g.standard_normal(rows)), 'valid': _valid(g, rows, valid),
         'rows_loss': rows if rows_loss is None else rows_loss, 'gscale': gscale, 'act': act}
    relu = not bce or bool(act)
    if bce:
        z = _head_core(c, relu)[8]
        c['w2'] = f32(f64(c['w2']) * (2.5 / max(float(np.sqrt(np.mean(np.square(z - (0.0 if c['b2'] is None else float(c['b2'][0])))))), 1e-3)))
    inl = np.arange(rows) < c['rows_loss']
    am = (BCE_RELU if bce else MARGIN) if relu else 0.0

    def bad_rows():
        _, _, _, a, _, _, _, _, z, _ = _head_core(c, relu)
        bad = (np.abs(a) < am).any(1) if relu else np.zeros(rows, bool)
        if bce:
            return bad | (inl & ((np.abs(z) < BCE_Z[0]) | (np.abs(z) > BCE_Z[1])))
        return bad | (inl & (np.abs(z - f64(c['y'])) < MARGIN))

    rounds = 1
    bad = bad_rows()
    while bad.any():
        assert rounds < 50, ('the redraw does not end', rows, nin, nh, key)
        k = int(bad.sum())
        c['p'][bad] = f32(g.standard_normal((k, nin)))
        if not bce:
            c['y'][bad] = f32(g.standard_normal(k))
        rounds += 1
        bad = bad_rows()
    assert not bad_rows().any()
    return c, rounds


def head_inputs_dyadic(rows, nin, nh, key=(), rows_loss=None, valid='w', bias=True, gscale=1.5):
    """Everything a multiple of 1/8 (b1 whole numbers): every pre-activation (a multiple of 1/64), every logit (1/512) and pre - y
    are exact in fp32 in any order.  Every fifth row has p = 0 and y = w2 . relu(b1) + b2, a multiple of 1/8: its residual is exactly 0
    (sign(0) = 0, the row's gradient +0.0); units with a = 0 exactly occur throughout (relu'(0) = 0)."""
    g = rng('dyadic', rows, nin, nh, key, rows_loss, valid, bias, gscale)
    q = lambda lo, hi, shape: f32(g.integers(lo, hi + 1, shape) / 8.0)
    c = {'p': q(-8, 8, (rows, nin)), 'w1': q(-4, 4, (nh, nin)), 'b1': f32(g.integers(-1, 2, nh)) if bias in (True, 'b1') else None,
         'w2': q(-4, 4, nh), 'b2': q(-8, 8, 1) if bias in (True, 'b2') else None, 'valid': _valid(g, rows, valid), 'rows_loss': rows if rows_loss is None else rows_loss,
         'gscale': gscale, 'act': None}
    c['p'][::5] = 0.0
    z = _head_core(c)[8]
    y = np.floor(z * 8.0) / 8.0 + g.integers(-8, 9, rows) / 8.0
    y[::5] = z[::5]
    c['y'] = f32(y)
    assert np.array_equal(f64(c['y'][::5]), z[::5]) and np.array_equal(f64(f32(z)), z)
    return c


@functools.lru_cache(maxsize=256)
def _l1_small(rows, nin, nh, family, rows_loss, valid, bias, gscale, sums):
    c = head_inputs_dyadic(rows, nin, nh, (), rows_loss, valid, bias, gscale) if family == 'dyadic' else \
        head_inputs(rows, nin, nh, (), rows_loss, valid, bias, gscale)[0]
    return c, head_l1_ref(c, sums)


_l1_large = functools.lru_cache(maxsize=2)(_l1_small.__wrapped__)


def l1_case(rows, nin, nh, family='drawn', rows_loss=None, valid='01', bias=True, gscale=1.5, sums='one'):
    """(inputs, reference) of an L1-head case, cached: the CPU test and the GPU matrix see the same arrays"""
    return (_l1_small if rows <= 4096 else _l1_large)(rows, nin, nh, family, rows_loss, valid, bias, gscale, sums)


@functools.lru_cache(maxsize=4)
def bce_case(rows, nin, nh, act, rows_loss=None, valid='01', bias=True, gscale=1.5):
    c = head_inputs(rows, nin, nh, (), rows_loss, valid, bias, gscale, act)[0]
    return c, head_bce_ref(c)


# the matrix's value cases: (rows, nin, nh, family, rows_loss (None: rows, negative: rows + it), valid, bias, gscale)
L1_ROWS = (1, 2, 3, 63, 64, 65, 255, 256)
L1_WIDTHS = ((4, 4), (32, 32), (48, 12), (12, 48), (64, 4), (4, 64), (64, 64))
L1_VARIANTS = {'loss rows = rows': dict(rows_loss=None), 'loss rows = rows - 1': dict(rows_loss=-1), 'no loss row': dict(rows_loss=0),
               'valid NULL': dict(valid=None), 'valid 0/1': dict(valid='01'), 'valid weights': dict(valid='w'),
               'no biases': dict(bias=False), 'b1 NULL': dict(bias='b2'), 'b2 NULL': dict(bias='b1'), 'gscale NULL': dict(gscale=None)}
L1_VARIANT_SHAPES = ((3, 12, 48), (65, 32, 32))
L1_EDGE = ((188, 64, 64), (189, 64, 64), (256, 64, 64))     # predicate, backward, forward: the largest rows each takes at 64 -> 64
BIG_ROWS = (1, 255, 256, 257, 1000, 65536, 65537)
BIG_VARIANTS = dict(L1_VARIANTS, **{'loss rows = rows - 3': dict(rows_loss=-3)})
BCE_BIG = ((65536, 48, 10, 1), (65537, 48, 10, 1), (65536, 64, 64, 0), (65537, 64, 64, 0))
BCE_ODD = (257, 5, 1, 1)
BCE_ONE = (200, 48, 10, 1)


def l1_fwd_fits(rows, nin, nh):
    """head_l1_fwd_impl, csrc/gml_head.hip:157-158"""
    return rows <= 256 and 4 * (rows * nin + rows * nh + rows + 4 + nh * nin + 256) <= 160 * 1024


def l1_bwd_fits(rows, nin, nh):
    """gml_head_l1_bwd, csrc/gml_head.hip:192-193"""
    return rows <= 256 and 4 * (rows * nin + 2 * rows * nh + 2 * rows + 8 + nh * nin) <= 160 * 1024


def l1_predicate(rows, nin, nh):
    """functional.head_l1_supported's shape part"""
    return rows <= 256 and nin <= 64 and nh <= 64 and nin % 4 == 0 and nh % 4 == 0 and \
        4 * (rows * nin + 2 * rows * nh + 2 * rows + nh * nin + 256) <= 160 * 1024


def l1_args(rows, variant):
    kw = dict(rows_loss=rows - 1 if rows > 1 else rows, valid='01', bias=True, gscale=1.5)
    kw.update(variant)
    if kw['rows_loss'] is None:
        kw['rows_loss'] = rows
    elif kw['rows_loss'] < 0:
        kw['rows_loss'] = max(rows + kw['rows_loss'], 0)
    return kw


def l1_value_cases():
    """every (rows, nin, nh, family, kw) the one-workgroup matrix launches; kw: l1_case's keywords"""
    out = []
    for rows in L1_ROWS:
        for nin, nh in L1_WIDTHS:
            if l1_fwd_fits(rows, nin, nh):
                out.append((rows, nin, nh, 'drawn', l1_args(rows, {})))
    for rows, nin, nh in L1_VARIANT_SHAPES:
        for v in L1_VARIANTS.values():
            out.append((rows, nin, nh, 'drawn', l1_args(rows, v)))
    for rows, nin, nh in ((3, 4, 4), (65, 32, 32), (64, 64, 64), (189, 64, 64)):
        out.append((rows, nin, nh, 'dyadic', l1_args(rows, dict(valid='w'))))
    for rows, nin, nh in L1_EDGE:
        out.append((rows, nin, nh, 'drawn', l1_args(rows, {})))
    return out


def big_value_cases():
    out = [(rows, 'drawn', l1_args(rows, {})) for rows in BIG_ROWS]
    out += [(rows, 'drawn', l1_args(rows, v)) for rows in (257, 1000) for v in BIG_VARIANTS.values()]
    out += [(rows, 'dyadic', l1_args(rows, dict(valid='w'))) for rows in (257, 1000, 65537)]
    return out


# -------------------------------------------------------------------------------------------------------------------- the node head
def node_inputs(N, F, mask='01', bias=True, g=0.75):
    """x ~ N(0, 1), y ~ N(2, 1) (ss_tot needs ybar first), mask: 'ones', 'zeros', '01', 'frac' (0, 0.5 and 1)"""
    r = rng('node', N, F, mask, bias, g)
    m = {'ones': np.ones(N), 'zeros': np.zeros(N), '01': (r.random(N) < 0.6) * 1.0, 'frac': r.choice(np.array([0.0, 0.5, 1.0]), N)}[mask]
    return {'x': f32(r.standard_normal((N, F))), 'w': f32(r.standard_normal(F) / math.sqrt(F)), 'b': f32(r.standard_normal(1)) if bias else None,
            'y': f32(2.0 + r.standard_normal(N)), 'mask': f32(m), 'g': g}


def node_chain_n(N, F):
    """forward: ceil(N / 1024) rows per thread, the 10-level tree, the dot product; backward: ceil(N / 16) rows per thread, 16 partials"""
    return -(-N // 1024) + 10.0 + F + 3.0, -(-N // 16) + 16.0 + 4.0


def node_head_ref(c, pre_in=None):
    """{'pre' [N, 1], 'loss' [1, 1], 'stats' [1, 4] = (loss, ss_res, ss_tot, count), 'dx' [N, F], 'dw' [1, F], 'db' [1, 1]}.  The backward
    reads `pre` as an input: pre_in (the float32 array it is handed), else the float32 rounding of the reference's own."""
    x, w, y, m = f64(c['x']), f64(c['w']), f64(c['y']), f64(c['mask'])
    b = 0.0 if c['b'] is None else float(c['b'][0])
    N, F = x.shape
    nf, nb = node_chain_n(N, F)
    pre, pt = x @ w + b, np.abs(x) @ np.abs(w) + abs(b)
    d, dt = pre - y, pt + np.abs(y)
    sq_t = lambda dd, e: dd * dd + 2.0 * np.abs(dd) * e       # a square whose argument carries the error basis e
    one = m == 1.0
    cnt = float(one.sum())
    ybar = float(y[one].sum() / cnt) if cnt else 0.0
    ybt = float(np.abs(y[one]).sum() / cnt) if cnt else 0.0
    loss, loss_t = np.sum((m * d) ** 2), np.sum(m * m * sq_t(d, dt))
    stats = np.array([[loss, np.sum(d[one] ** 2), np.sum((y[one] - ybar) ** 2), cnt]])
    stats_t = np.array([[loss_t, np.sum(sq_t(d[one], dt[one])), np.sum(sq_t(y[one] - ybar, ybt)), cnt]])
    r = {'pre': Ref(pre[:, None], pt[:, None], F + 1.0), 'loss': Ref(np.array([[loss]]), np.array([[loss_t]]), nf),
         'stats': Ref(stats, stats_t, nf), 'count': int(cnt)}
    p32 = f64(f32(pre) if pre_in is None else pre_in)
    dp = 2.0 * c['g'] * m * m * (p32 - y)
    dpt = 2.0 * abs(c['g']) * m * m * (np.abs(p32) + np.abs(y))
    r['dx'] = Ref(dp[:, None] * w[None, :], dpt[:, None] * np.abs(w)[None, :], 6.0)
    r['dw'] = Ref((dp @ x)[None, :], (dpt @ np.abs(x))[None, :], nb)
    r['db'] = Ref(np.array([[dp.sum()]]), np.array([[dpt.sum()]]), nb)
    return r


NODE_N = (0, 1, 15, 16, 17, 1023, 1024, 1025, 4099)
NODE_F = (1, 2, 63, 64)
NODE_MASKS = ('ones', 'zeros', '01', 'frac')


def node_value_cases():
    """(N, F, mask, bias): every N x F with a rotating mask, every mask and b = NULL on two shapes"""
    out = [(N, F, NODE_MASKS[(i + j) % 4], True) for i, N in enumerate(NODE_N) for j, F in enumerate(NODE_F)]
    out += [(N, F, mk, bias) for N, F in ((17, 2), (1025, 63)) for mk in NODE_MASKS for bias in (True, False)]
    return sorted(set(out))


@functools.lru_cache(maxsize=128)
def node_case(N, F, mask, bias):
    c = node_inputs(N, F, mask, bias)
    return c, node_head_ref(c)


# ----------------------------------------------------------------------------------------------------------------------- BatchNorm
def bn_inputs(N, C, key=()):
    """x like a layer output, relu(1.5 randn + 0.7); dy ~ N(1, 1/4): column sums of terms of mostly one sign; weight in [0.5, 1.5].  At
    N = 1 x sits on multiples of 1/8: x^2 is exact in fp32, so var is exactly 0 (E[x^2] - mean^2 of ONE rounded square is that
    square's rounding error, which eps = 1e-5 magnifies in rstd: a property of the formula at a shape no model has)."""
    r = rng('bn', N, C, key)
    x = np.maximum(1.5 * r.standard_normal((N, C)) + 0.7, 0.0)
    if N == 1:
        x = np.round(x * 8.0) / 8.0
    return {'x': f32(x), 'dy': f32(1.0 + 0.5 * r.standard_normal((N, C))), 'weight': f32(0.5 + r.random(C)), 'bias': f32(0.5 * r.standard_normal(C))}


BN_PATTERNS = ('all', 'none', 'one', 'two', 'tail', 'alternate', 'hole', 'last block')


def bn_valid(N, pattern, x=None):
    """row validity [N] (float32 0 / 1): all; none; exactly one; exactly two (rows whose columns differ by >= 1: x is changed so);
    padding rows at the end; alternating rows; a whole 2048-row block invalid between two valid ones; valid rows only in the last,
    partial block"""
    v = np.zeros(N, np.float32)
    if pattern == 'all':
        v[:] = 1
    elif pattern == 'one':
        v[N // 2] = 1
    elif pattern == 'two':
        a, b = N // 3, N - 1
        assert a != b
        v[[a, b]] = 1
        if x is not None:
            x[b] = x[a] + np.float32(1.25) + np.abs(x[b])    # the column spread >= 1
    elif pattern == 'tail':
        v[:max(N - max(N // 5, 1), 1)] = 1
    elif pattern == 'alternate':
        v[::2] = 1
    elif pattern == 'hole':
        assert N > 2 * BN_ROWS
        v[:] = 1
        v[BN_ROWS:2 * BN_ROWS] = 0
    elif pattern == 'last block':
        assert N % BN_ROWS and N > BN_ROWS
        v[N // BN_ROWS * BN_ROWS:] = 1
    else:
        assert pattern == 'none', pattern
    return v


def _rows(valid, N):
    return np.ones(N, bool) if valid is None else np.asarray(valid) != 0


def bn_stats_ref(x, eps=EPS, valid=None):
    """{'mean', 'var', 'rstd'} Ref [1, C], 'count'.  var carries T = E[x^2] + mean^2; rstd's bound follows from var's:
    |d rstd| = rstd / 2 |d var| / (var + eps), plus rstd itself for its own rounding.  No valid row: mean 0, var 0."""
    x = f64(x)
    k = _rows(valid, x.shape[0])
    n = int(k.sum())
    xs = x[k]
    C = x.shape[1]
    if n == 0:
        mean = var = ex2 = mt = np.zeros(C)
    else:
        mean, mt, ex2 = xs.sum(0) / n, np.abs(xs).sum(0) / n, (xs * xs).sum(0) / n
        var = ((xs - mean) ** 2).sum(0) / n                   # the two-pass value: no cancellation of its own
    vt = ex2 + mean * mean
    rstd = 1.0 / np.sqrt(var + eps)
    one = lambda a: np.asarray(a, np.float64).reshape(1, C)
    return {'mean': Ref(one(mean), one(mt), BN_N), 'var': Ref(one(var), one(vt), BN_N), 'rstd': Ref(one(rstd), one(rstd * (1.0 + 0.5 * vt / (var + eps))), BN_N),
            'count': n}


def bn_apply_ref(x, mean, rstd, weight=None, bias=None, valid=None):
    """(Ref [N, C], rows that are exactly +0.0).  mean / rstd: the float32 arrays the launch is handed."""
    x, mean, rstd = f64(x), f64(mean).ravel(), f64(rstd).ravel()
    w = np.ones_like(mean) if weight is None else f64(weight)
    b = np.zeros_like(mean) if bias is None else f64(bias)
    k = _rows(valid, x.shape[0])[:, None]
    return Ref(np.where(k, (x - mean) * rstd * w + b, 0.0), np.where(k, (np.abs(x) + np.abs(mean)) * rstd * np.abs(w) + np.abs(b), 0.0), 4.0), ~k[:, 0]


def bn_bwd_sums_ref(dy, x, mean, rstd, valid=None):
    """{'sum_dy', 'sum_dyxhat'} Ref [1, C] over the valid rows"""
    dy, x, mean, rstd = f64(dy), f64(x), f64(mean).ravel(), f64(rstd).ravel()
    k = _rows(valid, x.shape[0])
    dy, x = dy[k], x[k]
    one = lambda a: a.reshape(1, -1)
    return {'sum_dy': Ref(one(dy.sum(0)), one(np.abs(dy).sum(0)), BN_N),
            'sum_dyxhat': Ref(one((dy * (x - mean) * rstd).sum(0)), one((np.abs(dy) * (np.abs(x) + np.abs(mean)) * rstd).sum(0)), BN_N + 3.0)}


def bn_bwd_apply_ref(dy, x, mean, rstd, weight, sum_dy, sum_dyxhat, n, valid=None):
    """(Ref [N, C], rows that are exactly +0.0); n: the row count the launch divides by (num_rows, or count[0])"""
    dy, x, mean, rstd = f64(dy), f64(x), f64(mean).ravel(), f64(rstd).ravel()
    sdy, sdx = f64(sum_dy).ravel(), f64(sum_dyxhat).ravel()
    w = np.ones_like(mean) if weight is None else f64(weight)
    k = _rows(valid, x.shape[0])[:, None]
    n = max(float(n), 1.0)
    xh, xht = (x - mean) * rstd, (np.abs(x) + np.abs(mean)) * rstd
    v = (dy - sdy / n - xh * sdx / n) * rstd * w
    t = (np.abs(dy) + np.abs(sdy) / n + xht * np.abs(sdx) / n) * rstd * np.abs(w)
    with np.errstate(invalid='ignore'):
        return Ref(np.where(k, v, 0.0), np.where(k, t, 0.0), 8.0), ~k[:, 0]


def bn_dx_bar(n):
    """how dx is held at n rows.  At n = 2 the two xhat are +-c, c^2 = 1 - eps / (d^2 / 4 + eps), and dx = +-(dy1 - dy2) / 2 (1 - c^2) rstd w:
    zero but for eps, a difference of equal terms, so its max-norm measures nothing.  dx is then held elementwise on its term sum
    and to its derived bound only; everywhere else to the default bar."""
    return dict(maxnorm=False, bound=True) if n == 2 else {}


def bn_running_ref(rmean, rvar, mean, var, n, momentum):
    """(running_mean, running_var) Ref [1, C] after one update, the variance unbiased by n / (n - 1); n < 2: None (both untouched)"""
    if n < 2:
        return None
    rm, rv, mean, var = (f64(a).reshape(1, -1) for a in (rmean, rvar, mean, var))
    al = momentum * n / (n - 1.0)
    return (Ref(rm * (1 - momentum) + momentum * mean, np.abs(rm) * (1 - momentum) + momentum * np.abs(mean), 3.0),
            Ref(rv * (1 - momentum) + al * var, np.abs(rv) * (1 - momentum) + al * np.abs(var), 4.0))


BN_WIDTHS = tuple(range(4, 65, 4))
BN_N_LIST = (1, 2, 15, 16, 17, 63, 64, 65, 2047, 2048, 2049, 4097, 32769)
BN_N_WIDTHS = (4, 48, 64)
BN_HOLE_N = 6145


def bn_road(N):
    nblk = -(-N // BN_ROWS)
    return 'one block' if nblk == 1 else ('several blocks' if nblk <= 16 else '17 blocks')


def bn_shapes():
    """(N, C) of the unmasked and the masked matrix"""
    return [(257, C) for C in BN_WIDTHS] + [(N, C) for N in BN_N_LIST for C in BN_N_WIDTHS]


def bn_masked_cases():
    """(N, C, pattern)"""
    out = []
    for i, (N, C) in enumerate(bn_shapes()):
        pats = ['all', 'none', 'one'] + (['two', 'tail', 'alternate'] if N >= 3 else [])
        if N > BN_ROWS and N % BN_ROWS:
            pats.append('last block')
        out += [(N, C, p) for p in (pats if N in (2049, 32769) or C == 48 else pats[i % 3::3])]
    out += [(BN_HOLE_N, C, 'hole') for C in BN_N_WIDTHS]
    return out


@functools.lru_cache(maxsize=8)
def bn_case(N, C, pattern=None):
    """inputs (+ 'valid') and the chain of references, each launch fed the float32 rounding of the reference's own statistics:
    {'stats', 'mean32', 'rstd32', 'y', 'sums', 'sdy32', 'sdx32', 'dx'}"""
    c = dict(bn_inputs(N, C, (pattern,) if pattern not in (None, 'all') else ()))     # (all valid: the unmasked case's arrays)
    valid = None
    if pattern is not None:
        c['x'] = c['x'].copy()
        valid = c['valid'] = bn_valid(N, pattern, c['x'])
        if valid.sum() == 1:                                  # as at N = 1: the one square is exact in fp32, var is exactly 0
            c['x'][valid != 0] = np.round(c['x'][valid != 0] * 8.0) / 8.0
    r = {'stats': bn_stats_ref(c['x'], EPS, valid)}
    r['mean32'], r['rstd32'] = f32(r['stats']['mean'].v), f32(r['stats']['rstd'].v)
    r['y'] = bn_apply_ref(c['x'], r['mean32'], r['rstd32'], c['weight'], c['bias'], valid)
    r['sums'] = bn_bwd_sums_ref(c['dy'], c['x'], r['mean32'], r['rstd32'], valid)
    r['sdy32'], r['sdx32'] = f32(r['sums']['sum_dy'].v), f32(r['sums']['sum_dyxhat'].v)
    r['dx'] = bn_bwd_apply_ref(c['dy'], c['x'], r['mean32'], r['rstd32'], c['weight'], r['sdy32'], r['sdx32'],
                               N if pattern is None else r['stats']['count'], valid)
    return c, r


COND_R = (1, 10, 100)
COND_N = (2049, 32769)


def bn_cond_inputs(N, r):
    """x ~ N(r, 1), C = 4: the conditioning of E[x^2] - mean^2 as the mean leaves the spread behind"""
    return f32(r + rng('bn cond', N, r).standard_normal((N, 4)))
