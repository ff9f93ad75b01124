"""tests/_readout_ref.py held to float64 autograd at 1e-12, and the tolerances of tests/test_gpu_readout_abi.py shown to be reachable:
every output is evaluated here in PLAIN float32 numpy on the very arrays the GPU matrix uploads -- sequentially, in the kernels'
partial shapes (256-row slabs folded in order; 2048-row blocks of 16 chains of 128 rows, the blocks combined in double; the node
head's strided chains and its tree) -- and passed through the same _readout_ref.hold() with the same tolerances.  The generators'
margins are asserted with no row left out, and the one-workgroup head's shape predicate is checked against the two launchers' LDS
formulas over its whole grid.  No device."""
import numpy as np
import pytest
import torch

import _readout_ref as Q

F32 = np.float32


def _close(got, ref, what, tol=1e-12):
    got, ref = np.asarray(got, np.float64), np.asarray(ref.detach().numpy() if torch.is_tensor(ref) else ref, np.float64)
    e = np.abs(got.reshape(ref.shape) - ref).max() / max(np.abs(ref).max(), 1e-300) if ref.size else 0.0
    assert e <= tol, '%s: %.3e' % (what, e)


def _t(a, grad=False):
    return None if a is None else torch.tensor(np.asarray(a, np.float64), requires_grad=grad)


# ------------------------------------------------------------------------------------------- the reference against float64 autograd
def _head_autograd(c, bce):
    p, w1, w2 = _t(c['p'], True), _t(c['w1'], True), _t(c['w2'], True)
    b1, b2 = _t(c['b1'], True), _t(c['b2'], True)
    a = torch.nn.functional.linear(p, w1, b1)
    h = torch.relu(a) if (not bce or c['act']) else a
    z = h @ w2 + (b2[0] if b2 is not None else 0.0)
    y = _t(c['y'])
    v = torch.ones_like(y) if c['valid'] is None else _t(c['valid'])
    Rl = c['rows_loss']
    if bce:
        l = torch.nn.functional.binary_cross_entropy_with_logits(z, y, reduction='none')
    else:
        l = (z - y).abs()
    loss = (v * l)[:Rl].sum()
    (loss * (1.0 if c['gscale'] is None else c['gscale'])).backward()
    g = lambda t, like: np.zeros(like.shape) if t is None or t.grad is None else t.grad.numpy()
    return loss, z, g(p, c['p']), g(w1, c['w1']), None if b1 is None else g(b1, c['b1']), g(w2, c['w2']), None if b2 is None else g(b2, c['b2'])


def _against_autograd(c, r, bce, what):
    loss, z, gp, dw1, db1, dw2, db2 = _head_autograd(c, bce)
    _close(r['loss'].v, loss, what + ' loss')
    _close(r['pre'].v[:, 0], z, what + ' pre')
    for k, g in (('gp', gp), ('dw1', dw1), ('db1', db1), ('dw2', dw2), ('db2', db2)):
        if g is not None:
            _close(r[k].v, g, what + ' ' + k, 1e-11 if bce else 1e-12)
    assert not r['gp'].v[r['gp_zero']].any() and not r['gp'].t[r['gp_zero']].any(), what + ': a row of the select has terms'
    for k in ('loss', 'pre', 'gp', 'dw1', 'db1', 'dw2', 'db2'):
        assert (np.abs(r[k].v) <= r[k].t * (1 + 1e-12) + 1e-300).all(), what + ': %s exceeds its term sum' % k


SMALL_L1 = [c for c in Q.l1_value_cases() if c[0] in (3, 65, 189)]


@pytest.mark.parametrize('rows,nin,nh,family,kw', SMALL_L1, ids=lambda v: str(v).replace(' ', ''))
def test_l1_reference_is_autograd(rows, nin, nh, family, kw):
    c, r = Q.l1_case(rows, nin, nh, family, **kw)
    if family == 'dyadic':                                   # autograd's sign(0) = 0 and relu'(0) = 0 are the reference's
        assert (r['gp_zero'][:kw['rows_loss']:5]).all()
    _against_autograd(c, r, False, 'l1 %s' % ((rows, nin, nh, family, kw),))


@pytest.mark.parametrize('rows,nin,nh,act', [(257, 5, 1, 1), (300, 48, 10, 1), (300, 64, 64, 0)])
def test_bce_reference_is_autograd(rows, nin, nh, act):
    c, r = Q.bce_case(rows, nin, nh, act, rows - 1)
    _against_autograd(c, r, True, 'bce %s' % ((rows, nin, nh, act),))
    z, y = r['pre'].v[:, 0], c['y']
    v = c['valid'] * (np.arange(rows) < rows - 1)
    assert r['ok'] == int(np.sum(v * ((z > 0) == (y == 1)))) and r['n'] == int(np.sum(v != 0)) and r['ok_f'] == r['ok']


@pytest.mark.parametrize('N,F,mask,bias', [c for c in Q.node_value_cases() if c[0] in (17, 1025)], ids=str)
def test_node_head_reference_is_autograd(N, F, mask, bias):
    """filtering's square(mask (pre - y)).sum(); r2's sums over the rows with mask == 1"""
    c, r = Q.node_case(N, F, mask, bias)
    x, w, b = _t(c['x'], True), _t(c['w'], True), _t(c['b'], True)
    pre = x @ w + (b[0] if b is not None else 0.0)
    y, m = _t(c['y']), _t(c['mask'])
    loss = torch.square(m * (pre - y)).sum()
    _close(r['pre'].v[:, 0], pre, 'pre')
    _close(r['loss'].v, loss, 'loss')
    one = c['mask'] == 1
    yy, pp = y.numpy()[one], pre.detach().numpy()[one]
    want = [float(loss.detach()), ((yy - pp) ** 2).sum(), ((yy - yy.mean()) ** 2).sum() if one.any() else 0.0, one.sum()]
    _close(r['stats'].v[0], np.array(want), 'stats')
    # the backward from the float64 pre: the reference's backward reads a float32 pre, so restate it on the exact one
    rb = Q.node_head_ref(dict(c), pre_in=None)
    (loss * c['g']).backward()
    c64 = dict(c)
    r64 = _node_bwd_exact(c64, pre.detach().numpy())
    _close(r64['dx'], x.grad, 'dx')
    _close(r64['dw'], w.grad, 'dw')
    if b is not None:
        _close(r64['db'], b.grad, 'db')
    # ... and the float32 rounding of pre moves it by no more than its own term-sum allowance
    for k in ('dx', 'dw', 'db'):
        assert (np.abs(rb[k].v.ravel() - np.asarray(r64[k]).ravel()) <= 2.0 ** -23 * rb[k].t.ravel() + 1e-300).all(), k


def _node_bwd_exact(c, pre):
    """node_head_ref's backward on a float64 pre (np.float64 passes through f64(f32(.)) unchanged only if handed as pre_in)"""
    x, w, y, m = (np.asarray(c[k], np.float64) for k in ('x', 'w', 'y', 'mask'))
    dp = 2.0 * c['g'] * m * m * (pre - y)
    return {'dx': dp[:, None] * w[None, :], 'dw': dp @ x, 'db': dp.sum()}


@pytest.mark.parametrize('N,C', [(1, 4), (2, 48), (65, 12), (257, 64), (2049, 48)])
@pytest.mark.parametrize('pattern', [None, 'all', 'one', 'two', 'tail', 'alternate'])
def test_batchnorm_reference_is_torch_batchnorm_in_double(N, C, pattern):
    """torch.nn.BatchNorm1d(C).double() in training mode over all rows, and over the valid rows only"""
    if pattern in ('two', 'tail', 'alternate') and N < 3:
        pattern = 'all'
    x = Q.bn_inputs(N, C)['x'].copy()
    c = Q.bn_inputs(N, C)
    valid = None if pattern is None else Q.bn_valid(N, pattern, x)
    k = np.ones(N, bool) if valid is None else valid != 0
    n = int(k.sum())
    st = Q.bn_stats_ref(x, Q.EPS, valid)
    assert st['count'] == n
    if n < 2:                                                # torch refuses one row in training mode: the formulas directly
        _close(st['mean'].v, x[k].astype(np.float64).mean(0)[None], 'mean')
        assert not st['var'].v.any() and np.allclose(st['rstd'].v, Q.EPS ** -0.5, rtol=1e-14)
        return
    bn = torch.nn.BatchNorm1d(C, eps=Q.EPS, momentum=0.1).double()
    with torch.no_grad():
        bn.weight.copy_(_t(c['weight']))
        bn.bias.copy_(_t(c['bias']))
        bn.running_mean.copy_(_t(c['bias']))
        bn.running_var.copy_(_t(c['weight']))
    xs = _t(x[k], True)
    y = bn(xs)
    (y * _t(c['dy'][k])).sum().backward()
    mean, var = np.asarray(x[k], np.float64).mean(0), np.asarray(x[k], np.float64).var(0)
    _close(st['mean'].v[0], mean, 'mean')
    _close(st['var'].v[0], var, 'var', 1e-11)
    _close(st['rstd'].v[0], 1 / np.sqrt(var + Q.EPS), 'rstd', 1e-11)
    # the launches are handed float32 statistics; held to autograd, the reference is evaluated on the float64 ones
    yr, zero = Q.bn_apply_ref(x, st['mean'].v, st['rstd'].v, c['weight'], c['bias'], valid)
    _close(yr.v[k], y, 'y', 1e-11)
    assert np.array_equal(zero, ~k) and not yr.v[~k].any() and not yr.t[~k].any()
    sm = Q.bn_bwd_sums_ref(c['dy'], x, st['mean'].v, st['rstd'].v, valid)
    _close(sm['sum_dy'].v[0], bn.bias.grad, 'sum_dy', 1e-11)
    _close(sm['sum_dyxhat'].v[0], bn.weight.grad, 'sum_dyxhat', 1e-10)
    dx, zero = Q.bn_bwd_apply_ref(c['dy'], x, st['mean'].v, st['rstd'].v, c['weight'], sm['sum_dy'].v, sm['sum_dyxhat'].v, n, valid)
    _close(dx.v[k], xs.grad, 'dx', 1e-9)                    # (dx cancels dy against its mean: 1e-9 of the max-norm is 1e-12 of the terms)
    assert not dx.v[~k].any()
    run = Q.bn_running_ref(c['bias'], c['weight'], st['mean'].v, st['var'].v, n, 0.1)
    _close(run[0].v[0], bn.running_mean, 'running_mean')
    _close(run[1].v[0], bn.running_var, 'running_var', 1e-11)
    assert Q.bn_running_ref(c['bias'], c['weight'], st['mean'].v, st['var'].v, 1, 0.1) is None


# ---------------------------------------------------------------------------------------------------------- plain fp32 restatements
def _seq_dot(bias, A, B):
    """float32 [m, n]: bias + sum_k A[:, k] B[:, k] accumulated in ascending k (A [m, K], B [n, K])"""
    acc = np.zeros((A.shape[0], B.shape[0]), F32) + (F32(0) if bias is None else np.asarray(bias, F32))
    for k in range(A.shape[1]):
        acc = acc + A[:, k, None] * B[None, :, k]
    return acc


def _slab_sum(terms, rows):
    """float32 sum over the leading axis (rows): 256-row slabs, each summed in ascending row order, the slabs folded in ascending
    order (a workgroup's slabs and then the workgroups: one ascending chain is the longer one)"""
    nsl = -(-rows // Q.SLAB)
    pad = np.zeros((nsl * Q.SLAB,) + terms.shape[1:], F32)
    pad[:rows] = terms
    pad = pad.reshape((nsl, Q.SLAB) + terms.shape[1:])
    acc = np.zeros((nsl,) + terms.shape[1:], F32)
    for i in range(Q.SLAB):
        acc = acc + pad[:, i]
    out = acc[0]
    for s in range(1, nsl):
        out = out + acc[s]
    return out


def head_f32(c, bce):
    """every output of a head in plain float32"""
    p, w1, w2 = c['p'], c['w1'], c['w2'].reshape(1, -1)
    rows, nin = p.shape
    nh = w1.shape[0]
    a = _seq_dot(c['b1'], p, w1)
    h = np.maximum(a, F32(0)) if (not bce or c['act']) else a
    z = _seq_dot(c['b2'], h, w2)[:, 0]
    v = np.ones(rows, F32) if c['valid'] is None else c['valid']
    inl = np.arange(rows) < c['rows_loss']
    gs = F32(1.0 if c['gscale'] is None else c['gscale'])
    y = c['y']
    if bce:
        l1p = np.log1p(np.exp(-np.abs(z))).astype(F32)
        sp, sn = np.minimum(np.maximum(z, F32(0)) + l1p, F32(100)), np.minimum(np.maximum(-z, F32(0)) + l1p, F32(100))
        l = np.where(inl, v * (y * sn + (F32(1) - y) * sp), F32(0)).astype(F32)
        e = np.exp(-np.abs(z)).astype(F32)
        sg = lambda t: (np.where(t >= 0, F32(1), e) / (F32(1) + e)).astype(F32)
        s = np.where(inl, gs * v * np.where(y == 1, -sg(-z), sg(z) - y), F32(0)).astype(F32)
        on = h > 0 if c['act'] else np.ones(h.shape, bool)
    else:
        d = z - y
        l = np.where(inl, np.abs(d) * v, F32(0)).astype(F32)
        s = np.where(inl, np.sign(d) * v * gs, F32(0)).astype(F32)
        on = h > 0
    dh = np.where(on, s[:, None] * w2, F32(0)).astype(F32)
    out = {'pre': z, 'loss': _slab_sum(l, rows), 'gp': _seq_dot(None, dh, np.ascontiguousarray(w1.T)),
           'dw1': _slab_sum(dh[:, :, None] * p[:, None, :], rows) if rows * nh * nin <= 3 << 20 else _dw1_blocked(dh, p, rows),
           'db1': _slab_sum(dh, rows), 'dw2': _slab_sum(s[:, None] * h, rows), 'db2': _slab_sum(s, rows)}
    assert all(o.dtype == F32 for o in out.values())
    return out


def _dw1_blocked(dh, p, rows):
    """_slab_sum of dh[:, j, None] p[:, None, k] without the [rows, nh, nin] array"""
    nsl = -(-rows // Q.SLAB)
    pd = lambda a: np.concatenate([a, np.zeros((nsl * Q.SLAB - rows, a.shape[1]), F32)]).reshape(nsl, Q.SLAB, a.shape[1])
    A, B = pd(dh), pd(p)
    acc = np.zeros((nsl, dh.shape[1], p.shape[1]), F32)
    for i in range(Q.SLAB):
        acc += A[:, i, :, None] * B[:, i, None, :]
    out = acc[0]
    for s in range(1, nsl):
        out = out + acc[s]
    return out


def _hold_head(c, r, o, what, tol=Q.TOL_F32, bound=True):
    for k in ('pre', 'loss', 'gp', 'dw1', 'db1', 'dw2', 'db2'):
        Q.hold_values(o[k], r[k], what + ' ' + k, tol=tol, bound=bound and k in Q.SUMS)
    assert not o['gp'][r['gp_zero']].any(), what + ': a row of the select is not zero in fp32 either'


@pytest.mark.parametrize('rows,nin,nh,family,kw', Q.l1_value_cases(), ids=lambda v: str(v).replace(' ', ''))
def test_l1_tolerances_are_reachable_in_plain_fp32(rows, nin, nh, family, kw):
    c, r = Q.l1_case(rows, nin, nh, family, **kw)
    o = head_f32(c, False)
    _hold_head(c, r, o, 'l1 fp32 %s' % ((rows, nin, nh, family),))
    a_min, d_min = r['margin']
    if family == 'dyadic':
        assert np.array_equal(o['pre'].astype(np.float64), r['pre'].v[:, 0]), 'a dyadic logit is not exact in fp32'
        assert np.array_equal(o['db2'].astype(np.float64).ravel(), r['db2'].v.ravel()), 'db2 of the dyadic family is not exact in fp32'
        assert d_min == 0.0 and (a_min == 0.0 or rows < 64), 'the dyadic family no longer holds sign(0) and relu\'(0)'
    else:
        assert a_min >= Q.MARGIN and d_min >= Q.MARGIN, (a_min, d_min)
    if kw['rows_loss'] == 0:
        for k in ('loss', 'gp', 'dw1', 'db1', 'dw2', 'db2'):
            assert not r[k].v.any() and not np.asarray(o[k]).any()


@pytest.mark.parametrize('rows,family,kw', Q.big_value_cases(), ids=lambda v: str(v).replace(' ', ''))
def test_big_head_tolerances_are_reachable_in_plain_fp32(rows, family, kw):
    c, r = Q.l1_case(rows, 32, 32, family, sums='slabs', **kw)
    _hold_head(c, r, head_f32(c, False), 'big fp32 %s' % ((rows, family),))
    if family != 'dyadic':
        assert min(r['margin']) >= Q.MARGIN, r['margin']
    if rows > 4096:
        Q._l1_large.cache_clear()


@pytest.mark.parametrize('rows,nin,nh,act', Q.BCE_BIG + (Q.BCE_ODD, Q.BCE_ONE))
def test_bce_tolerances_are_reachable_in_plain_fp32(rows, nin, nh, act):
    c, r = Q.bce_case(rows, nin, nh, act, rows - 1)
    o = head_f32(c, True)
    _hold_head(c, r, o, 'bce fp32 %s' % ((rows, nin, nh, act),), tol=Q.TOL_BCE, bound=False)
    a_min, z_min, z_max = r['margin']
    assert a_min >= Q.BCE_RELU and Q.BCE_Z[0] <= z_min and z_max <= Q.BCE_Z[1], r['margin']
    z, y = o['pre'], c['y']
    v = c['valid'] * (np.arange(rows) < rows - 1)
    assert int(np.sum(v * ((z > 0) == (y == 1)))) == r['ok'] and int(np.sum(v != 0)) == r['n']
    Q.bce_case.cache_clear()


def test_the_redraw_leaves_no_row_out_and_needs_no_seed_list():
    """the rounds the issue's shapes need; SEEDS stays empty: every key serves, because rows are redrawn and none is dropped"""
    assert Q.SEEDS == {}
    for (rows, nin, nh), most in (((65537, 32, 32), 4), ((256, 64, 64), 4), ((189, 64, 64), 4)):
        c, rounds = Q.head_inputs(rows, nin, nh, rows_loss=rows - 1)
        assert c['p'].shape == (rows, nin) and c['y'].shape == (rows,) and 1 <= rounds <= most, (rows, rounds)
        a_min, d_min = Q.head_l1_ref(c)['margin']
        assert a_min >= Q.MARGIN and d_min >= Q.MARGIN


def _tree(v):
    v = v.copy()
    n = v.shape[0]
    while n > 1:
        n //= 2
        v[:n] = v[:n] + v[n:2 * n]
    return v[0]


def _strided(terms, stride):
    """float32 [stride, ...]: thread t's chain over rows t, t + stride, ... in ascending order"""
    N = terms.shape[0]
    k = -(-max(N, 1) // stride)
    pad = np.zeros((k * stride,) + terms.shape[1:], F32)
    pad[:N] = terms
    pad = pad.reshape((k, stride) + terms.shape[1:])
    acc = np.zeros((stride,) + terms.shape[1:], F32)
    for i in range(k):
        acc = acc + pad[i]
    return acc


@pytest.mark.parametrize('N,F,mask,bias', Q.node_value_cases(), ids=str)
def test_node_head_tolerances_are_reachable_in_plain_fp32(N, F, mask, bias):
    c, r = Q.node_case(N, F, mask, bias)
    x, w, y, m = c['x'], c['w'], c['y'], c['mask']
    pre = _seq_dot(c['b'], x, w.reshape(1, -1))[:, 0]
    d = pre - y
    one = m == 1
    sums = [_tree(_strided(t.astype(F32), 1024)) for t in ((m * d) * (m * d), np.where(one, d * d, F32(0)), np.where(one, y, F32(0)), one.astype(F32))]
    ybar = sums[2] / sums[3] if sums[3] > 0 else F32(0)
    tot = _tree(_strided(np.where(one, (y - ybar) * (y - ybar), F32(0)).astype(F32), 1024))
    what = 'node fp32 %s' % ((N, F, mask, bias),)
    if N:
        Q.hold_values(pre, Q.Ref(r['pre'].v.T, r['pre'].t.T, r['pre'].n), what + ' pre')
    Q.hold_values(np.array([sums[0]]), r['loss'], what + ' loss', bound=True)
    Q.hold_values(np.array([sums[0], sums[1], tot, sums[3]]), r['stats'], what + ' stats', bound=True)
    assert int(sums[3]) == r['count']
    p32 = Q.f32(r['pre'].v[:, 0])                              # the backward is handed the reference's pre
    dp = (F32(2.0) * F32(c['g'])) * m * m * (p32 - y)
    if N:
        Q.hold_values(dp[:, None] * w[None, :], r['dx'], what + ' dx')
    fold = lambda part: np.add.accumulate(np.concatenate([np.zeros((1,) + part.shape[1:], F32), part]), axis=0, dtype=F32)[-1]
    Q.hold_values(fold(_strided((dp[:, None] * x).astype(F32), 16)), r['dw'], what + ' dw', bound=True)
    Q.hold_values(np.array([fold(_strided(dp.astype(F32), 16))]), r['db'], what + ' db', bound=True)


def bn_colsums_f32(a, b=None, valid=None):
    """gml_k_bn_colsums in plain fp32: per 2048-row block, thread (ty, quad) walks rows ty, ty + 16, ... (128 of them) in order, the 16
    partials are folded in ascending ty, the blocks combined in double.  b None: (sum a, sum a^2); else (sum a, sum a b)."""
    N, C = a.shape
    nblk = -(-N // Q.BN_ROWS)
    k = np.ones(N, bool) if valid is None else valid != 0
    t0 = np.where(k[:, None], a, F32(0))
    t1 = np.where(k[:, None], a * (a if b is None else b), F32(0)).astype(F32)
    out = []
    for t in (t0, t1):
        pad = np.zeros((nblk * Q.BN_ROWS, C), F32)
        pad[:N] = t
        pad = pad.reshape(nblk, 128, 16, C)
        acc = np.zeros((nblk, 16, C), F32)
        for i in range(128):
            acc = acc + pad[:, i]
        part = acc[:, 0]
        for j in range(1, 16):
            part = part + acc[:, j]
        out.append(part.astype(np.float64).sum(0))
    return out


def bn_stats_f32(x, valid=None, eps=Q.EPS):
    s0, s1 = bn_colsums_f32(x, None, valid)
    n = float(x.shape[0] if valid is None else (valid != 0).sum())
    m = s0 / n if n else np.zeros_like(s0)
    v = np.maximum(s1 / n - m * m, 0.0) if n else np.zeros_like(s0)
    return Q.f32(m), Q.f32(v), Q.f32(1.0 / np.sqrt(v + eps))


def _bn_chain_f32(c, r, N, C, pattern, what):
    valid = c.get('valid')
    k = np.ones(N, bool) if valid is None else valid != 0
    x = np.where(k[:, None], c['x'], F32(0)) if valid is not None else c['x']          # (the selects: invalid rows take no part)
    dy = np.where(k[:, None], c['dy'], F32(0)) if valid is not None else c['dy']
    m, v, rs = bn_stats_f32(c['x'] if valid is None else x, valid)
    st = r['stats']
    for name, got in (('mean', m), ('var', v), ('rstd', rs)):
        Q.hold_values(got, st[name], what + ' ' + name, bound=True)
    mu, rstd, w, b = r['mean32'], r['rstd32'], c['weight'], c['bias']
    y = np.where(k[:, None], ((x - mu) * rstd) * w + b, F32(0)).astype(F32)
    Q.hold_values(y, r['y'][0], what + ' y')
    s0, s1 = bn_colsums_f32(dy, ((x - mu) * rstd).astype(F32), valid)
    Q.hold_values(Q.f32(s0), r['sums']['sum_dy'], what + ' sum_dy', bound=True)
    Q.hold_values(Q.f32(s1), r['sums']['sum_dyxhat'], what + ' sum_dyxhat', bound=True)
    n = N if pattern is None else st['count']
    if n:
        invn = F32(1) / F32(n)
        dx = np.where(k[:, None], ((dy - r['sdy32'] * invn - ((x - mu) * rstd) * (r['sdx32'] * invn)) * rstd) * w, F32(0)).astype(F32)
        Q.hold_values(dx, r['dx'][0], what + ' dx', **Q.bn_dx_bar(n))
        if N == 1:
            assert not dx.any() and not v.any() and np.allclose(rs, Q.EPS ** -0.5, rtol=1e-6), 'N = 1: var = 0, rstd = eps^-1/2, dx = 0'


@pytest.mark.parametrize('N,C', Q.bn_shapes())
def test_batchnorm_tolerances_are_reachable_in_plain_fp32(N, C):
    c, r = Q.bn_case(N, C)
    _bn_chain_f32(c, r, N, C, None, 'bn fp32 %s' % ((N, C),))


@pytest.mark.parametrize('N,C,pattern', Q.bn_masked_cases())
def test_masked_batchnorm_tolerances_are_reachable_in_plain_fp32(N, C, pattern):
    c, r = Q.bn_case(N, C, pattern)
    want = {'all': N, 'none': 0, 'one': 1, 'two': 2}.get(pattern)
    assert want is None or r['stats']['count'] == want
    if pattern == 'two':
        xs = c['x'][c['valid'] != 0]
        assert (np.abs(xs[0] - xs[1]) >= 1).all()
    _bn_chain_f32(c, r, N, C, pattern, 'masked bn fp32 %s' % ((N, C, pattern),))


@pytest.mark.parametrize('N', Q.COND_N)
def test_batchnorm_conditioning_in_plain_fp32(N):
    """E[x^2] - mean^2 on x ~ N(r, 1): var stays inside its derived bound and inside TOL_F32 of T = E[x^2] + mean^2 while its RELATIVE
    error grows like r^2 -- a property of the formula, so var is not held to the max-norm bar here"""
    rel = {}
    for r in Q.COND_R:
        x = Q.bn_cond_inputs(N, r)
        st = Q.bn_stats_ref(x)
        m, v, rs = bn_stats_f32(x)
        Q.hold_values(v, st['var'], 'cond var r=%d' % r, bound=True, maxnorm=False)
        Q.hold_values(rs, st['rstd'], 'cond rstd r=%d' % r, bound=True, maxnorm=False)
        rel[r] = float(np.abs(v - st['var'].v[0]).max() / st['var'].v[0].max())
    print('N = %d: relative error of var in plain fp32 at r = 1 / 10 / 100: %.1e / %.1e / %.1e' % (N, rel[1], rel[10], rel[100]))
    assert rel[1] < 2e-6 and rel[100] > rel[1]


# ---------------------------------------------------------------------------------------------------------------- the LDS predicate
def test_head_l1_supported_implies_both_launchers_accept():
    """functional.head_l1_supported restated (l1_predicate) and compared with the function itself; over rows in [1, 256] and nin, nh in
    {4, 8, ..., 64} the predicate implies that gml_head_l1_fwd and gml_head_l1_bwd accept; the three edges at 64 -> 64"""
    from gnn_matlang_amd import functional as Fn
    for rows in range(1, 257):
        for nin in range(4, 65, 4):
            for nh in range(4, 65, 4):
                if Q.l1_predicate(rows, nin, nh):
                    assert Q.l1_fwd_fits(rows, nin, nh) and Q.l1_bwd_fits(rows, nin, nh), (rows, nin, nh)
    edge = lambda f: max(r for r in range(1, 400) if f(r, 64, 64))
    assert (edge(Q.l1_predicate), edge(Q.l1_bwd_fits), edge(Q.l1_fwd_fits)) == (188, 189, 256)
    assert Q.L1_EDGE == ((188, 64, 64), (189, 64, 64), (256, 64, 64))

    class _T(object):                                        # what the predicate reads of a tensor
        def __init__(self, r, c):
            self.is_cuda, self.dtype, self._s = True, torch.float32, (r, c)

        def size(self, i):
            return self._s[i]

    for rows, nin, nh in ((188, 64, 64), (189, 64, 64), (256, 4, 4), (256, 64, 4), (100, 12, 48), (257, 4, 4), (3, 6, 4), (3, 4, 68)):
        assert bool(Fn.head_l1_supported(_T(rows, nin), _T(nh, nin), _T(1, nh))) == Q.l1_predicate(rows, nin, nh), (rows, nin, nh)


def test_roads_of_the_matrix():
    """the row counts of the matrix reach every road the GPU file's last test asks for"""
    assert {Q.road(r) for r in Q.BIG_ROWS} == {'one slab', 'several slabs', 'second trip'}
    assert {Q.road(c[0]) for c in Q.BCE_BIG + (Q.BCE_ODD, Q.BCE_ONE)} == {'one slab', 'several slabs', 'second trip'}
    assert {Q.bn_road(n) for n, _ in Q.bn_shapes()} == {'one block', 'several blocks', '17 blocks'}
    assert {c for n, c in Q.bn_shapes() if n == 257} == set(range(4, 65, 4))
    assert Q.rowsum_n(65537, 'slabs') == 256 + 2 + 256 and Q.rowsum_n(65536, 'slabs') == 256 + 1 + 256 and Q.rowsum_n(200, 'slabs') == 200
    pats = {p for _, _, p in Q.bn_masked_cases()}
    assert pats == set(Q.BN_PATTERNS), pats
