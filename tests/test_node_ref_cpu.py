"""tests/_node_ref.py against float64 autograd of the reference model's expressions, and the tolerances of tests/test_gpu_node_abi.py
against fp32 arithmetic itself.  No device.

1. Every reference of _node_ref is compared with torch float64 autograd of
       out = cat[relu(c), tanh(fc11 x) * tanh(fc12 x)]          (libs/spect_conv.py: the ML3Layer output stage)
       global_add_pool / global_mean_pool / global_max_pool     written with index_add_ / scatter_reduce
   at three small shapes; the term sums must dominate the values.
2. At every row count of the GPU matrix (the small list and the cap / cap + 1 sizes of each kernel class) every sum the kernels form
   -- dcb, dw11 / dw12, db11 / db12, the written dx, node-mix's accumulating dx, xty -- is evaluated in float32 numpy, on the very
   arrays the GPU matrix draws (_node_ref.stage_inputs / mix_inputs / xty_inputs, cut to N rows), twice, once sequentially over the rows and once as
   per-128-row partials folded in order (the kernels' shape), and both must pass _conv_ref.check() against the float64 reference at
   TOL_F32 = 2e-5 and at f32_bound.  A size that fails here has wrong inputs or a wrong tolerance, not a wrong kernel."""
import numpy as np
import pytest
import torch

import _conv_ref as R
import _node_ref as NR

TOL_F32 = 2e-5
N_SMALL = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000)
CAP = 131072                                                  # the row count at which each persistent grid stops growing
# (Fin, F2, nout1): the shapes the GPU matrix runs at the cap sizes, one per kernel class
CAP_SHAPES = ((16, 8, 24), (32, 2, 30), (48, 24, 40), (0, 0, 32))
XTY_CAP = (17, 33)
MIX_CAP = (17, 3)                                            # (Fin, F2) of the node-mix cap pair


def _t(a):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.abs(got - want).max(initial=0.0) <= 1e-12 * max(np.abs(want).max(initial=0.0), 1.0), what


SHAPES = ((5, 3, 1, 2), (37, 17, 5, 7), (130, 33, 16, 30))


@pytest.mark.parametrize('N,Fin,F2,nout1', SHAPES)
@pytest.mark.parametrize('form', ('plain', 'seg', 'premasked'))
def test_output_stage_reference_vs_autograd(N, Fin, F2, nout1, form):
    c = NR.stage_inputs(N, Fin, F2, nout1, pad=0)
    rng = NR.rng_of('auto', N, Fin, F2, nout1, form)
    conv = rng.standard_normal((N, nout1)).astype(np.float32)
    seg = gp = None
    gy = c['gy']
    if form == 'seg':
        nseg = max(N // 4, 1)
        seg = np.sort(rng.integers(0, nseg, N)).astype(np.int32)
        gp = gy[:nseg]
        gy = gp[seg]
    ct, xt = _t(conv).requires_grad_(), _t(c['x']).requires_grad_()
    w = [_t(c[k]).requires_grad_() for k in ('w11', 'b11', 'w12', 'b12')]
    out = torch.cat([torch.relu(ct), torch.tanh(xt @ w[0].T + w[1]) * torch.tanh(xt @ w[2].T + w[3])], 1)
    (out * _t(gy)).sum().backward()
    y = np.maximum(conv, np.float32(0.0))
    if form == 'premasked':
        gpre = gy.copy()
        gpre[:, :nout1] = ct.grad.numpy().astype(np.float32)
        r = NR.split_bwd_ref(gpre, None, None, c['x'], c['w11'], c['b11'], c['w12'], c['b12'], nout1, F2, premasked=True)
    else:
        r = NR.split_bwd_ref(gp if seg is not None else gy, seg, y, c['x'], c['w11'], c['b11'], c['w12'], c['b12'], nout1, F2)
    assert r['G'].dtype == np.float32
    _close(r['G'], ct.grad.numpy(), 'G')
    _close(r['dcb'].v, ct.grad.sum(0).numpy(), 'dcb')
    for k, t in (('dw11', w[0]), ('db11', w[1]), ('dw12', w[2]), ('db12', w[3])):
        _close(r[k].v, t.grad.numpy(), k)
    _close(r['dx'].v, xt.grad.numpy(), 'dx')
    for k in ('dcb', 'dw11', 'dw12', 'db11', 'db12', 'dx', 'dz'):
        assert (r[k].t >= np.abs(r[k].v) - 1e-300).all(), k + ': the term sum does not dominate'
    assert r['dz'].v.shape == (N, 4)
    if 2 * F2 <= 4:
        _close(r['dz'].v[:, :2 * F2] @ np.concatenate([c['w11'], c['w12']]).astype(np.float64), xt.grad.numpy(), 'dz')
        assert (r['dz'].v[:, 2 * F2:] == 0).all()
    # the forward and gml_node_mix_bwd: the same Hadamard part, dx joined to old values
    mv, mt = NR.mix_ref(c['x'], c['w11'], c['b11'], c['w12'], c['b12'])
    _close(mv, out[:, nout1:].detach().numpy(), 'mix')
    assert (mt >= np.abs(mv)).all()
    dx0 = rng.standard_normal((N, Fin)).astype(np.float32)
    m = NR.node_mix_bwd_ref(c['x'], gy[:, nout1:], c['w11'], c['b11'], c['w12'], c['b12'], dx0)
    _close(m['dx'].v, xt.grad.numpy() + dx0, 'node_mix dx')
    assert (m['dx'].t >= np.abs(dx0)).all() and float(m['dx'].n) == 2 * F2 + 1
    for k, t in (('dw11', w[0]), ('db11', w[1]), ('dw12', w[2]), ('db12', w[3])):
        _close(m[k].v, t.grad.numpy(), 'node_mix ' + k)
    assert 'dcb' not in m


def test_output_stage_reference_without_hadamard_branch_and_special_values():
    c = NR.stage_inputs(9, 0, 0, 6, pad=0)
    y = c['y'].copy()
    y[0, :4] = [0.0, -0.0, 1e-45, np.nan]
    r = NR.split_bwd_ref(c['gy'], None, y, None, None, None, None, None, 6, 0)
    want = np.where(np.nan_to_num(y, nan=-1.0) > 0, c['gy'], 0)
    assert np.array_equal(r['G'].view(np.int32), want.astype(np.float32).view(np.int32))
    assert r['G'][0, 2] == c['gy'][0, 2] and not np.signbit(r['G'][0, :2]).any() and r['G'][0, 3] == 0
    # torch's relu backward on the CPU decides the zeros and the denormal the same way.  For a NaN output it is written as
    # (y <= 0 ? 0 : g) and lets the gradient through where (y > 0) closes the gate: the kernels and this reference follow (y > 0),
    # the wording of include/gml.h -- a NaN activation has poisoned the step either way.
    g = torch.ops.aten.threshold_backward(torch.tensor(c['gy']), torch.tensor(y), 0.0).numpy()
    assert np.array_equal(g[0, :3], r['G'][0, :3]) and g[0, 3] == c['gy'][0, 3]
    assert np.array_equal(g[1:], r['G'][1:])
    assert set(r) == {'G', 'dcb'}


@pytest.mark.parametrize('n,a,b', ((1, 1, 1), (37, 17, 5), (300, 64, 49)))
def test_xty_reference(n, a, b):
    rng = NR.rng_of('xty', n, a, b)
    A, B = rng.standard_normal((n, a)).astype(np.float32), rng.standard_normal((n, b)).astype(np.float32)
    At, Bt = _t(A).requires_grad_(), _t(B)
    W = torch.zeros(a, b, dtype=torch.float64, requires_grad=True)
    ((At @ W) * Bt).sum().backward()                        # d/dW of a dense layer applied to every row: A^T B
    r = NR.xty_ref(A, B)
    _close(r.v, W.grad.numpy(), 'xty')
    assert (r.t >= np.abs(r.v)).all() and r.n == n


@pytest.mark.parametrize('sizes,F', (((3, 0, 1), 1), ((0, 5, 2, 0, 9), 7), (NR.SEG_SIZES, 32)))
def test_pool_references_vs_autograd(sizes, F):
    ptr = NR.seg_ptr(sizes)
    rows, nseg = int(ptr[-1]), len(sizes)
    rng = NR.rng_of('pool', sizes, F)
    x = rng.standard_normal((rows, F)).astype(np.float32)
    g = rng.standard_normal((nseg, F)).astype(np.float32)
    seg = torch.tensor(NR.seg_of(ptr), dtype=torch.int64)
    assert seg.numel() == rows
    ln = np.maximum(np.diff(ptr), 1)
    xt = _t(x).requires_grad_()
    add = torch.zeros(nseg, F, dtype=torch.float64).index_add_(0, seg, xt)
    s, m = NR.segment_sum_ref(x, ptr, 1)
    T = torch.zeros(nseg, F, dtype=torch.float64).index_add_(0, seg, _t(np.abs(x))).numpy()
    u = 2.0 ** -24
    assert s.dtype == np.float32 and (np.abs(s - add.detach().numpy()) <= ln[:, None] * u * T + 1e-300).all()
    assert (np.abs(m - add.detach().numpy() / ln[:, None]) <= (ln[:, None] + 1) * u * T / ln[:, None] + 1e-300).all()
    (add * _t(g)).sum().backward()
    assert np.array_equal(NR.segment_bcast_ref(g, ptr, 0), xt.grad.numpy().astype(np.float32))       # a select: exact
    xt.grad = None
    mean = torch.zeros(nseg, F, dtype=torch.float64).index_add_(0, seg, xt) / _t(ln)[:, None]
    (mean * _t(g)).sum().backward()
    bm = NR.segment_bcast_ref(g, ptr, 1)
    assert (np.abs(bm - xt.grad.numpy()) <= np.spacing(np.abs(bm)) / 2 + 1e-300).all()              # correctly rounded
    # skip-last: the last segment's row is +0.0 even where its rows are NaN
    xn = x.copy()
    xn[ptr[-2]:] = np.nan
    for flag in (2, 3):
        s2, m2 = NR.segment_sum_ref(xn, ptr, flag)
        assert np.array_equal(s2[:-1], s[:-1]) and np.array_equal(m2[:-1], m[:-1])
        assert (s2[-1].view(np.int32) == 0).all() and (m2[-1].view(np.int32) == 0).all()
    # max: random floats have no ties, so autograd's gradient is the first-row rule's
    xt.grad = None
    mx = torch.zeros(nseg, F, dtype=torch.float64).scatter_reduce(0, seg[:, None].expand(rows, F), xt, 'amax', include_self=False)
    v, arg = NR.segment_max_ref(x, ptr)
    assert np.array_equal(v, mx.detach().numpy().astype(np.float32))
    assert ((arg == -1) == (np.diff(ptr) == 0)[:, None]).all()
    (mx * _t(g)).sum().backward()
    assert np.array_equal(NR.segment_max_bwd_ref(g, ptr, arg), xt.grad.numpy().astype(np.float32))
    if F == 32:
        wds = NR.relu_words_ref(x)
        assert wds.dtype == np.uint32 and all(((int(wds[r]) >> c) & 1) == (x[r, c] > 0) for r in (0, rows // 2, rows - 1) for c in range(32))
        gm = torch.relu(_t(x)).numpy() > 0
        for nrelu in (0, 1, 30, 31, 32):
            keep = gm | (np.arange(32) >= nrelu)[None, :]
            assert np.array_equal(NR.segment_bcast_mask_ref(g, NR.seg_of(ptr), wds, nrelu), np.where(keep, g[NR.seg_of(ptr)], np.float32(0)))


def test_max_reference_takes_the_first_row_on_ties():
    ptr = NR.seg_ptr((4, 0, 3))
    x = np.array([[2, 1], [2, 5], [0, 5], [2, 5], [7, 7], [7, 8], [7, 8]], np.float32)
    v, arg = NR.segment_max_ref(x, ptr)
    assert v.tolist() == [[2, 5], [0, 0], [7, 8]] and arg.tolist() == [[0, 1], [-1, -1], [4, 5]]
    g = np.arange(6, dtype=np.float32).reshape(3, 2) + 1
    b = NR.segment_max_bwd_ref(g, ptr, arg)
    assert b.tolist() == [[1, 0], [0, 2], [0, 0], [0, 0], [5, 0], [0, 6], [0, 0]]


# ------------------------------------------------------------------------------------------------ the tolerances against fp32 itself
def _hold(val, ref, what):
    val = np.ascontiguousarray(val, np.float32).ravel()
    v, t = np.asarray(ref.v, np.float64).reshape(1, -1), np.asarray(ref.t, np.float64).reshape(1, -1)
    bound = np.broadcast_to(R.f32_bound(ref), np.asarray(ref.v).shape).reshape(1, -1)
    return R.check(val, v, t, 1, v.size, v.size, TOL_F32, what, guard_rows=0, bound=bound)


def _tanh_d32(z):
    """(tanh z, 1 - tanh^2 z) in float32, the derivative as 4 e / (1 + e)^2 with e = exp(-2 |z|): 1 - t * t loses every digit where
    tanh saturates, and a column sum whose units all saturate (Fin = F2 = 1 with a large weight) then misses the max-norm bar through
    that cancellation alone -- the kernels' gml_tanh_d avoids it the same way"""
    z = np.asarray(z, np.float32)
    e = np.exp(np.float32(-2.0) * np.abs(z)).astype(np.float32)
    return np.tanh(z), (np.float32(4.0) * e / ((np.float32(1.0) + e) * (np.float32(1.0) + e))).astype(np.float32)


def _two_orders(terms, N):
    """(sequential float32 sum over the rows, per-128-row partials folded in order) of terms(r0, r1) -> float32 [rows, K]"""
    seq = part = None
    for r0 in range(0, N, 128):
        t = terms(r0, min(r0 + 128, N))
        seq = np.add.accumulate(t if seq is None else np.concatenate([seq[None], t]), axis=0, dtype=np.float32)[-1]
        p = np.add.accumulate(t, axis=0, dtype=np.float32)[-1]
        part = p if part is None else (part + p).astype(np.float32)
    return seq, part


def _stage_in_fp32(N, Fin, F2, nout1):
    c = {k: (v[:N] if k in ('gy', 'y', 'x') else v) for k, v in NR.stage_inputs(N, Fin, F2, nout1).items()}   # the GPU matrix's own draw
    ref = NR.split_bwd_ref(c['gy'], None, c['y'], c['x'] if F2 else None, c['w11'], c['b11'], c['w12'], c['b12'], nout1, F2)
    G = ref['G']
    wc = np.concatenate([c['w11'], c['w12']])
    dxs = []

    def terms(r0, r1):
        cols = [G[r0:r1]]
        if F2:
            x = c['x'][r0:r1]
            z1, z2 = (x @ c['w11'].T + c['b11']).astype(np.float32), (x @ c['w12'].T + c['b12']).astype(np.float32)
            (t1, d1), (t2, d2) = _tanh_d32(z1), _tanh_d32(z2)
            g = c['gy'][r0:r1, nout1:]
            dz = np.concatenate([g * t2 * d1, g * t1 * d2], 1).astype(np.float32)
            dx = np.zeros((r1 - r0, Fin), np.float32)
            for o in range(2 * F2):                          # an fmaf chain's order, one rounding more per step
                dx = (dx + dz[:, o:o + 1] * wc[o]).astype(np.float32)
            dxs.append(dx)
            cols += [dz, (dz[:, :, None] * x[:, None, :]).reshape(r1 - r0, -1)]
        return np.concatenate(cols, 1)

    _hold_stage(terms, dxs, ref, N, Fin, F2, nout1)


def _hold_stage(terms, dxs, ref, N, Fin, F2, nout1):
    seq, part = _two_orders(terms, N)
    for name, v in (('sequential', seq), ('partials', part)):
        what = '%s N=%d Fin=%d F2=%d nout1=%d ' % (name, N, Fin, F2, nout1)
        if nout1:
            _hold(v[:nout1], ref['dcb'], what + 'dcb')
        if F2:
            o = nout1
            _hold(v[o:o + F2], ref['db11'], what + 'db11')
            _hold(v[o + F2:o + 2 * F2], ref['db12'], what + 'db12')
            dw = v[o + 2 * F2:].reshape(2 * F2, Fin)
            _hold(dw[:F2], ref['dw11'], what + 'dw11')
            _hold(dw[F2:], ref['dw12'], what + 'dw12')
    if F2:
        _hold(np.concatenate(dxs), ref['dx'], 'N=%d Fin=%d F2=%d dx' % (N, Fin, F2))


@pytest.mark.parametrize('Fin,F2,nout1', ((1, 1, 1), (17, 3, 5), (33, 16, 30), (64, 24, 64), (0, 0, 32)))
def test_fp32_meets_the_tolerances_at_the_small_row_counts(Fin, F2, nout1):
    for N in N_SMALL:
        _stage_in_fp32(N, Fin, F2, nout1)


@pytest.mark.parametrize('Fin,F2,nout1', CAP_SHAPES)
@pytest.mark.parametrize('N', (CAP, CAP + 1))
def test_fp32_meets_the_tolerances_at_the_grid_caps(N, Fin, F2, nout1):
    _stage_in_fp32(N, Fin, F2, nout1)


def _mix_in_fp32(N, Fin, F2):
    """gml_node_mix_bwd's sums: dw*, db* and the ACCUMULATING dx = dx0 + dz [w11; w12] (n = 2 F2 + 1), on the GPU matrix's own draw"""
    c = NR.mix_inputs(N, Fin, F2)
    x, g = c['x'][:N], c['g'][:N]
    ref = NR.node_mix_bwd_ref(x, g, c['w11'], c['b11'], c['w12'], c['b12'], c['dx0'])
    wc = np.concatenate([c['w11'], c['w12']])
    dxs = []

    def terms(r0, r1):
        xb = x[r0:r1]
        t1, d1 = _tanh_d32((xb @ c['w11'].T + c['b11']).astype(np.float32))
        t2, d2 = _tanh_d32((xb @ c['w12'].T + c['b12']).astype(np.float32))
        dz = np.concatenate([g[r0:r1] * t2 * d1, g[r0:r1] * t1 * d2], 1).astype(np.float32)
        dx = np.zeros((r1 - r0, Fin), np.float32)
        for o in range(2 * F2):
            dx = (dx + dz[:, o:o + 1] * wc[o]).astype(np.float32)
        dxs.append((c['dx0'][r0:r1] + dx).astype(np.float32))            # the kernel's order: the old value joins last
        return np.concatenate([dz, (dz[:, :, None] * xb[:, None, :]).reshape(r1 - r0, -1)], 1)

    _hold_stage(terms, dxs, ref, N, Fin, F2, 0)


@pytest.mark.parametrize('Fin,F2', ((1, 1), (15, 3), (32, 8), (33, 15), (64, 24)))
def test_fp32_node_mix_meets_the_tolerances_at_the_small_row_counts(Fin, F2):
    for N in N_SMALL:
        _mix_in_fp32(N, Fin, F2)


@pytest.mark.parametrize('N', (CAP, CAP + 1))
def test_fp32_node_mix_meets_the_tolerances_at_the_grid_cap(N):
    _mix_in_fp32(N, *MIX_CAP)


@pytest.mark.parametrize('n,a,b', [(n, 17, 49) for n in N_SMALL] + [(CAP,) + XTY_CAP, (CAP + 1,) + XTY_CAP, (1000, 64, 64)])
def test_fp32_xty_meets_the_tolerances(n, a, b):
    A, B = (m[:n] for m in NR.xty_inputs(n, a, b))          # the GPU matrix's own draw
    ref = NR.xty_ref(A, B)
    seq, part = _two_orders(lambda r0, r1: (A[r0:r1, :, None] * B[r0:r1, None, :]).reshape(r1 - r0, -1), n)
    _hold(seq, ref, 'sequential xty n=%d' % n)
    _hold(part, ref, 'partials xty n=%d' % n)
