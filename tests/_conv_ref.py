"""float64 restatement of the conv ABI of include/gml.h -- forward (gml_spectconv_fwd, gml_ml3_fwd, gml_spmm_fwd_ex) and fused
backward (gml_spectconv_bwd, _bwd_mix, _bwd_mix_relu, _bwd_mix_relu2, _bwd_had) -- and the checker the ABI tests hold a launch to.
Plain numpy, no device.

    H[r, s, :] = sum_{k in row r} val[k, s] x[col[k], :]                 spmm_ref
    out        = act(sum_s H[:, s, :] W_s + bias + out0)                 conv_ref
    mix        = tanh(x w11^T + b11) * tanh(x w12^T + b12)               mix_ref

`out0` is what the output held before a GML_ACCUM call.  GML_RELU is the flag's own wording, "out = max(out, 0) in the epilogue", so
with both flags the activation sees the accumulated value: the 64-row family's support passes accumulate into `out` and apply bias
and relu in the last pass only, which has no other meaning, and the 128-row kernels agree.  Without out0, or without relu, this is
out = act(sum + bias) (+ out0).

Every function also returns the element's TERM SUM: the same formula over |val|, |x|, |w|, plus |bias| and |out0|.  n u T bounds the
round-off of any fp32 evaluation order of the sum, so |got - ref| <= tol T stays meaningful for elements whose terms cancel -- the
criterion of oracle/parity_at_size.py, at its TOL.

The backward ("fused backward of the layer above"), over the edges e = (r = source, c = target) in source-keyed CSR order:

    dx[r]      = dx0[r] + sum_s (sum_{e out of r} val[e, s] g[c_e]) W_s^T + dz[r, :nmix] wmix,  times (x[r, f] > 0) for f < relu_cols
    dval[e, s] = dval0[e, s] + <x[r] W_s, g[c_e]>                                              conv_bwd_ref
    dw[s]      = sum_r x[r]^T (sum_{e out of r} val[e, s] g[c_e])
    dz11 = g[:, Fout:Fout+2] t12 (1 - t11^2),  dz12 = g[:, Fout:Fout+2] t11 (1 - t12^2),  t1k = tanh(fc1k x + b1k)
    dw1k = dz1k^T x,  db1k = column sums of dz1k,  dcb = column sums of g[:, :Fout]            had_ref

Each backward output comes as a Ref(value, term sum, number of terms): the count is what an fp32 bound n u T needs."""
import collections

import numpy as np

SENTINEL = np.int32(0x7FC5A5A5)        # a quiet NaN with a payload no kernel produces: guards are compared as int32
GUARD_ROWS = 8                         # rows allocated after row N - 1
GUARD_HEAD = 4                         # floats in front of the output when it is passed at an offset


def csr_order(edge_index, num_rows):
    """(rowptr, perm): the stable target sort gml_csr_from_coo performs; edge_index[:, perm] is the CSR order."""
    dst = np.asarray(edge_index[1])
    perm = np.argsort(dst, kind='stable')
    rowptr = np.zeros(num_rows + 1, np.int64)
    np.add.at(rowptr, dst + 1, 1)
    return np.cumsum(rowptr), perm


def _aggregate(ei_sorted, val, x):
    src, dst = np.asarray(ei_sorted[0]), np.asarray(ei_sorted[1])
    val, x = np.asarray(val, np.float64), np.asarray(x, np.float64)
    N, S = x.shape[0], val.shape[1]
    H = np.zeros((N, S, x.shape[1]))
    flat = dst.astype(np.int64) * N + src                     # dense A_s [target, source]: the graphs here have a few hundred rows
    for s in range(S):
        H[:, s, :] = np.bincount(flat, weights=val[:, s], minlength=N * N).reshape(N, N) @ x
    return H


def spmm_ref(ei_sorted, val, x):
    """(H [N, S, Fin], term sums): x is [N, Fin] (the caller cuts padding columns off)."""
    return _aggregate(ei_sorted, val, x), _aggregate(ei_sorted, np.abs(val), np.abs(x))


def conv_ref(ei_sorted, val, x, w, bias=None, relu=False, out0=None):
    """(out [N, Fout], term sums).  ei_sorted [2, E] = (source, target) in the CSR order the call under test reads, val [E, S] the
    value row of each of those edges (for an `epos` call: val_passed[epos]), w [S, Fin, Fout] as the call's strides address it."""
    w = np.asarray(w, np.float64)
    H, Ht = spmm_ref(ei_sorted, val, x)
    out = np.einsum('nsf,sfo->no', H, w)
    t = np.einsum('nsf,sfo->no', Ht, np.abs(w))
    if bias is not None:
        out = out + np.asarray(bias, np.float64)
        t = t + np.abs(np.asarray(bias, np.float64))
    if out0 is not None:
        out = out + np.asarray(out0, np.float64)
        t = t + np.abs(np.asarray(out0, np.float64))
    if relu:
        out = np.maximum(out, 0.0)
    return out, t


def mix_ref(x, w11, b11, w12, b12):
    """(Hadamard columns [N, F2], bound basis).  w11 / w12 [F2, Fin].  |d(t1 t2)| <= |dz1| + |dz2| since |tanh|, |tanh'| <= 1, so
    the basis is the term sum of z1 plus that of z2, plus 1 for the two tanh evaluations themselves (absolute error 4e-7 each,
    tests/test_gpu_parity.py::test_tanh_approximation_bound: far inside tol = 1e-4 of that 1)."""
    x = np.asarray(x, np.float64)
    w11, w12 = np.asarray(w11, np.float64), np.asarray(w12, np.float64)
    b11 = np.zeros(w11.shape[0]) if b11 is None else np.asarray(b11, np.float64)
    b12 = np.zeros(w12.shape[0]) if b12 is None else np.asarray(b12, np.float64)
    out = np.tanh(x @ w11.T + b11) * np.tanh(x @ w12.T + b12)
    t = np.abs(x) @ np.abs(w11).T + np.abs(b11) + np.abs(x) @ np.abs(w12).T + np.abs(b12) + 1.0
    return out, t


def alloc(N, ncols, ldo, head=False, out0=None, guard_rows=GUARD_ROWS):
    """(flat float32 buffer, offset of element [0, 0]): [GUARD_HEAD floats when head][N + guard_rows rows of ldo], every float the
    sentinel, then rows [0, N) x [0, ncols) = out0 when given (an accumulate call's old values).  Any row-major output is one of
    these: out / dx [N, F] in rows of ldo, dval [E, S] (N = E, ncols = ldo = S), dw [S Fin, Fout], a flat workspace of n floats
    with a tail of t (N = 1, ncols = n, ldo = n + t, guard_rows = 0); ncols = 0: a buffer that must stay untouched."""
    off = GUARD_HEAD if head else 0
    buf = np.full(off + (N + guard_rows) * ldo, SENTINEL, np.int32).view(np.float32)
    if out0 is not None:
        buf[off:].reshape(N + guard_rows, ldo)[:N, :ncols] = out0
    return buf, off


def split(buf, N, ncols, ldo, guard_rows=GUARD_ROWS):
    """(values [N, ncols], guard words int32) of a buffer laid out by alloc(); the head guard is whatever precedes the rows."""
    buf = np.ascontiguousarray(buf, np.float32)
    off = buf.size - (N + guard_rows) * ldo
    assert off in (0, GUARD_HEAD), 'not a buffer of alloc(): %d floats for N=%d ldo=%d' % (buf.size, N, ldo)
    rows = buf[off:].reshape(N + guard_rows, ldo)
    guards = np.concatenate([buf[:off], rows[:N, ncols:].ravel(), rows[N:].ravel()]).view(np.int32)
    return rows[:N, :ncols], guards


def errors(got, ref, termsum):
    """(max-norm figure, worst |got - ref| / term sum) in float64"""
    got, ref, t = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(termsum, np.float64)
    d = np.abs(got - ref)
    e_max = float(d.max() / max(np.abs(ref).max(), 1e-30)) if ref.size else 0.0
    e_ts = float((d / np.maximum(t, 1e-300)).max()) if ref.size else 0.0
    return e_max, e_ts


def check(out_buf, ref, termsum, N, Fout, ldo, tol, what='', guard_rows=GUARD_ROWS, bound=None):
    """out_buf: the whole buffer of alloc() after the call.  Asserts: finite values; rel_err <= tol (conftest.rel_err); every
    element within tol of its own term sum; every guard word still the sentinel; with `bound` (absolute, per element: a derived
    bound such as f32_bound's) also |got - ref| <= bound.  Returns the two figures."""
    got, guards = split(out_buf, N, Fout, ldo, guard_rows)
    assert ref.shape == (N, Fout) and termsum.shape == (N, Fout), (what, ref.shape, termsum.shape)
    hit = np.flatnonzero(guards != SENTINEL)
    assert hit.size == 0, '%s: %d guard words overwritten, first at guard index %d' % (what, hit.size, hit[0])
    assert np.isfinite(got).all(), '%s: %d values not finite' % (what, int((~np.isfinite(got)).sum()))
    e_max, e_ts = errors(got, ref, termsum)
    assert e_max <= tol, '%s: rel err %.3e > %.1e' % (what, e_max, tol)
    bad = np.abs(got.astype(np.float64) - ref) > tol * termsum + 1e-30
    assert not bad.any(), '%s: %d elements beyond %.1e of their term sum, worst %.3e at %s' % (
        what, int(bad.sum()), tol, e_ts, np.unravel_index(np.argmax(np.abs(got - ref) / np.maximum(termsum, 1e-300)), ref.shape))
    if bound is not None:
        over = np.abs(got.astype(np.float64) - ref) > np.asarray(bound, np.float64) + 1e-30
        assert not over.any(), '%s: %d elements beyond their derived bound, worst %.3e of its term sum at %s' % (
            what, int(over.sum()), float((np.abs(got - ref) / np.maximum(termsum, 1e-300))[over].max()), np.argwhere(over)[0])
    return e_max, e_ts


# --------------------------------------------------------------------------------------------------------------------- the backward
Ref = collections.namedtuple('Ref', 'v t n')               # value, term sum, number of terms: arrays of one shape (n: broadcastable)


def f32_bound(ref, c=8):
    """Absolute bound of an fp32 evaluation of ref.v, whatever its order.  fl(a b) = a b (1 + d), |d| <= u = 2^-24, and every
    addition of partial sums adds another (1 + d); a sum of n rounded products in ANY order (an fmaf chain, a tree, partial sums
    per workgroup folded later) therefore lies within ((1 + u)^n - 1) T ~ n u T of the exact sum, T the sum of |terms| (Higham,
    Accuracy and Stability of Numerical Algorithms, s3.1).  The kernels evaluate every output in two chained stages (Z = x W or the
    aggregate P first, then the contraction with g / the projection with W): each term of the outer sum carries the inner sum's
    relative error, at most n u again, so the figure doubles.  c covers the roundings outside the sums (the three-factor terms'
    second product, the old value joined, the store).  2 (n + c) u T."""
    return 2.0 * (np.asarray(ref.n, np.float64) + c) * 2.0 ** -24 * ref.t


def conv_bwd_ref(ei_sorted, val, x, g, w, dx0=None, dval0=None, dz=None, wmix=None, relu_cols=0, dz_t=None):
    """{'dx': Ref [N, Fin], 'dval': Ref [E, S], 'dw': Ref [S, Fin, Fout]}.  ei_sorted [2, E] = (source r, target c) in the
    source-keyed CSR order the call reads, val [E, S] in that order, x [N, Fin], g [N, Fout] (padding cut off), w [S, Fin, Fout].
    dz [N, nmix] / wmix [nmix, Fin]: the DZ hand-over (dz_t: the term basis of dz where dz is itself computed, had_ref)."""
    src, dst = np.asarray(ei_sorted[0]), np.asarray(ei_sorted[1])
    val, x, g, w = (np.asarray(a, np.float64) for a in (val, x, g, w))
    N, S = x.shape[0], val.shape[1]
    flip = np.stack([dst, src])                               # aggregate over the edges OUT of a row: gather g at the targets
    Q, Qt = _aggregate(flip, val, g), _aggregate(flip, np.abs(val), np.abs(g))                 # [N, S, Fout]
    deg = np.bincount(src, minlength=N).astype(np.float64)
    dx, dxt = np.einsum('nso,sfo->nf', Q, w), np.einsum('nso,sfo->nf', Qt, np.abs(w))
    dxn = deg[:, None] * S * w.shape[2] * np.ones_like(dx)
    if dz is not None:
        dz, wmix = np.asarray(dz, np.float64), np.asarray(wmix, np.float64)
        dx = dx + dz @ wmix
        dxt = dxt + (np.abs(dz) if dz_t is None else dz_t) @ np.abs(wmix)
        dxn = dxn + wmix.shape[0]
    if dx0 is not None:
        dx, dxt, dxn = dx + np.asarray(dx0, np.float64), dxt + np.abs(np.asarray(dx0, np.float64)), dxn + 1
    if relu_cols:
        keep = x[:, :relu_cols] > 0                           # (-0.0 > 0 is false: an exact zero either way)
        dx[:, :relu_cols] *= keep
        dxt[:, :relu_cols] *= keep                            # a masked element has no terms: it must be exactly zero
    Z, Zt = np.einsum('nf,sfo->nso', x, w), np.einsum('nf,sfo->nso', np.abs(x), np.abs(w))     # [N, S, Fout]
    dval, dvalt = np.einsum('eso,eo->es', Z[src], g[dst]), np.einsum('eso,eo->es', Zt[src], np.abs(g[dst]))
    dvaln = np.full(dval.shape, float(w.shape[1] * w.shape[2]))
    if dval0 is not None:
        dval, dvalt, dvaln = dval + np.asarray(dval0, np.float64), dvalt + np.abs(np.asarray(dval0, np.float64)), dvaln + 1
    dw, dwt = np.einsum('nf,nso->sfo', x, Q), np.einsum('nf,nso->sfo', np.abs(x), Qt)
    dwn = np.full(dw.shape, float(src.size))
    return {'dx': Ref(dx, dxt, dxn), 'dval': Ref(dval, dvalt, dvaln), 'dw': Ref(dw, dwt, dwn)}


def had_ref(x, g, fout, w11, b11, w12, b12):
    """The ML3Layer output stage inside gml_spectconv_bwd_had: g [N, >= fout + F2], w11 / w12 [F2, Fin].  Returns (dz [N, 2 F2] =
    [dz11 | dz12] -- the rows that join dx through wmix = [w11; w12] -- , its term basis, {'dw11', 'dw12', 'db11', 'db12', 'dcb'}).
    The basis of dz is |g| (1 + T11 + T12), T1k the term sum of the pre-activation: |tanh|, |tanh'| and |tanh''| are <= 1, so an
    error e in a pre-activation or in a tanh moves dz by at most 3 |g| e (mix_ref's argument, one derivative further)."""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    w11, w12 = np.asarray(w11, np.float64), np.asarray(w12, np.float64)
    F2, N = w11.shape[0], x.shape[0]
    b11 = np.zeros(F2) if b11 is None else np.asarray(b11, np.float64)
    b12 = np.zeros(F2) if b12 is None else np.asarray(b12, np.float64)
    t1, t2 = np.tanh(x @ w11.T + b11), np.tanh(x @ w12.T + b12)
    gh = g[:, fout:fout + F2]
    dz11, dz12 = gh * t2 * (1 - t1 * t1), gh * t1 * (1 - t2 * t2)
    basis = np.abs(gh) * (1.0 + np.abs(x) @ np.abs(w11).T + np.abs(b11) + np.abs(x) @ np.abs(w12).T + np.abs(b12))
    ax, n = np.abs(x), float(N)
    out = {'dw11': Ref(dz11.T @ x, basis.T @ ax, n), 'dw12': Ref(dz12.T @ x, basis.T @ ax, n),
           'db11': Ref(dz11.sum(0), basis.sum(0), n), 'db12': Ref(dz12.sum(0), basis.sum(0), n),
           'dcb': Ref(g[:, :fout].sum(0), np.abs(g[:, :fout]).sum(0), n)}
    return np.concatenate([dz11, dz12], 1), np.concatenate([basis, basis], 1), out
