"""float64 restatement of the conv-forward ABI of include/gml.h (gml_spectconv_fwd, gml_ml3_fwd, gml_spmm_fwd_ex) and the checker the
ABI tests hold a launch to.  Plain numpy, no device.

    H[r, s, :] = sum_{k in row r} val[k, s] x[col[k], :]                 spmm_ref
    out        = act(sum_s H[:, s, :] W_s + bias + out0)                 conv_ref
    mix        = tanh(x w11^T + b11) * tanh(x w12^T + b12)               mix_ref

`out0` is what the output held before a GML_ACCUM call.  GML_RELU is the flag's own wording, "out = max(out, 0) in the epilogue", so
with both flags the activation sees the accumulated value: the 64-row family's support passes accumulate into `out` and apply bias
and relu in the last pass only, which has no other meaning, and the 128-row kernels agree.  Without out0, or without relu, this is
out = act(sum + bias) (+ out0).

Every function also returns the element's TERM SUM: the same formula over |val|, |x|, |w|, plus |bias| and |out0|.  n u T bounds the
round-off of any fp32 evaluation order of the sum, so |got - ref| <= tol T stays meaningful for elements whose terms cancel -- the
criterion of oracle/parity_at_size.py, at its TOL."""
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


def alloc(N, ncols, ldo, head=False, out0=None):
    """(flat float32 buffer, offset of element [0, 0]): [GUARD_HEAD floats when head][N + GUARD_ROWS rows of ldo], every float the
    sentinel, then rows [0, N) x [0, ncols) = out0 when given (an accumulate call's old values)."""
    off = GUARD_HEAD if head else 0
    buf = np.full(off + (N + GUARD_ROWS) * ldo, SENTINEL, np.int32).view(np.float32)
    if out0 is not None:
        buf[off:].reshape(N + GUARD_ROWS, ldo)[:N, :ncols] = out0
    return buf, off


def split(buf, N, ncols, ldo):
    """(values [N, ncols], guard words int32) of a buffer laid out by alloc(); the head guard is whatever precedes the rows."""
    buf = np.ascontiguousarray(buf, np.float32)
    off = buf.size - (N + GUARD_ROWS) * ldo
    assert off in (0, GUARD_HEAD), 'not a buffer of alloc(): %d floats for N=%d ldo=%d' % (buf.size, N, ldo)
    rows = buf[off:].reshape(N + GUARD_ROWS, ldo)
    guards = np.concatenate([buf[:off], rows[:N, ncols:].ravel(), rows[N:].ravel()]).view(np.int32)
    return rows[:N, :ncols], guards


def errors(got, ref, termsum):
    """(max-norm figure, worst |got - ref| / term sum) in float64"""
    got, ref, t = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(termsum, np.float64)
    d = np.abs(got - ref)
    e_max = float(d.max() / max(np.abs(ref).max(), 1e-30)) if ref.size else 0.0
    e_ts = float((d / np.maximum(t, 1e-300)).max()) if ref.size else 0.0
    return e_max, e_ts


def check(out_buf, ref, termsum, N, Fout, ldo, tol, what=''):
    """out_buf: the whole buffer of alloc() after the call.  Asserts: finite values; rel_err <= tol (conftest.rel_err); every
    element within tol of its own term sum; every guard word still the sentinel.  Returns the two figures."""
    got, guards = split(out_buf, N, Fout, ldo)
    assert ref.shape == (N, Fout) and termsum.shape == (N, Fout), (what, ref.shape, termsum.shape)
    hit = np.flatnonzero(guards != SENTINEL)
    assert hit.size == 0, '%s: %d guard words overwritten, first at guard index %d' % (what, hit.size, hit[0])
    assert np.isfinite(got).all(), '%s: %d values not finite' % (what, int((~np.isfinite(got)).sum()))
    e_max, e_ts = errors(got, ref, termsum)
    assert e_max <= tol, '%s: rel err %.3e > %.1e' % (what, e_max, tol)
    bad = np.abs(got.astype(np.float64) - ref) > tol * termsum + 1e-30
    assert not bad.any(), '%s: %d elements beyond %.1e of their term sum, worst %.3e at %s' % (
        what, int(bad.sum()), tol, e_ts, np.unravel_index(np.argmax(np.abs(got - ref) / np.maximum(termsum, 1e-300)), ref.shape))
    return e_max, e_ts
