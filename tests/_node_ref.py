"""float64 restatement of the ML3Layer node side of include/gml.h -- the output-stage backward (gml_ml3_split_bwd / _ex), the Hadamard
branch (gml_node_mix_fwd / _bwd), gml_relu_bwd, gml_xty and the pools (gml_segment_sum / _sum_mask / _bcast / _bcast_mask / _max /
_max_bwd) -- with the TERM SUM of every element.  Plain numpy, no device, nothing imported from the package:
tests/test_node_ref_cpu.py holds it to float64 autograd of the reference model's expressions.

    out  = cat[relu(c), tanh(fc11 x) * tanh(fc12 x)]                       (mix_ref: the Hadamard columns)
    G    = gy[:, :nout1] (y > 0)            -- a select, exact in float32; the pre-masked form hands gy[:, :nout1] through
    dcb  = column sums of G,  dz11 / dz12, dw1k = dz1k^T x, db1k = column sums of dz1k         (_conv_ref.had_ref)
    dx   = dz11 w11 + dz12 w12              -- WRITTEN by gml_ml3_split_bwd, ACCUMULATED onto dx0 by gml_node_mix_bwd
    xty  = A^T B

The pools are float32 statements: the kernels promise the ascending row order of index_add_, so a segment's sum is the float32
sum accumulated SEQUENTIALLY (np.add.accumulate on float32) and is held bit-exact; mean = that sum / float32(max(len, 1)); the
broadcasts, the relu pattern words, max / argmax (the first row on ties, 0 / -1 for an empty segment) and max backward are selects."""
import numpy as np

from _conv_ref import Ref, had_ref, mix_ref                  # noqa: F401  (mix_ref: the forward's reference, re-exported)

POOL_SKIP_LAST = 2                                           # GML_POOL_SKIP_LAST of include/gml.h


def relu_bwd_ref(gy, y):
    """gy (y > 0) as a float32 select: -0.0, +0.0 and NaN close the gate, a positive denormal opens it; closed elements are +0.0"""
    gy, y = np.asarray(gy, np.float32), np.asarray(y, np.float32)
    with np.errstate(invalid='ignore'):
        return np.where(y > 0, gy, np.float32(0.0)).astype(np.float32)


def _dx_ref(dz, basis, w11, w12, dx0=None):
    w11, w12 = np.asarray(w11, np.float64), np.asarray(w12, np.float64)
    F2 = w11.shape[0]
    v = dz[:, :F2] @ w11 + dz[:, F2:] @ w12
    t = basis[:, :F2] @ np.abs(w11) + basis[:, F2:] @ np.abs(w12)
    n = 2.0 * F2
    if dx0 is not None:
        v, t, n = v + np.asarray(dx0, np.float64), t + np.abs(np.asarray(dx0, np.float64)), n + 1
    return Ref(v, t, n)


def split_bwd_ref(gy, gy_seg, y, x, w11, b11, w12, b12, nout1, F2, premasked=False):
    """gy [N or segments, >= nout1 + F2], y [N, >= nout1] (None when pre-masked), x [N, Fin] (None at F2 = 0).  Returns a dict:
    'G' float32 [N, nout1] (exact), 'dcb' Ref [nout1], and at F2 > 0 'dw11' / 'dw12' Ref [F2, Fin], 'db11' / 'db12' Ref [F2],
    'dx' Ref [N, Fin], 'dz' Ref [N, 4] = (dz11 | dz12 | 0) (only meaningful at 2 F2 <= 4)."""
    gy = np.asarray(gy, np.float32)
    if gy_seg is not None:
        gy = gy[np.asarray(gy_seg, np.int64)]
    G = gy[:, :nout1].copy() if premasked else relu_bwd_ref(gy[:, :nout1], np.asarray(y)[:, :nout1])
    N = gy.shape[0]
    g64 = np.concatenate([G.astype(np.float64), gy[:, nout1:nout1 + F2].astype(np.float64)], 1)
    r = {'G': G}
    if F2 == 0:
        r['dcb'] = Ref(g64.sum(0), np.abs(g64).sum(0), float(N))
        return r
    dz, basis, h = had_ref(x, g64, nout1, w11, b11, w12, b12)
    r.update(h)
    r['dx'] = _dx_ref(dz, basis, w11, w12)
    pad = np.zeros((N, max(4 - 2 * F2, 0)))
    r['dz'] = Ref(np.concatenate([dz, pad], 1)[:, :4], np.concatenate([basis, pad], 1)[:, :4], 1.0)
    return r


def node_mix_bwd_ref(x, gout, w11, b11, w12, b12, dx0=None):
    """gout [N, F2].  {'dw11', 'dw12', 'db11', 'db12', 'dx'}: dx = dx0 + dz11 w11 + dz12 w12 (dx0 joins the term sum)."""
    dz, basis, h = had_ref(x, np.asarray(gout, np.float64), 0, w11, b11, w12, b12)
    h.pop('dcb')
    h['dx'] = _dx_ref(dz, basis, w11, w12, dx0)
    return h


def xty_ref(A, B):
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return Ref(A.T @ B, np.abs(A).T @ np.abs(B), float(A.shape[0]))


# ------------------------------------------------------------------------------------------------------------------------- pools
def seq_sum32(a):
    """float32 column sums of a [n, F], accumulated sequentially in ascending row order onto +0.0, as index_add_ into a zero
    tensor does: a segment whose only row holds -0.0 sums to +0.0"""
    a = np.asarray(a, np.float32)
    return np.add.accumulate(np.concatenate([np.zeros((1, a.shape[1]), np.float32), a]), axis=0, dtype=np.float32)[-1]


def segment_sum_ref(x, ptr, mean=0):
    """(sums float32 [segments, F], means float32): `mean` is the flag word of gml_segment_sum -- with POOL_SKIP_LAST the last
    segment's row is +0.0 whatever its rows hold."""
    x, ptr = np.asarray(x, np.float32), np.asarray(ptr, np.int64)
    nseg = ptr.size - 1
    s = np.zeros((nseg, x.shape[1]), np.float32)
    ln = np.maximum(np.diff(ptr), 1).astype(np.float32)
    for g in range(nseg):
        if (mean & POOL_SKIP_LAST) and g == nseg - 1:
            ln[g] = 1.0
            continue
        s[g] = seq_sum32(x[ptr[g]:ptr[g + 1]])
    return s, (s / ln[:, None]).astype(np.float32)


def relu_words_ref(x):
    """uint32 [rows]: bit c = (x[row, c] > 0), x [rows, 32]"""
    x = np.asarray(x, np.float32)
    assert x.shape[1] == 32
    with np.errstate(invalid='ignore'):
        return ((x > 0).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)


def seg_of(ptr):
    ptr = np.asarray(ptr, np.int64)
    return np.repeat(np.arange(ptr.size - 1), np.diff(ptr)).astype(np.int32)


def segment_bcast_ref(g, ptr, mean=0):
    """float32 [rows, F]: row r holds g[seg(r)], divided by float32(len) when mean (the kernel multiplies by 1 / len: 1 ulp)"""
    g, ptr = np.asarray(g, np.float32), np.asarray(ptr, np.int64)
    out = g[seg_of(ptr)]
    if mean:
        out = (out / np.repeat(np.diff(ptr), np.diff(ptr)).astype(np.float32)[:, None]).astype(np.float32)
    return out


def segment_bcast_mask_ref(g, seg, words, nrelu):
    """out[row, c] = g[seg[row], c] where c >= nrelu or bit c of words[row], else +0.0"""
    g = np.asarray(g, np.float32)[np.asarray(seg, np.int64)][:, :32]
    c = np.arange(32)
    keep = (c >= nrelu)[None, :] | (((np.asarray(words, np.uint32)[:, None] >> c.astype(np.uint32)) & 1) == 1)
    return np.where(keep, g, np.float32(0.0)).astype(np.float32)


def segment_max_ref(x, ptr):
    """(max float32 [segments, F], argmax int32: the FIRST row that attains it); an empty segment: 0 / -1"""
    x, ptr = np.asarray(x, np.float32), np.asarray(ptr, np.int64)
    nseg = ptr.size - 1
    out, arg = np.zeros((nseg, x.shape[1]), np.float32), np.full((nseg, x.shape[1]), -1, np.int32)
    for g in range(nseg):
        if ptr[g + 1] > ptr[g]:
            blk = x[ptr[g]:ptr[g + 1]]
            a = blk.argmax(0)                                # numpy: the first occurrence
            out[g], arg[g] = blk[a, np.arange(x.shape[1])], ptr[g] + a
    return out, arg


def segment_max_bwd_ref(g, ptr, arg):
    g, ptr = np.asarray(g, np.float32), np.asarray(ptr, np.int64)
    s = seg_of(ptr)
    rows = np.arange(s.size)[:, None]
    return np.where(np.asarray(arg)[s] == rows, g[s], np.float32(0.0)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------- inputs
def rng_of(*key):
    import zlib
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def stage_inputs(N, Fin, F2, nout1, pad=8):
    """Host operands of one output-stage case, shared by the CPU tolerance test and the GPU matrix.  y = relu of an N(0, 1) draw
    (about half of it exact +0.0: a saved layer output); gy's conv columns ~ N(0.5, 1), its Hadamard columns ~ N(1, 0.25);
    x = 0.5 + |N(0, 1)| (positive, as behind a relu); weights N(0, 1) 0.3 Fin ** -0.5; biases of magnitude 0.8 .. 1.2 and either sign.

    Why these: dcb, db1k and dw1k have ONE element at nout1 = F2 = Fin = 1, and the max-norm figure of a tensor of one or two
    elements whose terms cancel measures the cancellation, not the arithmetic -- with zero-mean operands plain sequential fp32
    misses 2e-5 there itself (tests/test_node_ref_cpu.py was the first to say so), and so does any kernel through its tanh (absolute
    error 4e-7, test_tanh_approximation_bound) wherever a tanh factor is near 0.  So the pre-activations z = x w + b stay near b
    (|x w| ~ 0.4): a unit's tanh keeps its bias's sign and 0.3 <= |tanh| <= 0.95, 1 - tanh^2 >= 0.1, the Hadamard gradients are
    mostly positive and x is positive (with x ~ N(1, 1) its negative sixth met the unsaturated tanh' of a unit with a large negative
    weight and a one-element dw12 cancelled to 5e-4 of its terms), so every column sum adds terms of mostly one sign.  The elementwise term-sum criterion never needed this.
    `pad` readable rows follow row N - 1."""
    r = rng_of('stage', N, Fin, F2, nout1)
    f = lambda *s: np.ascontiguousarray(r.standard_normal(s), np.float32)
    gy = f(N + pad, nout1 + F2)
    gy[:, :nout1] += np.float32(0.5)
    gy[:, nout1:] = gy[:, nout1:] * np.float32(0.5) + np.float32(1.0)
    c = {'gy': gy, 'y': np.maximum(f(N + pad, nout1), np.float32(0.0)), 'x': f(N + pad, max(Fin, 1)) * np.float32(0.5) + np.float32(1.0)}
    sc = np.float32(0.3 * max(Fin, 1) ** -0.5)
    b = lambda: (np.sign(f(F2)) * (np.float32(0.8) + np.float32(0.4) * r.random(F2).astype(np.float32))).astype(np.float32)
    c.update(w11=f(F2, max(Fin, 1)) * sc, w12=f(F2, max(Fin, 1)) * sc, b11=b(), b12=b())
    return c


def mix_inputs(N, Fin, F2, pad=8):
    """stage_inputs for gml_node_mix_*: 'g' [N + pad, F2] the Hadamard gradient columns, 'dx0' [N, Fin] ~ N(0, 1) the old values of an
    accumulating dx"""
    c = dict(stage_inputs(N, Fin, F2, 1, pad))
    c['g'] = c['gy'][:, 1:]
    c['dx0'] = np.ascontiguousarray(rng_of('dx0', N, Fin, F2).standard_normal((N, Fin)), np.float32)
    return c


def xty_inputs(n, a, b, pad=8):
    """A [n + pad, a], B [n + pad, b] ~ N(1, 1): at a = b = 1 the one output element adds terms of mostly one sign"""
    r = rng_of('xty', n, a, b)
    f = lambda *s: np.ascontiguousarray(r.standard_normal(s) + 1.0, np.float32)
    return f(n + pad, a), f(n + pad, b)


SEG_SIZES = (0, 1, 31, 32, 33, 63, 64, 65, 3, 1, 0, 7, 64, 2, 129, 1700, 5, 40, 17, 0, 2, 30, 0)


def seg_ptr(sizes=SEG_SIZES):
    """int32 ptr of the pool cases.  Two 32-lane segments share a wave of gml_segment_sum_mask (segments 2k and 2k + 1): the list
    puts an empty segment first and last, 1 / 31 / 32 / 33 / 63 / 64 / 65 rows, one of 1700, and neighbours of different lengths
    -- shorter first and longer first, by less and by more than the 32-row step of the loop -- in the two halves of a wave."""
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
