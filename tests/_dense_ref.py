"""float64 restatement of the equal-size dense-block ABI of include/gml.h (csrc/gml_dense.hip and gml_xty_wide), the case tables the
ABI matrix (tests/test_gpu_dense_abi.py) and its CPU companion (tests/test_dense_ref_cpu.py) share, and a numpy emulation of the
kernels' arithmetic.  Plain numpy, no device.

    pack         img[blk][0 | 1][r][k] = hi | lo of block[r][k] (transpose: block[k][r]),  k < n;  0 for n <= k < KP           (exact)
    support_mm   out[b n + r, s so + f] = sum_k D[b, s, r, k] act[b n + k, s sa + f]         (sum_s: summed over s into columns [0, F))
    conv_fwd     out2 = act?(sum_s sum_f (sum_k D_s x) W_s + bias),   hcat = support_mm(sum_s = 0, sa = 0, so = Fin) at ldo = S Fin
    conv_bwd_x   dx = sum_s D_s^T (g W_s^T)
    conv_bwd_w   dW[s, f, o] = sum_b sum_j (D[b, s] X[b])[j, f] g[b n + j, o];  partials [slices][S][Fin][Fout], slice i owns the graphs
                 [i per, min((i + 1) per, B)), per = ceil(B / slices); a slice that owns no graph holds zeros
    xty_wide     out = A^T B

Every function returns Ref(value, TERM SUM, number of terms) of _conv_ref: the same formula over absolute values, nested for the
chained outputs (|D| |x| contracted with |W|, plus |bias|).  |got - ref| <= TOL T stays meaningful where an element's terms cancel.

The bar.  TOL = 1e-4 on the max-norm and on each element's own term sum, the bar of every bf16-piece chain of this project.  The
arithmetic the header of csrc/gml_dense.hip documents keeps a correct kernel inside it with room to spare, so no other bar is derived:
an operand x = hi + lo + r with |r| <= 2^-17 |x| (two bf16 pieces of 8 significant bits each); a product drops lo.lo (<= 2^-16) and the
two r terms (<= 2^-16 together): at most 2^-15 = 3.1e-5 of the term sum per split product, twice that for the chained outputs
(6.1e-5), whatever the signs.  The fp32 accumulation adds _conv_ref.f32_bound's n u T in the worst case (2.2e-3 T for the 36,864
terms of the largest case) but sqrt(n) u T ~ 1e-5 T for roundings that do not conspire; the CPU companion evaluates the emulation
below on every case's arrays and asserts that it meets the bar the device is held to, so a case whose data could not be held by
correct arithmetic fails there, without a GPU.

relu: a zero the activation selects is bitwise +0.0.  An element whose float64 pre-activation lies within the value bar of zero may
fall on either side; `near` marks those, the cases keep them below 1 % of an output (asserted by the CPU companion)."""
import zlib

import numpy as np

from _conv_ref import Ref

TOL = 1e-4
NUM_CU = 256                                               # GML_NUM_CU, csrc/gml_common.h: gml_dense_pack's grid cap is 64 of these
IMG_TAIL = 128                                             # sentinel uint16 words behind a packed image (256 bytes)


# ------------------------------------------------------------------------------------------------------------------ bf16 pieces
def bf16_bits(v):
    """float32 -> the bf16 bit pattern (uint16) by round-to-nearest-even on the float32 bits (finite values)"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_rne(v):
    """float32 -> the nearest bf16 value, as float32"""
    return (bf16_bits(v).astype(np.uint32) << 16).view(np.float32)


def split_bf16(v):
    """(hi, lo) float32: hi = bf16(v), lo = bf16(v - hi); v - hi is exact in float32"""
    v = np.ascontiguousarray(v, np.float32)
    hi = bf16_rne(v)
    return hi, bf16_rne(v - hi)


def kp_min(n):
    return 32 * ((n + 31) // 32)


def pack_ref(blocks, KP, transpose):
    """blocks [nblocks, n, n] float32 -> uint16 [nblocks, 2, n, KP], bit for bit what gml_dense_pack writes"""
    blocks = np.ascontiguousarray(blocks, np.float32)
    nb, n = blocks.shape[0], blocks.shape[1]
    v = np.zeros((nb, n, KP), np.float32)
    v[:, :, :n] = blocks.transpose(0, 2, 1) if transpose else blocks
    hi = bf16_rne(v)
    return np.stack([bf16_bits(v), bf16_bits(v - hi)], 1)


def packed_values(blocks):
    """the float64 value the packed pair stands for: hi + lo (what every consumer multiplies by; block = hi + lo to 2^-17)"""
    hi, lo = split_bf16(blocks)
    return hi.astype(np.float64) + lo.astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------ the restatement
def _H(D, x):
    """D [B, S, n, n], x [B n, F] -> H [B, S, n, F] = D x per graph, and its term sum"""
    B, S, n, _ = D.shape
    D, x = np.asarray(D, np.float64), np.asarray(x, np.float64).reshape(B, n, -1)
    return np.einsum('bsrk,bkf->bsrf', D, x), np.einsum('bsrk,bkf->bsrf', np.abs(D), np.abs(x))


def support_mm_ref(D, act, sa, so, sum_s, F):
    """D [B, S, n, n] (the blocks the image was packed from: transposed already for the adjoint form), act [B n, >= (S - 1) sa + F].
    Returns (Ref [B n, width], written [width] bool): width = F when sum_s, else (S - 1) so + F; columns no support owns (so > F)
    are not written and hold ref 0, term sum 1."""
    B, S, n, _ = D.shape
    D, act = np.asarray(D, np.float64), np.asarray(act, np.float64)
    width = F if sum_s else (S - 1) * so + F
    v, t, w = np.zeros((B * n, width)), np.zeros((B * n, width)), np.zeros(width, bool)
    for s in range(S):
        a = act[:, s * sa:s * sa + F].reshape(B, n, F)
        hv = np.einsum('brk,bkf->brf', D[:, s], a).reshape(B * n, F)
        ht = np.einsum('brk,bkf->brf', np.abs(D[:, s]), np.abs(a)).reshape(B * n, F)
        c0 = 0 if sum_s else s * so
        v[:, c0:c0 + F] += hv
        t[:, c0:c0 + F] += ht
        w[c0:c0 + F] = True
    t[:, ~w] = 1.0
    return Ref(v, t, float(n * (S if sum_s else 1))), w


def conv_fwd_ref(D, x, w, bias, relu):
    """D [B, S, n, n], x [B n, Fin], w [S, Fin, Fout] -> {'out2': Ref [B n, Fout], 'hcat': Ref [B n, S Fin], 'pre': float64
    pre-activation, 'near': bool [B n, Fout], the elements relu may put on either side}"""
    B, S, n, _ = D.shape
    w = np.asarray(w, np.float64)
    H, Ht = _H(D, x)
    pre = np.einsum('bsrf,sfo->bro', H, w).reshape(B * n, -1)
    t = np.einsum('bsrf,sfo->bro', Ht, np.abs(w)).reshape(B * n, -1)
    if bias is not None:
        pre = pre + np.asarray(bias, np.float64)
        t = t + np.abs(np.asarray(bias, np.float64))
    near = (np.abs(pre) <= TOL * t) if relu else np.zeros(pre.shape, bool)
    out = np.maximum(pre, 0.0) if relu else pre
    nterms = float(S * w.shape[1] * n + 1)
    hc = Ref(H.transpose(0, 2, 1, 3).reshape(B * n, -1), Ht.transpose(0, 2, 1, 3).reshape(B * n, -1), float(n))
    return {'out2': Ref(out, t, nterms), 'hcat': hc, 'pre': pre, 'near': near}


def conv_bwd_x_ref(D, g, w):
    """dx [B n, Fin] = sum_s D_s^T (g W_s^T): D the UNtransposed blocks [B, S, n, n], g [B n, Fout], w [S, Fin, Fout]"""
    B, S, n, _ = D.shape
    D, w = np.asarray(D, np.float64), np.asarray(w, np.float64)
    g = np.asarray(g, np.float64).reshape(B, n, -1)
    T, Tt = np.einsum('bjo,sfo->bsjf', g, w), np.einsum('bjo,sfo->bsjf', np.abs(g), np.abs(w))
    v, t = np.einsum('bsji,bsjf->bif', D, T), np.einsum('bsji,bsjf->bif', np.abs(D), Tt)
    return Ref(v.reshape(B * n, -1), t.reshape(B * n, -1), float(S * n * w.shape[2]))


def dw_slices(B):
    """gml_dense_dw_slices"""
    return max(1, min(B, 64))


def conv_bwd_w_ref(D, x, g):
    """{'dw': Ref [S, Fin, Fout], 'partials': Ref [slices, S, Fin, Fout]} -- the documented layout of the workspace"""
    B, S, n, _ = D.shape
    H, Ht = _H(D, x)
    g = np.asarray(g, np.float64).reshape(B, n, -1)
    pv, pt = np.einsum('bsjf,bjo->bsfo', H, g), np.einsum('bsjf,bjo->bsfo', Ht, np.abs(g))      # per graph
    slices = dw_slices(B)
    per = -(-B // slices)
    v, t = np.zeros((slices,) + pv.shape[1:]), np.zeros((slices,) + pv.shape[1:])
    for i in range(slices):
        v[i], t[i] = pv[i * per:(i + 1) * per].sum(0), pt[i * per:(i + 1) * per].sum(0)       # (an empty range sums to zero)
    return {'dw': Ref(pv.sum(0), pt.sum(0), float(B * n * n)), 'partials': Ref(v, t, float(per * n * n)), 'per': per}


def xty_ref(A, Bm):
    A, Bm = np.asarray(A, np.float64), np.asarray(Bm, np.float64)
    return Ref(A.T @ Bm, np.abs(A).T @ np.abs(Bm), float(A.shape[0]))


# ------------------------------------------------------------------------------------------------------------------ the emulation
def _mm3(a, b):
    """a @ b over the last two axes as the kernels form it: both operands split to bf16 pairs, lo.hi + hi.lo + hi.hi (every product
    of two bf16 values is exact in float32), float32 accumulation"""
    ah, al = split_bf16(a)
    bh, bl = split_bf16(b)
    return (np.matmul(al, bh, dtype=np.float32) + np.matmul(ah, bl, dtype=np.float32)) + np.matmul(ah, bh, dtype=np.float32)


def emu_H(D, x):
    B, S, n, _ = D.shape
    return _mm3(np.asarray(D, np.float32), np.asarray(x, np.float32).reshape(B, 1, n, -1))     # [B, S, n, F]


def emu_support_mm(D, act, sa, so, sum_s, F):
    B, S, n, _ = D.shape
    width = F if sum_s else (S - 1) * so + F
    out = np.zeros((B * n, width), np.float32)
    act = np.asarray(act, np.float32)
    for s in range(S):
        h = _mm3(np.asarray(D[:, s], np.float32), act[:, s * sa:s * sa + F].reshape(B, n, F)).reshape(B * n, F)
        c0 = 0 if sum_s else s * so
        out[:, c0:c0 + F] += h
    return out


def emu_conv_fwd(D, x, w, bias, relu):
    B, S, n, _ = D.shape
    H = emu_H(D, x)
    out = np.zeros((B, n, w.shape[2]), np.float32)
    for s in range(S):
        out += _mm3(H[:, s], np.asarray(w[s], np.float32))
    out = out.reshape(B * n, -1)
    if bias is not None:
        out = out + np.asarray(bias, np.float32)
    return np.maximum(out, np.float32(0)) if relu else out


def emu_conv_bwd_x(D, g, w):
    B, S, n, _ = D.shape
    g = np.asarray(g, np.float32).reshape(B, n, -1)
    dx = np.zeros((B, n, w.shape[1]), np.float32)
    for s in range(S):
        T = _mm3(g, np.asarray(w[s], np.float32).T)                                            # [B, n, Fin]
        dx += _mm3(np.asarray(D[:, s], np.float32).transpose(0, 2, 1), T)
    return dx.reshape(B * n, -1)


def emu_conv_bwd_w(D, x, g):
    B, S, n, _ = D.shape
    H = emu_H(D, x)                                                                            # [B, S, n, Fin]
    g = np.asarray(g, np.float32).reshape(B, 1, n, -1)
    return _mm3(H.transpose(0, 1, 3, 2), g).sum(0, dtype=np.float32)


def emu_xty(A, Bm):
    return _mm3(np.asarray(A, np.float32).T, np.asarray(Bm, np.float32))


# ------------------------------------------------------------------------------------------------------------------ inputs
# (rng and f32 restate _rng / _f32 of test_gpu_conv_fwd_abi.py: this module also serves the CPU companion, which must not import a
# GPU test module -- torch, the device fixtures and the gpu marks come with it)
def rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def blocks(B, S, n):
    """[B, S, n, n] float32: half the entries nonzero, mixed sign and magnitude, no symmetry, no two alike; every row keeps an entry"""
    r = rng('blocks', B, S, n)
    keep = r.random((B, S, n, n)) < 0.5
    keep[..., np.arange(n), r.integers(0, n, n)] = True
    return f32(r.standard_normal((B, S, n, n)) * keep * (0.05 + r.random((B, S, 1, 1))))


def inputs(B, S, n, Fin, Fout=0, act_cols=None):
    """the operands of one case, by shape alone: two cases of one shape share their data, so that their outputs can be compared
    bit for bit across roads.  'x' [B n, Fin], 'act' [B n, act_cols] (the adjoint form's d Hcat), 'w' [S, Fin, Fout] scaled by
    Fin ** -0.5, 'bias' in [0.25, 0.75) -- off zero: fewer pre-activations near it --, 'g' [B n, Fout]"""
    r = rng('inputs', B, S, n, Fin, Fout, act_cols)
    c = {'D': blocks(B, S, n), 'x': f32(r.standard_normal((B * n, Fin)))}
    if act_cols:
        c['act'] = f32(r.standard_normal((B * n, act_cols)))
    if Fout:
        c['w'] = f32(r.standard_normal((S, Fin, Fout)) * Fin ** -0.5)
        c['bias'] = f32(r.random(Fout) * 0.5 + 0.25)
        c['g'] = f32(r.standard_normal((B * n, Fout)))
    return c


# ------------------------------------------------------------------------------------------------------------------ the cases
def _case(**kw):
    return kw


def _road(**conds):
    """'vec', or 'scalar:' and the conditions that take the operand off the float4 road"""
    why = [k for k, v in conds.items() if v]
    return 'scalar:' + '+'.join(why) if why else 'vec'


def nft_of(F):
    t = (F + 15) // 16
    return 1 if t <= 1 else 2 if t <= 2 else 4 if t <= 4 else 8


def not_of(Fout):
    return 4 if Fout <= 64 else 8


# (n, Fin, Fout): the wave counts 1 .. 6 with a last wave of one live row, every KP boundary, the NFT templates 1, 2, 4, 8 on both sides
# of each edge against NOT 4 and 8 (all eight pairs), widths on and off the float4 road
SHAPES = ((1, 1, 1), (15, 3, 65), (16, 4, 63), (17, 16, 128), (32, 17, 64), (33, 32, 65), (64, 33, 4), (65, 64, 128), (75, 65, 63),
          (96, 128, 128))

# gml_dense_support_mm.  form 'f': forward (sa = 0, so = F, one row of S F columns per node), 'a': adjoint (sa = F, summed over s).
# Fields: sa / so override the form's; lda / ldo: columns beyond the ones used; alead / off4: the pointer 4 bytes past a 16-byte
# boundary; road_in / road_out: what the launcher decides (csrc/gml_dense.hip, gml_dense_support_mm); same: the case whose output this
# one must equal bit for bit (same data by shape, another road or a larger KP).
def _mm(name, n, F, form, S=3, B=2, KP=None, sa=None, so=None, lda=4, ldo=4, alead=0, off4=False, same=None):
    KP = KP or kp_min(n)
    sum_s = 1 if form == 'a' else 0
    sa = (F if form == 'a' else 0) if sa is None else sa
    so = (0 if form == 'a' else F) if so is None else so
    acols = (S - 1) * sa + F
    width = F if sum_s else (S - 1) * so + F
    rin = _road(F=F % 4, ld=(acols + lda) % 4, sa=sa % 4, ptr=alead)
    rout = _road(F=F % 4, ld=(width + ldo) % 4, so=so % 4, ptr=off4)
    return _case(name=name, n=n, F=F, form=form, S=S, B=B, KP=KP, sa=sa, so=so, sum_s=sum_s, acols=acols, width=width, lda=acols + lda,
                 ldo=width + ldo, alead=alead, off4=off4, same=same, road_in=rin, road_out=rout)


MM_CASES = [_mm('%s-n%d-F%d' % (form, n, F), n, F, form) for n, F, _ in SHAPES for form in 'fa'] + [
    _mm('f-S1', 33, 32, 'f', S=1), _mm('a-S1', 33, 32, 'a', S=1), _mm('f-B1-n75', 75, 64, 'f', B=1, S=1), _mm('f-B3', 17, 4, 'f', B=3),
    # a KP larger than needed: the zero columns are inert and the K steps past the needed ones add nothing
    _mm('f-n17-KP64', 17, 16, 'f', KP=64, same='f-n17-F16'), _mm('f-n17-KP96', 17, 16, 'f', KP=96, same='f-n17-F16'),
    _mm('a-n17-KP96', 17, 16, 'a', KP=96, same='a-n17-F16'), _mm('f-n33-KP96', 33, 32, 'f', KP=96, same='f-n33-F32'),
    _mm('a-n33-KP96', 33, 32, 'a', KP=96, same='a-n33-F32'),
    # the scalar roads, one condition each, on the data of the vector case f-n33-F32 / a-n33-F32
    _mm('f-lda%4', 33, 32, 'f', lda=5, same='f-n33-F32'), _mm('f-alead', 33, 32, 'f', alead=1, same='f-n33-F32'),
    _mm('f-ldo%4', 33, 32, 'f', ldo=5, same='f-n33-F32'), _mm('f-off4', 33, 32, 'f', off4=True, same='f-n33-F32'),
    _mm('a-lda%4', 33, 32, 'a', lda=5, same='a-n33-F32'), _mm('a-alead', 33, 32, 'a', alead=1, same='a-n33-F32'),
    _mm('a-ldo%4', 33, 32, 'a', ldo=5, same='a-n33-F32'), _mm('a-off4', 33, 32, 'a', off4=True, same='a-n33-F32'),
    # sa / so off the float4 grid, and slices of wider buffers: so > F leaves sentinel gaps, sa > F skips junk columns
    _mm('f-so%4', 33, 32, 'f', so=33, ldo=6), _mm('a-sa%4', 33, 32, 'a', sa=33, lda=6),
    _mm('f-so>F', 33, 32, 'f', so=36), _mm('a-sa>F', 33, 32, 'a', sa=36), _mm('f-so>F-odd', 15, 3, 'f', so=5),
    _mm('f-ld-wide', 65, 64, 'f', lda=12, ldo=16, same='f-n65-F64'), _mm('f-ld-exact', 33, 32, 'f', lda=0, ldo=0, same='f-n33-F32'),
    # sum_s without the adjoint's column stride: every support reads the same tile (sa = 0) and the sums join in registers
    _mm('a-sa0', 33, 32, 'a', sa=0),
    # a width off the float4 grid in rows and strides that are on it: F % 4 alone
    _mm('f-F%4-alone', 15, 3, 'f', lda=1, so=4, ldo=1), _mm('a-F%4-alone', 15, 3, 'a', sa=4, lda=1, ldo=1),
]


# gml_dense_conv_fwd.  Each case runs with hcat NULL and non-NULL (both instantiations).  ldx / ldo2: columns beyond the ones used;
# xlead / off4 / hoff4: x, out2, hcat 4 bytes past a 16-byte boundary.
def _cf(name, n, Fin, Fout, S=3, B=2, KP=None, bias=True, relu=False, ldx=4, ldo2=4, xlead=0, off4=False, hoff4=False, same=None):
    rx, rh = _road(F=Fin % 4, ld=(Fin + ldx) % 4, ptr=xlead), _road(F=Fin % 4, ptr=hoff4)
    ro = _road(F=Fout % 4, ld=(Fout + ldo2) % 4, ptr=off4)
    return _case(name=name, n=n, Fin=Fin, Fout=Fout, S=S, B=B, KP=KP or kp_min(n), bias=bias, relu=relu, ldx=Fin + ldx, ldo2=Fout + ldo2,
                 xlead=xlead, off4=off4, hoff4=hoff4, same=same, road_x=rx, road_h=rh, road_o=ro)


_BR = ((True, False), (False, False), (True, True), (False, True))
CF_CASES = [_cf('n%d-Fin%d-Fout%d' % s, *s, bias=_BR[i % 4][0], relu=_BR[i % 4][1]) for i, s in enumerate(SHAPES)] + [
    _cf('base', 33, 32, 64), _cf('base-relu', 33, 32, 64, relu=True), _cf('S1-B1', 75, 64, 64, S=1, B=1), _cf('B3-nobias', 17, 4, 4, B=3, bias=False),
    _cf('n17-KP32', 17, 16, 64), _cf('n17-KP64', 17, 16, 64, KP=64, same='n17-KP32'), _cf('n17-KP96', 17, 16, 64, KP=96, same='n17-KP32'),
    _cf('n33-KP96', 33, 32, 64, KP=96, same='base'),
    _cf('ldx%4', 33, 32, 64, ldx=5, same='base'), _cf('xlead', 33, 32, 64, xlead=1, same='base'), _cf('hoff4', 33, 32, 64, hoff4=True, same='base'),
    _cf('ldo2%4', 33, 32, 64, ldo2=5, same='base'), _cf('out2-off4', 33, 32, 64, off4=True, same='base'),
    _cf('out2-slice', 33, 32, 64, ldo2=64, same='base'), _cf('out2-exact', 33, 32, 64, ldx=0, ldo2=0, same='base'),
    _cf('out2-off4-NOT8', 65, 64, 128, off4=True, bias=False, relu=True, same='n65-Fin64-Fout128'),
    _cf('Fin%4-alone', 33, 30, 64, ldx=2), _cf('Fout%4-alone', 33, 32, 62, ldo2=2),
    _cf('hcat-odd-Fin', 33, 33, 65, relu=True), _cf('Fin96', 17, 96, 64), _cf('Fin80-NOT8', 16, 80, 128, relu=True),
]


# gml_dense_conv_bwd_x: NFT from Fin (Fin > 64: the FQ = 2 variant), NOT from Fout; ldg / lddx: columns beyond; off4: dx off alignment
# (g is read element by element and its pointer is not looked at by the launcher: it stays aligned, like every unchecked pointer)
def _bx(name, n, Fin, Fout, S=3, B=2, KP=None, ldg=4, lddx=4, off4=False, same=None):
    ro = _road(F=Fin % 4, ld=(Fin + lddx) % 4, ptr=off4)
    return _case(name=name, n=n, Fin=Fin, Fout=Fout, S=S, B=B, KP=KP or kp_min(n), ldg=Fout + ldg, lddx=Fin + lddx, off4=off4, same=same,
                 road_o=ro)


BX_CASES = [_bx('n%d-Fin%d-Fout%d' % s, *s) for s in SHAPES] + [
    _bx('base', 33, 32, 64), _bx('S1-B1', 75, 64, 64, S=1, B=1), _bx('B3', 17, 4, 4, B=3),
    _bx('n17-KP32', 17, 16, 64), _bx('n17-KP64', 17, 16, 64, KP=64, same='n17-KP32'), _bx('n17-KP96', 17, 16, 64, KP=96, same='n17-KP32'),
    _bx('n33-KP96', 33, 32, 64, KP=96, same='base'),
    _bx('lddx%4', 33, 32, 64, lddx=5, same='base'), _bx('dx-off4', 33, 32, 64, off4=True, same='base'),
    _bx('ld-wide', 33, 32, 64, ldg=9, lddx=12, same='base'), _bx('ld-exact', 33, 32, 64, ldg=0, lddx=0, same='base'),
    _bx('Fin%4-alone', 33, 30, 64, lddx=2), _bx('FQ2-off4', 65, 128, 65, off4=True), _bx('Fin96', 17, 96, 64),
]


# gml_dense_conv_bwd_w: NFT from Fin, ceil(Fout / 64) column blocks (at most 255: Fout <= 16320, include/gml.h), min(B, 64) slices of ceil(B / slices)
# graphs.  ldx / ldg: columns beyond; xlead: x off alignment (the scalar staging road); nodw: dw == NULL, the partials stay.
def _bw(name, n, Fin, Fout, S=2, B=2, KP=None, ldx=4, ldg=4, xlead=0, same=None):
    return _case(name=name, n=n, Fin=Fin, Fout=Fout, S=S, B=B, KP=KP or kp_min(n), ldx=Fin + ldx, ldg=Fout + ldg, xlead=xlead, same=same,
                 road_x=_road(F=Fin % 4, ld=(Fin + ldx) % 4, ptr=xlead))


BW_CASES = [_bw('n%d-Fin%d-Fout%d' % s, *s) for s in SHAPES] + [
    _bw('base', 33, 32, 64), _bw('S1-B1', 75, 64, 64, S=1, B=1), _bw('S3-B3', 17, 4, 4, S=3, B=3), _bw('Fout144', 17, 16, 144),
    _bw('Fout144-Fin33', 16, 33, 144, S=1), _bw('Fout16320', 1, 1, 16320, S=1, B=1), _bw('Fout16257-Fin4', 2, 4, 16257, S=1, B=1),
    _bw('n17-KP32', 17, 16, 64), _bw('n17-KP64', 17, 16, 64, KP=64, same='n17-KP32'), _bw('n17-KP96', 17, 16, 64, KP=96, same='n17-KP32'),
    _bw('n33-KP96', 33, 32, 64, KP=96, same='base'),
    _bw('ldx%4', 33, 32, 64, ldx=5, same='base'), _bw('xlead', 33, 32, 64, xlead=1, same='base'), _bw('ld-exact', 33, 32, 64, ldx=0, ldg=0, same='base'),
    _bw('ldg-odd', 33, 32, 64, ldg=7, same='base'), _bw('Fin%4-alone', 33, 30, 64, ldx=2),
    # the slices: B = 63, 64 one graph each; 65 -> per = 2, 33 slices used, 31 empty; 129 -> per = 3, 43 used, 21 empty
    _bw('B63', 16, 4, 4, S=1, B=63), _bw('B64', 15, 3, 4, S=1, B=64), _bw('B65', 17, 4, 5, S=1, B=65), _bw('B129', 15, 4, 4, S=2, B=129),
]

# gml_xty_wide at ABI level: (rows, a, b, lda beyond a, ldb beyond b): two column tiles and several row ranges; one ragged tile
XW_CASES = [_case(name='n300-a130-b65', n=300, a=130, b=65, lda=134, ldb=68), _case(name='n129-a16-b128', n=129, a=16, b=128, lda=16, ldb=128),
            _case(name='n1-a1-b1', n=1, a=1, b=1, lda=5, ldb=3)]


def xw_inputs(c):
    r = rng('xw', c['n'], c['a'], c['b'])
    return f32(r.standard_normal((c['n'], c['a']))), f32(r.standard_normal((c['n'], c['b'])))


# values for gml_dense_pack that exercise the split: exactly bf16 (lo == 0), both pieces, a tie in the hi rounding (to even, both
# ways), a residual that is itself rounded, a residual of subnormal size, the smallest normal, negative zero, zero
PACK_SPECIALS = np.array([1.0, -2.5, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23, 3.14159274, -1e-3, 1 / 3,
                          2.0 ** -120 * (1 + 2.0 ** -9), -2.0 ** -126, 2.0 ** -126 * (1 + 2.0 ** -10), -0.0, 0.0, 65280.0, -1e30], np.float32)


def pack_blocks(nblocks, n, key=0):
    """[nblocks, n, n] float32 with the special values scattered in (where the block has room)"""
    r = rng('pack', nblocks, n, key)
    b = f32(r.standard_normal((nblocks, n, n)) * np.exp(r.uniform(-8, 8, (nblocks, n, n))))
    flat = b.reshape(-1)
    k = min(PACK_SPECIALS.size, flat.size)
    flat[r.choice(flat.size, k, replace=False)] = PACK_SPECIALS[:k]
    return b


# ------------------------------------------------------------------------------------------------------------------ the plan
MM, CF, BX, BW = 0, 1, 2, 3                                 # GML_DENSE_SUPPORT_MM .. GML_DENSE_CONV_BWD_W
VEC_IN, VEC_OUT, VEC_OUT2 = 1, 2, 4


def plan_want(kind, c, with_h=True):
    """what gml_dense_plan must answer for a case, from the case's own road names (not from the launcher's code)"""
    v = lambda road, bit: bit if road == 'vec' else 0
    if kind == MM:
        return v(c['road_in'], VEC_IN) | v(c['road_out'], VEC_OUT) | nft_of(c['F']) << 8
    if kind == CF:
        return v(c['road_x'], VEC_IN) | (v(c['road_h'], VEC_OUT) if with_h else 0) | v(c['road_o'], VEC_OUT2) | nft_of(c['Fin']) << 8 | not_of(c['Fout']) << 16
    if kind == BX:
        return v(c['road_o'], VEC_OUT) | nft_of(c['Fin']) << 8 | not_of(c['Fout']) << 16
    return v(c['road_x'], VEC_IN) | nft_of(c['Fin']) << 8 | -(-c['Fout'] // 64) << 16


def plan_ask(L, kind, c, p_in=0, p_out=0, p_out2=0):
    """gml_dense_plan for a case with the operands at the given addresses (integers; never dereferenced)"""
    if kind == MM:
        return int(L.gml_dense_plan(MM, p_in, c['lda'], c['sa'], p_out, c['ldo'], c['so'], None, 0, c['F'], 0))
    if kind == CF:
        return int(L.gml_dense_plan(CF, p_in, c['ldx'], 0, p_out or None, 0, 0, p_out2, c['ldo2'], c['Fin'], c['Fout']))
    if kind == BX:
        return int(L.gml_dense_plan(BX, None, 0, 0, p_out, c['lddx'], 0, None, 0, c['Fin'], c['Fout']))
    return int(L.gml_dense_plan(BW, p_in, c['ldx'], 0, None, 0, 0, None, 0, c['Fin'], c['Fout']))
