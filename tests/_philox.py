"""CPU restatement (numpy) of the dropout mask contract of include/gml.h (gml_dropout_fwd): Philox4x32-10 (Salmon, Moraes, Dror,
Shaw, SC'11) keyed by the 64-bit seed, counter block (j lo, j hi, site, counter lo) for j = e >> 2, word e & 3 = the draw of the
logical element e = r C + c; keep e iff draw >= t with t = floor(p 2^32)."""
import math

import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LO = np.uint64(0xffffffff)
_32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """four uint32 arrays (broadcast) of the Philox4x32-10 output block for counter (c0, c1, c2, c3) and key (k0, k1)"""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) & _LO for v in (c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xffffffff), np.uint64(int(k1) & 0xffffffff)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                       # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> _32) ^ c1 ^ k0, p1 & _LO, (p0 >> _32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return tuple(v.astype(np.uint32) for v in (c0, c1, c2, c3))


def threshold(p):
    """t of the keep rule (2^32 for p = 1: nothing kept)"""
    return 1 << 32 if p == 1 else int(math.floor(float(p) * 4294967296.0))


def draws(n, seed, counter, site):
    """uint32 [n]: the draw of every logical element 0 .. n-1"""
    seed, counter = int(seed) & 0xffffffffffffffff, int(counter) & 0xffffffffffffffff
    j = np.arange((n + 3) // 4, dtype=np.uint64)
    w = philox4x32_10(j & _LO, j >> _32, np.uint64(site & 0xffffffff), np.uint64(counter & 0xffffffff), seed & 0xffffffff, seed >> 32)
    return np.stack(w, 1).reshape(-1)[:n]


def keep_mask(N, C, p, seed, counter, site):
    """bool [N, C]"""
    return (draws(N * C, seed, counter, site).astype(np.uint64) >= np.uint64(threshold(p))).reshape(N, C)


def pack(keep):
    """uint32 [ceil(n / 32)] packed keep bits of the flattened mask: bit e & 31 of word e >> 5"""
    k = np.asarray(keep, dtype=np.uint64).reshape(-1)
    k = np.concatenate([k, np.zeros((-k.size) % 32, dtype=np.uint64)]).reshape(-1, 32)
    return (k << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)


def scale(p):
    """float32(1 / (1 - p)), one rounding"""
    return np.float32(0.0) if p == 1 else np.float32(1.0 / (1.0 - float(p)))


def apply(x, keep, p):
    """y = keep ? x * scale : +0.0 in float32"""
    x = np.asarray(x, dtype=np.float32)
    return np.where(keep, x * scale(p), np.float32(0.0)).astype(np.float32)
