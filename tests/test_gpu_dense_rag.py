"""ABI-level checks of csrc/gml_dense_rag.hip (include/gml.h: gml_dense_rag_pack / _mask / _support_mm) on a bank of 14 graphs whose
sizes sit on the kernel's limits: row tiles of 16, K steps of 32, NP = 128.  References are float64 (tolerance: the bf16x3 one of every
dense test, conftest.rel_err <= 1e-4); keep bits are compared exactly with the numpy restatement of the dropout contract."""
import ctypes

import numpy as np
import pytest
import torch

import _philox
from conftest import rel_err
from gnn_matlang_amd import _lib
from gnn_matlang_amd import functional as Fn
from gnn_matlang_amd.graph import _ptr, _stream

pytestmark = pytest.mark.gpu

NP = 128
SIZES = [1, 2, 15, 16, 17, 31, 32, 33, 64, 96, 97, 127, 128, 40]
UNUSED = (8, 13)                                    # the slots no batch position names: poisoned with bf16 NaN
ORDER = [11, 3, 0, 12, 6, 1, 10, 5, 9, 2, 7, 4]     # the batch: 12 slots, shuffled
TOL = 1e-4
SENTINEL = -777.0


def _blocks(S, seed):
    """random NON-symmetric blocks [S, n, n] per graph: fill 5 % .. 100 %, mixed sign, magnitudes over four decades"""
    rng = np.random.default_rng(seed)
    out = []
    for g, n in enumerate(SIZES):
        fill = (0.05, 0.3, 0.7, 1.0)[g % 4]
        m = rng.random((n, n)) < fill
        m[rng.integers(n), rng.integers(n)] = True
        v = rng.normal(size=(S, n, n)) * 10.0 ** rng.integers(-2, 2, size=(S, n, n))
        out.append((v * m).astype(np.float32))
    return out


class Bank(object):
    def __init__(self, S, dev, seed):
        self.S, self.G = S, len(SIZES)
        self.blocks = _blocks(S, seed)
        ptr = np.concatenate([[0], np.cumsum(SIZES)])
        src, dst, val, batch = [], [], [], []
        for g, (n, blk) in enumerate(zip(SIZES, self.blocks)):
            j, i = np.nonzero(np.abs(blk).sum(0) > 0)               # block[s][j][i] = value of edge i -> j
            src.append(i + ptr[g]); dst.append(j + ptr[g]); val.append(blk[:, j, i].T)
            batch.append(np.full(n, g))
        ei = torch.tensor(np.stack([np.concatenate(src), np.concatenate(dst)]), dtype=torch.int64, device=dev)
        ea = torch.tensor(np.concatenate(val), dtype=torch.float32, device=dev).contiguous()
        bt = torch.tensor(np.concatenate(batch), dtype=torch.int64, device=dev)
        self.ptr = torch.tensor(ptr, dtype=torch.int32, device=dev)
        self.fwd = torch.full((self.G, S, 2, NP, NP), 0x1234, dtype=torch.int16, device=dev)   # (the pack zero-fills itself)
        self.bwd = torch.full_like(self.fwd, 0x1234)
        _lib.call('gml_dense_rag_pack', _ptr(ei), _ptr(ea), _ptr(bt), _ptr(self.ptr), _ptr(self.fwd), _ptr(self.bwd), int(ei.size(1)),
                  int(bt.numel()), self.G, S, _stream(dev))
        self.fwd_nan, self.bwd_nan = self.fwd.clone(), self.bwd.clone()
        for u in UNUSED:
            self.fwd_nan[u] = 0x7fc0
            self.bwd_nan[u] = 0x7fc0


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda')


@pytest.fixture(scope='module')
def banks(dev):
    return {1: Bank(1, dev, 11), 4: Bank(4, dev, 12)}


def _batch(order, dev):
    sizes = [SIZES[g] for g in order]
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    return sizes, ptr, torch.tensor(ptr, dtype=torch.int32, device=dev), torch.tensor(order, dtype=torch.int32, device=dev)


def _bf16_to_f64(img):
    return (img.cpu().numpy().astype(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


@pytest.mark.parametrize('S', [1, 4])
def test_pack(banks, S):
    bank = banks[S]
    f, t = _bf16_to_f64(bank.fwd), _bf16_to_f64(bank.bwd)
    f, t = f[:, :, 0] + f[:, :, 1], t[:, :, 0] + t[:, :, 1]           # hi + lo
    for g, n in enumerate(SIZES):
        ref = bank.blocks[g].astype(np.float64)
        assert np.all(np.abs(f[g, :, :n, :n] - ref) <= 2.0 ** -16 * np.abs(ref)), g
        pad = f[g].copy()
        pad[:, :n, :n] = 0
        assert not pad.any(), g                                       # everything outside n x n is zero
    assert np.array_equal(t, f.transpose(0, 1, 3, 2))                 # the second image is the transpose
    raw_f, raw_t = bank.fwd.cpu().numpy(), bank.bwd.cpu().numpy()
    assert np.array_equal(raw_t, raw_f.transpose(0, 1, 2, 4, 3))      # piece by piece


def _keep(sizes, S, p, seed, counter, site):
    """bool [B, S, NP, NP]: decision of element e = ((b S + s) NP + r) NP + k, False outside n_b x n_b"""
    B = len(sizes)
    k = _philox.keep_mask(B * S * NP, NP, p, seed, counter, site).reshape(B, S, NP, NP).copy()
    for b, n in enumerate(sizes):
        k[b, :, n:, :] = False
        k[b, :, :, n:] = False
    return k


def _words(keep):
    """uint32 [..., NP, 4]: bit k & 31 of word k >> 5 of row r"""
    k = keep.reshape(keep.shape[:-1] + (4, 32)).astype(np.uint64)
    return (k << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def _mask(ptr_d, B, S, p, state, site, bwd=True):
    dev = ptr_d.device
    mf = torch.full((B, S, NP, 4), -1, dtype=torch.int32, device=dev)
    mb = torch.full((B, S, NP, 4), -1, dtype=torch.int32, device=dev) if bwd else None
    t, scale = Fn.dropout_threshold(p)
    _lib.call('gml_dense_rag_mask', _ptr(ptr_d), _ptr(mf), _ptr(mb), B, S, ctypes.c_uint64(t), _ptr(state), ctypes.c_uint32(site), _stream(dev))
    return mf, mb, scale


@pytest.mark.parametrize('counter', [0, 5])
@pytest.mark.parametrize('site', [1, 3])
@pytest.mark.parametrize('p', [0.1, 0.5])
def test_mask_bits(dev, p, site, counter):
    sizes, _, ptr_d, _ = _batch(ORDER, dev)
    seed = 20240917
    state = Fn.dropout_state(seed, dev)
    state[1] = counter
    mf, mb, _ = _mask(ptr_d, len(sizes), 4, p, state, site)
    keep = _keep(sizes, 4, p, seed, counter, site)
    assert np.array_equal(mf.cpu().numpy().view(np.uint32), _words(keep))
    assert np.array_equal(mb.cpu().numpy().view(np.uint32), _words(keep.transpose(0, 1, 3, 2)))
    frac = keep[sizes.index(128)].mean()
    assert abs(frac - (1 - p)) < 0.02


def test_mask_p0_keeps_all_p1_keeps_none(dev):
    sizes, _, ptr_d, _ = _batch(ORDER, dev)
    state = Fn.dropout_state(7, dev)
    ones = np.zeros((len(sizes), 4, NP, NP), dtype=bool)
    for b, n in enumerate(sizes):
        ones[b, :, :n, :n] = True
    mf, mb, _ = _mask(ptr_d, len(sizes), 4, 0.0, state, 0)
    assert np.array_equal(mf.cpu().numpy().view(np.uint32), _words(ones))
    assert np.array_equal(mb.cpu().numpy().view(np.uint32), _words(ones))
    mf, mb, _ = _mask(ptr_d, len(sizes), 4, 1.0, state, 0)
    assert not mf.any() and not mb.any()


def _product(bank, img, mask, scale, gid, ptr_d, N, S, F, setting, dev, seed):
    """one launch in the forward setting (sa = 0, so = F, one output block per support) or the backward setting (sa = F, summed
    over s); the activation buffer carries NaN in its pad columns, the output buffer a sentinel in the columns never written"""
    rng = np.random.default_rng(seed)
    fwd_setting = setting == 'fwd'
    cin = F if fwd_setting else S * F
    cout = S * F if fwd_setting else F
    act = rng.normal(size=(N, cin)).astype(np.float32)
    buf = torch.full((N, cin + 4), float('nan'), dtype=torch.float32, device=dev)
    buf[:, :cin] = torch.tensor(act, device=dev)
    outs = []
    for _ in range(2):
        out = torch.full((N, cout + 4), SENTINEL, dtype=torch.float32, device=dev)
        _lib.call('gml_dense_rag_support_mm', _ptr(img), _ptr(mask), ctypes.c_float(scale), _ptr(gid), _ptr(ptr_d), _ptr(buf), cin + 4,
                  0 if fwd_setting else F, _ptr(out), cout + 4, F if fwd_setting else 0, 0 if fwd_setting else 1, int(ptr_d.numel() - 1),
                  S, bank.G, F, _stream(dev))
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])                            # no atomics: two launches agree bitwise
    assert np.all(outs[0][:, cout:] == SENTINEL)
    return act.astype(np.float64), outs[0][:, :cout]


def _reference(bank, order, ptr, act, S, F, setting, transposed, keep=None, scale=1.0):
    N = int(ptr[-1])
    ref = np.zeros((N, S * F if setting == 'fwd' else F))
    for b, g in enumerate(order):
        r0, r1 = int(ptr[b]), int(ptr[b + 1])
        n = r1 - r0
        for s in range(S):
            D = bank.blocks[g][s].astype(np.float64)
            if keep is not None:
                D = D * keep[b, s, :n, :n] * float(scale)
            if transposed:
                D = D.T
            if setting == 'fwd':
                ref[r0:r1, s * F:(s + 1) * F] = D @ act[r0:r1, :F]
            else:
                ref[r0:r1] += D @ act[r0:r1, s * F:(s + 1) * F]
    return ref


@pytest.mark.parametrize('setting', ['fwd', 'bwd'])
@pytest.mark.parametrize('F', [1, 22, 128, 129, 200, 256])
@pytest.mark.parametrize('S', [1, 4])
@pytest.mark.parametrize('direction', ['fwd', 'bwd'])
def test_product(banks, dev, direction, S, F, setting):
    bank = banks[S]
    sizes, ptr, ptr_d, gid = _batch(ORDER, dev)
    img = bank.fwd_nan if direction == 'fwd' else bank.bwd_nan
    act, got = _product(bank, img, None, 1.0, gid, ptr_d, int(ptr[-1]), S, F, setting, dev, 100 + F)
    ref = _reference(bank, ORDER, ptr, act, S, F, setting, direction == 'bwd')
    assert np.isfinite(got).all()
    err = rel_err(got, ref)
    print('rel_err', direction, S, F, setting, err)
    assert err <= TOL
    for b in range(len(sizes)):                                        # graph by graph: a small graph's rows are not hidden by a large one's
        sl = slice(int(ptr[b]), int(ptr[b + 1]))
        assert rel_err(got[sl], ref[sl]) <= TOL, (b, sizes[b])


@pytest.mark.parametrize('F', [22, 200])
def test_product_identity_batch_without_gid(banks, dev, F):
    bank = banks[4]
    order = list(range(len(SIZES)))
    sizes, ptr, ptr_d, _ = _batch(order, dev)
    act, got = _product(bank, bank.fwd, None, 1.0, None, ptr_d, int(ptr[-1]), 4, F, 'fwd', dev, 7)
    assert rel_err(got, _reference(bank, order, ptr, act, 4, F, 'fwd', False)) <= TOL


@pytest.mark.parametrize('F', [22, 200])
@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('direction', ['fwd', 'bwd'])
def test_product_with_mask(banks, dev, direction, p, F):
    bank = banks[4]
    sizes, ptr, ptr_d, gid = _batch(ORDER, dev)
    seed, counter, site = 99, 3, 5
    state = Fn.dropout_state(seed, dev)
    state[1] = counter
    mf, mb, scale = _mask(ptr_d, len(sizes), 4, p, state, site)
    keep = _keep(sizes, 4, p, seed, counter, site)
    # the transposed product uses the decision of (r, k) for the entry D[r][k] it reads as D^T[k][r]: random masks are not symmetric
    assert not np.array_equal(keep, keep.transpose(0, 1, 3, 2))
    img, bits = (bank.fwd_nan, mf) if direction == 'fwd' else (bank.bwd_nan, mb)
    setting = direction
    act, got = _product(bank, img, bits, scale, gid, ptr_d, int(ptr[-1]), 4, F, setting, dev, 300 + F)
    ref = _reference(bank, ORDER, ptr, act, 4, F, setting, direction == 'bwd', keep, _philox.scale(p))
    err = rel_err(got, ref)
    print('rel_err masked', direction, p, F, err)
    assert err <= TOL
    swapped = _reference(bank, ORDER, ptr, act, 4, F, setting, direction == 'bwd', keep.transpose(0, 1, 3, 2), _philox.scale(p))
    assert rel_err(got, swapped) > 100 * TOL


def test_range_limits_launch_nothing(banks, dev):
    bank = banks[4]
    sizes, ptr, ptr_d, gid = _batch(ORDER, dev)
    N = int(ptr[-1])
    act = torch.zeros(N, 1024, dtype=torch.float32, device=dev)
    out = torch.full((N, 1024), SENTINEL, dtype=torch.float32, device=dev)
    L = _lib.lib()

    def call(F=22, S=4, lda=1024, ldo=1024, sa=0, so=22, sum_s=0, img=None, a=None, o=None, pt=None, mask=None):
        return L.gml_dense_rag_support_mm(_ptr(bank.fwd) if img is None else img, mask, ctypes.c_float(1.0), _ptr(gid),
                                          _ptr(ptr_d) if pt is None else pt, _ptr(act) if a is None else a, lda, sa,
                                          _ptr(out) if o is None else o, ldo, so, sum_s, len(sizes), S, bank.G, F, _stream(dev))

    assert call(F=0) == _lib.GML_E_UNSUPPORTED
    assert call(F=257, so=257) == _lib.GML_E_UNSUPPORTED
    assert call(S=0) == _lib.GML_E_UNSUPPORTED
    assert call(lda=21) == _lib.GML_E_BADARG                           # lda < F
    assert call(sa=22, lda=87) == _lib.GML_E_BADARG                    # lda < (S - 1) sa + F
    assert call(ldo=87) == _lib.GML_E_BADARG                           # ldo < (S - 1) so + F
    assert call(sum_s=1, ldo=21) == _lib.GML_E_BADARG
    assert call(img=bank.fwd.data_ptr() + 2) == _lib.GML_E_BADARG      # images: 16 bytes
    assert call(a=act.data_ptr() + 2) == _lib.GML_E_BADARG
    assert call(o=out.data_ptr() + 2) == _lib.GML_E_BADARG
    assert call(pt=ptr_d.data_ptr() + 2) == _lib.GML_E_BADARG
    assert call(mask=act.data_ptr() + 4) == _lib.GML_E_BADARG          # keep bits: 16 bytes
    assert call(img=None, a=0) == _lib.GML_E_BADARG                    # NULL
    state = Fn.dropout_state(1, dev)
    mf = torch.full((len(sizes), 4, NP, 4), -1, dtype=torch.int32, device=dev)
    assert L.gml_dense_rag_mask(_ptr(ptr_d), _ptr(mf), None, len(sizes), 0, ctypes.c_uint64(5), _ptr(state), 0, _stream(dev)) == _lib.GML_E_BADARG
    assert L.gml_dense_rag_mask(_ptr(ptr_d), _ptr(mf), None, len(sizes), 4, ctypes.c_uint64((1 << 32) + 1), _ptr(state), 0,
                                _stream(dev)) == _lib.GML_E_BADARG
    assert L.gml_dense_rag_mask(_ptr(ptr_d), mf.data_ptr() + 4, None, len(sizes), 4, ctypes.c_uint64(5), _ptr(state), 0,
                                _stream(dev)) == _lib.GML_E_BADARG
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((mf == -1).all())    # nothing was launched
    assert call() == _lib.GML_OK                                       # and the same call with valid arguments runs
    torch.cuda.synchronize()
    assert not bool((out[:, :88] == SENTINEL).any())
