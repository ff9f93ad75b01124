"""CPU side of the expressivity evaluation (gnn_matlang_amd/expressivity.py, csrc/gml_pairs.hip): the summation order the
kernel follows, the graph8c and EXP loaders, the model factories' seeded parameters and the ABI's argument checks."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

RAW = os.path.join(GOLDEN, 'raw')
# sha256 over (x float32, edge_index int64, y int64) of every graph of EXP's GRAPHSAT.pkl, in file order, little-endian
EXP_PKL_SHA256 = 'c30b117b0cadf741fde07e74598ed19d5d1e4397cdf46d334e58ffd518fa9560'


def l1_numpy_order(a, b):
    """sum_k |a_k - b_k| over the last axis in float32, in the order csrc/gml_pairs.hip states for numpy's sum(axis=-1):
    D < 8 sequential from 0; else eight accumulators over the full 8-blocks, a pairwise combine, then the tail in order"""
    x = np.abs(a.astype(np.float32) - b.astype(np.float32))
    D = x.shape[-1]
    if D < 8:
        s = np.zeros(x.shape[:-1], dtype=np.float32)
        for k in range(D):
            s = s + x[..., k]
        return s
    nb = D // 8
    r = [x[..., m].copy() for m in range(8)]
    for blk in range(1, nb):
        for m in range(8):
            r[m] = r[m] + x[..., 8 * blk + m]
    s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for k in range(8 * nb, D):
        s = s + x[..., k]
    return s


@pytest.mark.parametrize('D', [1, 6, 7, 8, 9, 10, 16, 17, 64, 128])
def test_summation_order_matches_numpy(D):
    rng = np.random.default_rng(D)
    n = 96
    mag = 10.0 ** rng.uniform(-12, 12, size=(n, D))
    E = (rng.standard_normal((n, D)) * mag).astype(np.float32)
    mine = l1_numpy_order(E[:, None, :], E[None, :, :])
    ref = np.abs(np.expand_dims(E, 1) - np.expand_dims(E, 0)).sum(2)        # graph8c.py:298
    assert mine.dtype == ref.dtype == np.float32
    assert np.array_equal(mine.view(np.int32), ref.view(np.int32))
    ref2 = np.abs(E[0::2] - E[1::2]).sum(1)                                # exp_iso.py:300
    assert np.array_equal(l1_numpy_order(E[0::2], E[1::2]).view(np.int32), ref2.view(np.int32))


def test_threshold_is_float32():
    """numpy 2 compares a float32 array with float32(0.001): a distance equal to it does not separate"""
    t = np.float32(1e-3)
    d = np.array([t, np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0))], dtype=np.float32)
    assert (d > 0.001).tolist() == [False, True, False]


def test_graph8c_loader():
    from gnn_matlang_amd import readers
    gs = readers.load_graph8c(os.path.join(RAW, 'graph8c.g6'))
    assert len(gs) == 11117
    for x, ei, y in gs:
        assert x.shape == (8, 1) and x.dtype == np.float32 and (x == 1).all() and y == 0
        A = np.zeros((8, 8), dtype=np.int64)
        A[ei[0], ei[1]] = 1
        assert (A == A.T).all() and A.trace() == 0 and A.sum() == ei.shape[1]
    nodes = sum(g[0].shape[0] for g in gs)
    assert nodes == 88936


def test_exp_loader_equals_the_pickle():
    from gnn_matlang_amd import readers
    gs = readers.load_exp(os.path.join(RAW, 'exp.npz'))
    assert len(gs) == 1200
    h = hashlib.sha256()
    for x, ei, y in gs:
        assert x.dtype == np.float32 and x.ndim == 2 and x.shape[1] == 1
        assert ei.dtype == np.int64 and ei.shape[0] == 2 and ei.min() >= 0 and ei.max() < x.shape[0]
        h.update(np.ascontiguousarray(x, dtype='<f4').tobytes())
        h.update(np.ascontiguousarray(ei, dtype='<i8').tobytes())
        h.update(np.int64(y).astype('<i8').tobytes())
    assert h.hexdigest() == EXP_PKL_SHA256
    y = np.array([g[2] for g in gs])
    assert (y[0::2] != y[1::2]).all()          # 600 pairs (2k, 2k + 1), one of each label


def _params(m):
    return [(n, p.detach().clone()) for n, p in m.named_parameters()]


@pytest.mark.parametrize('name,oracle', [('graph8c_gnnml3', 'ml3'), ('exp_gnnml3', 'ml3'), ('graph8c_gnnml1', 'ml1')])
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_factories_seed_like_the_oracle(name, oracle, seed):
    from gnn_matlang_amd import models
    from oracle import models_oracle as MO
    torch.manual_seed(seed)
    mine = _params(getattr(models, name)())
    torch.manual_seed(seed)
    ref = _params(MO.sr25_gnnml3(ninp=2, ne=6) if oracle == 'ml3' else MO.OracleGNNML1Sum(2))
    assert [n for n, _ in mine] == [n for n, _ in ref]
    for (n, a), (_, b) in zip(mine, ref):
        assert a.shape == b.shape and torch.equal(a, b), n


def test_pair_abi_argument_checks():
    """the entry points reject bad arguments before touching a device"""
    from gnn_matlang_amd import _lib
    L = _lib.lib()
    assert L.gml_pair_bitmap_words(65536, -1) == 65536 * 1024
    assert L.gml_pair_bitmap_words(65536, -1) * 8 <= 0.6e9
    assert L.gml_pair_bitmap_words(65537, -1) == -1
    assert L.gml_pair_bitmap_words(1000, 130) == 3
    assert L.gml_pair_list_workspace_bytes(65536, -1) == 65536 * 8
    fake = ctypes.c_void_p(4096)
    tol = ctypes.c_float(1e-3)
    for G, D, ld in [(65537, 10, 10), (100, 0, 10), (100, 129, 129), (100, 10, 9), (-1, 10, 10)]:
        assert L.gml_pair_distinct_all(fake, ld, G, D, tol, fake, None) == _lib.GML_E_BADARG
    assert L.gml_pair_distinct_all(None, 10, 100, 10, tol, fake, None) == _lib.GML_E_BADARG
    assert L.gml_pair_distinct_list(fake, 10, 100, None, 5, 10, tol, fake, None) == _lib.GML_E_BADARG
    assert L.gml_pair_count_similar(fake, 65537, None, 0, fake, None) == _lib.GML_E_BADARG
    assert L.gml_pair_list_similar(fake, 100, None, 0, fake, -1, fake, fake, 8, None) == _lib.GML_E_BADARG
    assert L.gml_pair_list_similar(fake, 100, None, 0, fake, 10, fake, fake, 0, None) == _lib.GML_E_WORKSPACE


def test_tracker_needs_a_gpu_device():
    from gnn_matlang_amd import expressivity
    with pytest.raises(ValueError):
        expressivity.PairTracker(10, device='cpu')
    with pytest.raises(ValueError):
        expressivity.PairTracker(70000)
    assert expressivity.exp_pairs(6).tolist() == [[0, 1], [2, 3], [4, 5]]
