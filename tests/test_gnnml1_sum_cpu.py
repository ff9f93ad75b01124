"""The host side of the enzymes_contfeat GNNML1 (enzymes_contfeat.py:284-370) without a GPU: the reader's continuous features, the
training-split standardisation, the factory's state_dict against the reference class's keys and shapes, and the predicate of the
sum-and-factors block through the CPU-loaded library."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

ENZYMES = os.path.join(GOLDEN, 'raw', 'enzymes.mat')


@pytest.fixture(scope='module')
def contfeat():
    from gnn_matlang_amd import readers
    return readers.load_tu(ENZYMES, 'enzymes', contfeat=True)


def test_load_tu_contfeat_keeps_every_column(contfeat):
    from gnn_matlang_amd import readers
    assert len(contfeat) == 600 and all(x.shape[1] == 21 and x.dtype == np.float32 for x, _, _ in contfeat)
    assert contfeat[0][0].shape == (37, 21)
    np.testing.assert_allclose(contfeat[0][0][0, :6], [1, 0, 0, 11, 15.887014, 37.78], rtol=1e-7)
    ys = np.array([int(y) for _, _, y in contfeat])
    assert ys.min() == 0 and ys.max() == 5
    plain = readers.load_tu(ENZYMES, 'enzymes')
    assert len(plain) == 600
    for (x, ei, y), (xc, eic, yc) in zip(plain, contfeat):
        assert x.shape[1] == 3 and np.array_equal(x, xc[:, :3]) and np.array_equal(ei, eic) and y == yc


def test_standardize_tu_against_numpy_float64(contfeat):
    from gnn_matlang_amd import readers
    gs = []
    for x, ei, y in contfeat[:120]:                              # the degree column first, as the script does
        deg = np.bincount(ei[0], minlength=x.shape[0]).astype(np.float32)
        gs.append((np.concatenate((x, deg[:, None]), 1), ei, y))
    train = [i for i in range(len(gs)) if i % 10 != 0]
    out, (mean, std) = readers.standardize_tu(gs, train)
    tr = np.concatenate([gs[i][0] for i in train], 0).astype(np.float64)
    m64, s64 = tr.mean(0), tr.std(0, ddof=1)
    np.testing.assert_allclose(mean, m64, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(std, s64, rtol=1e-6, atol=1e-6)
    assert len(out) == len(gs)
    for (x, ei, y), (xs, eis, ysd) in zip(gs, out):
        assert xs.dtype == np.float32 and xs.shape == x.shape and eis is ei and ysd == y
        assert np.abs(xs - (x.astype(np.float64) - m64) / s64).max() <= 1e-6 * max(1.0, np.abs(xs).max())
    st = np.concatenate([out[i][0] for i in train], 0).astype(np.float64)
    assert np.abs(st.mean(0)).max() <= 1e-4 and np.abs(st.std(0, ddof=1) - 1).max() <= 1e-4
    # records of SpectralDesign.design_many pass as well
    recs, _ = readers.standardize_tu([dict(x=g[0], edge_index=g[1], y=g[2]) for g in gs], train)
    assert all(np.array_equal(r['x'], o[0]) and r['edge_index'] is o[1] for r, o in zip(recs, out))


# the reference class's parameters and buffers (enzymes_contfeat.py:295-315)
def _reference_shapes(ninp=22):
    sh = {}
    for i, fin in ((1, ninp), (2, 192)):
        sh['bn%d.weight' % i] = sh['bn%d.bias' % i] = sh['bn%d.running_mean' % i] = sh['bn%d.running_var' % i] = (192,)
        sh['bn%d.num_batches_tracked' % i] = ()
        sh['conv%d1.weight' % i], sh['conv%d1.bias' % i] = (1, fin, 128), (128,)
        sh['fc%d1.weight' % i], sh['fc%d1.bias' % i] = (128, fin), (128,)
        for j in (2, 3):
            sh['fc%d%d.weight' % (i, j)], sh['fc%d%d.bias' % (i, j)] = (64, fin), (64,)
    sh['fc2.weight'], sh['fc2.bias'] = (6, 384), (6,)
    return sh


def test_factory_state_dict_is_the_reference_class(contfeat):
    from gnn_matlang_amd import models
    m = models.enzymes_contfeat_gnnml1()
    assert m.dropout == 0.2 and m.form == 'sum_factors' and m.pool == ('mean', 'max')
    sd = m.state_dict()
    ref = _reference_shapes()
    assert set(sd) == set(ref), set(sd) ^ set(ref)
    assert 'fc1.weight' not in sd
    for k, shape in ref.items():
        assert tuple(sd[k].shape) == shape, k
    torch.manual_seed(0)
    ck = {k: (torch.randn(shape) if k != 'bn1.num_batches_tracked' and k != 'bn2.num_batches_tracked' else torch.tensor(7))
          for k, shape in ref.items()}
    m.load_state_dict(ck, strict=True)
    assert torch.equal(m.fc2.weight, ck['fc2.weight']) and int(m.bn2.num_batches_tracked) == 7
    with pytest.raises(ValueError):
        models.GNNML1Blocks(22, (128, 64, 64), 2, form='sum_factors')
    # the other forms keep three parts
    assert models.GNNML1Blocks(4, (16, 16, 16), 1, form='factors').fc2.in_features == 32
    assert models.GNNML1Blocks(4, (16, 16, 8), 1, form='sum_factors', head='log_softmax').fc2.in_features == 24


def test_predicates_through_the_cpu_loaded_library():
    from gnn_matlang_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)                               # loads without a GPU
    s = L.gml_gnnml1_sum_supported
    s.restype, s.argtypes = ctypes.c_int, [ctypes.c_int32] * 4
    assert s(192, 128, 128, 64) == 1 and s(22, 128, 128, 64) == 1 and s(1, 1, 1, 1) == 1
    assert s(193, 128, 128, 64) == 0 and s(192, 129, 129, 64) == 0 and s(192, 128, 128, 65) == 0
    assert s(192, 128, 64, 64) == 0 and s(0, 1, 1, 1) == 0
    o = L.gml_gnnml1_supported                                   # modes 0 .. 3: as before
    o.restype, o.argtypes = ctypes.c_int, [ctypes.c_int32] * 5
    assert o(144, 64, 64, 64, 2) == 1 and o(145, 64, 64, 16, 2) == 0 and o(64, 64, 64, 65, 2) == 0
    assert o(192, 128, 128, 64, 4) == 0                          # (mode 4 has its own entry points)
    g = L.gml_gnnml1_sum_g4_cols
    g.restype, g.argtypes = ctypes.c_int, [ctypes.c_int32] * 3
    f = L.gml_gnnml1_sum_dw_floats
    f.restype, f.argtypes = ctypes.c_int64, [ctypes.c_int32] * 4
    assert g(128, 128, 64) == 384 and g(10, 10, 7) == 64
    assert f(192, 128, 128, 64) == 192 * (128 + 128 + 64 + 64) + 384
