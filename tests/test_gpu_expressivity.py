"""Expressivity evaluation on the MI355X (csrc/gml_pairs.hip, gnn_matlang_amd/expressivity.py): the pair bitmap, the count and the
list equal numpy's `d > tol` exactly; the reference loops of sr25.py, graph8c.py and exp_iso.py give the reference's counts."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

RAW = os.path.join(GOLDEN, 'raw')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


def np_dist(E, rows=None, slab=64):
    """numpy's float32 d[i, j] = |E_i - E_j|_1 in the reference's form (graph8c.py:298), slab by slab"""
    G = E.shape[0]
    out = np.empty((G, G), dtype=np.float32)
    for a in range(0, G, slab):
        out[a:a + slab] = np.abs(np.expand_dims(E[a:a + slab], 1) - np.expand_dims(E, 0)).sum(2)
    return out


def np_bitmap(sep):
    """the all-pairs bitmap of include/gml.h for a bool [G, G] separation matrix: bits j > i of row i, W = ceil(G / 64) words"""
    G = sep.shape[0]
    W = (G + 63) // 64
    m = np.zeros((G, W * 64), dtype=bool)
    m[:, :G] = np.triu(sep, 1)
    return np.packbits(m, axis=1, bitorder='little').view('<u8').reshape(G, W)


def similar_pairs_np(sep):
    i, j = np.nonzero(np.triu(~sep, 1))
    return np.stack([i, j], 1).astype(np.int64)


def embeddings(G, D, seed, ld=None):
    """float32 [G, D] with many near-equal rows (so that both outcomes occur), as a view of a [G, ld] array when ld > D"""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((max(G // 3, 1), D)).astype(np.float32)
    E = base[rng.integers(0, base.shape[0], G)] + (rng.standard_normal((G, D)) * 10.0 ** rng.uniform(-7, -2, (G, 1))).astype(np.float32)
    E = E.astype(np.float32)
    if ld is None:
        return E, None
    wide = rng.standard_normal((G, ld)).astype(np.float32)
    wide[:, :D] = E
    return E, wide


def check_tracker(tr, sep):
    G = sep.shape[0]
    bits = tr.bits[:G * ((G + 63) // 64)].cpu().numpy().view('<u8').reshape(G, -1) if G else np.zeros((0, 0), '<u8')
    assert np.array_equal(bits, np_bitmap(sep))
    ref = similar_pairs_np(sep)
    assert tr.similar() == ref.shape[0]
    assert np.array_equal(tr.similar_pairs().cpu().numpy().reshape(-1, 2), ref)


@pytest.mark.parametrize('G', [1, 2, 63, 64, 65, 1000, 4097])
@pytest.mark.parametrize('D', [1, 6, 10, 16, 33, 128])
def test_all_pairs_equal_numpy(dev, G, D):
    from gnn_matlang_amd.expressivity import PairTracker
    tr = PairTracker(G, device=dev)
    sep = np.zeros((G, G), dtype=bool)
    for u in range(3):                      # three cumulative updates; the second one through strided rows
        E, wide = embeddings(G, D, 1000 * G + 10 * D + u, ld=D + 3 if u == 1 else None)
        if wide is not None:
            t = torch.from_numpy(wide).to(dev)[:, :D]
            assert t.stride(0) == D + 3
        else:
            t = torch.from_numpy(E).to(dev)
        tr.update(t)
        sep |= np_dist(E) > 0.001
        check_tracker(tr, sep)
    tr.reset()
    assert tr.similar() == G * (G - 1) // 2


@pytest.mark.parametrize('D', [6, 10, 33])
def test_tol_at_exact_distances(dev, D):
    """tol = numpy distances of chosen pairs and their float32 neighbours: d > tol decided exactly as numpy decides it"""
    from gnn_matlang_amd.expressivity import PairTracker
    G = 300
    E, _ = embeddings(G, D, 7 + D)
    d = np_dist(E)
    iu = np.triu_indices(G, 1)
    vals = np.sort(d[iu])
    for q in (0.1, 0.5, 0.9):
        t0 = vals[int(q * (vals.size - 1))]
        for tol in (np.nextafter(t0, np.float32(0)), t0, np.nextafter(t0, np.float32(np.inf))):
            tr = PairTracker(G, tol=float(tol), device=dev)
            tr.update(torch.from_numpy(E).to(dev))
            check_tracker(tr, d > tol)


def test_nan_and_inf_rows(dev):
    from gnn_matlang_amd.expressivity import PairTracker
    G, D = 130, 10
    E, _ = embeddings(G, D, 3)
    E[5] = np.nan
    E[17, 3] = np.nan
    E[40] = np.inf
    E[41] = np.inf                   # inf - inf = nan: never separated
    E[90, 0] = -np.inf
    E[128, 9] = np.inf
    tr = PairTracker(G, device=dev)
    tr.update(torch.from_numpy(E).to(dev))
    with np.errstate(invalid='ignore'):
        sep = np_dist(E) > 0.001
    check_tracker(tr, sep)


@pytest.mark.parametrize('D', [1, 10, 128])
def test_pair_list_equals_numpy(dev, D):
    from gnn_matlang_amd.expressivity import PairTracker
    G, P = 500, 1000
    rng = np.random.default_rng(D)
    pairs = rng.integers(0, G, (P, 2))
    pairs[:50] = pairs[50:100]                    # repeated pairs and i == j pairs are allowed
    pairs[100:110, 1] = pairs[100:110, 0]
    tr = PairTracker(G, pairs=pairs, device=dev)
    sep = np.zeros(P, dtype=bool)
    for u in range(3):
        E, _ = embeddings(G, D, 50 + u)
        tr.update(torch.from_numpy(E).to(dev))
        sep |= np.abs(E[pairs[:, 0]] - E[pairs[:, 1]]).sum(1) > 0.001
        words = tr.bits.cpu().numpy().view('<u8')
        exp = np.packbits(np.concatenate([sep, np.zeros(-P % 64, bool)]), bitorder='little').view('<u8')
        assert np.array_equal(words[:exp.size], exp)
        assert tr.similar() == int((~sep).sum())
        assert np.array_equal(tr.similar_pairs().cpu().numpy(), pairs[~sep])


def test_list_cap_smaller_than_count(dev):
    from gnn_matlang_amd.expressivity import PairTracker
    G, D = 1000, 10
    E, _ = embeddings(G, D, 11)
    tr = PairTracker(G, device=dev)
    tr.update(torch.from_numpy(E).to(dev))
    ref = similar_pairs_np(np_dist(E) > 0.001)
    assert ref.shape[0] > 100
    for cap in (0, 1, 37, ref.shape[0] - 1):
        got = tr.similar_pairs(cap=cap).cpu().numpy().reshape(-1, 2)
        assert np.array_equal(got, ref[:cap])
    assert tr.similar() == ref.shape[0]


def test_bad_inputs_raise(dev):
    from gnn_matlang_amd.expressivity import PairTracker
    tr = PairTracker(10, device=dev)
    with pytest.raises(TypeError):
        tr.update(torch.zeros(10, 4, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        tr.update(torch.zeros(10, 4))
    with pytest.raises(ValueError):
        tr.update(torch.zeros(9, 4, device=dev))
    with pytest.raises(ValueError):
        tr.update(torch.zeros(10, 129, device=dev))
    with pytest.raises(ValueError):
        PairTracker(10, pairs=[[0, 10]], device=dev)


def test_captured_update_and_count(dev):
    """update + count captured in a graph and replayed on new embeddings equal the eager result"""
    from gnn_matlang_amd.expressivity import PairTracker
    G, D = 2000, 10
    embs = [embeddings(G, D, 100 + u)[0] for u in range(4)]
    eager = PairTracker(G, device=dev)
    eager_counts = []
    for E in embs:
        eager.update(torch.from_numpy(E).to(dev))
        eager_counts.append(eager.similar())
    tr = PairTracker(G, device=dev)
    static = torch.zeros(G, D, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):              # warm-up outside the capture
        tr.update(static)
        tr.count_device()
    torch.cuda.current_stream().wait_stream(s)
    tr.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tr.update(static)
        cnt = tr.count_device()
    tr.reset()
    got = []
    for E in embs:
        static.copy_(torch.from_numpy(E))
        g.replay()
        got.append(int(cnt.item()))
    assert got == eager_counts
    assert torch.equal(tr.bits, eager.bits)
    assert np.array_equal(tr.similar_pairs().cpu().numpy(), eager.similar_pairs().cpu().numpy())


def _golden_batch(g, dev):
    from gnn_matlang_amd.graph import Batch
    b = {k[len('batch/'):]: g[k] for k in g.files if k.startswith('batch/')}
    ptr = np.concatenate([[0], np.cumsum(np.bincount(b['batch']))]).astype(np.int32)
    T = torch.from_numpy
    return Batch(x=T(b['x']), edge_index=T(b['edge_index']), edge_index2=T(b['edge_index2']), edge_attr2=T(b['edge_attr2']),
                 batch=T(b['batch']), ptr=T(ptr), y=T(b['y'])).to(dev)


@pytest.mark.parametrize('fname,factory', [('model_sr25_gnnml3.npz', 'sr25_gnnml3'), ('model_sr25_gnnml1.npz', 'sr25_gnnml1')])
def test_count_similar_sr25_golden(dev, fname, factory):
    """sr25.py:281-300 through count_similar: seeded models, no load_state_dict, the reference's printed counts"""
    from gnn_matlang_amd import expressivity, models
    g = np.load(os.path.join(GOLDEN, fname))
    counts = expressivity.count_similar(getattr(models, factory), _golden_batch(g, dev), seeds=[0, 1, 2])
    assert counts == [int(g['seed%d/similar' % s]) for s in range(3)]


@pytest.fixture(scope='module')
def fixture():
    return np.load(os.path.join(GOLDEN, 'expressivity.npz'))


@pytest.fixture(scope='module')
def graph8c(dev):
    from gnn_matlang_amd import SpectralDesign, collate, readers
    gs = readers.load_graph8c(os.path.join(RAW, 'graph8c.g6'))
    return collate(SpectralDesign(nmax=8, recfield=1, dv=2, nfreq=5, adddegree=True).design_many(gs)).to(dev)   # graph8c.py:16


@pytest.fixture(scope='module')
def exp(dev):
    from gnn_matlang_amd import SpectralDesign, collate, readers
    gs = readers.load_exp(os.path.join(RAW, 'exp.npz'))
    return collate(SpectralDesign(nmax=64, recfield=1, dv=2, nfreq=5, adddegree=True).design_many(gs)).to(dev)  # exp_iso.py:16


@pytest.mark.parametrize('run,factory,data', [('g8c_ml3', 'graph8c_gnnml3', 'graph8c'), ('g8c_ml1', 'graph8c_gnnml1', 'graph8c'),
                                              ('exp_ml3', 'exp_gnnml3', 'exp')])
def test_reference_counts(dev, fixture, graph8c, exp, run, factory, data):
    """graph8c.py:282-302 and exp_iso.py:284-304: cumulative counts and never-separated pairs equal the reference's"""
    from gnn_matlang_amd import expressivity, models
    b = graph8c if data == 'graph8c' else exp
    pairs = expressivity.exp_pairs(b.num_graphs) if data == 'exp' else None
    tr = expressivity.PairTracker(b.num_graphs, pairs=pairs, device=dev)
    counts = expressivity.count_similar(getattr(models, factory), b, seeds=fixture[run + '/seeds'].tolist(), tracker=tr)
    assert counts == fixture[run + '/counts'].tolist()
    assert np.array_equal(tr.similar_pairs().cpu().numpy().reshape(-1, 2), fixture[run + '/pairs'])


def test_graph8c_seed0_embeddings(dev, fixture, graph8c):
    from gnn_matlang_amd import models
    torch.manual_seed(0)
    m = models.graph8c_gnnml3().to(dev).eval()
    with torch.no_grad():
        E = m(graph8c).cpu().numpy()
    ref = fixture['g8c_ml3/emb0']
    assert E.shape == ref.shape
    assert np.abs(E - ref).max() <= 1e-5
