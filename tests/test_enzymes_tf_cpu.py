"""CPU checks of the enzymes_contfeats_gnnml3_tf.py port: the design against a float64 restatement of the script's lines 52-115,
standardize_tu(ddof=0) against its normalize_wrt_train, the loss, the factory's state and the conditioning of the inputs the GPU
model tests use (tests/test_gpu_enzymes_tf.py)."""
import os

import numpy as np
import pytest
import torch

import _dssgcn_ref as ref
from conftest import GOLDEN, rel_err
from gnn_matlang_amd import dense_block, models, readers

ORDER = (3, 0, 1, 2)           # script support i = project support ORDER[i]


def _script_supports(A, recfield=5, dv=1.0, nkernel=4):
    """lines 52-70 and 98-111 of the script for one graph, float64: (M bool [n, n], SP [nkernel, n, n])"""
    n = A.shape[0]
    W = 1.0 * A
    d = W.sum(axis=0)
    with np.errstate(divide='ignore'):
        dis = 1 / np.sqrt(d)
    dis[~np.isfinite(dis)] = 0
    D = np.diag(dis)
    nL = np.eye(n) - (W.dot(D)).T.dot(D)
    V, U = np.linalg.eigh(nL)
    V[V < 0] = 0
    M = A + np.eye(n)
    for _ in range(1, recfield):
        M = M.dot(M)
        M = np.minimum(M, 1.0)                     # (the pattern is all that is used: keeps the powers finite)
    M = M > 0
    SP = np.zeros((nkernel, n, n))
    SP[0] = np.eye(n)
    for ii, fc in enumerate(np.linspace(V.min(), V.max(), nkernel - 1)):
        SP[ii + 1] = M * (U.dot(np.diag(np.exp(-(dv * (V - fc) ** 2)))).dot(U.T))
    return M, SP


def test_design_against_the_script():
    raw, recs, _, _ = ref.enzymes_design(GOLDEN)
    assert len(raw) == 600
    sizes = [g[0].shape[0] for g in raw]
    assert sum(sizes) == 19580 and max(sizes) == 126
    worst, nmask = 0.0, 0
    for (x, ei, y), r in zip(raw, recs):
        n = x.shape[0]
        A = np.zeros((n, n))
        A[ei[0], ei[1]] = 1
        M, SP = _script_supports(A)
        got = np.zeros((n, n), dtype=bool)
        got[r['edge_index2'][0], r['edge_index2'][1]] = True
        assert np.array_equal(got, M)                                       # the masks are equal
        assert r['edge_index2'].shape[1] == int(M.sum())
        nmask += int(M.sum())
        for i in range(4):
            d = np.abs(r['edge_attr2'][:, ORDER[i]].astype(np.float64) - SP[i][r['edge_index2'][0], r['edge_index2'][1]]).max()
            worst = max(worst, d)
        assert np.array_equal(r['x'][:, :21], x) and np.array_equal(r['x'][:, 21], A.sum(0).astype(np.float32))
    print('largest absolute support difference', worst)
    assert nmask == 728438
    assert worst <= 1e-6            # float32 storage of O(1) values (6e-8) with a 10 x margin


def test_standardize_tu_ddof0_is_normalize_wrt_train():
    raw, recs, std, train = ref.enzymes_design(GOLDEN)
    tmp = np.vstack([recs[i]['x'].astype(np.float64) for i in train])       # normalize_wrt_train, lines 119-129
    avg, st = tmp.mean(0), tmp.std(0)
    for i in (0, 18, 37, 296, 599):
        want = (recs[i]['x'].astype(np.float64) - avg) / st
        assert np.abs(std[i]['x'] - want).max() <= 1e-6 * max(1.0, np.abs(want).max())
    # the default stays the unbiased estimate
    d1, (m1, s1) = readers.standardize_tu(recs[:40], list(range(30)))
    t = np.vstack([recs[i]['x'].astype(np.float64) for i in range(30)])
    assert np.array_equal(s1, t.std(0, ddof=1)) and np.array_equal(m1, t.mean(0))
    d0, (m0, s0) = readers.standardize_tu(recs[:40], list(range(30)), ddof=0)
    assert np.array_equal(s0, t.std(0)) and not np.array_equal(s0, s1)


def test_dssgcn_loss_formula():
    m, P = ref.new_model()
    rng = np.random.default_rng(0)
    logits = rng.normal(size=(7, 6))
    y = rng.integers(0, 6, size=7)
    got = float(models.dssgcn_loss(m, torch.tensor(logits, dtype=torch.float32), torch.tensor(y), weight_decay=1e-4).detach())
    lse = np.log(np.exp(logits).sum(1))
    want = (lse - logits[np.arange(7), y]).mean() + 1e-4 * sum(0.5 * (v ** 2).sum() for k, v in P.items() if not k.endswith('bias'))
    assert abs(got - want) <= 1e-5 * abs(want)
    assert sum(1 for k in P if not k.endswith('bias')) == 4


def test_factory_state():
    m, _ = ref.new_model()
    sd = m.state_dict()
    assert dict((k, tuple(v.shape)) for k, v in sd.items()) == {
        'conv1.weight': (4, 22, 200), 'conv2.weight': (4, 200, 200), 'fc1.weight': (100, 400), 'fc1.bias': (100,),
        'fc2.weight': (6, 100), 'fc2.bias': (6,)}
    assert 'dropout_state' not in sd and m.dropout_state.dtype == torch.int64 and m.dropout == 0.1
    for conv in (m.conv1, m.conv2):                                          # every slice: glorot([Fin, Fout])
        a = np.sqrt(6.0 / (conv.weight.shape[1] + conv.weight.shape[2]))
        w = conv.weight.detach().numpy()
        assert np.abs(w).max() <= a and np.abs(w).max() > 0.95 * a and abs(w.mean()) < 0.05 * a


def test_ragged_supports_refuse_129_nodes():
    ptr = torch.tensor([0, 5, 134, 140], dtype=torch.int32)
    with pytest.raises(ValueError, match='graph 1 has 129 nodes'):
        dense_block.RaggedSupports(torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, 4), torch.zeros(140, dtype=torch.int64), ptr)


@pytest.mark.parametrize('training', [False, True])
def test_fp32_restatement_against_float64(training):
    """the inputs of the GPU model tests do not sit on a relu edge: the restatement in float32 stays within the GPU tolerance of itself
    in float64 (a seed that fails this is changed, not the tolerance).  The HIP road's products carry the rounding of the bf16x3 format
    (2^-16 per product, a hundred times float32's), so the same condition is also asked at THAT precision: the restatement with the
    value of every support product rounded as bf16x3 rounds it (_dssgcn_ref.conv_layer).  Measured while choosing the parameter seed,
    largest rel_err over logits and gradients, eval / training: seed 1234: 2.1e-3 / 2.1e-5, seed 1: 8.3e-6 / 2.6e-2, seed 2: 7.4e-6 /
    1.0e-5 (float32: below 2e-6 for all of them) -- a relu pattern that flips under 1e-5 of noise moves a whole row of the first
    layer's weight gradient; seed 2 is the one in use."""
    graphs = [ref.enzymes8(GOLDEN)[i] for i in ref.PERM]
    sizes = [g['x'].shape[0] for g in graphs]
    assert sorted(sizes)[0] == 2 and set((2, 4, 100, 124, 126, 122)) <= set(sizes)
    _, P = ref.new_model()
    y = [int(g['y']) for g in graphs]
    masks = ref.philox_masks(sizes, 4, ref.DIMS, ref.DROP_P, ref.DROP_SEED, 1) if training else None
    hi = ref.model(graphs, P, y, masks, ref.DROP_P, dtype=torch.float64)
    for what, lo in (('float32', ref.model(graphs, P, y, masks, ref.DROP_P, dtype=torch.float32)),
                     ('bf16x3', ref.model(graphs, P, y, masks, ref.DROP_P, bf16x3=True))):
        assert rel_err(lo[0], hi[0]) <= 1e-4, what
        assert abs(lo[1] - hi[1]) <= 1e-4 * abs(hi[1]), what
        for k in hi[2]:
            e = rel_err(lo[2][k], hi[2][k])
            print(what, k, e)
            assert e <= 1e-4, (what, k)
