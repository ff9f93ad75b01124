"""freqclass.py's GNNML3 without a GPU: the factory's parameters against the reference's state_dict layout, the bandclass stand-in
generator, the bandclass.mat reader and the batched-blocks predicate."""
import numpy as np
import pytest
import torch


def _reference_layout():
    """key -> shape of the state_dict of freqclass.py:300-318 (three ML3Layer(learnedge=False, nout1=64, nout2=2) over ne = 6
    supports on one input feature, fc1: 66 -> 32, fc2: 32 -> 1)"""
    table = {}
    for i, fin in enumerate((1, 66, 66)):
        c = 'conv%d.' % (i + 1)
        table[c + 'conv1.weight'] = (6, fin, 64)
        table[c + 'conv1.bias'] = (64,)
        for fc in ('fc11', 'fc12'):
            table[c + fc + '.weight'] = (2, fin)
            table[c + fc + '.bias'] = (2,)
    table.update({'fc1.weight': (32, 66), 'fc1.bias': (32,), 'fc2.weight': (1, 32), 'fc2.bias': (1,)})
    return table


def test_factory_loads_the_reference_state_dict():
    from gnn_matlang_amd import models
    m = models.freqclass_gnnml3()
    table = _reference_layout()
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == table
    g = torch.Generator().manual_seed(0)
    sd = {k: torch.randn(*s, generator=g) for k, s in table.items()}
    m.load_state_dict(sd, strict=True)
    assert all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
    assert m.dropout == 0.2 and models.freqclass_gnnml3(dropout=0.0).dropout == 0.0
    assert m.pool == 'mean' and m.head == 'mlp' and m.nlayers == 3
    assert not any(getattr(m, 'conv%d' % i).learnedge for i in (1, 2, 3))
    assert models.freqclass_step_loss is models.exp_classify_step_loss and callable(models.accuracy_from_stats)


def test_bandclass_generator():
    from gnn_matlang_amd import synthetic
    a = synthetic.make_graphs('bandclass', 4, seed=3)
    b = synthetic.make_graphs('bandclass', 4, seed=3)
    c = synthetic.make_graphs('bandclass', 4, seed=4)
    for (xa, ea, ya), (xb, eb, yb) in zip(a, b):
        assert np.array_equal(xa, xb) and np.array_equal(ea, eb) and ya == yb          # deterministic per seed
    assert not np.array_equal(a[0][0], c[0][0])
    for n, k in ((200, 5), (120, 5), (97, 4)):
        for x, ei, y in synthetic.make_graphs('bandclass', 3, seed=1, n=n, k=k):
            assert x.shape == (n, 1) and x.dtype == np.float32 and np.isfinite(x).all() and int(y) in (0, 1)
            assert ei.dtype == np.int64 and ei.min() >= 0 and ei.max() < n
            A = np.zeros((n, n), dtype=np.int64)
            A[ei[0], ei[1]] += 1
            assert A.max() == 1 and np.array_equal(A, A.T) and not A.diagonal().any()      # symmetric, simple, no self loops
            assert (A.sum(1) >= k).all()
            assert abs(float(x.std()) - 1.0) < 1e-3
    ys = [int(y) for _, _, y in synthetic.make_graphs('bandclass', 32, seed=0)]
    assert 0 < sum(ys) < 32                                    # both labels occur


def test_load_bandclass(tmp_path):
    sio = pytest.importorskip('scipy.io')
    from gnn_matlang_amd import readers
    rng = np.random.default_rng(5)
    G, n = 3, 9
    U = np.triu((rng.random((G, n, n)) < 0.4), 1)
    A = (U | U.transpose(0, 2, 1)).astype(np.float64)
    Fm = rng.normal(size=(G, n))
    Y = np.array([[1.0], [0.0], [1.0]])
    path = str(tmp_path / 'bandclass.mat')
    sio.savemat(path, {'A': A, 'F': Fm, 'Y': Y})
    graphs = readers.load_bandclass(path)
    assert len(graphs) == G
    for i, (x, ei, y) in enumerate(graphs):
        assert x.dtype == np.float32 and x.shape == (n, 1) and np.array_equal(x[:, 0], Fm[i].astype(np.float32))
        r, c = np.where(A[i] > 0)
        assert ei.dtype == np.int64 and np.array_equal(ei, np.vstack((r, c)))
        assert float(y) == Y[i, 0]
    sio.savemat(path, {'A': A, 'F': Fm[:, :-1], 'Y': Y})
    with pytest.raises(ValueError):
        readers.load_bandclass(path)


def test_mid_applies_without_the_library():
    from gnn_matlang_amd import dense_block as DB
    assert (DB.SMALL_N, DB.MID_N, DB.MID_F) == (96, 256, 128)
    t = DB.mid_applies
    assert t(2, 97, 1) and t(64, 200, 66) and t(2, 256, 128)
    assert t(1, 200, 66, bank=True) and not t(1, 200, 66) and not t(0, 200, 66, bank=True)
    assert not t(2, 96, 66) and not t(2, 257, 66) and not t(2, 200, 129) and not t(2, 200, 0)
    # one graph keeps the large-graph kernel, small graphs the per-graph kernel
    assert DB.big_applies(1, 200, 64) and not DB.big_applies(2, 200, 64)
