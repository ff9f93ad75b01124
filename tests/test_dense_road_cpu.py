"""The two road records of the dense blocks without a GPU and without a library call: dense_block.dense_road (which kernel serves a
support product, whether the layer is one launch, its feature limit, its path label) against the kernel ranges of DESIGN.md s4.7 /
s4.12 / s4.17 written out here, and models.gnnml3_road (which road one GNNML3 forward takes, whether the relu hand-over is declared)
against written-out cases; then a CPU model whose executors are stubs: forward re-declares the hand-over on a change only."""
import itertools
import types

import pytest
import torch

from gnn_matlang_amd import dense_block as DB, models

# ---------------------------------------------------------------------------------------------------- dense_block.dense_road
# the size class of (n, number of graphs): s = gml_dense.hip, b = gml_dense_big.hip, m = gml_dense_mid.hip, - = no dense kernel.
# One column per number of graphs 0, 1, 2: first for plain supports, then for the slots of an EqualSupports bank.
CLASS = {
    1:    ('sss', 'sss'),
    96:   ('sss', 'sss'),
    97:   ('-bm', '-mm'),          # one graph: the large-graph kernel, unless it names a bank slot; two: batched blocks
    256:  ('-bm', '-mm'),
    257:  ('-b-', '---'),
    1024: ('-b-', '---'),
    1025: ('---', '---'),
}
KERNEL = {'s': ('small', 128, ''), 'b': ('big', 64, ', large graph'), 'm': ('mid', 128, ', batched blocks')}
GRID = list(itertools.product(sorted(CLASS), (0, 1, 2), (False, True), (1, 64, 65, 128, 129), (128, 129, None), (False, True)))


def _expected(n, graphs, bank, Fin, Fout, library):
    c = CLASS[n][int(bank)][graphs]
    if c == '-':
        return (None, False, 0, '')
    if library:                                               # torch.bmm serves the same size classes, at any width
        return ('library', False, None, '')
    product, fmax, label = KERNEL[c]
    if Fin > fmax:
        return (None, False, fmax, label)
    return (product, c == 's' and Fout == 128, fmax, label)   # one launch: the small kernel with a projection of <= 128 columns


def test_dense_road_table():
    assert (DB.SMALL_N, DB.SMALL_F, DB.CHAIN_FOUT, DB.MID_N, DB.MID_F, DB.BIG_N, DB.BIG_F) == (96, 128, 128, 256, 128, 1024, 64)
    assert len(GRID) == 7 * 3 * 2 * 5 * 3 * 2
    for n, graphs, bank, Fin, Fout, library in GRID:
        got = DB.dense_road(graphs, n, Fin, Fout, bank, library)
        assert isinstance(got, DB.DenseRoad) and tuple(got) == _expected(n, graphs, bank, Fin, Fout, library), (n, graphs, bank, Fin, Fout, library, got)
    # the shapes the experiments run, letter for letter
    R = DB.DenseRoad
    assert DB.dense_road(1024, 75, 64, 128) == R('small', True, 128, '')                       # MNIST-75, a layer 64 -> 128
    assert DB.dense_road(1024, 75, 64) == R('small', False, 128, '')                           # its bare support product
    assert DB.dense_road(1024, 75, 64, 129) == R('small', False, 128, '')
    assert DB.dense_road(1, 900, 48, 32) == R('big', False, 64, ', large graph')               # filtering.py's 30 x 30 grid
    assert DB.dense_road(64, 200, 66, 64, bank=True) == R('mid', False, 128, ', batched blocks')   # freqclass.py's bank
    assert DB.dense_road(64, 200, 66, 64, bank=True, library=True) == R('library', False, None, '')
    assert DB.dense_road(1, 900, 65, 32) == R(None, False, 64, ', large graph')
    assert DB.dense_road(3, 300, 1) == R(None, False, 0, '')
    assert DB.dense_road(2, 75, 0, 64).product is None and DB.dense_road(2, 0, 8, 64).product is None


def test_applies_agree_with_the_record():
    for n, graphs, bank, F, _, _ in GRID:
        product = DB.dense_road(graphs, n, F, None, bank).product
        assert DB.mid_applies(graphs, n, F, bank=bank) == (product == 'mid') == (CLASS[n][int(bank)][graphs] == 'm' and F <= 128)
        if not bank:
            assert DB.big_applies(graphs, n, F) == (product == 'big') == (CLASS[n][0][graphs] == 'b' and F <= 64)
    # tests/test_freqclass_cpu.py::test_mid_applies_without_the_library, as it stands there
    assert (DB.SMALL_N, DB.MID_N, DB.MID_F) == (96, 256, 128)
    t = DB.mid_applies
    assert t(2, 97, 1) and t(64, 200, 66) and t(2, 256, 128)
    assert t(1, 200, 66, bank=True) and not t(1, 200, 66) and not t(0, 200, 66, bank=True)
    assert not t(2, 96, 66) and not t(2, 257, 66) and not t(2, 200, 129) and not t(2, 200, 0)
    assert DB.big_applies(1, 200, 64) and not DB.big_applies(2, 200, 64)


# ---------------------------------------------------------------------------------------------------- models.gnnml3_road
MIN = models.DENSE_BIG_MIN_FILL
E_LO, E_HI = 235, 236            # 97 nodes: 0.025 * 97 * 97 = 235.225 edges is the threshold


def road(head='node', dense_n=0, bn=False, learnedge=False, fmax=48, chain=True, graphs=1, N=97, E=E_HI, pad_graph=False, bank=False,
         road=None, drop=False):
    return tuple(models.gnnml3_road(head, dense_n, bn, learnedge, fmax, chain, graphs, N, E, pad_graph, bank, road, drop))


CASES = [
    # ---- one graph of 97 nodes, no bank: the fill decides for a node-level model, never for a pooled one
    (dict(), ('big', False)),
    (dict(E=E_LO), ('sparse', True)),
    (dict(head='mlp32'), ('sparse', True)),
    (dict(head='mlp32', E=E_LO), ('sparse', True)),
    (dict(N=96, E=96 * 96), ('sparse', True)),                     # the small kernel's sizes are dense_n's, not this road's
    (dict(N=1024, E=1024 * 1024), ('big', False)),
    (dict(N=1025, E=1025 * 1025), ('sparse', True)),
    (dict(graphs=2, N=194, E=194 * 194), ('sparse', True)),
    (dict(fmax=64), ('big', False)),
    (dict(fmax=65), ('sparse', True)),
    (dict(bn=True, chain=False), ('sparse', False)),
    (dict(learnedge=True), ('sparse', True)),
    (dict(pad_graph=True), ('sparse', True)),
    # ---- the override, unchecked
    (dict(road='sparse'), ('sparse', True)),
    (dict(road='dense', E=E_LO), ('big', False)),
    (dict(road='dense', head='mlp32'), ('big', False)),            # a pooled model forced onto the dense road: chain withdrawn
    (dict(road='dense', head='mlp32', learnedge=True), ('big', False)),
    # ---- dropout passes and models that do not chain
    (dict(E=E_LO, drop=True), ('sparse', False)),
    (dict(E=E_LO, chain=False), ('sparse', False)),
    (dict(drop=True), ('big', False)),
    # ---- the model's own dense blocks (MNIST-75): 75 nodes per graph, with and without BatchNorm
    (dict(head='mlp32', dense_n=75, chain=False, graphs=4, N=300, E=20000), ('dense_n', False)),
    (dict(head='mlp32', dense_n=75, bn=True, chain=False, graphs=4, N=300, E=20000, drop=True), ('dense_n', False)),
    (dict(head='mlp32', dense_n=75, chain=False, graphs=4, N=300, E=20000, road='sparse'), ('dense_n', False)),
    (dict(head='mlp32', dense_n=75, chain=False, graphs=4, N=300, E=20000, road='dense'), ('big', False)),
    (dict(dense_n=75, chain=False, N=97), ('dense_n', False)),      # a node-level dense_n model: the fill does not pick 'big'
    # ---- a bank of equal-size graphs: with edge tensors
    (dict(head='mlp', bank=True, graphs=2, N=194, E=5000), ('mid', False)),
    (dict(head='node', bank=True, graphs=2, N=194, E=5000), ('mid', False)),
    (dict(head='mlp', bank=True, graphs=2, N=194, E=5000, drop=True), ('mid', False)),
    (dict(head='mlp', bank=True, graphs=2, N=194, E=5000, road='dense'), ('mid', False)),      # never 'big' together with 'mid'
    (dict(head='mlp', bank=True, graphs=2, N=194, E=5000, road='sparse'), ('sparse', True)),
    (dict(head='mlp', bank=True, graphs=2, N=194, E=5000, road='sparse', drop=True), ('sparse', False)),
    (dict(head='mlp', bank=True, graphs=2, N=194, E=5000, learnedge=True), ('sparse', True)),
    (dict(head='mlp', bank=True, graphs=2, N=194, E=5000, bn=True, chain=False), ('sparse', False)),
    (dict(head='mlp', bank=True, graphs=2, N=194, E=5000, pad_graph=True), ('sparse', True)),
    (dict(head='mlp', bank=True, graphs=2, N=150, E=5000, dense_n=75, chain=False), ('dense_n', False)),
    (dict(head='node', bank=True, graphs=1, N=97, E=E_HI, learnedge=True), ('sparse', True)),
    (dict(head='node', bank=True, graphs=1, N=97, E=E_HI, pad_graph=True), ('sparse', True)),
    (dict(head='node', bank=True, graphs=1, N=97, E=E_HI, road='sparse'), ('sparse', True)),
    # ---- and without them (DeviceDataset.batch_dense): 'mid' or an error
    (dict(head='mlp', bank=True, graphs=2, N=194, E=None), ('mid', False)),
    (dict(head='mlp', bank=True, graphs=2, N=194, E=None, road='dense'), ('mid', False)),
    (dict(head='mlp', bank=True, graphs=2, N=194, E=None, road='sparse'), ValueError),
    (dict(head='mlp', bank=True, graphs=2, N=194, E=None, learnedge=True), ValueError),
    (dict(head='mlp', bank=True, graphs=2, N=194, E=None, bn=True, chain=False), ValueError),
    (dict(head='mlp', bank=True, graphs=2, N=194, E=None, pad_graph=True), ValueError),
    (dict(head='mlp', bank=True, graphs=2, N=150, E=None, dense_n=75, chain=False), ValueError),
    # ---- no bank and no edge tensors (an assembled batch that carries its CSR): the sparse road, never 'big' by itself
    (dict(head='mlp32', graphs=4, N=300, E=None, learnedge=True), ('sparse', True)),
    (dict(head='mlp32', graphs=4, N=300, E=None, learnedge=True, pad_graph=True, drop=True), ('sparse', False)),
    (dict(head='node', E=None), ('sparse', True)),
]


@pytest.mark.parametrize('i', range(len(CASES)))
def test_gnnml3_road_cases(i):
    kw, want = CASES[i]
    if want is ValueError:
        with pytest.raises(ValueError, match='no edge tensors'):
            road(**kw)
    else:
        assert road(**kw) == want, kw


def test_gnnml3_road_fill_threshold():
    assert E_LO < MIN * 97 * 97 < E_HI
    assert road(E=E_LO) == ('sparse', True) and road(E=E_HI) == ('big', False)
    assert tuple(models.gnnml3_road('node', 0, False, False, 48, True, 1, 97, E_HI, False, False, None, False, min_fill=0.5)) == ('sparse', True)


# ---------------------------------------------------------------------------------------------------- forward declares on a change
def _batch(N, E, graphs=1, bank=None):
    ptr = torch.arange(graphs + 1, dtype=torch.int32) * (N // graphs)
    return types.SimpleNamespace(x=torch.zeros(N, 1), ptr=ptr, bank=bank,
                                 edge_index2=None if E is None else torch.zeros(2, E, dtype=torch.int64))


def _stubbed(m, monkeypatch):
    """m with counting stubs in place of _declare_chain and of everything that would launch: (declared values, executor names)"""
    declared, ran = [], []
    monkeypatch.setattr(m, '_declare_chain', lambda on: declared.append(on))
    monkeypatch.setattr(m, '_forward_sparse', lambda data, *a: (ran.append('sparse'), (data.x, False))[1])
    monkeypatch.setattr(m, '_forward_dense', lambda x, drop, nvalid, sp, n, gid: (ran.append(('dense', sp, n)), x)[1])
    monkeypatch.setattr(m, '_readout', lambda x, *a: x)
    monkeypatch.setattr(DB, 'batch_supports', lambda data, n: 'own')
    return declared, ran


def test_forward_declares_the_chain_on_a_change_only(monkeypatch):
    torch.manual_seed(0)
    bank = object.__new__(DB.EqualSupports)                     # (no launch: the road reads its type, the executor stub its n)
    bank.n = 97
    sparse, big, mid = _batch(97, E_LO), _batch(97, E_HI), _batch(194, None, graphs=2, bank=bank)
    m = models.filtering_gnnml3(1, 11)
    assert m._chain and m._chain_on and m._road_of(sparse) == ('sparse', True) and m._road_of(big) == ('big', False)
    assert m._road_of(mid) == ('mid', False) and (m._fin_max, m._learnedge) == (48, False)
    declared, ran = _stubbed(m, monkeypatch)
    for data in (sparse, sparse, mid, mid, sparse, big, sparse, sparse):
        m(data)
    assert declared == [False, True, False, True]               # sparse -> mid -> sparse -> big -> sparse: one call per change
    assert ran == ['sparse', 'sparse', ('dense', bank, 97), ('dense', bank, 97), 'sparse', ('dense', 'own', 97), 'sparse', 'sparse']
    m(big, _road='sparse')
    m(sparse, _road='dense')
    assert declared == [False, True, False, True, False] and ran[-2:] == ['sparse', ('dense', 'own', 97)]
    # a model without dropout on plain sparse batches (the ZINC step): no call at all
    z = models.zinc_gnnml3()
    declared, ran = _stubbed(z, monkeypatch)
    for _ in range(3):
        z(_batch(100, 700, graphs=4))
    assert declared == [] and ran == ['sparse'] * 3 and (z._fin_max, z._learnedge) == (32, True)
    # dropout: withdrawn for training passes, back in eval
    f = models.freqclass_gnnml3()
    declared, ran = _stubbed(f, monkeypatch)
    edges = _batch(194, 5000, graphs=2)
    f.train()
    f(edges), f(edges)
    f.eval()
    f(edges), f(edges)
    f(mid)
    f.train()
    f(mid), f(edges)
    assert declared == [False, True, False] and f._chain_on is False
    # a model that does not chain never declares
    d = models.mnist_gnnml3(dense_n=75)
    declared, ran = _stubbed(d, monkeypatch)
    d.eval()
    d(_batch(300, 20000, graphs=4))
    assert declared == [] and ran == [('dense', 'own', 75)] and not d._chain_on
