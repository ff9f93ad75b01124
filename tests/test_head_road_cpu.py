"""The road record of the readout head and loss without a GPU and without a library call: functional.head_road against the kernel
ranges of DESIGN.md s4.4c written out here and against the decision sequence of the step losses it replaced (restated below: four
predicates in their order); then models whose features and fused heads are stubs: every road of the three step losses runs the
model's features exactly once, with the record's pad_grad_zero."""
import itertools
import types

import pytest
import torch

from gnn_matlang_amd import functional as Fn, models

MLP32, MLP, LIN2, NODE = models._MLP32, models._MLP, models._LIN2, models._NODE
LDS = lambda R, nin, nh: 4 * (R * nin + 2 * R * nh + 2 * R + nh * nin + 256) <= 160 * 1024


def road(loss, head, listed, nin, nh, nout, R, nl, ng, f32=True, aligned=True, override=None, no_big=False, no_bce=False):
    env = dict(([('GML_NO_HEAD_BIG', '1')] if no_big else []) + ([('GML_NO_HEAD_BCE', '1')] if no_bce else []))
    got = Fn.head_road(loss, head, listed, nin, nh, nout, R, nl, ng, f32, aligned, override, env)
    assert isinstance(got, Fn.HeadRoad) and isinstance(got.label, str) and got.label
    return got


# ---------------------------------------------------------------------------------------------------- the table, written out
def _expected(loss, listed, nin, nh, nout, R, nl, ng, f32, aligned, no_big, no_bce):
    """(kind, pad_grad_zero): the ranges of the four kernels, in the order of preference"""
    if not listed or nout != 1:
        return 'torch', False
    if loss == 'l1':
        if f32 and aligned and nl <= R:
            if R <= 256 and nin <= 64 and nh <= 64 and nin % 4 == 0 and nh % 4 == 0 and LDS(R, nin, nh):
                return 'l1_small', ng <= 256 and nl <= ng
            if nin == nh == 32 and R >= 1 and not no_big:
                return 'l1_big', False
        return 'torch', False
    if loss == 'bce':                                             # features run before the support check: True on both roads
        return ('bce' if f32 and aligned and 1 <= nin <= 64 and 1 <= nh <= 64 and R >= 1 and nl <= R and not no_bce else 'torch'), True
    return ('node' if f32 and 1 <= nin <= 64 else 'torch'), False


# ---------------------------------------------------------------------------------------------------- the sequence it replaced
def _parent(loss, listed, nin, nh, nout, R, nl, ng, f32, aligned, no_big, no_bce):
    """(kind, the pad_grad_zero of the last features call, whether features ran twice) of the step losses before the record:
    head_l1_supported, head_l1_big_supported, head_bce_supported and node_head_supported as they stood, asked in their order.  f32:
    the rows are float32 on the device; aligned: what head_bce_supported asked of the weights (contiguity) -- the two L1 predicates
    did not look."""
    l1 = f32 and R <= 256 and nin <= 64 and nh <= 64 and nout == 1 and nin % 4 == 0 and nh % 4 == 0 and LDS(R, nin, nh)
    l1_big = f32 and nin == 32 and nh == 32 and nout == 1 and R > 0 and not no_big
    bce = f32 and R >= 1 and 1 <= nin <= 64 and 1 <= nh <= 64 and nout == 1 and aligned and not no_bce
    node = f32 and 1 <= nin <= 64 and nout == 1
    if loss == 'l1':
        if not (listed and nout == 1 and f32):
            return 'torch', False, False                          # model(data)
        pgz = ng <= 256 and nl <= ng
        if l1 and nl <= R:
            return 'l1_small', pgz, False
        redo = pgz                                                # "not the fused head after all": features(data) again
        return ('l1_big' if l1_big and nl <= R else 'torch'), False, redo
    if loss == 'bce':
        if not (listed and nout == 1):
            return 'torch', False, False
        return ('bce' if bce and nl <= R else 'torch'), True, False
    return ('node' if node else 'torch'), False, False            # (asked of whatever model it was handed)


GRID = [(loss, listed, nin, nh, nout, R, nl, ng, f32, aligned, no_big, no_bce)
        for loss, listed, nin, nh, nout, R in itertools.product(('l1', 'bce', 'node_sq'), (True, False), (4, 32, 33, 48, 64, 65, 66), (10, 32, 64, 65),
                                                                (1, 2), (0, 1, 256, 257))
        if listed or loss != 'node_sq'                          # (filtering_step_loss asks the node head of whatever model it gets)
        for nl in (R - 1, R, R + 1) if nl >= 0
        for ng in sorted({R, nl, 300})
        for f32, aligned, no_big, no_bce in itertools.product((True, False), repeat=4)]


def test_head_road_table():
    assert len(GRID) == 5 * 7 * 4 * 2 * (5 + 8 + 8 + 8) * 16 == 129920
    for c in GRID:
        loss, listed, nin, nh, nout, R, nl, ng, f32, aligned, no_big, no_bce = c
        got = road(loss, MLP32, listed, nin, nh, nout, R, nl, ng, f32, aligned, None, no_big, no_bce)
        assert (got.kind, got.pad_grad_zero) == _expected(*c), (c, got)
        # the override: that kind alone where it serves the input, else the torch ops; pad_grad_zero as the loss has it
        forced = road(loss, MLP32, listed, nin, nh, nout, R, nl, ng, f32, aligned, 'torch', no_big, no_bce)
        assert forced.kind == 'torch' and forced.pad_grad_zero == (loss == 'bce' and listed and nout == 1), (c, forced)


def test_head_road_on_the_shapes_the_experiments_run():
    R_ = Fn.HeadRoad
    small, big = 'fused L1 head, one workgroup (%d -> %d -> 1)', 'fused L1 head, one pass + fold (32 -> 32 -> 1)'
    # ZINC, GNNML3 32 -> 32 -> 1: the reference's batch 64 plain (64 rows) and padded (65 rows, 64 labels), and the bench's 131,072
    assert road('l1', MLP32, True, 32, 32, 1, 64, 64, 64) == R_('l1_small', True, small % (32, 32))
    assert road('l1', MLP32, True, 32, 32, 1, 65, 64, 65) == R_('l1_small', True, small % (32, 32))
    assert road('l1', MLP32, True, 32, 32, 1, 131072, 131072, 131072) == R_('l1_big', False, big)
    assert road('l1', MLP32, True, 32, 32, 1, 256, 256, 256).kind == 'l1_small' and road('l1', MLP32, True, 32, 32, 1, 257, 257, 257) == R_('l1_big', False, big)
    assert road('l1', MLP32, True, 32, 32, 1, 131072, 131072, 131072, no_big=True) == R_('torch', False, 'torch ops (L1 head outside the fused kernels)')
    # GNNML1 ZINC 48 -> 32: the small road up to its 256 rows, the torch ops beyond
    assert road('l1', MLP32, True, 48, 32, 1, 64, 64, 64) == R_('l1_small', True, small % (48, 32))
    assert road('l1', MLP32, True, 48, 32, 1, 257, 257, 257) == R_('torch', False, 'torch ops (L1 head outside the fused kernels)')
    # zinc_gin's 64 -> 32 -> 1 'mlp' head is not the 'mlp32' row: its own forward
    assert road('l1', MLP, False, 64, 32, 1, 64, 64, 64) == R_('torch', False, "torch ops (L1 on the model's own head)")
    # exp_classify: GNNML3 48 -> 10 (relu), GNNML1 64 -> 10 (identity); GNNML3 'mlp32' under BCE is not listed
    assert road('bce', MLP, True, 48, 10, 1, 3, 3, 3) == R_('bce', True, 'fused BCE head (48 -> 10 -> 1, relu)')
    assert road('bce', LIN2, True, 64, 10, 1, 9, 8, 9) == R_('bce', True, 'fused BCE head (64 -> 10 -> 1, identity)')
    assert road('bce', MLP, True, 48, 10, 1, 3, 3, 3, no_bce=True) == R_('torch', True, 'torch ops (BCE head outside the fused kernel)')
    assert road('bce', MLP32, False, 32, 32, 1, 3, 3, 3) == R_('torch', False, "torch ops (BCE on the model's own head)")
    # freqclass: GNNML3 66 -> 32 and GNNML1 96 -> 32, both on the torch ops
    assert road('bce', MLP, True, 66, 32, 1, 64, 64, 64) == R_('torch', True, 'torch ops (BCE head outside the fused kernel)')
    assert road('bce', MLP32, True, 96, 32, 1, 64, 64, 64) == R_('torch', True, 'torch ops (BCE head outside the fused kernel)')
    # filtering 48 -> 1 on the 900 nodes of the 30 x 30 grid; GAT's 8 x 8 = 64 and a width beyond the kernel
    assert road('node_sq', NODE, True, 48, 0, 1, 900, 0, 1) == R_('node', False, 'fused node head (48 -> 1)')
    assert road('node_sq', NODE, True, 64, 0, 1, 900, 0, 1).kind == 'node'
    assert road('node_sq', NODE, True, 65, 0, 1, 900, 0, 1) == R_('torch', False, 'torch ops (node head outside the fused kernel)')
    # the one workgroup's LDS: 48 -> 32 holds 343 rows, so inside its 256 rows the bound never decides for the 'mlp32' heads up to 64 wide
    assert LDS(343, 48, 32) and not LDS(344, 48, 32) and LDS(256, 64, 32) and not LDS(256, 64, 64)


def test_sweep_against_the_sequence_it_replaced():
    """every difference from the parent's decisions over the grid is the one deliberate deviation"""
    seen = dict(same=0, aligned=0, redo=0)
    for c in GRID:
        loss, listed, nin, nh, nout, R, nl, ng, f32, aligned, no_big, no_bce = c
        got = road(loss, MLP32, listed, nin, nh, nout, R, nl, ng, f32, aligned, None, no_big, no_bce)
        kind, pgz, redo = _parent(*c)
        seen['redo'] += redo            # the parent ran features twice here; the record gives its SECOND call's pad_grad_zero, once
        if (got.kind, got.pad_grad_zero) == (kind, pgz):
            seen['same'] += 1
        else:
            # fc1 / fc2 weights that are not contiguous or not on 16-byte boundaries: the launchers answer GML_E_UNSUPPORTED and the
            # parent raised; now the torch ops
            assert loss == 'l1' and not aligned and kind in ('l1_small', 'l1_big'), (c, got, kind, pgz)
            assert got == Fn.HeadRoad('torch', False, 'torch ops (L1 head outside the fused kernels)'), (c, got)
            seen['aligned'] += 1
    assert seen['same'] + seen['aligned'] == len(GRID) == 129920 and seen['aligned'] > 0 and seen['redo'] > 0, seen
    print('swept %d inputs: %s' % (len(GRID), seen))


def test_predicates_are_the_record():
    class _T(object):                                        # what head_l1_supported reads of a tensor
        def __init__(self, r, c, cuda=True, dtype=torch.float32):
            self.is_cuda, self.dtype, self._s = cuda, dtype, (r, c)

        def size(self, i):
            return self._s[i]

    for R, nin, nh, nout in itertools.product((0, 1, 188, 189, 256, 257), (4, 32, 33, 64, 65), (4, 32, 64, 65), (1, 2)):
        want = R <= 256 and nin <= 64 and nh <= 64 and nout == 1 and nin % 4 == 0 and nh % 4 == 0 and LDS(R, nin, nh)
        assert Fn.head_l1_supported(_T(R, nin), _T(nh, nin), _T(nout, nh)) == want, (R, nin, nh, nout)
        assert not Fn.head_l1_supported(_T(R, nin, cuda=False), _T(nh, nin), _T(nout, nh))
        assert not Fn.head_l1_supported(_T(R, nin, dtype=torch.float64), _T(nh, nin), _T(nout, nh))
    # CPU tensors: refused by every predicate that reads real tensors
    p, w1, w2 = torch.zeros(4, 32), torch.zeros(32, 32), torch.zeros(1, 32)
    assert not Fn.head_bce_supported(p, w1, w2) and not Fn.head_l1_big_supported(p, w1, w2)
    assert not Fn.node_head_supported(p, torch.nn.Linear(32, 1)) and not Fn.head_bce_supported(None, w1, w2)
    assert not Fn.head_bce_supported(p, None, w2) and not Fn.head_bce_supported(p, w1, 'x')


# ---------------------------------------------------------------------------------------------------- one features call per step
def _batch(B, nodes=4, pad=False, num_graphs=True, node_level=False):
    """B graphs (pad: plus the padding graph of a static batch, graph_valid [B] with one absent slot)"""
    rows = B + int(pad)
    d = types.SimpleNamespace(x=torch.zeros(rows * nodes, 1), ptr=torch.arange(rows + 1, dtype=torch.int32) * nodes, y=torch.zeros(B))
    if num_graphs:
        d.num_graphs = rows
    if pad:
        d.graph_valid = torch.tensor([1.0] * (B - 1) + [0.0])
    if node_level:
        d.y, d.mask = torch.zeros(rows * nodes, 3), torch.ones(rows * nodes, 1)
    return d


def _stubbed(m, monkeypatch):
    """m with a counting stub in place of its layers, and the fused heads as stubs: (calls of features, calls of the fused heads)"""
    feats, fused = [], []
    nin = int((m.fc1 if hasattr(m, 'fc1') else m.fc2).weight.size(1))

    def rows(data, pgz, node):
        models._dropout_pass(m)
        feats.append(pgz)
        return torch.zeros(int(data.x.size(0)) if node else int(data.ptr.numel()) - 1, nin)

    monkeypatch.setattr(m, 'features', lambda data, pad_grad_zero=False: rows(data, pad_grad_zero, False))

    def forward(data, _features=False, _road=None):
        x = rows(data, None, m.pool is None)
        return x if _features else models._apply_head(m, x)

    monkeypatch.setattr(m, 'forward', forward)
    monkeypatch.setattr(Fn, 'head_flags', lambda *a: (True, True))
    monkeypatch.setattr(Fn, 'POOLED_HEADS', {k: types.SimpleNamespace(apply=lambda p, *a, k=k: (fused.append((k, tuple(p.shape))), p.sum())[1])
                                             for k in Fn.POOLED_HEADS})
    monkeypatch.setattr(Fn.NodeHeadLossFunction, 'apply', lambda x, *a: (fused.append(('node', tuple(x.shape))), (x.sum(), None))[1])
    monkeypatch.setattr(Fn, 'VERBOSE', True)
    monkeypatch.setattr(Fn, 'PATHS', {})
    return feats, fused


def _one_step(fn, m, data, feats, fused, **kw):
    """(pad_grad_zero values features saw, fused calls, PATHS) of one call"""
    del feats[:], fused[:]
    Fn.PATHS.clear()
    loss = fn(m, data, **kw)
    assert isinstance(loss, torch.Tensor) and loss.dim() == 0
    return list(feats), list(fused), dict(Fn.PATHS)


def test_every_road_runs_the_features_once(monkeypatch):
    torch.manual_seed(0)
    z = models.zinc_gnnml3()
    feats, fused = _stubbed(z, monkeypatch)
    step = lambda data, **kw: _one_step(models.zinc_step_loss, z, data, feats, fused, **kw)
    assert step(_batch(64)) == ([True], [('l1_small', (64, 32))], {'head: fused L1 head, one workgroup (32 -> 32 -> 1)': 1})
    assert step(_batch(64, pad=True)) == ([True], [('l1_small', (65, 32))], {'head: fused L1 head, one workgroup (32 -> 32 -> 1)': 1})
    assert step(_batch(257)) == ([False], [('l1_big', (257, 32))], {'head: fused L1 head, one pass + fold (32 -> 32 -> 1)': 1})
    # 256 labels on 257 rows, a batch object without num_graphs: the parent promised pad_grad_zero, found the small head refusing 257
    # rows and ran the layers again without the promise -- one call now, with what the second one was given
    assert step(_batch(256, pad=True, num_graphs=False)) == ([False], [('l1_big', (257, 32))], {'head: fused L1 head, one pass + fold (32 -> 32 -> 1)': 1})
    assert step(_batch(64), _head_road='torch') == ([False], [], {'head: torch ops (L1 head outside the fused kernels)': 1})
    monkeypatch.setenv('GML_NO_HEAD_BIG', '1')
    assert step(_batch(257)) == ([False], [], {'head: torch ops (L1 head outside the fused kernels)': 1})
    monkeypatch.delenv('GML_NO_HEAD_BIG')
    loss_sum = torch.zeros(())
    assert step(_batch(3, pad=True), _head_road='torch', loss_sum=loss_sum)[0] == [False] and float(loss_sum) > 0
    # the parent's redo branch on a model with dropout: small batch, 96 -> 32 'mlp32' head (head_l1_supported false: nin > 64).  One
    # features call, so the dropout counter advances by one per step
    f = models.freqclass_gnnml1().train()
    feats, fused = _stubbed(f, monkeypatch)
    assert Fn.head_road('l1', models._MLP32, True, 96, 32, 1, 3, 3, 3).kind == 'torch' and _parent('l1', True, 96, 32, 1, 3, 3, 3, True, True, False, False)[2]
    for i in range(3):
        assert int(f.dropout_state[1]) == i
        assert _one_step(models.zinc_step_loss, f, _batch(3), feats, fused) == ([False], [], {'head: torch ops (L1 head outside the fused kernels)': 1})
    # ... and under its own loss: features once with pad_grad_zero, the torch ops (96 inputs), stats accumulated
    stats = torch.zeros(3)
    for fn in (models.freqclass_step_loss, models.exp_classify_step_loss):
        assert _one_step(fn, f, _batch(3), feats, fused, stats=stats) == ([True], [], {'head: torch ops (BCE head outside the fused kernel)': 1})
    assert int(f.dropout_state[1]) == 5 and stats.tolist()[2] == 6.0
    # exp_classify: fused, by switch, by override, plain and padded
    e = models.exp_classify_gnnml3()
    feats, fused = _stubbed(e, monkeypatch)
    step = lambda data, **kw: _one_step(models.exp_classify_step_loss, e, data, feats, fused, **kw)
    for data in (_batch(3), _batch(3, pad=True)):
        assert step(data) == ([True], [('bce', (int(data.ptr.numel()) - 1, 48))], {})
        assert step(data, _head_road='torch') == ([True], [], {'head: torch ops (BCE head outside the fused kernel)': 1})
        monkeypatch.setenv('GML_NO_HEAD_BCE', '1')
        assert step(data, stats=torch.zeros(3)) == ([True], [], {'head: torch ops (BCE head outside the fused kernel)': 1})
        monkeypatch.delenv('GML_NO_HEAD_BCE')
    # a head its class does not list for BCE (GNNML3 'mlp32'): the model's own forward, once
    zf, zfused = _stubbed(z, monkeypatch)
    assert _one_step(models.exp_classify_step_loss, z, _batch(3, node_level=False), zf, zfused) == ([None], [], {"head: torch ops (BCE on the model's own head)": 1})
    # filtering: the node head on every node row
    n = models.filtering_gnnml3()
    feats, fused = _stubbed(n, monkeypatch)
    grid = _batch(1, nodes=16, node_level=True)
    assert _one_step(models.filtering_step_loss, n, grid, feats, fused, stats=torch.zeros(4)) == ([None], [('node', (16, 48))], {'head: fused node head (48 -> 1)': 1})
    st = torch.zeros(4)
    assert _one_step(models.filtering_step_loss, n, grid, feats, fused, stats=st, _head_road='torch') == ([None], [], {'head: torch ops (node head outside the fused kernel)': 1})
    assert st.tolist()[3] == 16.0
