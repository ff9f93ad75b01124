"""The road of one ML3Layer backward -- functional._ml3_bwd_road over functional._conv_bwd_road / _bwd_plan -- against a table written
from DESIGN.md s4.2 (the conv backward's kernel classes, the dz hand-over, the 48-wide layers), s4.4 (rounds 2, 3, 6: the pool
gradient per segment, the relu hand-over between stacked layers, the output stage inside the conv backward, the masked pool
gradient) and include/gml.h (gml_spectconv_bwd_mix_supported, gml_spectconv_bwd_had_parts), not from the dispatch code.  The road
functions touch no tensor and launch nothing: the library loads and answers its host queries on a CPU, the csr is a stub with the
group maxima of a small ZINC batch."""
import itertools
import os

import pytest
import torch

from gnn_matlang_amd import functional as Fn

# the library reads these once per process; each would change what a table row means
assert not [k for k in ('GML_BWD_DMA', 'GML_BWD_WIDE48', 'GML_BWD_HAD', 'GML_NO_DZ', 'GML_NO_POOL_FUSE', 'GML_F32_MFMA') if k in os.environ]

ALL = tuple(i < 12 for i in range(23))     # needs_input_grad of ML3LayerFunction: x, val, w1..w4, cw, cb, w11, b11, w12, b12, then non-tensors
X, VAL, CW, W11, W12 = 0, 1, 6, 8, 10


def without(*idx):
    return tuple(n and i not in idx for i, n in enumerate(ALL))


class StubCsr(object):
    def __init__(self, N=300):
        self.N, self.E = N, 6 * N
        self.gmax_t = self.gmax_t128 = (640, 140)
        self.ginfo_t = self.ginfo_t128 = None


def road(S, Fin, nout1, nout2, N=300, need=ALL, learnedge=True, has_cb=True, exact=False, had=True, dma=False, chain=True, pool=False,
         pool_mask=False, premasked=False, chain_in=None, gy=None, x4=True):
    conv = Fn._conv_bwd_road(StubCsr(N), S, Fin, nout1, exact, x4)
    return Fn._ml3_bwd_road(S, Fin, nout1, nout2, N, need, learnedge, has_cb, conv, exact, had, dma, chain, pool, pool_mask, premasked,
                            chain_in, gy if gy is not None else (nout1 + nout2, 0), x4)


# ZINC's layers (Zinc12k.py:338-341): 8 supports, 32 -> 30 + 2; a middle layer's gradient arrives pre-masked from the layer above and its
# own dx leaves with the relu of the layer below (30 columns) applied
ZINC = dict(S=8, Fin=32, nout1=30, nout2=2)
MID = dict(ZINC, premasked=True, chain_in=30)
TOP = dict(ZINC, pool=True, chain_in=30)

# expected: (pool_grad, stage, parts, want_dx, premasked, dz_out, mixk, lib_hadamard, use_dz, relu_cols, conv_accum, conv kind)
HAD3 = (None, 'had', 3, True, False, False, True, False, False, 30, False, 'one128')
TABLE = {
    # s4.4 round 6: pre-masked gradient, 30 + 2 -> the stage inside the conv backward; 300 rows = 3 groups of 128 = 3 partial rows
    'zinc middle layer': (MID, HAD3),
    # "the first layer (no dx wanted: HAD without DZ ...) takes the same road"; gml.h: without dx any count in 17 .. 32
    'zinc bottom layer': (dict(ZINC, Fin=20, premasked=True, need=without(X)),
                          (None, 'had', 3, False, False, False, True, False, False, 0, False, 'one128')),
    # gml.h: with dx, Fin % 4 == 0 (dz form and had form): the one-pass stage writes dx, the conv accumulates
    'Fin = 18 with dx': (dict(ZINC, Fin=18, premasked=True),
                         (None, 'one_pass', 0, True, True, False, True, False, False, 0, True, 'one128')),
    # s4.4 "The top layer too": the pool left the relu pattern -> masked pool gradient, then like the layers below
    'pooled top layer, pool mask': (dict(TOP, pool_mask=True), ('masked',) + HAD3[1:]),
    # s4.4 round 2: gy_seg, never expanded; the one-pass stage hands dz over; round 3: the relu of the layer below rides on the dz form
    'pooled top layer, no pool mask': (TOP, ('per_segment', 'one_pass', 0, True, False, True, True, False, True, 30, False, 'one128')),
    'pooled top layer, GML_NO_POOL_FUSE': (dict(TOP, pool_mask=True, env='GML_NO_POOL_FUSE'),
                                           ('expanded', 'one_pass', 0, True, False, True, True, False, True, 30, False, 'one128')),
    # GML_BWD_HAD=0: round 3's road -- pre-masked one-pass stage (y = G = NULL), dz, relu hand-over
    'BWD_HAD off': (dict(MID, had=False), (None, 'one_pass', 0, True, True, True, True, False, True, 30, False, 'one128')),
    # the LDS-DMA ring kernel has no had and no relu form (gml.h: none of the ring ... flags); it takes dz
    'BWD_DMA on': (dict(MID, dma=True), (None, 'one_pass', 0, True, True, True, True, False, True, 0, False, 'one128')),
    # s4.2 GML_NO_DZ=1: dx = dz [w11; w12] WRITTEN, the conv backward accumulates into it
    'GML_NO_DZ': (dict(MID, env='GML_NO_DZ'), (None, 'one_pass', 0, True, True, False, True, False, False, 0, True, 'one128')),
    # exact f32 products: the 64-row f32-MFMA kernel, which has no hand-over form
    'exact': (dict(MID, exact=True), (None, 'one_pass', 0, True, True, False, True, False, False, 0, True, 'one64')),
    # a gradient whose rows are not float4-readable is neither handed on as G nor read by the had form
    'gy row stride 33': (dict(MID, gy=(33, 0)), (None, 'one_pass', 0, True, False, True, True, False, True, 30, False, 'one128')),
    'gy pointer % 16 == 4': (dict(MID, gy=(32, 4)), (None, 'one_pass', 0, True, False, True, True, False, True, 30, False, 'one128')),
    # s4.2 round 5: 33 .. 48 features in ONE launch for S = 4, 6; 2 nout2 > 4: no dz
    'sr25 48-wide': (dict(S=6, Fin=48, nout1=32, nout2=16), (None, 'one_pass', 0, True, False, False, True, False, False, 0, True, 'one128')),
    'mutag 48-wide': (dict(S=4, Fin=48, nout1=24, nout2=24), (None, 'one_pass', 0, True, False, False, True, False, False, 0, True, 'one128')),
    # S = 8 has no 48-wide launch: two launches over [0, 32) and [32, 48) (Fout <= 16: the kernel with dval +=)
    'S = 8, 48 features, 16 columns': (dict(S=8, Fin=48, nout1=16, nout2=16),
                                       (None, 'one_pass', 0, True, False, False, True, False, False, 0, True, 'split48')),
    # ... which read x as float4 from column 32 on; no one-launch plan exists for the shape
    'the same, x rows misaligned': (dict(S=8, Fin=48, nout1=16, nout2=16, x4=False),
                                    (None, 'one_pass', 0, True, False, False, True, False, False, 0, True, 'unfused')),
    # counting.py: 12 supports, one 16-wide output block (the narrow plan); the dz form is S = 8 only
    'counting 16 + 16': (dict(S=12, Fin=32, nout1=16, nout2=16), (None, 'one_pass', 0, True, False, False, True, False, False, 0, True, 'one128')),
    'S = 5': (dict(S=5, Fin=32, nout1=30, nout2=2, premasked=True, chain_in=30),
              (None, 'one_pass', 0, True, True, False, True, False, False, 0, True, 'unfused')),
    # ptc.py: 11 supports, 64 + 16 = 80 inputs: the Hadamard branch as library GEMMs beside a one-pass relu / bias stage
    'ptc 80 inputs': (dict(S=11, Fin=80, nout1=64, nout2=16), (None, 'one_pass', 0, True, False, False, False, True, False, 0, False, 'unfused')),
    'nout2 = 0': (dict(S=8, Fin=32, nout1=32, nout2=0), (None, 'one_pass', 0, True, False, False, False, False, False, 0, False, 'one128')),
    'learnedge off': (dict(MID, learnedge=False, need=without(VAL)), HAD3),
}
FIELDS = ('pool_grad', 'stage', 'parts', 'want_dx', 'premasked', 'dz_out', 'mixk', 'lib_hadamard', 'use_dz', 'relu_cols', 'conv_accum')


def run_case(name, monkeypatch):
    kw = dict(TABLE[name][0])
    env = kw.pop('env', None)
    if env:
        monkeypatch.setenv(env, '1')
    return road(**kw)


@pytest.mark.parametrize('name', sorted(TABLE))
def test_road_table(name, monkeypatch):
    r = run_case(name, monkeypatch)
    assert tuple(getattr(r, f) for f in FIELDS) + (r.conv.kind,) == TABLE[name][1], r
    # every hand-over rides on the one-launch 128-row conv backward
    if r.use_dz or r.relu_cols or r.stage == 'had':
        assert r.conv.kind == 'one128' and r.conv.plan.rows == 128
    assert r.dz_out == r.use_dz and not (r.use_dz and r.conv_accum) and (r.parts > 0) == (r.stage == 'had')
    assert r.want_cw and r.want_cb and r.learnedge == TABLE[name][0].get('learnedge', True)


def test_need_val_follows_the_edge_branch():
    """the supports' gradient is wanted for themselves or for the edge branch's weights"""
    assert road(need=without(VAL), **MID).need_val and not road(need=without(VAL), learnedge=False, **MID).need_val
    assert road(need=without(2, 3, 4, 5), **MID).need_val and not road(need=without(VAL, 2, 3, 4, 5), **MID).need_val
    assert not road(has_cb=False, **MID).want_cb and not road(need=without(7), **MID).want_cb


@pytest.mark.parametrize('drop', [c for n in range(5) for c in itertools.combinations((X, CW, W11, W12), n)])
def test_zinc_middle_layer_over_every_subset_of_wanted_gradients(drop):
    """gml_spectconv_bwd_had writes dW, dw11 and dw12 unconditionally: the road is taken only when all three are wanted"""
    r = road(need=without(*drop), **MID)
    assert r.stage in ('had', 'one_pass', 'separate')
    assert (r.stage == 'had') == (not set(drop) & {CW, W11, W12})
    assert r.want_dx == (X not in drop) and r.want_cw == (CW not in drop)
    assert r.relu_cols == (30 if r.want_dx else 0)            # (without had: the dz form carries it, and dz exists only with dx)
    if r.use_dz or r.relu_cols or r.stage == 'had':
        assert r.conv.kind == 'one128'


def test_chain_switch_turns_both_hand_overs_off():
    r = road(chain=False, **MID)
    assert (r.stage, r.premasked, r.relu_cols, r.use_dz) == ('one_pass', False, 0, True)


def test_forward_and_backward_share_the_pool_mask_predicate(monkeypatch):
    """the forward pools with the relu pattern and the backward takes the masked road by the SAME function: both resolve the module's
    _pool_relu_pattern, the backward's answer implies the forward's on every pooled row of the table, and replacing the function
    moves the backward"""
    assert '_pool_relu_pattern' in Fn._ml3_fwd_road.__code__.co_names       # (the forward's road: ML3LayerFunction.forward reads its .pool)
    assert '_pool_relu_pattern' in Fn._ml3_bwd_road.__code__.co_names
    for name, (kw, _) in TABLE.items():
        if kw.get('pool'):
            with monkeypatch.context() as mp:
                r = run_case(name, mp)
            fwd = Fn._pool_relu_pattern(kw.get('had', True), r.mixk, kw['nout1'], kw['nout2'], kw.get('exact', False), any(kw.get('need', ALL)))
            assert fwd or r.pool_grad != 'masked', name
    assert Fn._pool_relu_pattern(True, True, 30, 2, False, True) and not Fn._pool_relu_pattern(True, True, 30, 2, False, False)
    assert not [a for a in [(False, True, 30, 2, False), (True, False, 30, 2, False), (True, True, 32, 2, False), (True, True, 30, 1, False),
                            (True, True, 30, 2, True)] if Fn._pool_relu_pattern(*a, True)]
    monkeypatch.setattr(Fn, '_pool_relu_pattern', lambda *a: False)
    assert road(pool_mask=True, **TOP).pool_grad == 'per_segment'


# ---- the conv road ---------------------------------------------------------------------------------------------------------------------
def test_bwd_plan_is_a_named_record():
    p = Fn._bwd_plan(StubCsr(), 8, 32, 30, False)
    assert p._fields == ('flags', 'ginfo', 'max_edges', 'max_window', 'ws_bytes', 'rows')
    assert (p.flags, p.max_edges, p.max_window, p.ws_bytes, p.rows) == (0, 640, 140, 3 * 8 * 32 * 30 * 4, 128)
    e = Fn._bwd_plan(StubCsr(), 8, 32, 30, True)
    assert (e.flags, e.rows, e.ws_bytes) == (Fn._lib.GML_F32_MFMA, 64, 5 * 8 * 32 * 30 * 4)
    with Fn.exact_products():                                  # (exact=None: as the thread runs)
        assert Fn._bwd_plan(StubCsr(), 8, 32, 30) == e
    assert Fn._bwd_plan(StubCsr(), 5, 32, 30) is None and Fn._bwd_plan(StubCsr(), 8, 48, 16) is None


@pytest.mark.parametrize('shape, kw, kind', [
    ((8, 32, 30), {}, 'one128'), ((8, 32, 30), {'exact': True}, 'one64'), ((8, 32, 30), {'wants_handover': True}, 'one128'),
    ((6, 48, 32), {}, 'one128'), ((4, 48, 24), {}, 'one128'), ((4, 64, 32), {}, 'one64'), ((12, 32, 16), {}, 'one128'),
    ((8, 48, 16), {}, 'split48'), ((8, 40, 16), {}, 'split48'), ((12, 48, 16), {}, 'split48'),
    ((8, 48, 16), {'x_rows4': False}, 'unfused'), ((8, 48, 16), {'wants_handover': True}, 'unfused'), ((8, 48, 16), {'exact': True}, 'unfused'),
    ((8, 46, 16), {}, 'unfused'),                              # (Fin - 32) % 4: the second slice's x rows would not be float4-readable
    ((8, 48, 32), {}, 'unfused'),                              # S = 8, 32 columns: no dval += in that kernel
    ((5, 32, 30), {}, 'unfused'), ((4, 48, 24), {'exact': True}, 'one64'),
])
def test_conv_road_table(shape, kw, kind):
    """DESIGN s4.2 / s4.2a: the 8-wave kernel's classes (128 rows), the f32-MFMA kernel's (64), the two feature slices of a 48-wide
    layer the 8-wave kernel has no launch for, the composition"""
    kw = dict(kw)
    r = Fn._conv_bwd_road(StubCsr(), *shape, kw.pop('exact', False), **kw)
    assert r.kind == kind, r
    assert (r.plan is not None) == kind.startswith('one') and (r.halves is not None) == (kind == 'split48')
    if kind == 'split48':
        assert [p.rows for p in r.halves] == [128, 128] and not (r.halves[0].flags | r.halves[1].flags)
    if kind.startswith('one'):
        assert r.plan.rows == int(kind[3:])


def test_a_hand_over_on_another_road_raises():
    """mix / relu_cols / had off the one-launch 128-row road: an error, not silently dropped (before any tensor is touched)"""
    csr = StubCsr()
    x, val, G = torch.zeros(300, 48), torch.zeros(1800, 8), torch.zeros(300, 16)
    for kw in ({'relu_cols': 30}, {'mix': (None, None)}, {'had': {}}):
        for S, fin in ((8, 48), (5, 32)):
            with pytest.raises(AssertionError, match='hand-overs ride on the one-launch 128-row'):
                Fn._conv_backward(csr, x[:, :fin], val[:, :S], torch.zeros(S, fin, 16), G, True, True, True, **kw)
    exact = Fn._conv_bwd_road(csr, 8, 32, 30, True)
    with pytest.raises(AssertionError, match='hand-overs ride on the one-launch 128-row'):
        Fn.fused_conv_bwd(csr, exact.plan, val, x[:, :32], torch.zeros(300, 32)[:, :30], torch.zeros(8, 32, 30), True, True, True, relu_cols=30)
