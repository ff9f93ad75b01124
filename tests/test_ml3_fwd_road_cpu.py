"""The road of one ML3Layer forward -- functional._ml3_fwd_road over functional._conv_fwd_road and functional._edge_fwd_family -- against
a table written from DESIGN.md s4.1 / s4.1b / s4.1c (the conv forward's kernel classes, a work item's 1,024 edges, the chunked ring and
its one-window form), s4.3 / s4.3a (the edge branch in source order, the stack, the unique rows, the plan's rules), s4.4 (the pool that
leaves the relu pattern, the hand-over tokens) and include/gml.h, not from the dispatch code.  The road functions touch no tensor and
launch nothing: the library loads and answers its host queries on a CPU, the csr is a stub with the group maxima of a small ZINC batch."""
import os

import pytest

from gnn_matlang_amd import functional as Fn
from gnn_matlang_amd import _lib

# the library reads these once per process; each would change what a table row means
assert not [k for k in ('GML_EDGE_VALU', 'GML_BWD_DMA', 'GML_BWD_WIDE48', 'GML_F32_MFMA') if k in os.environ]

G128, CHUNKED, ONEWIN = _lib.GML_GROUPS128, _lib.GML_FWD_CHUNKED, _lib.GML_FWD_ONEWIN
TWO, THREE, EXACT = _lib.GML_EDGE_TWO_PIECE, _lib.GML_EDGE_THREE_PIECE, _lib.GML_EDGE_EXACT
WAVE8 = (128, G128, 'fused 8-wave bf16x3')
WAVE4, WAVE4_F32 = (64, 0, 'fused 4-wave (bf16x3)'), (64, 0, 'fused 4-wave (f32 MFMA)')


class StubCsr(object):
    def __init__(self, N=300, gmax=(640, 140), src_sorted=True):
        self.N, self.E = N, 6 * N
        self.gmax128, self.src_sorted = gmax, src_sorted
        self.gmax_t = self.gmax_t128 = (640, 140)
        self.ginfo_t = self.ginfo_t128 = None


def road(Se=8, S=None, Fin=32, nout1=30, nout2=2, learnedge=True, grad=True, wanted=None, plain=True, width=True, sup_grad=False,
         src_sorted=True, stash=False, succ=0, pooled=False, exact=False, fwd6=True, chain_in=None, stack=True, sym=True, chain=True,
         had=True, wide_lib=False, **conv_kw):
    S = Se if S is None else S
    csr = StubCsr(src_sorted=src_sorted)
    conv = conv_road(S, Fin, nout1, exact=exact, **conv_kw)
    bwd = bool(learnedge and grad and max(Se, S) <= 16 and Fn._bwd_plan(csr, S, Fin, nout1, exact) is not None)
    return Fn._ml3_fwd_road(Se, S, Fin, nout1, nout2, csr.E, learnedge, grad, grad if wanted is None else wanted,
                            (plain, width, sup_grad, csr.src_sorted), stash, succ, pooled, exact, EXACT if exact else THREE if fwd6 else TWO,
                            bwd, conv, chain_in, stack, sym, chain, had, wide_lib)


def conv_road(S, Fin, Fout, exact=False, gmax=(640, 140), N=300, stride=None, ptr16=0, chunks=True):
    return Fn._conv_fwd_road(S, Fin, Fout, exact, gmax, N, (Fin + 3) // 4 * 4 if stride is None else stride, ptr16, chunks)


def family(r, Se, S, exact=False, fwd6=True, E=1800, pairs=False):
    # (pairs: the batch's answer where the road asks; where it does not ask there are none)
    f = Fn._edge_fwd_family(Se, S, r.layers, EXACT if exact else THREE if fwd6 else TWO, Se <= 16 and E > 0, r.order == 'dual',
                            pairs and r.pairs is not None)
    return f.family, f.arith, f.entry


# ZINC's layers (Zinc12k.py:338-341): 8 supports, 32 -> 30 + 2, source-sorted raw supports without gradient
SYM6, CHAIN6 = _lib.GML_EDGE_FAM_SYM6, _lib.GML_EDGE_FAM_CHAIN6
FAM_STACK = ((SYM6, THREE, 'gml_edge_mlp_fwd_stack6_sym'), (CHAIN6, THREE, 'gml_edge_mlp_fwd_stack6'))
FAM_ONE = ((SYM6, THREE, 'gml_edge_mlp_fwd_stack6_sym'), (CHAIN6, THREE, 'gml_edge_mlp_fwd6'))
PLAIN6 = ((CHAIN6, THREE, 'gml_edge_mlp_fwd6'),) * 2
NONE = ((0, TWO, None),) * 2

# name: (inputs, (edge, order, layers, pairs, hadamard, pool, chain_in, chain_out), conv (rows, flags, label),
#        (family, arithmetic, entry) where the batch has pairs / where it has none; None: no edge launch inside the layer)
TABLE = {
    # s4.3: the branch in source order on the supports as given, the stacked layers' branches in the same pass, over the unique rows
    'zinc bottom layer, three stackable successors': (dict(succ=3), ('branch', 'source_raw', 4, 'source', 'fused', None, False, True), WAVE8, FAM_STACK),
    'the same on a stash hit': (dict(succ=3, stash=True, chain_in=30), ('branch', 'source_raw', 0, None, 'fused', None, True, True), WAVE8, None),
    'EDGE_STACK off': (dict(succ=3, stack=False), ('branch', 'source_raw', 1, 'source', 'fused', None, False, True), WAVE8, FAM_ONE),
    'EDGE_SYM off': (dict(succ=3, sym=False), ('branch', 'source_raw', 4, None, 'fused', None, False, True), WAVE8, FAM_STACK[1:] * 2),
    'two-piece forward (EDGE_FWD6 off)': (dict(succ=3, fwd6=False), ('branch', 'source_raw', 4, 'source', 'fused', None, False, True), WAVE8,
                                          ((_lib.GML_EDGE_FAM_CHAIN, TWO, 'gml_edge_mlp_fwd_stack'),) * 2),
    # trained supports change every step: sorted (differentiably), gathered into source order, nothing cached, shared or stacked
    'supports that carry a gradient': (dict(succ=3, sup_grad=True), ('branch', 'source', 1, None, 'fused', None, False, True), WAVE8, PLAIN6),
    # inference: target order, unique rows in the target view
    'grad disabled': (dict(succ=3, grad=False), ('branch', 'target', 1, 'target', 'fused', None, False, True), WAVE8, FAM_ONE),
    'unsorted sources': (dict(succ=3, src_sorted=False), ('branch', 'source', 1, 'source', 'fused', None, False, True), WAVE8, FAM_ONE),
    'supports of another dtype / strided': (dict(succ=3, plain=False), ('branch', 'source', 1, 'source', 'fused', None, False, True), WAVE8, FAM_ONE),
    # exact products: the 64-row f32-MFMA forward does not gather -> both orders from the edge kernel (exact entry), no stacked kernel
    'exact': (dict(succ=3, exact=True), ('branch', 'dual', 1, None, 'fused', None, False, True), WAVE4_F32,
              ((_lib.GML_EDGE_FAM_VALU, EXACT, 'gml_edge_mlp_fwd_exact'),) * 2),
    # s4.3a: S = 1 has no three-piece form -> the default entry's VALU kernel (no fused conv backward at S = 1: target order)
    'S = 1': (dict(Se=1, grad=False), ('branch', 'target', 1, 'target', 'fused', None, False, True), WAVE4,
              ((_lib.GML_EDGE_FAM_VALU, TWO, 'gml_edge_mlp_fwd'),) * 2),
    # counting.py: 12 supports, 16 + 16 (fwd2, the narrow backward plan): no stack beyond S in {4, 8}; chain16x6 / its unique-row form
    'S = 12': (dict(Se=12, nout1=16, nout2=16, succ=2), ('branch', 'source_raw', 1, 'source', 'fused', None, False, True), WAVE8,
               ((_lib.GML_EDGE_FAM_SYM16X6, THREE, 'gml_edge_mlp_fwd_stack6_sym'), (_lib.GML_EDGE_FAM_CHAIN16X6, THREE, 'gml_edge_mlp_fwd6'))),
    # nedgeoutput != nedgeinput: never the raw supports, no pairs; the plan has no family, edge_mlp_fwd pads to a square branch
    'So != S (8 -> 6, sr25 48-wide)': (dict(Se=8, S=6, Fin=48, nout1=32, nout2=16, succ=3, gmax=(400, 140)), ('branch', 'source', 1, None, 'fused', None, False, True),
                                      WAVE8, NONE),
    '17 supports': (dict(Se=17), ('wide', None, 0, None, 'fused', None, False, False), WAVE4, None),
    '48 supports': (dict(Se=48), ('wide', None, 0, None, 'fused', None, False, False), WAVE4, None),
    '49 supports': (dict(Se=49), ('library', None, 0, None, 'fused', None, False, False), WAVE4, None),
    '20 supports, 24 columns given': (dict(Se=20, width=False), ('library', None, 0, None, 'fused', None, False, False), WAVE4, None),
    'GML_EDGE_WIDE_LIB': (dict(Se=20, wide_lib=True), ('library', None, 0, None, 'fused', None, False, False), WAVE4, None),
    'nout2 = 0': (dict(nout1=32, nout2=0), ('branch', 'source_raw', 1, 'source', None, None, False, True), WAVE8, FAM_ONE),
    # ptc.py: 11 supports, 64 + 16 = 80 inputs: Hadamard branch as library GEMMs; no fused backward -> target order even in training
    'Fin = 80': (dict(Se=11, Fin=80, nout1=64, nout2=16), ('branch', 'target', 1, 'target', 'library', None, False, True), WAVE4_F32,
                 ((_lib.GML_EDGE_FAM_SYM16X6, THREE, 'gml_edge_mlp_fwd_stack6_sym'), (_lib.GML_EDGE_FAM_CHAIN16X6, THREE, 'gml_edge_mlp_fwd6'))),
    'nout2 = 32': (dict(nout1=32, nout2=32), ('branch', 'source_raw', 1, 'source', 'library', None, False, True), WAVE8, FAM_ONE),
    # s4.4 "The top layer too": the pool leaves the relu pattern when a gradient will come back; a pooled output has no consumer token
    'pooled 30 + 2, gradient wanted': (dict(pooled=True, chain_in=30), ('branch', 'source_raw', 1, 'source', 'fused', 'pattern', True, False), WAVE8, FAM_ONE),
    'pooled 30 + 2, no gradient wanted': (dict(pooled=True, grad=False), ('branch', 'target', 1, 'target', 'fused', 'plain', False, False), WAVE8, FAM_ONE),
    'pooled 30 + 2, BWD_HAD off': (dict(pooled=True, had=False), ('branch', 'source_raw', 1, 'source', 'fused', 'plain', False, False), WAVE8, FAM_ONE),
    'pooled 32 + 0': (dict(pooled=True, nout1=32, nout2=0), ('branch', 'source_raw', 1, 'source', None, 'plain', False, False), WAVE8, FAM_ONE),
    'CHAIN off': (dict(chain=False, chain_in=30), ('branch', 'source_raw', 1, 'source', 'fused', None, False, False), WAVE8, FAM_ONE),
    'a token of a wider layer below': (dict(chain_in=64), ('branch', 'source_raw', 1, 'source', 'fused', None, False, True), WAVE8, FAM_ONE),
    'learnedge off': (dict(learnedge=False, chain_in=30), (None, None, 0, None, 'fused', None, True, True), WAVE8, None),
    # s4.1c: sr25's 13 entries per row = 1,664 edges in a 128-row group, windows of 176 rows: edge chunks, ONE X window at 48 features
    'sr25 48-wide': (dict(Se=6, Fin=48, nout1=32, nout2=16, gmax=(1664, 176)), ('branch', 'source_raw', 1, 'source', 'fused', None, False, True),
                     (128, G128 | ONEWIN, 'fused 8-wave bf16x3, edge chunks, one X window'), FAM_ONE),
}


@pytest.mark.parametrize('name', sorted(TABLE))
def test_road_table(name):
    kw, want, conv, fams = TABLE[name]
    r = road(**kw)
    assert tuple(r[:8]) == want and tuple(r.conv[:3]) == conv, r
    # source order exists for the fused backward's sake and rides on the gathering forward; raw supports, a stack and a stash hit on it alone
    assert r.conv.gathers or r.order not in ('source_raw', 'source')
    assert r.order == 'source_raw' or r.layers == (1 if r.edge == 'branch' else 0)
    assert not (r.pairs and (r.layers == 0 or r.order == 'dual' or kw.get('sup_grad')))
    fkw = {k: v for k, v in kw.items() if k in ('exact', 'fwd6')}
    Se = kw.get('Se', 8)
    if fams is None:
        assert r.layers == 0
    else:
        assert (family(r, Se, kw.get('S', Se), pairs=True, **fkw), family(r, Se, kw.get('S', Se), pairs=False, **fkw)) == fams
        if r.layers > 1:                                       # the road asked the plan: a stack it names has a kernel either way
            assert all('stack' in f[2] for f in fams)


def test_a_stack_needs_a_stacked_kernel():
    """s4.3a: stacks at S in {4, 8}, 2 .. 4 layers; the two-piece one on the pre-split rows (an empty batch has none); exact: none"""
    assert [road(Se=S, succ=1).layers for S in (2, 4, 5, 8, 12, 16)] == [1, 2, 1, 2, 1, 1]
    assert [road(succ=n).layers for n in (0, 1, 2, 3)] == [1, 2, 3, 4]
    assert Fn._edge_fwd_family(8, 8, 4, EXACT, True, False, False).entry is None
    assert Fn._edge_fwd_family(8, 8, 4, TWO, False, False, False).entry is None
    assert Fn._edge_fwd_family(8, 8, 5, THREE, True, False, True).entry is None


@pytest.mark.parametrize('args, want', [
    # (S, So, L, arithmetic, has pre-split, dual, pairs)
    ((8, 8, 1, THREE, True, True, False), (CHAIN6, THREE, 'gml_edge_mlp_fwd6')),
    ((8, 8, 1, TWO, True, False, True), (_lib.GML_EDGE_FAM_CHAIN, TWO, 'gml_edge_mlp_fwd')),        # unique rows: three-piece only
    ((12, 12, 1, TWO, True, False, False), (_lib.GML_EDGE_FAM_CHAIN16, TWO, 'gml_edge_mlp_fwd')),
    ((12, 12, 1, TWO, False, False, False), (_lib.GML_EDGE_FAM_VALU, TWO, 'gml_edge_mlp_fwd')),     # chain16 needs the pre-split rows
    ((5, 5, 1, THREE, False, False, True), (SYM6, THREE, 'gml_edge_mlp_fwd_stack6_sym')),           # single layers: 2 .. 16
    ((5, 5, 2, THREE, False, False, True), (0, THREE, None)),
    ((1, 1, 1, EXACT, False, False, False), (_lib.GML_EDGE_FAM_VALU, EXACT, 'gml_edge_mlp_fwd_exact')),
    ((1, 1, 1, THREE, False, True, False), (_lib.GML_EDGE_FAM_VALU, TWO, 'gml_edge_mlp_fwd')),      # the one three-piece -> two-piece retry
    ((17, 17, 1, THREE, False, False, False), (0, TWO, None)),
    ((8, 6, 1, THREE, True, False, False), (0, TWO, None)),
])
def test_edge_family_table(args, want):
    assert tuple(Fn._edge_fwd_family(*args)) == want


# ---- the conv forward ------------------------------------------------------------------------------------------------------------------
BIG = 1 << 24        # (N + 16) * 32 floats * 4 bytes >= 2^31


@pytest.mark.parametrize('shape, kw, want, gathers', [
    ((8, 32, 30), {}, WAVE8, True),
    # s4.1: a group beyond one work item of the ring kernel (960 edges / 200 window rows at S = 8): its chunked form
    ((8, 32, 30), {'gmax': (1700, 150)}, (128, G128 | CHUNKED, 'fused 8-wave bf16x3, edge chunks'), True),
    ((8, 32, 30), {'gmax': (1700, 150), 'chunks': False}, WAVE8, True),          # (fwd2's global-gather road, same records)
    ((8, 32, 30), {'gmax': None}, WAVE8, True),
    ((8, 32, 30), {'gmax': (1700, 150), 'stride': 33}, WAVE8, True),
    ((8, 32, 30), {'gmax': (1700, 150), 'ptr16': 4}, WAVE8, True),
    ((8, 32, 30), {'gmax': (1700, 150), 'N': BIG}, WAVE8, True),
    ((8, 32, 30), {'gmax': (1700, 100000)}, WAVE8, True),
    ((12, 32, 16), {'gmax': (5000, 150)}, WAVE8, True),                          # fwd2: register-staged, no chunks
    # s4.1c: the chunked ring kernel alone serves these shapes on 128-row records
    ((6, 48, 32), {'gmax': (1664, 176)}, (128, G128 | ONEWIN, 'fused 8-wave bf16x3, edge chunks, one X window'), True),
    ((6, 32, 32), {'gmax': (1664, 176)}, (128, G128, 'fused 8-wave bf16x3, edge chunks'), True),
    # (at 48 features two X windows leave a work item 512 edges)
    ((6, 48, 32), {'gmax': (400, 140)}, WAVE8, True),
    ((4, 48, 24), {'gmax': (400, 140)}, WAVE8, True),
    ((6, 48, 32), {'gmax': (1664, 176), 'chunks': False}, WAVE4, True),
    ((6, 48, 32), {'gmax': (400, 140), 'chunks': False}, WAVE8, True),
    ((6, 48, 32), {'gmax': None}, WAVE4, True),
    ((6, 48, 32), {'stride': 49}, WAVE4, True),
    ((6, 48, 32), {'ptr16': 8}, WAVE4, True),
    ((6, 48, 32), {'N': BIG}, WAVE4, True),
    ((6, 48, 32), {'gmax': (1664, 328)}, WAVE4, True),                           # a window it cannot stage
    # shapes the library only serves on 64-row records
    ((5, 32, 30), {}, WAVE4, False), ((8, 64, 32), {}, WAVE4, False), ((8, 32, 64), {}, WAVE4_F32, False), ((8, 16, 30), {'exact': True}, WAVE4_F32, False),
    ((11, 80, 64), {}, WAVE4_F32, False), ((8, 32, 30), {'exact': True}, WAVE4_F32, False), ((6, 48, 32), {'exact': True}, WAVE4_F32, False),
])
def test_conv_fwd_road_table(shape, kw, want, gathers):
    r = conv_road(*shape, **kw)
    assert tuple(r[:3]) == want and r.gathers == gathers, r
    assert (r.rows == 128) == bool(r.flags & G128) and (r.gathers or r.rows == 64)


def test_the_thin_readers_agree_with_the_road():
    """fwd_groups reads tensor properties over the road; fwd_gathers and ml3_edge_in_source_order are its shape-only answers"""
    class X(object):
        def __init__(self, stride, ptr):
            self.s, self.p = stride, ptr

        def stride(self, d):
            return self.s

        def data_ptr(self):
            return self.p
    csr = StubCsr(gmax=(1664, 176))
    csr.ginfo128, csr.ginfo = 'g128', 'g64'
    assert Fn.fwd_groups(csr, X(48, 4096), 6, 48, 32) == ('g128', G128 | ONEWIN)
    assert Fn.fwd_groups(csr, X(48, 4100), 6, 48, 32) == ('g64', 0)
    assert Fn.fwd_groups(csr, X(32, 4096), 8, 32, 30) == ('g128', G128 | CHUNKED)
    assert Fn.fwd_gathers(6, 48, 32) and Fn.fwd_gathers(8, 32, 30) and not Fn.fwd_gathers(5, 32, 30)
    assert Fn.ml3_edge_in_source_order(csr, 8, 32, 30) and not Fn.ml3_edge_in_source_order(csr, 5, 32, 30)
    with Fn.exact_products():
        assert not Fn.fwd_gathers(8, 32, 30) and Fn.fwd_groups(csr, X(32, 4096), 8, 32, 30) == ('g64', 0)
