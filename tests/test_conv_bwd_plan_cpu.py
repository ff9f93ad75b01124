"""The host-only queries of the fused conv backward -- gml_spectconv_bwd_group_rows / _workspace_bytes / _mix_supported / _had_parts and
the two staging queries _stage_edges / _stage_window -- against a table written from include/gml.h and DESIGN.md s4.2 / s4.2a, not
from the dispatch code.  functional._bwd_plan, _conv_bwd_road, conv_bwd_takes_dz and _ml3_bwd_road choose group records, flags and
fallbacks from these answers (their own table: tests/test_ml3_bwd_road_cpu.py), so a change of the plan that moves one shows up here,
without a GPU: the library loads and answers on the host."""
import itertools
import os

import pytest

from gnn_matlang_amd import _lib

# the library reads these once per process; each would change what a table row means
assert not [k for k in ('GML_BWD_DMA', 'GML_BWD_WIDE48', 'GML_BWD_HAD') if k in os.environ]

F32, RING, ACC, DACC, NOFOLD = _lib.GML_F32_MFMA, _lib.GML_DMA_RING, _lib.GML_ACCUM, _lib.GML_DVAL_ACCUM, _lib.GML_NO_FOLD
SS = [2, 4, 6, 8, 12, 3, 5, 16]                            # the compiled support counts, and three outside
FINS = [1, 16, 17, 32, 33, 48, 49, 64, 65]
FOUTS = [1, 16, 17, 32, 33]
GRID = list(itertools.product(SS, FINS, FOUTS))
NUM_CU = 256                                               # MI355X
# the 64-row f32-MFMA kernel's compiled (S, ceil(Fin / 16), ceil(Fout / 16)) (DESIGN s4.2a)
F32_SHAPES = {(8, 2, 2), (8, 1, 2), (4, 2, 2), (4, 1, 2), (12, 2, 1), (12, 1, 1), (6, 3, 2), (6, 1, 2), (4, 3, 2), (6, 2, 2), (8, 2, 1), (4, 4, 2)}


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def main_shape(S, fin, fout):
    """DESIGN s4.2: S in {2, 4, 6, 8}, Fin <= 32, 16 < Fout <= 32"""
    return S in (2, 4, 6, 8) and fin <= 32 and 16 < fout <= 32


def narrow_shape(S, fin, fout):
    """one 16-wide output block: 12 supports (counting.py) and 8 supports with Fout <= 16"""
    return S in (8, 12) and fin <= 32 and fout <= 16


def wide_shape(S, fin, fout):
    """33 .. 48 input features in one launch: S in {4, 6}"""
    return S in (4, 6) and 32 < fin <= 48 and 16 < fout <= 32


def rows(S, fin, fout, flags):
    if not (flags & F32) and (main_shape(S, fin, fout) or narrow_shape(S, fin, fout) or wide_shape(S, fin, fout)):
        return 128
    return 64 if (S, (fin + 15) // 16, (fout + 15) // 16) in F32_SHAPES else 0


def grid_of(n, r):
    """persistent workgroups over ceil(n / r) groups: one per CU (128-row kernel) or two (64-row), each the same number of groups"""
    ng = -(-n // r)
    per = -(-ng // min(ng, NUM_CU * (1 if r == 128 else 2)))
    return -(-ng // per)


def ring_applies(S, fin, fout, flags):
    """gml.h, GML_DMA_RING: "where it applies" -- the 8-wave kernel's shapes with S in {4, 8} and Fin <= 32, dx from zero or dz"""
    return bool(flags & RING) and rows(S, fin, fout, flags) == 128 and S in (4, 8) and fin <= 32 and not flags & (ACC | DACC)


def L():
    return _lib.lib()


# ---- group rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flags', [0, F32])
def test_group_rows_table(flags):
    for S, fin, fout in GRID:
        assert int(L().gml_spectconv_bwd_group_rows(S, fin, fout, flags)) == rows(S, fin, fout, flags), (S, fin, fout, flags)
    for bad in [(0, 32, 32), (8, 0, 32), (8, 32, 0), (-1, 32, 32)]:
        assert int(L().gml_spectconv_bwd_group_rows(*bad, flags)) == 0


def test_group_rows_class_edges():
    """the edges every caller's fallback sits on, written out"""
    g = lambda S, fin, fout, fl=0: int(L().gml_spectconv_bwd_group_rows(S, fin, fout, fl))
    assert [g(8, 32, fo) for fo in (16, 17, 32, 33)] == [128, 128, 128, 0]
    assert [g(12, 32, fo) for fo in (16, 17, 32, 33)] == [128, 0, 0, 0]
    assert [g(8, fi, 32) for fi in (32, 33, 48, 49, 64, 65)] == [128, 0, 0, 0, 0, 0]
    assert [g(6, fi, 32) for fi in (32, 33, 48, 49, 64, 65)] == [128, 128, 128, 0, 0, 0]
    assert [g(4, fi, 32) for fi in (32, 33, 48, 49, 64, 65)] == [128, 128, 128, 64, 64, 0]
    assert [g(4, fi, 32, F32) for fi in (32, 33, 48, 49, 64, 65)] == [64, 64, 64, 64, 64, 0]
    assert [g(2, 32, 32, fl) for fl in (0, F32)] == [128, 0] and g(5, 32, 32) == 0 and g(5, 32, 32, F32) == 0


def test_group_rows_ignore_the_flags_that_choose_no_kernel_family():
    for S, fin, fout in GRID:
        for base in (0, F32):
            want = rows(S, fin, fout, base)
            for f in (RING, ACC, DACC, NOFOLD, RING | ACC | DACC | NOFOLD):
                assert int(L().gml_spectconv_bwd_group_rows(S, fin, fout, base | f)) == want, (S, fin, fout, base, f)


# ---- workspace -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flags', [0, F32])
@pytest.mark.parametrize('n', [1, 64, 65, 300, 128 * 255 + 1, 128 * 1000, 128 * 1000 + 1])
def test_workspace_bytes_is_one_partial_per_workgroup(flags, n):
    """non-zero exactly where group_rows is, for a batch of small groups; then grid S Fin Fout 4"""
    for S, fin, fout in GRID:
        r = rows(S, fin, fout, flags)
        got = int(L().gml_spectconv_bwd_workspace_bytes(n, S, fin, fout, 640, 140, flags))
        assert got == (grid_of(n, r) * S * fin * fout * 4 if r else 0), (n, S, fin, fout, flags, got)
    assert int(L().gml_spectconv_bwd_workspace_bytes(0, 8, 32, 32, 640, 140, flags)) == 0


def test_workspace_bytes_zero_past_the_lds_limit():
    """s4.2a: the 8-wave kernel at S = 8, 32 x 32 keeps 115,744 bytes of images, record and wmix rows and adds 4 bytes per staged
    edge and 144 per window row, both rounded up to 16 (at least 64): 160 KB = 163,840 ends at 9,712 edges beside a 64-row window"""
    ws = lambda e, w, S=8, fl=0: int(L().gml_spectconv_bwd_workspace_bytes(300, S, 32, 32, e, w, fl))
    assert 115744 + 9712 * 4 + 64 * 144 <= 160 * 1024 < 115744 + 9728 * 4 + 64 * 144
    assert ws(9712, 64) == 3 * 8 * 32 * 32 * 4 and ws(9713, 64) == 0
    assert ws(1088, 304) == 0 and ws(1072, 304) > 0           # 300-row windows: 1,080 edges
    for S, fin, fout in GRID:                                   # a group no kernel holds: every shape refuses, whatever its family
        for fl in (0, F32):
            assert int(L().gml_spectconv_bwd_workspace_bytes(300, S, fin, fout, 200000, 300, fl)) == 0
            assert int(L().gml_spectconv_bwd_group_rows(S, fin, fout, fl)) == rows(S, fin, fout, fl)
    # what the 128-row kernel refuses the 64-row kernel may still take, with ITS records' maxima (half the rows, about half the edges)
    assert ws(6200, 190, 4) == 0 and ws(3100, 130, 4, F32) == 5 * 4 * 32 * 32 * 4


# ---- DZ / HAD ------------------------------------------------------------------------------------------------------------------------
def test_mix_supported_table():
    """gml.h: "the 8-wave bf16x3 kernel, S = 8, 16 < Fin <= 32", dx float4-addressable (Fin % 4 == 0), nmix <= 4"""
    for S, fin, fout in GRID + [(8, f, 30) for f in (18, 20, 24, 28, 30)]:
        for flags in (0, F32):
            for nmix in (0, 1, 2, 3, 4, 5):
                want = 1 <= nmix <= 4 and S == 8 and 16 < fin <= 32 and fin % 4 == 0 and main_shape(S, fin, fout) and not flags
                assert bool(L().gml_spectconv_bwd_mix_supported(S, fin, fout, nmix, flags)) == want, (S, fin, fout, nmix, flags)


def test_had_parts_table():
    """gml.h: S = 8, Fout = 30, F2 = 2; with dx 17 .. 32 features in multiples of 4, without dx any count in 17 .. 32; none of the ring,
    accumulate and exact-arithmetic flags; the answer is the number of workgroups"""
    parts = lambda n, S, fin, fout, F2, dx, fl=0, e=640, w=140: int(L().gml_spectconv_bwd_had_parts(n, S, fin, fout, F2, dx, e, w, fl))
    for fin in range(12, 36):
        for dx in (0, 1):
            want = 17 <= fin <= 32 and (fin % 4 == 0 or not dx)
            assert parts(300, 8, fin, 30, 2, dx) == (3 if want else 0), (fin, dx)
    assert parts(128 * 1000, 8, 32, 30, 2, 1) == 250 and parts(1, 8, 20, 30, 2, 0) == 1 and parts(0, 8, 32, 30, 2, 1) == 0
    for S, fout, F2 in [(4, 30, 2), (12, 30, 2), (8, 32, 2), (8, 29, 2), (8, 30, 1), (8, 30, 4), (8, 16, 2)]:
        assert parts(300, S, 32, fout, F2, 1) == 0, (S, fout, F2)
    for fl in (F32, RING, ACC, DACC):
        assert parts(300, 8, 32, 30, 2, 1, fl) == 0, fl
    assert parts(300, 8, 32, 30, 2, 1, NOFOLD) == 3
    # the output stage adds 16 + 128 * 16 + 8 * 36 * 4 = 3,216 bytes to the plan's: refused a little before the plain launch is
    assert 115744 + 3216 + 8912 * 4 + 64 * 144 <= 160 * 1024 < 115744 + 3216 + 8928 * 4 + 64 * 144
    assert parts(300, 8, 32, 30, 2, 1, 0, 8912, 64) == 3 and parts(300, 8, 32, 30, 2, 1, 0, 8913, 64) == 0
    assert int(L().gml_spectconv_bwd_workspace_bytes(300, 8, 32, 30, 8913, 64, 0)) > 0


# ---- staging -------------------------------------------------------------------------------------------------------------------------
def stage_table(S, fin, fout, flags):
    """(edges, window rows) of one group inside the staging of the kernel the call runs on (gml.h; DESIGN s4.2a)"""
    r = rows(S, fin, fout, flags)
    if r == 64:
        return (1024, 192) if S % 4 == 0 else (0, 0)         # the 64-row kernel stages float4 value rows only
    if r == 0:
        return 0, 0
    if ring_applies(S, fin, fout, flags):
        return {8: 960, 4: 1024}[S] - 3, 200 - 7
    return {12: 12 * 128, 6: 16 * 128}.get(S, 8 * 128), 224


@pytest.mark.parametrize('flags', [0, F32, RING, RING | F32, RING | ACC, RING | DACC, ACC, DACC | NOFOLD])
def test_stage_queries_table(flags):
    for S, fin, fout in GRID:
        got = (int(L().gml_spectconv_bwd_stage_edges(S, fin, fout, flags)), int(L().gml_spectconv_bwd_stage_window(S, fin, fout, flags)))
        assert got == stage_table(S, fin, fout, flags), (S, fin, fout, flags, got)


def test_stage_queries_class_edges():
    e = lambda S, fin, fout, fl=0: int(L().gml_spectconv_bwd_stage_edges(S, fin, fout, fl))
    w = lambda S, fin, fout, fl=0: int(L().gml_spectconv_bwd_stage_window(S, fin, fout, fl))
    assert [e(S, 32, 32) for S in (2, 4, 6, 8)] == [1024, 1024, 2048, 1024] and [e(S, 32, 16) for S in (8, 12)] == [1024, 1536]
    assert [e(S, 48, 32) for S in (4, 6)] == [1024, 2048] and [w(S, 48, 32) for S in (4, 6)] == [224, 224]
    assert [e(S, 32, 32, RING) for S in (2, 4, 6, 8)] == [1024, 1021, 2048, 957] and [w(S, 32, 32, RING) for S in (2, 4, 6, 8)] == [224, 193, 224, 193]
    assert (e(8, 32, 16, RING), w(8, 32, 16, RING)) == (957, 193)          # S = 8, Fout <= 16: the ring's one form serves it too
    assert (e(4, 48, 32, RING), w(4, 48, 32, RING)) == (1024, 224)         # 33 .. 48 features: no ring form
    assert [e(S, 32, 32, F32) for S in (4, 6, 8)] == [1024, 0, 1024] and [w(S, 32, 32, F32) for S in (4, 6, 8)] == [192, 0, 192]
    assert (e(4, 64, 32), w(4, 64, 32)) == (1024, 192) and (e(12, 32, 32), w(12, 32, 32), e(5, 32, 32)) == (0, 0, 0)
