"""The three shape queries of the conv forward (gml_spectconv_fwd_group_rows / _stage_edges / _stage_window) against a table written
from include/gml.h and DESIGN.md s4.1 / s4.1b / s4.1c -- not from the dispatch code.  Callers (functional.fwd_groups, any user of the
C ABI) choose their group records and flags from these answers, so a change of the plan that moves one shows up here, without a GPU:
the library loads and answers on the host."""
import itertools

import pytest

from gnn_matlang_amd import _lib

SS = list(range(1, 17)) + [24]
FINS = [1, 16, 17, 32, 33, 48, 49, 64]
FOUTS = [1, 16, 17, 32, 33]
ARITH = [0, _lib.GML_F32_MFMA, _lib.GML_FWD_CHUNKED]
NEUTRAL = [0, _lib.GML_RELU, _lib.GML_ACCUM, _lib.GML_F16X3, _lib.GML_FWD_ONEWIN]
GRID = list(itertools.product(SS, FINS, FOUTS))


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def ring_shape(S, fin):
    """fwd3's shapes (DESIGN s4.1: S in {4, 8}, Fin <= 32), the class fwd2 also serves"""
    return S in (4, 8) and fin <= 32


def chunked_only_shape(S, fin):
    """the two classes only the chunked ring kernel serves on 128-row records (gml.h: "6 supports, 33..48 input features";
    DESIGN s4.1c: sr25's S = 6 with 2 / 32 / 48 features, mutag's S = 4 with 24 + 24)"""
    return (S == 6 and fin <= 48) or (S == 4 and 33 <= fin <= 48)


def rows128(S, fin, fout, flags):
    eight_wave = ring_shape(S, fin) or (S == 12 and fin <= 32) or chunked_only_shape(S, fin)      # S = 12: fwd2 (DESIGN s4.1b)
    return not (flags & _lib.GML_F32_MFMA) and fout <= 32 and eight_wave


def answers(S, fin, fout, flags):
    L = _lib.lib()
    return (int(L.gml_spectconv_fwd_group_rows(S, fin, fout, flags)), int(L.gml_spectconv_fwd_stage_edges(S, fin, fout, flags)),
            int(L.gml_spectconv_fwd_stage_window(S, fin, fout, flags)))


@pytest.mark.parametrize('arith', ARITH)
def test_group_rows_table(arith):
    for S, fin, fout in GRID:
        rows = answers(S, fin, fout, arith)[0]
        assert rows == (128 if rows128(S, fin, fout, arith) else 64), (S, fin, fout, arith, rows)


def test_window_bound_without_the_chunked_flag_marks_the_chunked_only_shapes():
    """functional.fwd_groups reads a non-zero window without GML_FWD_CHUNKED as "fwd4 alone serves this shape"."""
    for arith in (0, _lib.GML_F32_MFMA):
        for S, fin, fout in GRID:
            win = answers(S, fin, fout, arith)[2]
            only4 = rows128(S, fin, fout, arith) and chunked_only_shape(S, fin)
            assert (win != 0) == only4, (S, fin, fout, arith, win)
            assert win >= 0


def test_window_bound_with_the_chunked_flag():
    """every 128-row shape the chunked kernel can be asked for has a bound.  (The library also answers non-zero for S = 12, which
    has no chunked instantiation and runs on fwd2 whatever the flag says: left unpinned.)"""
    for S, fin, fout in GRID:
        win = answers(S, fin, fout, _lib.GML_FWD_CHUNKED)[2]
        if not rows128(S, fin, fout, 0):
            assert win == 0, (S, fin, fout, win)
        elif S != 12:
            assert win > 0, (S, fin, fout, win)
            # the flag does not widen what the chunked-only shapes already report
            if chunked_only_shape(S, fin):
                assert win == answers(S, fin, fout, 0)[2]


@pytest.mark.parametrize('arith', ARITH)
def test_stage_edges_table(arith):
    """> 0 exactly for the ring shapes and the chunked-only shapes; 0 for S = 12 (register-staged) and every 64-row shape"""
    for S, fin, fout in GRID:
        cap = answers(S, fin, fout, arith)[1]
        want = rows128(S, fin, fout, arith) and (ring_shape(S, fin) or chunked_only_shape(S, fin))
        assert (cap > 0) == want and cap >= 0, (S, fin, fout, arith, cap)
        if want:
            assert cap <= 1024, (S, fin, fout, cap)                # DESIGN s4.1 / s4.1c: a work item stages at most 1,024 edges


def test_answers_do_not_depend_on_the_neutral_flags():
    for arith in ARITH:
        for S, fin, fout in GRID:
            base = answers(S, fin, fout, arith)
            for f in NEUTRAL[1:]:
                assert answers(S, fin, fout, arith | f) == base, (S, fin, fout, arith, f)
            assert answers(S, fin, fout, arith | _lib.GML_RELU | _lib.GML_ACCUM | _lib.GML_F16X3 | _lib.GML_FWD_ONEWIN) == base
