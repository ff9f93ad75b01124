"""gml_edge_mlp_plan -- which kernel family serves an ML3Layer edge-branch call -- against a table written from include/gml.h,
INTEGRATION.md and DESIGN.md s4.3, not from the dispatch code (csrc/gml_edge_plan.h), and the three size queries of the backward
against what the planned family prescribes.  The library loads and answers on the host: no GPU.  GML_EDGE_VALU is read once per
process, so the other setting of it runs in a child process."""
import itertools
import os
import subprocess
import sys

from gnn_matlang_amd import _lib as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUM_CU = 256                                                  # MI355X (csrc/gml_common.h)
ES = (1, 16, 17, 98305, 200003)
ARITH = (G.GML_EDGE_TWO_PIECE, G.GML_EDGE_THREE_PIECE, G.GML_EDGE_EXACT)
BITS = (G.GML_EDGE_HAS_SPLIT, G.GML_EDGE_WANT_GIN, G.GML_EDGE_DUAL, G.GML_EDGE_UNIQUE)


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def expect_fwd(S, So, L, arith, split, gin, dual, sym, valu):
    if S != So or S > 16 or L > 4 or gin:                    # gml.h: S = Sout <= 16; stacks of up to 4 layers; gin is a backward flag
        return G.GML_EDGE_FAM_NONE
    if sym:                                                   # gml.h: three-piece, 2 <= S <= 16, layer stacks S in {4, 8}; no second order
        ok = arith == G.GML_EDGE_THREE_PIECE and 1 <= L and S >= 2 and (L == 1 or S in (4, 8)) and not dual
        return (G.GML_EDGE_FAM_SYM6 if S <= 8 else G.GML_EDGE_FAM_SYM16X6) if ok else G.GML_EDGE_FAM_NONE
    if L == 0:                                                # the single-layer entry points
        if arith == G.GML_EDGE_EXACT:
            return G.GML_EDGE_FAM_VALU
        if arith == G.GML_EDGE_THREE_PIECE:                   # gml_edge_mlp_fwd6: 2 <= S = Sout <= 16
            return G.GML_EDGE_FAM_NONE if S < 2 else (G.GML_EDGE_FAM_CHAIN6 if S <= 8 else G.GML_EDGE_FAM_CHAIN16X6)
        if S == 1 or valu:                                    # DESIGN s4.3: S = 1 and GML_EDGE_VALU=1 stay on the VALU kernels
            return G.GML_EDGE_FAM_VALU
        if S <= 8:
            return G.GML_EDGE_FAM_CHAIN
        return G.GML_EDGE_FAM_CHAIN16 if split else G.GML_EDGE_FAM_VALU       # chain16 needs the 64-byte pre-split rows
    if dual or arith == G.GML_EDGE_EXACT or S not in (4, 8):  # stacks: S in {4, 8}, one order, matrix-core chains only
        return G.GML_EDGE_FAM_NONE
    if arith == G.GML_EDGE_THREE_PIECE:                       # gml_edge_mlp_fwd_stack6: 1 <= nlayers <= 4
        return G.GML_EDGE_FAM_CHAIN6
    return G.GML_EDGE_FAM_CHAIN if (L >= 2 and split and not valu) else G.GML_EDGE_FAM_NONE    # gml_edge_mlp_fwd_stack: 2 .. 4, on ea_split


def expect_bwd(S, So, arith, split, gin, dual, sym, valu):
    if S != So or S > 16 or dual:                             # dual is a forward flag
        return G.GML_EDGE_FAM_NONE
    exact = arith == G.GML_EDGE_EXACT                         # (two- and three-piece forwards share the two-piece backward)
    if sym:                                                   # gml_edge_mlp_bwd_sym: 2 <= S <= 16, on ea_split, no gin
        ok = not exact and S >= 2 and split and not gin
        return (G.GML_EDGE_FAM_SYM_CHAIN if S <= 8 else G.GML_EDGE_FAM_SYM_CHAIN16) if ok else G.GML_EDGE_FAM_NONE
    if exact or S == 1 or valu:
        return G.GML_EDGE_FAM_VALU
    if S <= 8:
        return G.GML_EDGE_FAM_CHAIN
    return G.GML_EDGE_FAM_CHAIN16 if (split and not gin) else G.GML_EDGE_FAM_VALU   # chain16: pre-split rows, no supports' gradient


def cdiv(a, b):
    return -(-a // b)


def expect_parts(fam, n, S):
    """partial rows of a backward of `fam` over n edges (unique-row forms: n entries), DESIGN s4.3"""
    if fam == G.GML_EDGE_FAM_VALU:                            # one per wave, <= 8 waves per CU; workgroups of 4 waves, 2 where the
        W = 4 if ((7 * S) | 1) * 64 * 4 * 4 <= 64 * 1024 else 2   # transposition tile of 4 would pass 64 KB of LDS
        return max(cdiv(min(NUM_CU * 8, cdiv(n, 64)), W) * W, W)
    per_cu = {G.GML_EDGE_FAM_CHAIN: 6, G.GML_EDGE_FAM_SYM_CHAIN: 6, G.GML_EDGE_FAM_CHAIN16: 2, G.GML_EDGE_FAM_SYM_CHAIN16: 2}[fam]
    return max(1, min(cdiv(cdiv(n, 16), 4), per_cu * NUM_CU))   # one per persistent workgroup of 4 waves x 16-edge tiles


# ---- the checks (run in this process and, under the other GML_EDGE_VALU, in a child) -------------------------------------------------
def check_plan(valu):
    L_ = G.lib()
    n = 0
    for S, So in itertools.product(range(1, 18), repeat=2):
        for arith, bits in itertools.product(ARITH, itertools.product((0, 1), repeat=4)):
            split, gin, dual, sym = bits
            flags = arith | sum(b for b, on in zip(BITS, bits) if on)
            for L in range(0, 6):
                got = int(L_.gml_edge_mlp_plan(G.GML_EDGE_FWD, S, So, L, flags))
                assert got == expect_fwd(S, So, L, arith, split, gin, dual, sym, valu), ('fwd', S, So, L, arith, bits, valu, got)
                # the backward does not read nlayers
                got = int(L_.gml_edge_mlp_plan(G.GML_EDGE_BWD, S, So, L, flags))
                assert got == expect_bwd(S, So, arith, split, gin, dual, sym, valu), ('bwd', S, So, L, arith, bits, valu, got)
                n += 2
    assert int(L_.gml_edge_mlp_plan(2, 8, 8, 0, 0)) == G.GML_EDGE_FAM_NONE              # no such direction
    assert int(L_.gml_edge_mlp_plan(G.GML_EDGE_FWD, 8, 8, 0, 3)) == G.GML_EDGE_FAM_NONE  # no such arithmetic
    assert int(L_.gml_edge_mlp_plan(G.GML_EDGE_FWD, 8, 8, 0, 64)) == G.GML_EDGE_FAM_NONE  # no such flag
    assert int(L_.gml_edge_mlp_plan(G.GML_EDGE_FWD, 0, 0, 0, 0)) == G.GML_EDGE_FAM_NONE
    return n


def check_sizes(valu):
    L_ = G.lib()
    for S, E in itertools.product(range(1, 17), ES):
        most = 0
        for split, gin in itertools.product((0, 1), repeat=2):
            fam = int(L_.gml_edge_mlp_plan(G.GML_EDGE_BWD, S, S, 0, (G.GML_EDGE_HAS_SPLIT if split else 0) | (G.GML_EDGE_WANT_GIN if gin else 0)))
            parts = int(L_.gml_edge_mlp_bwd_parts(E, S, S, split, gin))
            assert parts == expect_parts(fam, E, S), (E, S, split, gin, fam, parts)
            most = max(most, parts)
        exact = int(L_.gml_edge_mlp_plan(G.GML_EDGE_BWD, S, S, 0, G.GML_EDGE_EXACT))
        most = max(most, expect_parts(exact, E, S))           # gml_edge_mlp_bwd_exact takes the same workspace
        fam = int(L_.gml_edge_mlp_plan(G.GML_EDGE_BWD, S, S, 0, G.GML_EDGE_HAS_SPLIT | G.GML_EDGE_UNIQUE))
        if fam != G.GML_EDGE_FAM_NONE:
            for U in sorted({1, E // 2 + 1, E}):              # the unique rows of E edges: at most E entries
                sp = int(L_.gml_edge_mlp_bwd_sym_parts(U, S))
                assert sp == expect_parts(fam, U, S), (U, S, fam, sp)
                most = max(most, sp)
        row = (6 * S * S + 4 * S * S) * 4                     # [dw1 | dw2 | dw3 | dw4] in fp32
        assert int(L_.gml_edge_mlp_bwd_workspace_bytes(E, S, S)) >= most * row, (E, S, most)
        for So in range(1, 18):
            if So != S:
                assert int(L_.gml_edge_mlp_bwd_workspace_bytes(E, S, So)) == 0 and int(L_.gml_edge_mlp_bwd_parts(E, S, So, 1, 0)) == 0
    assert int(L_.gml_edge_mlp_bwd_parts(0, 8, 8, 1, 0)) == 0 and int(L_.gml_edge_mlp_bwd_sym_parts(0, 8)) == 0


def environment_says_valu():
    return os.environ.get('GML_EDGE_VALU', '')[:1] == '1'


def test_plan_table_and_backward_sizes():
    valu = environment_says_valu()
    assert check_plan(valu) == 17 * 17 * 3 * 16 * 6 * 2
    check_sizes(valu)


def test_plan_table_and_backward_sizes_under_the_other_setting_of_the_environment():
    other = not environment_says_valu()
    code = ("import sys\nsys.path.insert(0, %r)\nsys.path.insert(0, %r)\nimport test_edge_plan_cpu as t\n"
            "assert t.environment_says_valu() == %r\nt.check_plan(%r)\nt.check_sizes(%r)\nprint('PLAN OK')\n"
            % (ROOT, os.path.join(ROOT, 'tests'), other, other, other))
    env = dict(os.environ, GML_EDGE_VALU='1' if other else '0')
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'PLAN OK' in out.stdout, out.stderr[-2000:]
