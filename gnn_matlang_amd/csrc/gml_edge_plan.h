// Which kernel family serves an ML3Layer edge-branch call (S <= 16) is decided here and nowhere else: every entry point of
// gml_edge_mlp.hip, gml_edge_chain_e.hip, gml_edge_chain6_a/b.hip and gml_edge_chain_sym.hip reads edge_plan_fwd / edge_plan_bwd, the
// size queries derive the partial-row counts from the same answer, and the host side asks gml_edge_mlp_plan (include/gml.h).
// Host code only.
#pragma once
#include "gml_common.h"

enum EdgeArith { EDGE_TWO_PIECE = GML_EDGE_TWO_PIECE, EDGE_THREE_PIECE = GML_EDGE_THREE_PIECE, EDGE_EXACT = GML_EDGE_EXACT };

// GML_EDGE_VALU=1 in the environment keeps the one-edge-per-lane fp32 kernels wherever a call would take a two-piece chain
// (ablation / exact-fp32 arithmetic); read once per process.  The three-piece and unique-row entry points are explicit requests.
static inline bool edge_plan_valu() {
    static const bool valu = [] { const char* e = getenv("GML_EDGE_VALU"); return e && e[0] == '1'; }();
    return valu;
}

// nlayers = 0: the single-layer entry points (gml_edge_mlp_fwd, _fwd6, _fwd_exact); >= 1: the stacked ones
static inline int edge_plan_fwd(int S, int Sout, int nlayers, int arith, bool has_split, bool dual, bool sym) {
    if (S < 1 || S > 16 || S != Sout || nlayers < 0 || nlayers > 4) return GML_EDGE_FAM_NONE;   // every reference script: nedgeoutput == nedgeinput
    const bool s48 = S == 4 || S == 8;
    if (nlayers > 0 && dual) return GML_EDGE_FAM_NONE;            // the scattered second copy belongs to the single-layer form
    if (sym)                                                  // unique rows: three-piece only; stacks at S in {4, 8}, single layers 2..16
        return (arith == EDGE_THREE_PIECE && S >= 2 && nlayers >= 1 && (s48 || nlayers == 1)) ? (S <= 8 ? GML_EDGE_FAM_SYM6 : GML_EDGE_FAM_SYM16X6)
                                                                                              : GML_EDGE_FAM_NONE;
    switch (arith) {
        case EDGE_EXACT: return nlayers == 0 ? GML_EDGE_FAM_VALU : GML_EDGE_FAM_NONE;
        case EDGE_THREE_PIECE:
            if (nlayers > 0) return s48 ? GML_EDGE_FAM_CHAIN6 : GML_EDGE_FAM_NONE;
            return S < 2 ? GML_EDGE_FAM_NONE : (S <= 8 ? GML_EDGE_FAM_CHAIN6 : GML_EDGE_FAM_CHAIN16X6);
        case EDGE_TWO_PIECE:
            if (nlayers > 0) return (s48 && nlayers >= 2 && has_split && !edge_plan_valu()) ? GML_EDGE_FAM_CHAIN : GML_EDGE_FAM_NONE;
            // S = 1 stays on the VALU kernels: its contractions are single products, so the split's 2^-17 rounding is not averaged
            // over a sum (measured 5e-5 .. 1e-4 of the output scale against 1e-5 for S >= 2), and there is no arithmetic to save
            if (S < 2 || edge_plan_valu()) return GML_EDGE_FAM_VALU;
            if (S <= 8) return GML_EDGE_FAM_CHAIN;
            return has_split ? GML_EDGE_FAM_CHAIN16 : GML_EDGE_FAM_VALU;   // the K = 16-slot chain needs the 64-byte pre-split rows
    }
    return GML_EDGE_FAM_NONE;
}

// the backward is two-piece (or exact) whatever the forward was; chain16 produces no gradient for the raw supports, and the
// unique-row forms neither (those cases stay on the VALU kernels, resp. are not offered)
static inline int edge_plan_bwd(int S, int Sout, bool has_split, bool want_gin, bool sym, bool exact) {
    if (S < 1 || S > 16 || S != Sout) return GML_EDGE_FAM_NONE;
    if (sym) return (!exact && S >= 2 && has_split && !want_gin) ? (S <= 8 ? GML_EDGE_FAM_SYM_CHAIN : GML_EDGE_FAM_SYM_CHAIN16) : GML_EDGE_FAM_NONE;
    if (exact || S < 2 || edge_plan_valu()) return GML_EDGE_FAM_VALU;
    if (S <= 8) return GML_EDGE_FAM_CHAIN;
    return (has_split && !want_gin) ? GML_EDGE_FAM_CHAIN16 : GML_EDGE_FAM_VALU;
}

// a kernel that scatters rows through ONE buffer descriptor addresses them with 32-bit byte offsets
static inline bool edge_plan_offsets_fit(int64_t num_edges, int S, uint64_t limit) { return (uint64_t)num_edges * (uint64_t)S * 4u < limit; }

// ------------------------------------------------------------------------------------------ backward launch geometry
// persistent workgroups of the two-piece chains: 6 per CU for S <= 8 (24.5 KB of LDS each), 2 per CU for 8 < S <= 16 (<= 256 VGPRs)
static inline int64_t gml_edge_chain_bwd_groups(int64_t E, int wgs_per_cu = 6) {
    int64_t grid = gml_cdiv(gml_cdiv(E, 16), 4);
    if (grid > wgs_per_cu * GML_NUM_CU) grid = wgs_per_cu * GML_NUM_CU;
    return grid < 1 ? 1 : grid;
}
static inline int64_t gml_edge_chain16_bwd_groups(int64_t E) { return gml_edge_chain_bwd_groups(E, 2); }
// the VALU family: one partial row per wave, <= 8 waves per CU hold accumulators; waves per workgroup = GmlEdgeMlpBwdCfg<S, S>::WAVES
// (its launcher asserts the two agree)
constexpr int edge_plan_valu_bwd_wg_waves(int S) { return ((7 * S) | 1) * 64 * 4 * 4 <= 64 * 1024 ? 4 : 2; }
static inline int64_t gml_edge_mlp_bwd_waves(int64_t E, int waves_per_wg) {
    const int64_t nbatch = gml_cdiv(E, 64);
    int64_t nw = (int64_t)GML_NUM_CU * 8;
    if (nw > nbatch) nw = nbatch;
    nw = gml_cdiv(nw, waves_per_wg) * waves_per_wg;
    return nw < waves_per_wg ? waves_per_wg : nw;
}
// partial rows [dw1 | dw2 | dw3 | dw4] a backward of `family` leaves in the workspace for n edges (unique-row forms: n entries)
static inline int64_t edge_plan_bwd_parts(int family, int64_t n, int S) {
    switch (family) {
        case GML_EDGE_FAM_VALU: return gml_edge_mlp_bwd_waves(n, edge_plan_valu_bwd_wg_waves(S));
        case GML_EDGE_FAM_CHAIN: case GML_EDGE_FAM_SYM_CHAIN: return gml_edge_chain_bwd_groups(n);
        case GML_EDGE_FAM_CHAIN16: case GML_EDGE_FAM_SYM_CHAIN16: return gml_edge_chain16_bwd_groups(n);
    }
    return 0;
}

// ------------------------------------------------------------------------------------------ tails every backward shares
__global__ void gml_k_reduce_partials(const float* __restrict__ partial, int64_t nwaves, int nw, float* __restrict__ d0, int n0,
                                      float* __restrict__ d1, int n1, float* __restrict__ d2, int n2, float* __restrict__ d3, int n3);

// after the backward kernel's launch: fold the `parts` partial rows of ws into dw1 .. dw4 in a fixed order, or (dw1 == NULL) leave
// them there for gml_fold_many
static inline int gml_edge_fold_tail(const void* ws, int64_t parts, int S, float* dw1, float* dw2, float* dw3, float* dw4, hipStream_t st) {
    const int rc = gml_launch_status();
    if (rc != GML_OK || !dw1) return rc;
    const int n123 = 2 * S * S, n4 = S * 4 * S;
    hipLaunchKernelGGL(gml_k_reduce_partials, dim3((unsigned)gml_cdiv(3 * n123 + n4, 16)), dim3(256), 0, st, (const float*)ws, parts,
                       3 * n123 + n4, dw1, n123, dw2, n123, dw3, n123, dw4, n4);
    return gml_launch_status();
}

// no edges: the weight gradients are zeros
static inline int gml_edge_zero_dw(float* dw1, float* dw2, float* dw3, float* dw4, int S, int Sout, hipStream_t st) {
    gml_zero_async(dw1, sizeof(float) * 2 * S * S, st);
    gml_zero_async(dw2, sizeof(float) * 2 * S * S, st);
    gml_zero_async(dw3, sizeof(float) * 2 * S * S, st);
    gml_zero_async(dw4, sizeof(float) * 4 * S * Sout, st);
    return gml_launch_status();
}
