// C-ABI of the edge branch over a batch's UNIQUE support rows (gml_edge_chain_sym_impl.h): the pairing pass, the forward of a layer
// stack (three-piece products; stacks: S in {4, 8}, single layers: 2 <= S <= 16) and the backward (two-piece chains), 2 <= S = Sout <= 16
#include "gml_edge_chain_sym_impl.h"
#include "gml_edge_chain16_impl.h"
#include "gml_edge_chain16x6_impl.h"

extern "C" int gml_edge_sym_flags(const int32_t* rowptr_t, const int32_t* col_t, const float* val_s, int64_t num_rows,
                                  int64_t num_edges, int32_t S, int32_t* flag, int32_t* mirror, gml_stream_t stream) {
    if (num_rows < 0 || num_edges < 0 || S <= 0) return GML_E_BADARG;
    if (num_edges == 0) return GML_OK;
    if (!rowptr_t || !col_t || !val_s || !flag || !mirror || num_rows == 0) return GML_E_BADARG;
    // lanes per source row: the power of two nearest the mean row length
    int lps = 0;
    while (lps < 4 && (num_rows << (lps + 1)) <= num_edges) ++lps;        // 2^lps <= edges per row
    hipLaunchKernelGGL(gml_k_edge_sym_flags, dim3((unsigned)gml_cdiv(num_rows << lps, 256)), dim3(256), 0, (hipStream_t)stream, rowptr_t,
                       col_t, reinterpret_cast<const uint32_t*>(val_s), num_rows, num_edges, (int)S, lps, flag, mirror);
    return gml_launch_status();
}

// ucount != NULL: num_unique is the capacity of uid / mir and *ucount (device) the number of entries (gml_edge_mlp_fwd_stack6_sym_dev)
static int fwd_stack6_sym(const float* ea, const int32_t* uid, const int32_t* mir, int64_t num_unique, const int32_t* ucount,
                          int32_t nlayers, const float* const* w1, const float* const* w2, const float* const* w3,
                          const float* const* w4, float* const* out, int64_t num_edges, int32_t S, int32_t Sout, gml_stream_t stream) {
    if (num_edges < 0 || num_unique < 0 || num_unique > num_edges || S <= 0 || Sout <= 0 || nlayers <= 0 || !w1 || !w2 || !w3 || !w4 || !out)
        return GML_E_BADARG;
    if (edge_plan_fwd(S, Sout, nlayers, EDGE_THREE_PIECE, false, false, true) == GML_EDGE_FAM_NONE) return GML_E_UNSUPPORTED;
    if (!edge_plan_offsets_fit(num_edges, S, 0x7fffff00ull)) return GML_E_UNSUPPORTED;          /* 32-bit store offsets */
    if (num_edges == 0) return GML_OK;
    if (num_unique == 0 || !ea || !uid || !mir || (S % 4 == 0 && (((uintptr_t)ea) & 15) != 0)) return GML_E_BADARG;
    for (int l = 0; l < nlayers; ++l)
        if (!w1[l] || !w2[l] || !w3[l] || !w4[l] || !out[l] || (S % 4 == 0 && (((uintptr_t)out[l]) & 15) != 0)) return GML_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
#define GML_SYM_GO(SV, LV)                                                                                                              \
    if (S == SV && nlayers == LV)                                                                                                       \
        return gml_launch_edge_chain6_fwd_sym<SV, LV>(ea, uid, mir, gml_chain_stack_args<GmlChain6Stack<LV>>(LV, w1, w2, w3, w4, out), num_edges, \
                                                      num_unique, st, ucount);
    GML_ECHAIN6_STACKS(GML_SYM_GO)
    GML_ESYM_SINGLES(GML_SYM_GO)
#define GML_SYM16_GO(SV) if (S == SV) return gml_launch_edge_chain16x6_fwd_sym<SV>(ea, uid, mir, num_unique, w1[0], w2[0], w3[0], w4[0], out[0], st, ucount);
    GML_ECHAIN16_S(GML_SYM16_GO)
    return GML_E_UNSUPPORTED;
}

extern "C" int gml_edge_mlp_fwd_stack6_sym(const float* ea, const int32_t* uid, const int32_t* mir, int64_t num_unique, int32_t nlayers,
                                           const float* const* w1, const float* const* w2, const float* const* w3,
                                           const float* const* w4, float* const* out, int64_t num_edges, int32_t S, int32_t Sout,
                                           gml_stream_t stream) {
    return fwd_stack6_sym(ea, uid, mir, num_unique, nullptr, nlayers, w1, w2, w3, w4, out, num_edges, S, Sout, stream);
}

extern "C" int gml_edge_mlp_fwd_stack6_sym_dev(const float* ea, const int32_t* uid, const int32_t* mir, const int32_t* count,
                                               int64_t capacity, int32_t nlayers, const float* const* w1, const float* const* w2,
                                               const float* const* w3, const float* const* w4, float* const* out, int64_t num_edges,
                                               int32_t S, int32_t Sout, gml_stream_t stream) {
    if (!count || capacity <= 0) return GML_E_BADARG;
    return fwd_stack6_sym(ea, uid, mir, capacity, count, nlayers, w1, w2, w3, w4, out, num_edges, S, Sout, stream);
}

// (a shape the backward refuses: the count of the family of its S range)
extern "C" int64_t gml_edge_mlp_bwd_sym_parts(int64_t num_unique, int32_t S) {
    if (num_unique <= 0) return 0;
    const int fam = edge_plan_bwd(S, S, true, false, true, false);
    return edge_plan_bwd_parts(fam != GML_EDGE_FAM_NONE ? fam : (S > 8 ? GML_EDGE_FAM_SYM_CHAIN16 : GML_EDGE_FAM_SYM_CHAIN), num_unique, S);
}

template <int S>
static int sym_bwd16_go(const uint32_t* es, const int32_t* uid, const int32_t* mir, int64_t U, const float* w1, const float* w2,
                        const float* w3, const float* w4, const float* gout, float* dw1, float* dw2, float* dw3, float* dw4, void* ws,
                        size_t ws_bytes, hipStream_t st, const int32_t* ucount) {
    const int64_t ntiles = gml_cdiv(U, 16);
    const int64_t grid = edge_plan_bwd_parts(GML_EDGE_FAM_SYM_CHAIN16, U, S);
    if (ws_bytes < (size_t)grid * GML_CHAIN16_NW(S) * sizeof(float)) return GML_E_WORKSPACE;
    if (ucount)
        hipLaunchKernelGGL((gml_k_edge_chain16_bwd<S, true, true>), dim3((unsigned)grid), dim3(256), 0, st, es, w1, w2, w3, w4, gout, (float*)ws, U,
                           ntiles, uid, mir, ucount);
    else
        hipLaunchKernelGGL((gml_k_edge_chain16_bwd<S, true>), dim3((unsigned)grid), dim3(256), 0, st, es, w1, w2, w3, w4, gout, (float*)ws, U, ntiles,
                           uid, mir);
    return gml_edge_fold_tail(ws, grid, S, dw1, dw2, dw3, dw4, st);
}

template <int S>
static int sym_bwd_go(const uint32_t* es, const int32_t* uid, const int32_t* mir, int64_t U, const float* w1, const float* w2,
                      const float* w3, const float* w4, const float* gout, float* dw1, float* dw2, float* dw3, float* dw4, void* ws,
                      size_t ws_bytes, hipStream_t st, const int32_t* ucount) {
    const int64_t ntiles = gml_cdiv(U, 16);
    const int64_t grid = edge_plan_bwd_parts(GML_EDGE_FAM_SYM_CHAIN, U, S);
    if (ws_bytes < (size_t)grid * GML_CHAIN_NW(S) * sizeof(float)) return GML_E_WORKSPACE;
    if (ucount)
        hipLaunchKernelGGL((gml_k_edge_chain_bwd_sym<S, true>), dim3((unsigned)grid), dim3(256), 0, st, es, uid, mir, w1, w2, w3, w4, gout,
                           (float*)ws, U, ntiles, ucount);
    else
        hipLaunchKernelGGL((gml_k_edge_chain_bwd_sym<S>), dim3((unsigned)grid), dim3(256), 0, st, es, uid, mir, w1, w2, w3, w4, gout,
                           (float*)ws, U, ntiles);
    return gml_edge_fold_tail(ws, grid, S, dw1, dw2, dw3, dw4, st);
}

// ucount != NULL: num_unique is the capacity of uid / mir and *ucount (device) the number of entries (gml_edge_mlp_bwd_sym_dev)
static int bwd_sym(const void* ea_split, const int32_t* uid, const int32_t* mir, int64_t num_unique, const int32_t* ucount, const float* w1,
                   const float* w2, const float* w3, const float* w4, const float* gout, float* dw1, float* dw2, float* dw3, float* dw4,
                   int64_t num_edges, int32_t S, int32_t Sout, void* ws, size_t ws_bytes, gml_stream_t stream) {
    if (num_edges <= 0 || num_unique <= 0 || num_unique > num_edges || S <= 0 || Sout <= 0) return GML_E_BADARG;
    const bool nofold = !dw1 && !dw2 && !dw3 && !dw4;
    if (!w1 || !w2 || !w3 || !w4 || (!nofold && (!dw1 || !dw2 || !dw3 || !dw4))) return GML_E_BADARG;
    if (edge_plan_bwd(S, Sout, true, false, true, false) == GML_EDGE_FAM_NONE) return GML_E_UNSUPPORTED;
    if (!ea_split || !uid || !mir || !gout || !ws || (((uintptr_t)ea_split) & 15) != 0 || (S % 4 == 0 && (((uintptr_t)gout) & 15) != 0)) return GML_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t* es = (const uint32_t*)ea_split;
#define GML_SYM_BWD(SV) case SV: return sym_bwd_go<SV>(es, uid, mir, num_unique, w1, w2, w3, w4, gout, dw1, dw2, dw3, dw4, ws, ws_bytes, st, ucount);
#define GML_SYM_BWD16(SV) case SV: return sym_bwd16_go<SV>(es, uid, mir, num_unique, w1, w2, w3, w4, gout, dw1, dw2, dw3, dw4, ws, ws_bytes, st, ucount);
    switch (S) {
        GML_ECHAIN6_S(GML_SYM_BWD)
        GML_ECHAIN16_S(GML_SYM_BWD16)
    }
    return GML_E_UNSUPPORTED;
}

extern "C" int gml_edge_mlp_bwd_sym(const void* ea_split, const int32_t* uid, const int32_t* mir, int64_t num_unique, const float* w1,
                                    const float* w2, const float* w3, const float* w4, const float* gout, float* dw1, float* dw2,
                                    float* dw3, float* dw4, int64_t num_edges, int32_t S, int32_t Sout, void* ws, size_t ws_bytes,
                                    gml_stream_t stream) {
    return bwd_sym(ea_split, uid, mir, num_unique, nullptr, w1, w2, w3, w4, gout, dw1, dw2, dw3, dw4, num_edges, S, Sout, ws, ws_bytes, stream);
}

extern "C" int gml_edge_mlp_bwd_sym_dev(const void* ea_split, const int32_t* uid, const int32_t* mir, const int32_t* count, int64_t capacity,
                                        const float* w1, const float* w2, const float* w3, const float* w4, const float* gout, float* dw1,
                                        float* dw2, float* dw3, float* dw4, int64_t num_edges, int32_t S, int32_t Sout, void* ws,
                                        size_t ws_bytes, gml_stream_t stream) {
    if (!count) return GML_E_BADARG;
    return bwd_sym(ea_split, uid, mir, capacity, count, w1, w2, w3, w4, gout, dw1, dw2, dw3, dw4, num_edges, S, Sout, ws, ws_bytes, stream);
}
