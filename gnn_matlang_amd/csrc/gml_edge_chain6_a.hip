// gml_edge_mlp_fwd6: one layer's edge branch, three-piece products: 2 <= S = Sout <= 8 (gml_edge_chain6_impl.h), 9 .. 16 (gml_edge_chain16x6_impl.h)
#include "gml_edge_chain6_impl.h"
#include "gml_edge_chain16_impl.h"
#include "gml_edge_chain16x6_impl.h"

extern "C" int gml_edge_mlp_fwd6(const float* ea, const float* w1, const float* w2, const float* w3, const float* w4, float* out,
                                 const int32_t* tpos, float* out_t, int64_t num_edges, int32_t S, int32_t Sout, gml_stream_t stream) {
    if (num_edges < 0 || S <= 0 || Sout <= 0) return GML_E_BADARG;
    const int fam = edge_plan_fwd(S, Sout, 0, EDGE_THREE_PIECE, false, out_t != nullptr, false);
    if (fam == GML_EDGE_FAM_NONE) return GML_E_UNSUPPORTED;
    if (num_edges == 0) return GML_OK;
    if (!ea || !w1 || !w2 || !w3 || !w4 || !out) return GML_E_BADARG;
    if ((S <= 8 || S % 4 == 0) && (((uintptr_t)ea | (uintptr_t)out | (uintptr_t)out_t) & 15) != 0) return GML_E_BADARG;
    if (out_t && !tpos) return GML_E_BADARG;
    // the second (source-order) copy is scattered through one buffer descriptor: 32-bit byte offsets
    if (out_t && !edge_plan_offsets_fit(num_edges, S, 0xffffff00ull)) return GML_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const float* const w1a[1] = {w1}, * const w2a[1] = {w2}, * const w3a[1] = {w3}, * const w4a[1] = {w4};
    float* const outa[1] = {out};
#define GML_C6(SV) \
    case SV: return gml_launch_edge_chain6_fwd<SV, 1>(ea, gml_chain_stack_args<GmlChain6Stack<1>>(1, w1a, w2a, w3a, w4a, outa), tpos, out_t, num_edges, st);
#define GML_C16X6(SV) case SV: return gml_launch_edge_chain16x6_fwd<SV>(ea, w1, w2, w3, w4, out, tpos, out_t, num_edges, st);
    switch (S) {
        GML_ECHAIN6_S(GML_C6)
        GML_ECHAIN16_S(GML_C16X6)
    }
    return GML_E_UNSUPPORTED;
}
