// gml_edge_mlp_fwd_stack6: the edge branches of a stack of ML3Layers in one pass over the raw supports, three-piece products
// (gml_edge_chain6_impl.h): S = Sout in {4, 8}, 1 .. 4 layers
#include "gml_edge_chain6_impl.h"

extern "C" int gml_edge_mlp_fwd_stack6(const float* ea, int32_t nlayers, const float* const* w1, const float* const* w2,
                                       const float* const* w3, const float* const* w4, float* const* out,
                                       int64_t num_edges, int32_t S, int32_t Sout, gml_stream_t stream) {
    if (num_edges < 0 || S <= 0 || Sout <= 0 || nlayers <= 0 || !w1 || !w2 || !w3 || !w4 || !out) return GML_E_BADARG;
    if (edge_plan_fwd(S, Sout, nlayers, EDGE_THREE_PIECE, false, false, false) != GML_EDGE_FAM_CHAIN6) return GML_E_UNSUPPORTED;
    if (num_edges == 0) return GML_OK;
    if (!ea || (((uintptr_t)ea) & 15) != 0) return GML_E_BADARG;
    for (int l = 0; l < nlayers; ++l)
        if (!w1[l] || !w2[l] || !w3[l] || !w4[l] || !out[l] || (((uintptr_t)out[l]) & 15) != 0) return GML_E_BADARG;
#define GML_STACK6_GO(SV, LV)                                                                                                        \
    if (S == SV && nlayers == LV)                                                                                                    \
        return gml_launch_edge_chain6_fwd<SV, LV>(ea, gml_chain_stack_args<GmlChain6Stack<LV>>(LV, w1, w2, w3, w4, out), nullptr, nullptr, \
                                                  num_edges, (hipStream_t)stream);
    GML_ECHAIN6_STACKS(GML_STACK6_GO)
    return GML_E_UNSUPPORTED;
}
