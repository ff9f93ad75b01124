// Edge branches of a stack of ML3Layers in one pass over the raw supports (gml_edge_mlp_fwd_stack): S = Sout in {4, 8}, 2..4 layers
#include "gml_edge_chain_impl.h"

// out[l] = relu(W4_l [relu(W1_l e) ; tanh(W2_l e) * tanh(W3_l e)]) for l < nlayers, e = the rows of ea whose bf16 (hi, lo) split is
// ea_split (gml_edge_presplit).  The pointer arrays live on the HOST.  GML_E_UNSUPPORTED where the plan has no stacked two-piece
// kernel: the caller launches gml_edge_mlp_fwd per layer.
extern "C" int gml_edge_mlp_fwd_stack(const void* ea_split, int32_t nlayers, const float* const* w1, const float* const* w2,
                                      const float* const* w3, const float* const* w4, float* const* out,
                                      int64_t num_edges, int32_t S, int32_t Sout, gml_stream_t stream) {
    if (num_edges < 0 || S <= 0 || Sout <= 0 || nlayers <= 0 || !w1 || !w2 || !w3 || !w4 || !out) return GML_E_BADARG;
    if (edge_plan_fwd(S, Sout, nlayers, EDGE_TWO_PIECE, true, false, false) != GML_EDGE_FAM_CHAIN) return GML_E_UNSUPPORTED;
    if (num_edges == 0) return GML_OK;
    if (!ea_split || (((uintptr_t)ea_split) & 15) != 0) return GML_E_BADARG;
    for (int l = 0; l < nlayers; ++l)
        if (!w1[l] || !w2[l] || !w3[l] || !w4[l] || !out[l] || (((uintptr_t)out[l]) & 15) != 0) return GML_E_BADARG;
#define GML_STACK_GO(SV, LV)                                                                                                      \
    if (S == SV && nlayers == LV)                                                                                                 \
        return gml_launch_edge_chain_fwd_stack<SV, LV>((const uint32_t*)ea_split, gml_chain_stack_args<GmlChainStack<LV>>(LV, w1, w2, w3, w4, out), \
                                                       num_edges, (hipStream_t)stream);
    GML_ECHAIN_STACKS(GML_STACK_GO)
    return GML_E_UNSUPPORTED;
}
