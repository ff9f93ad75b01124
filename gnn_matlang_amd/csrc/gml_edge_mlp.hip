// C-ABI dispatch of the ML3Layer edge-branch kernels + the partial-sum fold.
#include "gml_edge_mlp_impl.h"
#include "gml_edge_chain_impl.h"
#include "gml_edge_chain16_impl.h"

// Which family a call takes: gml_edge_plan.h.  The launchers are instantiated in the fam files (gml_edge_chain_a/b, gml_edge_chain16_a..d,
// gml_edge_mlp_a..f) from the same S lists as the ladders below.
#define GML_DECL_ECHAIN(SV)                                                                                  \
    template <> int gml_launch_edge_chain_fwd<SV>(const float*, const uint32_t*, const float*, const float*, \
                                                  const float*, const float*, float*, const int32_t*, float*, \
                                                  int64_t, hipStream_t);                                     \
    template <> int gml_launch_edge_chain_bwd<SV>(const float*, const uint32_t*, const float*, const float*, \
                                                  const float*, const float*, const float*, float*, float*,  \
                                                  float*, float*, float*, int64_t, void*, size_t, hipStream_t);
GML_ECHAIN_S(GML_DECL_ECHAIN)
#define GML_DECL_ECHAIN16(SV)                                                                                \
    template <> int gml_launch_edge_chain16_fwd<SV>(const uint32_t*, const float*, const float*, const float*, \
                                                    const float*, float*, const int32_t*, float*, int64_t, hipStream_t); \
    template <> int gml_launch_edge_chain16_bwd<SV>(const uint32_t*, const float*, const float*, const float*, \
                                                    const float*, const float*, float*, float*, float*, float*, \
                                                    int64_t, void*, size_t, hipStream_t);
GML_ECHAIN16_S(GML_DECL_ECHAIN16)
#define GML_DECL_EMLP(SV)                                                                                    \
    template <> int gml_launch_edge_mlp_fwd<SV, SV>(const float*, const float*, const float*, const float*,  \
                                                    const float*, float*, const int32_t*, float*, int64_t,   \
                                                    hipStream_t);                                            \
    template <> int gml_launch_edge_mlp_bwd<SV, SV>(const float*, const float*, const float*, const float*,  \
                                                    const float*, const float*, float*, float*, float*,      \
                                                    float*, float*, int64_t, void*, size_t, hipStream_t);
GML_EMLP_S(GML_DECL_EMLP)

extern "C" int32_t gml_edge_mlp_plan(int32_t direction, int32_t S, int32_t Sout, int32_t nlayers, uint32_t flags) {
    const int arith = (int)(flags & GML_EDGE_ARITH_MASK);
    const bool split = flags & GML_EDGE_HAS_SPLIT, gin = flags & GML_EDGE_WANT_GIN, dual = flags & GML_EDGE_DUAL, sym = flags & GML_EDGE_UNIQUE;
    if (arith > EDGE_EXACT || (flags & ~63u)) return GML_EDGE_FAM_NONE;
    if (direction == GML_EDGE_FWD) return gin ? GML_EDGE_FAM_NONE : edge_plan_fwd(S, Sout, nlayers, arith, split, dual, sym);
    if (direction == GML_EDGE_BWD) return dual ? GML_EDGE_FAM_NONE : edge_plan_bwd(S, Sout, split, gin, sym, arith == EDGE_EXACT);
    return GML_EDGE_FAM_NONE;
}

// dst[j] = sum_w partial[w][j] in a fixed order: 16 lanes split the partial index, LDS tree in fixed order
__global__ __launch_bounds__(256) void gml_k_reduce_partials(const float* __restrict__ partial, int64_t nwaves, int nw,
                                                            float* __restrict__ d0, int n0, float* __restrict__ d1, int n1,
                                                            float* __restrict__ d2, int n2, float* __restrict__ d3, int n3) {
    __shared__ float red[16][17];
    const int jl = threadIdx.x & 15, wl = threadIdx.x >> 4;
    const int j = blockIdx.x * 16 + jl;
    float a = 0.f;
    if (j < nw) a = gml_fold_column(partial, nwaves, nw, j, wl);
    red[wl][jl] = a;
    __syncthreads();
    if (wl == 0 && j < nw) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[k][jl];
        if (j < n0) d0[j] = t;
        else if (j < n0 + n1) d1[j - n0] = t;
        else if (j < n0 + n1 + n2) d2[j - n0 - n1] = t;
        else if (j < n0 + n1 + n2 + n3) d3[j - n0 - n1 - n2] = t;
    }
}

// (x0, x1) -> packed bf16 pairs: hi = the values truncated to bf16, lo = their rounded residuals (the split of gml_chain_b1)
__device__ __forceinline__ uint2 gml_presplit_pair(float x0, float x1) {
    const float t0 = __uint_as_float(__float_as_uint(x0) & 0xffff0000u);
    const float t1 = __uint_as_float(__float_as_uint(x1) & 0xffff0000u);
    return uint2{gml_pack2(t0, t1), gml_pack2(x0 - t0, x1 - t1)};
}

// hi[8] | lo[8] bf16 per edge (32 bytes): the layer-1 operand of the matrix-core kernels, made once per batch
// 8 < S <= 16: hi[16] | lo[16] per edge (64 bytes), the operand rows of gml_edge_chain16_impl.h
__global__ __launch_bounds__(256) void gml_k_edge_presplit16(const float* __restrict__ ea, uint32_t* __restrict__ es,
                                                            int64_t E, int S) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    uint32_t hi[8], lo[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float x0 = (2 * j < S) ? ea[e * S + 2 * j] : 0.f, x1 = (2 * j + 1 < S) ? ea[e * S + 2 * j + 1] : 0.f;
        const uint2 p = gml_presplit_pair(x0, x1);
        hi[j] = p.x;
        lo[j] = p.y;
    }
    u32x4* o = reinterpret_cast<u32x4*>(es + e * 16);
    o[0] = u32x4{hi[0], hi[1], hi[2], hi[3]};
    o[1] = u32x4{hi[4], hi[5], hi[6], hi[7]};
    o[2] = u32x4{lo[0], lo[1], lo[2], lo[3]};
    o[3] = u32x4{lo[4], lo[5], lo[6], lo[7]};
}

__global__ __launch_bounds__(256) void gml_k_edge_presplit(const float* __restrict__ ea, uint32_t* __restrict__ es,
                                                          int64_t E, int S) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    uint32_t hi[4], lo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float x0 = (2 * j < S) ? ea[e * S + 2 * j] : 0.f, x1 = (2 * j + 1 < S) ? ea[e * S + 2 * j + 1] : 0.f;
        const uint2 p = gml_presplit_pair(x0, x1);
        hi[j] = p.x;
        lo[j] = p.y;
    }
    u32x4* o = reinterpret_cast<u32x4*>(es + e * 8);
    o[0] = u32x4{hi[0], hi[1], hi[2], hi[3]};
    o[1] = u32x4{lo[0], lo[1], lo[2], lo[3]};
}

// the same with the row gather of the value sort in front: out[k] = in[perm[k]] and its pre-split in ONE pass (a fresh
// batch otherwise reads and writes the supports twice: gml_gather_rows, then gml_edge_presplit)
__global__ __launch_bounds__(256) void gml_k_gather_presplit(const float* __restrict__ in, const int32_t* __restrict__ perm,
                                                            float* __restrict__ out, uint32_t* __restrict__ es,
                                                            int64_t E, int S) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const float* src = in + (int64_t)perm[e] * S;
    float x[8];
    if (S == 8) {
        const f32x4 a = reinterpret_cast<const f32x4*>(src)[0], b = reinterpret_cast<const f32x4*>(src)[1];
        x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
        reinterpret_cast<f32x4*>(out + e * 8)[0] = a;
        reinterpret_cast<f32x4*>(out + e * 8)[1] = b;
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            x[j] = (j < S) ? src[j] : 0.f;
            if (j < S) out[e * S + j] = x[j];
        }
    }
    uint32_t hi[4], lo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint2 p = gml_presplit_pair(x[2 * j], x[2 * j + 1]);
        hi[j] = p.x;
        lo[j] = p.y;
    }
    u32x4* o = reinterpret_cast<u32x4*>(es + e * 8);
    o[0] = u32x4{hi[0], hi[1], hi[2], hi[3]};
    o[1] = u32x4{lo[0], lo[1], lo[2], lo[3]};
}

extern "C" int gml_gather_rows_presplit(const float* in, const int32_t* perm, float* out, void* out_split, int64_t rows,
                                        int32_t S, gml_stream_t stream) {
    if (rows < 0 || S <= 0) return GML_E_BADARG;
    if (S > 8) return GML_E_UNSUPPORTED;
    if (rows == 0) return GML_OK;
    if (!in || !perm || !out || !out_split) return GML_E_BADARG;
    if ((((uintptr_t)out_split) & 15) != 0 || (S == 8 && ((((uintptr_t)in) | ((uintptr_t)out)) & 15) != 0)) return GML_E_BADARG;
    hipLaunchKernelGGL(gml_k_gather_presplit, dim3((unsigned)gml_cdiv(rows, 256)), dim3(256), 0, (hipStream_t)stream, in, perm,
                       out, (uint32_t*)out_split, rows, S);
    return gml_launch_status();
}

extern "C" int gml_edge_presplit(const float* ea, void* ea_split, int64_t num_edges, int32_t S, gml_stream_t stream) {
    if (num_edges < 0 || S <= 0) return GML_E_BADARG;
    if (S > 16) return GML_E_UNSUPPORTED;
    if (num_edges == 0) return GML_OK;
    if (!ea || !ea_split || (((uintptr_t)ea_split) & 15) != 0) return GML_E_BADARG;
    if (S > 8) {
        hipLaunchKernelGGL(gml_k_edge_presplit16, dim3((unsigned)gml_cdiv(num_edges, 256)), dim3(256), 0, (hipStream_t)stream,
                           ea, (uint32_t*)ea_split, num_edges, S);
        return gml_launch_status();
    }
    hipLaunchKernelGGL(gml_k_edge_presplit, dim3((unsigned)gml_cdiv(num_edges, 256)), dim3(256), 0, (hipStream_t)stream, ea,
                       (uint32_t*)ea_split, num_edges, S);
    return gml_launch_status();
}

extern "C" int gml_edge_mlp_fwd(const float* ea, const void* ea_split, const float* w1, const float* w2, const float* w3,
                                const float* w4, float* out, const int32_t* tpos, float* out_t,
                                int64_t num_edges, int32_t S, int32_t Sout, gml_stream_t stream) {
    if (num_edges < 0 || S <= 0 || Sout <= 0) return GML_E_BADARG;
    if (num_edges == 0) return GML_OK;
    if (!ea || !w1 || !w2 || !w3 || !w4 || !out) return GML_E_BADARG;
    if (S != Sout) return GML_E_UNSUPPORTED;   // every reference script uses nedgeoutput == nedgeinput
    if ((((uintptr_t)ea | (uintptr_t)out | (uintptr_t)out_t | (uintptr_t)ea_split) & 15) != 0) return GML_E_BADARG;
    if (out_t && !tpos) return GML_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t* es = (const uint32_t*)ea_split;
#define GML_CASE_CF(SV) case SV: return gml_launch_edge_chain_fwd<SV>(ea, es, w1, w2, w3, w4, out, tpos, out_t, num_edges, st);
#define GML_CASE_CF16(SV) case SV: return gml_launch_edge_chain16_fwd<SV>(es, w1, w2, w3, w4, out, tpos, out_t, num_edges, st);
#define GML_CASE_F(SV) case SV: return gml_launch_edge_mlp_fwd<SV, SV>(ea, w1, w2, w3, w4, out, tpos, out_t, num_edges, st);
    switch (edge_plan_fwd(S, Sout, 0, EDGE_TWO_PIECE, es != nullptr, out_t != nullptr, false)) {
        case GML_EDGE_FAM_CHAIN:
            // the second (source-order) copy is scattered through one buffer descriptor: 32-bit byte offsets
            if (out_t && !edge_plan_offsets_fit(num_edges, S, 0xffffff00ull)) return GML_E_UNSUPPORTED;
            switch (S) { GML_ECHAIN_S(GML_CASE_CF) }
            break;
        case GML_EDGE_FAM_CHAIN16: switch (S) { GML_ECHAIN16_S(GML_CASE_CF16) } break;
        case GML_EDGE_FAM_VALU: switch (S) { GML_EMLP_S(GML_CASE_F) } break;
    }
    return GML_E_UNSUPPORTED;
}

// the same on the exact-arithmetic family whatever the shape (one edge per lane, fp32 FMAs, f32-input MFMA for the weight gradients, the
// library's tanh): what GML_F32_MFMA is to the conv kernels.  The matrix-core chains split their operands into bf16 pairs and use a
// short tanh (~2e-7 absolute): 5e-7 rms on the learned supports where this family -- like torch's fp32 on the CPU -- carries ~1e-8.
extern "C" int gml_edge_mlp_fwd_exact(const float* ea, const float* w1, const float* w2, const float* w3, const float* w4, float* out,
                                      const int32_t* tpos, float* out_t, int64_t num_edges, int32_t S, int32_t Sout, gml_stream_t stream) {
    if (num_edges < 0 || S <= 0 || Sout <= 0) return GML_E_BADARG;
    if (num_edges == 0) return GML_OK;
    if (!ea || !w1 || !w2 || !w3 || !w4 || !out) return GML_E_BADARG;
    if (S != Sout) return GML_E_UNSUPPORTED;
    if ((((uintptr_t)ea | (uintptr_t)out | (uintptr_t)out_t) & 15) != 0) return GML_E_BADARG;
    if (out_t && !tpos) return GML_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (edge_plan_fwd(S, Sout, 0, EDGE_EXACT, false, out_t != nullptr, false) == GML_EDGE_FAM_VALU) switch (S) { GML_EMLP_S(GML_CASE_F) }
    return GML_E_UNSUPPORTED;
}

// every family the shape can take is covered, so the size does not depend on the call's pointers or on the environment (the S <= 8
// chain is counted at 8 workgroups per CU, above the 6 it launches: the size callers have always been given)
extern "C" size_t gml_edge_mlp_bwd_workspace_bytes(int64_t num_edges, int32_t S, int32_t Sout) {
    if (num_edges <= 0 || S <= 0 || Sout != S) return 0;
    int64_t parts = edge_plan_bwd_parts(GML_EDGE_FAM_VALU, num_edges, S);
    if (S <= 8 && gml_edge_chain_bwd_groups(num_edges, 8) > parts) parts = gml_edge_chain_bwd_groups(num_edges, 8);
    if (S > 8 && S <= 16 && gml_edge_chain16_bwd_groups(num_edges) > parts) parts = gml_edge_chain16_bwd_groups(num_edges);
    return (size_t)parts * (size_t)(6 * S * S + Sout * 4 * S) * sizeof(float);
}

// partial rows gml_edge_mlp_bwd leaves in ws for this call shape (a shape it refuses: the VALU family's count)
extern "C" int64_t gml_edge_mlp_bwd_parts(int64_t num_edges, int32_t S, int32_t Sout, int32_t has_split, int32_t want_gin) {
    if (num_edges <= 0 || S <= 0 || Sout != S) return 0;
    const int fam = edge_plan_bwd(S, Sout, has_split != 0, want_gin != 0, false, false);
    return edge_plan_bwd_parts(fam == GML_EDGE_FAM_NONE ? GML_EDGE_FAM_VALU : fam, num_edges, S);
}

extern "C" int gml_edge_mlp_bwd(const float* ea, const void* ea_split, const float* w1, const float* w2, const float* w3,
                                const float* w4, const float* gout, float* gin, float* dw1, float* dw2,
                                float* dw3, float* dw4, int64_t num_edges, int32_t S, int32_t Sout,
                                void* ws, size_t ws_bytes, gml_stream_t stream) {
    if (num_edges < 0 || S <= 0 || Sout <= 0) return GML_E_BADARG;
    const bool nofold = !dw1 && !dw2 && !dw3 && !dw4;        /* all four NULL: the partials stay in ws (gml_fold_many, gml_edge_mlp_bwd_parts) */
    if (!w1 || !w2 || !w3 || !w4 || (!nofold && (!dw1 || !dw2 || !dw3 || !dw4))) return GML_E_BADARG;
    if (S != Sout) return GML_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (num_edges == 0) {
        if (nofold) return GML_OK;                           /* (gml_edge_mlp_bwd_parts is 0: the fold writes zeros) */
        return gml_edge_zero_dw(dw1, dw2, dw3, dw4, S, Sout, st);
    }
    if (!ea || !gout || !ws) return GML_E_BADARG;
    if ((((uintptr_t)ea | (uintptr_t)gout | (uintptr_t)gin | (uintptr_t)ea_split) & 15) != 0) return GML_E_BADARG;
    const uint32_t* es = (const uint32_t*)ea_split;
#define GML_CASE_CB(SV) \
    case SV: return gml_launch_edge_chain_bwd<SV>(ea, es, w1, w2, w3, w4, gout, gin, dw1, dw2, dw3, dw4, num_edges, ws, ws_bytes, st);
#define GML_CASE_CB16(SV) \
    case SV: return gml_launch_edge_chain16_bwd<SV>(es, w1, w2, w3, w4, gout, dw1, dw2, dw3, dw4, num_edges, ws, ws_bytes, st);
#define GML_CASE_B(SV) \
    case SV: return gml_launch_edge_mlp_bwd<SV, SV>(ea, w1, w2, w3, w4, gout, gin, dw1, dw2, dw3, dw4, num_edges, ws, ws_bytes, st);
    switch (edge_plan_bwd(S, Sout, es != nullptr, gin != nullptr, false, false)) {
        case GML_EDGE_FAM_CHAIN: switch (S) { GML_ECHAIN_S(GML_CASE_CB) } break;
        case GML_EDGE_FAM_CHAIN16: switch (S) { GML_ECHAIN16_S(GML_CASE_CB16) } break;
        case GML_EDGE_FAM_VALU: switch (S) { GML_EMLP_S(GML_CASE_B) } break;
    }
    return GML_E_UNSUPPORTED;
}

// gml_edge_mlp_bwd on the exact-arithmetic family (see gml_edge_mlp_fwd_exact); dw1 .. dw4 are required (no deferred fold);
// ws: gml_edge_mlp_bwd_workspace_bytes (it covers both families)
extern "C" int gml_edge_mlp_bwd_exact(const float* ea, const float* w1, const float* w2, const float* w3, const float* w4,
                                      const float* gout, float* gin, float* dw1, float* dw2, float* dw3, float* dw4,
                                      int64_t num_edges, int32_t S, int32_t Sout, void* ws, size_t ws_bytes, gml_stream_t stream) {
    if (num_edges < 0 || S <= 0 || Sout <= 0) return GML_E_BADARG;
    if (!w1 || !w2 || !w3 || !w4 || !dw1 || !dw2 || !dw3 || !dw4) return GML_E_BADARG;
    if (S != Sout) return GML_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (num_edges == 0) {
        return gml_edge_zero_dw(dw1, dw2, dw3, dw4, S, Sout, st);
    }
    if (!ea || !gout || !ws) return GML_E_BADARG;
    if ((((uintptr_t)ea | (uintptr_t)gout | (uintptr_t)gin) & 15) != 0) return GML_E_BADARG;
    if (edge_plan_bwd(S, Sout, false, gin != nullptr, false, true) == GML_EDGE_FAM_VALU) switch (S) { GML_EMLP_S(GML_CASE_B) }
    return GML_E_UNSUPPORTED;
}
