// The pieces every GNNML1 block kernel shares (gml_gnnml1_impl.h: modes 0 .. 3 and 5; gml_gnnml1_sum.hip: the sum-and-factors form): the
// kernel parameters, the activation, and 4-column accesses of a row that take a 16-byte path where stride and base allow it and a
// scalar path otherwise.
#pragma once
#include "gml_common.h"

struct GmlG1Params {
    const int32_t* rowptr; const int32_t* col; const float* val;      // fwd: target-keyed CSR; bwd: source-keyed (rowptr_t, col_t, val_t)
    const float* x; int64_t ldx;
    const float* w1; const float* b1; const float* wc; const float* bc;
    const float* w2; const float* b2; const float* w3; const float* b3;
    float* out; int64_t ldo;                                             // fwd: written; bwd: the saved output (read)
    const float* gout; int64_t ldgo;
    float* dx; int64_t lddx; float* g4; int64_t ldg4; float* q; int64_t ldq;
    int64_t nrows; int32_t Fin, n1, n2, n3, mode, act, ntiles;
};


#define G1_NW 8

__device__ __forceinline__ float g1_act(float v, int act) { return act == 0 ? gml_tanh(v) : fmaxf(v, 0.f); }
// derivative of the activation from its OUTPUT value (tanh: 1 - y^2; relu: y > 0)
__device__ __forceinline__ float g1_dact_out(float y, int act) { return act == 0 ? fmaf(-y, y, 1.f) : (y > 0.f ? 1.f : 0.f); }


__device__ __forceinline__ f32x4 g1_bias4(const float* b, int c0, int n) {
    f32x4 r;
#pragma unroll
    for (int u = 0; u < 4; ++u) r[u] = (b && c0 + u < n) ? b[c0 + u] : 0.f;
    return r;
}

__device__ __forceinline__ void g1_store4(float* base, int64_t ld, int64_t row, int c0, int n, bool valid, f32x4 v) {
    if (!valid) return;
    float* p = base + row * ld + c0;
    if (c0 + 4 <= n && ld % 4 == 0 && ((reinterpret_cast<uintptr_t>(p) & 15) == 0)) { *reinterpret_cast<f32x4*>(p) = v; return; }
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (c0 + u < n) p[u] = v[u];
}

__device__ __forceinline__ f32x4 g1_load4(const float* base, int64_t ld, int64_t row, int c0, int n, bool valid) {
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!valid) return v;
    const float* p = base + row * ld + c0;
    if (c0 + 4 <= n && ld % 4 == 0 && ((reinterpret_cast<uintptr_t>(p) & 15) == 0)) return *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (c0 + u < n) v[u] = p[u];
    return v;
}
