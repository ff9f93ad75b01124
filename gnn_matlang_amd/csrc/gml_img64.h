// What the layers of widths up to 64 share (gml_gin.hip, gml_cheb.hip): a weight matrix as a zero-padded [64][64] fp32 image in the LDS,
// tiles of 32 rows (8 per wave of a 256-thread workgroup) and the product of a wave's 8 rows with an image, plain fmaf in one order.
#ifndef GML_IMG64_H_
#define GML_IMG64_H_
#include "gml_common.h"

#define GML_I64_W 64        // the widest layer; the row length of every LDS image and tile
#define GML_I64_TR 32       // rows of a tile (8 per wave)
#define GML_I64_RPW 8

// act 0 none / 1 relu / 2 tanh
static __device__ __forceinline__ float gml_i64_act(float v, int act) {
    if (act == 1) return fmaxf(v, 0.f);
    if (act == 2) return tanhf(v);
    return v;
}
// act'(pre-activation) as a function of y = act(pre-activation)
static __device__ __forceinline__ float gml_i64_dact(float y, int act) {
    if (act == 1) return y > 0.f ? 1.f : 0.f;
    if (act == 2) return 1.f - y * y;
    return 1.f;
}

// acc[r] += sum over k < K4 (ascending) of a[(8 wave + r) 64 + k] w[k 64 + lane]: a = a tile (broadcast reads), w = an image
static __device__ __forceinline__ void gml_i64_prod8(const float* a, const float* w, int K4, int wave, int lane, float (&acc)[GML_I64_RPW]) {
    const float* ar = a + wave * GML_I64_RPW * GML_I64_W;
    for (int k = 0; k < K4; k += 4) {
        const float w0 = w[k * GML_I64_W + lane], w1 = w[(k + 1) * GML_I64_W + lane], w2 = w[(k + 2) * GML_I64_W + lane],
                    w3 = w[(k + 3) * GML_I64_W + lane];
#pragma unroll
        for (int r = 0; r < GML_I64_RPW; ++r) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(ar + r * GML_I64_W + k);
            acc[r] = fmaf(v.w, w3, fmaf(v.z, w2, fmaf(v.y, w1, fmaf(v.x, w0, acc[r]))));
        }
    }
}

// img[a 64 + b] = TRANSPOSE ? w[b ldw + a] : w[a ldw + b] for a < na, b < nb, 0 elsewhere (w: [rows][ldw] row-major, dense)
template <bool TRANSPOSE>
static __device__ __forceinline__ void gml_i64_load_image(float* img, const float* __restrict__ w, int na, int nb, int ldw) {
    for (int e = threadIdx.x; e < GML_I64_W * GML_I64_W; e += 256) {
        const int a = e / GML_I64_W, b = e % GML_I64_W;
        float v = 0.f;
        if (w && a < na && b < nb) v = TRANSPOSE ? w[b * ldw + a] : w[a * ldw + b];
        img[e] = v;
    }
}

#endif  // GML_IMG64_H_
