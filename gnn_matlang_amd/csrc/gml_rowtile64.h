// The 64-wide row-tile plan that the message-passing layers of widths up to 64 share (gml_gin.hip, gml_cheb.hip): a weight matrix as a
// zero-padded [64][64] fp32 image in the LDS, tiles of 32 rows (8 per wave of a 256-thread workgroup), one lane per (row, column) in a
// CSR row walk that loads in chunks of 4, the product of a wave's 8 rows with an image, a 16 x 1 piece of v^T s per thread in a row
// pass, one partial per workgroup and one fold in workgroup order.  Plain fmaf, every sum in one order.  A layer writes its edge
// contribution, the sequence of its kernels and its entry points; DESIGN 4.23 lists what is here.
#ifndef GML_ROWTILE64_H_
#define GML_ROWTILE64_H_
#include "gml_common.h"

#define GML_RT_W 64         // the widest layer; the row length of every LDS image and tile
#define GML_RT_TR 32        // rows of a tile (8 per wave)
#define GML_RT_RPW 8
#define GML_RT_MAXWG 768    // workgroups of a tile-walking launch and of a row pass (3 per CU)

// act 0 none / 1 relu / 2 tanh
static __device__ __forceinline__ float gml_rt_act(float v, int act) {
    if (act == 1) return fmaxf(v, 0.f);
    if (act == 2) return tanhf(v);
    return v;
}
// act'(pre-activation) as a function of y = act(pre-activation)
static __device__ __forceinline__ float gml_rt_dact(float y, int act) {
    if (act == 1) return y > 0.f ? 1.f : 0.f;
    if (act == 2) return 1.f - y * y;
    return 1.f;
}

// acc[r] += sum over k < K4 (ascending) of a[(8 wave + r) 64 + k] w[k 64 + lane]: a = a tile (broadcast reads), w = an image
static __device__ __forceinline__ void gml_rt_prod8(const float* a, const float* w, int K4, int wave, int lane, float (&acc)[GML_RT_RPW]) {
    const float* ar = a + wave * GML_RT_RPW * GML_RT_W;
    for (int k = 0; k < K4; k += 4) {
        const float w0 = w[k * GML_RT_W + lane], w1 = w[(k + 1) * GML_RT_W + lane], w2 = w[(k + 2) * GML_RT_W + lane],
                    w3 = w[(k + 3) * GML_RT_W + lane];
#pragma unroll
        for (int r = 0; r < GML_RT_RPW; ++r) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(ar + r * GML_RT_W + k);
            acc[r] = fmaf(v.w, w3, fmaf(v.z, w2, fmaf(v.y, w1, fmaf(v.x, w0, acc[r]))));
        }
    }
}

// img[a 64 + b] = TRANSPOSE ? w[b ldw + a] : w[a ldw + b] for a < na, b < nb, 0 elsewhere (w: [rows][ldw] row-major, dense)
template <bool TRANSPOSE>
static __device__ __forceinline__ void gml_rt_load_image(float* img, const float* __restrict__ w, int na, int nb, int ldw) {
    for (int e = threadIdx.x; e < GML_RT_W * GML_RT_W; e += 256) {
        const int a = e / GML_RT_W, b = e % GML_RT_W;
        float v = 0.f;
        if (w && a < na && b < nb) v = TRANSPOSE ? w[b * ldw + a] : w[a * ldw + b];
        img[e] = v;
    }
}

// One (row, column) of a sum over a CSR row, from acc, the edges in CSR order: 4 column loads, 4 guarded row loads, 4 accumulations,
// then the tail.  Column indices outside [0, N) are skipped.  What an edge to column index j contributes is the layer's Edge:
//   bool keep(int64_t j)  float weight(int64_t j)  float add(float acc, float w, float v)     (v = src[j][c]; the self term: the caller's)
template <class Edge>
static __device__ __forceinline__ float gml_rt_walk(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* src,
                                                    int64_t ld, int64_t row, int c, int64_t N, float acc, const Edge& e) {
    const int k0 = rowptr[row], k1 = rowptr[row + 1];
    int k = k0;
    for (; k + 4 <= k1; k += 4) {
        int64_t j[4];
        float v[4], w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) j[u] = col[k + u];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool on = j[u] >= 0 && j[u] < N && e.keep(j[u]);
            v[u] = on ? src[j[u] * ld + c] : 0.f;
            w[u] = on ? e.weight(j[u]) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = e.add(acc, w[u], v[u]);
    }
    for (; k < k1; ++k) {
        const int64_t j = col[k];
        if (j >= 0 && j < N && e.keep(j)) acc = e.add(acc, e.weight(j), src[j * ld + c]);
    }
    return acc;
}

// The gather pass of a wave over its 8 rows of a tile, one lane per (row, column), 64 / gp rows at once (gp = gml_rt_gp(F)):
// tile[(8 wave + r) 64 + c] = value(row, c) for row < N and c < F, 0 elsewhere.  value() also stores what the layer keeps in global memory.
// on: whether this launch gathers at all (uniform; joined with the lane's own condition into one branch, not a branch of the caller's)
template <class Value>
static __device__ __forceinline__ void gml_rt_gather_rows(float* tile, int64_t r0, int64_t N, int F, int gp, int wave, int lane, bool on, Value value) {
    const int rpp = 64 / gp < GML_RT_RPW ? 64 / gp : GML_RT_RPW;            // rows of one gather pass
    const int sub = lane / gp, c = lane % gp;
    if (!on || sub >= rpp) return;
    for (int p = 0; p < GML_RT_RPW; p += rpp) {
        const int64_t row = r0 + p + sub;
        float v = 0.f;
        if (row < N && c < F) v = value(row, c);
        tile[(wave * GML_RT_RPW + p + sub) * GML_RT_W + c] = v;
    }
}

// the rows of a wave, lane = column: tile[(8 wave + r) 64 + lane] = src[row][lane] (0 beyond N and F)
static __device__ __forceinline__ void gml_rt_load_rows(float* tile, const float* src, int64_t ld, int64_t r0, int64_t N, int F, int wave, int lane) {
#pragma unroll
    for (int r = 0; r < GML_RT_RPW; ++r) {
        const int64_t row = r0 + r;
        tile[(wave * GML_RT_RPW + r) * GML_RT_W + lane] = (row < N && lane < F) ? src[row * ld + lane] : 0.f;
    }
}

// the same for g = dy act'(y)
static __device__ __forceinline__ void gml_rt_load_g(float* tile, const float* __restrict__ dy, int64_t lddy, const float* __restrict__ y,
                                                     int64_t ldy, int64_t r0, int64_t N, int F, int act, int wave, int lane) {
#pragma unroll
    for (int r = 0; r < GML_RT_RPW; ++r) {
        const int64_t row = r0 + r;
        float g = 0.f;
        if (row < N && lane < F) g = dy[row * lddy + lane] * gml_rt_dact(y[row * ldy + lane], act);
        tile[(wave * GML_RT_RPW + r) * GML_RT_W + lane] = g;
    }
}

// acc[u] = fmaf(v[r][16 wave + u], s[r][lane], acc[u]) over the 32 rows of the tiles v and s, ascending: a 16 x 1 piece of v^T s
static __device__ __forceinline__ void gml_rt_outer16(const float* v, const float* s, int wave, int lane, float (&acc)[16]) {
#pragma unroll 2
    for (int r = 0; r < GML_RT_TR; ++r) {
        const float b = s[r * GML_RT_W + lane];
#pragma unroll
        for (int u = 0; u < 16; u += 4) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(v + r * GML_RT_W + wave * 16 + u);
            acc[u] = fmaf(a.x, b, acc[u]); acc[u + 1] = fmaf(a.y, b, acc[u + 1]);
            acc[u + 2] = fmaf(a.z, b, acc[u + 2]); acc[u + 3] = fmaf(a.w, b, acc[u + 3]);
        }
    }
}

// acc += tile[r][lane] over the 32 rows, ascending
static __device__ __forceinline__ void gml_rt_colsum(const float* tile, int lane, float& acc) {
#pragma unroll 4
    for (int r = 0; r < GML_RT_TR; ++r) acc += tile[r * GML_RT_W + lane];
}

// dflat = the sum of the row pass's partials, workgroups in ascending order
static __global__ void gml_rt_k_fold(const float* __restrict__ part, int nwg, int64_t P, float* __restrict__ dflat) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= P) return;
    float s = 0.f;
    for (int w = 0; w < nwg; ++w) s += part[(int64_t)w * P + e];
    dflat[e] = s;
}

// ---------------------------------------------------------------------------------------------------------------- host
static inline int gml_rt_gp(int Fin) {                                       // max(4, pow2(Fin)): the lanes of one row of a gather pass
    int g = 4;
    while (g < Fin) g *= 2;
    return g;
}
static inline int64_t gml_rt_tiles(int64_t N) { return gml_cdiv(N, GML_RT_TR); }
static inline unsigned gml_rt_grid(int64_t N) {                              // a launch whose workgroups walk tile = block, block + grid, ...
    const int64_t nt = gml_rt_tiles(N);
    return (unsigned)(nt < GML_RT_MAXWG ? nt : GML_RT_MAXWG);
}
static inline void gml_rt_row_plan(int64_t N, int64_t* tpw, int* nwg) {     // a row pass: workgroup w owns the tiles [w tpw, (w + 1) tpw)
    const int64_t nt = gml_rt_tiles(N);
    *tpw = gml_cdiv(nt, GML_RT_MAXWG);
    *nwg = (int)gml_cdiv(nt, *tpw);
}
static inline bool gml_rt_range(int64_t N, int64_t E) { return N <= 0x7fffffff && E <= 0x7fffffff; }
static inline void gml_rt_fold(const float* part, int nwg, int64_t P, float* dflat, hipStream_t st) {
    hipLaunchKernelGGL(gml_rt_k_fold, dim3((unsigned)gml_cdiv(P, 256)), dim3(256), 0, st, part, nwg, P, dflat);
}

#endif  // GML_ROWTILE64_H_
