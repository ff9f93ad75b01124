// PPGN (Maron et al., "Provably powerful graph networks") on dense [B, C, nmax, nmax] tensors: the input tensors of a batch and one
// block forward / backward (include/gml.h: gml_ppgn_*).  Channel-major planes, P = nmax * nmax pixels per plane, pixel (i, j) of graph
// g is real where i < n_g and j < n_g.  Exact fp32 everywhere: the 1x1 channel mixes and the per-channel n x n products are chains of
// fmaf in ascending index order; the weight gradients run on the f32-input matrix instruction (16x16x4), itself a k-ordered fmaf chain.
//
//   forward   A  a12 = relu(m (W12 x + b12))                 one workgroup per (graph, 8 of the 2C stacked output channels)
//             B  p_c = a1_c @ a2_c                           one workgroup per (graph, channel): both planes in LDS, loops to n_g
//             C  y = relu(m (W3 [p ; x] + b3)), readout      one workgroup per (graph, 8 output channels): the readout sums of its
//                                                            channels are complete inside the workgroup (no atomics, fixed order)
//   backward  C' dz3 = (dy + readout gradient) [y > 0],  dp = W3p^T dz3
//             B' dz1 = (dp_c @ a2_c^T) [a1 > 0],  dz2 = (a1_c^T @ dp_c) [a2 > 0]
//             X  dx = W3x^T dz3 + W1^T dz1 + W2^T dz2       (only when asked for; zero in the padding)
//             W  per-workgroup partials of dz3 [p ; x ; 1]^T and dz12 [x ; 1]^T over 32-pixel chunks, then one ordered fold
// Only real pixels are computed; the padding of y and dx is written as zeros, the internal tensors (a12, p, dz*) are never read there.
#include "gml_common.h"

#define PP_CB 8            // output channels of one workgroup of the channel mixes
#define PP_CHUNK 32        // pixels of one staged chunk of the weight-gradient kernel
#define PP_LD 36           // its LDS row stride: 36 r + k (r < 16, k < 4) hits 64 different banks
#define PP_MAXT 10         // 16 x 16 tiles of one wave of it (at most 40 tiles over 4 waves)
#define PP_MAXWG 256       // partials of it

static __device__ __forceinline__ int pp_nodes(const int32_t* __restrict__ n, int64_t g, int nmax) {
    const int v = n[g];
    return v < 0 ? 0 : (v > nmax ? nmax : v);
}

// acc[u] += w[k][u] * src[k * plane], k ascending
static __device__ __forceinline__ void pp_acc(float (&acc)[PP_CB], const float* __restrict__ src, int K, int64_t plane, const float* wS) {
    for (int k = 0; k < K; ++k) {
        const float v = src[(int64_t)k * plane];
        const f32x4 wa = *reinterpret_cast<const f32x4*>(wS + k * PP_CB), wb = *reinterpret_cast<const f32x4*>(wS + k * PP_CB + 4);
        acc[0] = fmaf(wa.x, v, acc[0]); acc[1] = fmaf(wa.y, v, acc[1]); acc[2] = fmaf(wa.z, v, acc[2]); acc[3] = fmaf(wa.w, v, acc[3]);
        acc[4] = fmaf(wb.x, v, acc[4]); acc[5] = fmaf(wb.y, v, acc[5]); acc[6] = fmaf(wb.z, v, acc[6]); acc[7] = fmaf(wb.w, v, acc[7]);
    }
}

// ---------------------------------------------------------------------------------------------------------------- inputs
// one thread per node and per edge; X2 and M arrive zero filled.  Every store writes its own element or the same value.
static __global__ void ppgn_k_inputs(const float* __restrict__ x, int64_t ldx, int nfeat, const int64_t* __restrict__ src,
                                     const int64_t* __restrict__ dst, int64_t E, const int32_t* __restrict__ ptr,
                                     const int64_t* __restrict__ batch, int64_t N, int64_t B, int nmax, float* __restrict__ X2,
                                     float* __restrict__ M, int32_t* __restrict__ nout) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t P = (int64_t)nmax * nmax;
    if (t < B) nout[t] = ptr[t + 1] - ptr[t];
    if (t < N) {
        const int64_t g = batch[t];
        if (g >= 0 && g < B) {
            const int64_t i = t - ptr[g];
            const int64_t ng = ptr[g + 1] - ptr[g];
            if (i >= 0 && i < nmax && ng <= nmax) {
                float* X = X2 + g * (nfeat + 2) * P + i * nmax + i;
                X[P] = 1.f;
                for (int f = 0; f < nfeat; ++f) X[(2 + f) * P] = x[t * ldx + f];
                float* Mg = M + g * 2 * P;
                Mg[i * nmax + i] = 1.f;
                for (int64_t j = 0; j < ng; ++j)
                    if (j != i) Mg[P + i * nmax + j] = 1.f;
            }
        }
    }
    if (t < E) {
        const int64_t s = src[t], d = dst[t];
        if (s >= 0 && s < N && d >= 0 && d < N) {
            const int64_t g = batch[s];
            if (g >= 0 && g < B) {
                const int64_t i = s - ptr[g], j = d - ptr[g];
                const int64_t ng = ptr[g + 1] - ptr[g];
                if (ng <= nmax && i >= 0 && i < ng && j >= 0 && j < ng) X2[g * (nfeat + 2) * P + i * nmax + j] = 1.f;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- forward
// a12[g, o, pix] = relu(sum_k W12[o, k] x[g, k, pix] + b12[o]) on the real pixels, o < 2C (rows of w1, then rows of w2)
static __global__ void ppgn_k_fwd_a(const float* __restrict__ x, const int32_t* __restrict__ n, int nmax, int Cin, int C,
                                    const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                    const float* __restrict__ b2, float* __restrict__ a12, int nblk) {
    __shared__ __attribute__((aligned(16))) float wS[64 * PP_CB];
    __shared__ float bS[PP_CB];
    const int64_t g = blockIdx.x / nblk;
    const int o0 = (int)(blockIdx.x % nblk) * PP_CB, C2 = 2 * C;
    const int ng = pp_nodes(n, g, nmax);
    const int64_t P = (int64_t)nmax * nmax;
    for (int t = threadIdx.x; t < Cin * PP_CB; t += blockDim.x) {
        const int k = t / PP_CB, o = o0 + t % PP_CB;
        wS[t] = o < C ? w1[o * Cin + k] : (o < C2 ? w2[(o - C) * Cin + k] : 0.f);
    }
    if (threadIdx.x < PP_CB) {
        const int o = o0 + threadIdx.x;
        bS[threadIdx.x] = o < C ? (b1 ? b1[o] : 0.f) : (o < C2 ? (b2 ? b2[o - C] : 0.f) : 0.f);
    }
    __syncthreads();
    const float* xg = x + g * Cin * P;
    float* ag = a12 + g * C2 * P;
    for (int q = threadIdx.x; q < ng * ng; q += blockDim.x) {
        const int64_t pix = (int64_t)(q / ng) * nmax + q % ng;
        float acc[PP_CB];
#pragma unroll
        for (int u = 0; u < PP_CB; ++u) acc[u] = bS[u];
        pp_acc(acc, xg + pix, Cin, P, wS);
#pragma unroll
        for (int u = 0; u < PP_CB; ++u)
            if (o0 + u < C2) ag[(int64_t)(o0 + u) * P + pix] = fmaxf(acc[u], 0.f);
    }
}

// out(r, c) = sum_s L[r lr + s ls] * R[s rs + c rc], r, c, s < ng, s ascending; four rows per thread, lanes along c
template <class Store>
static __device__ __forceinline__ void pp_mm(const float* L, int lr, int ls, const float* R, int rs, int rc, int ng, Store store) {
    const int nrb = (ng + 3) / 4;
    for (int t = threadIdx.x; t < nrb * ng; t += blockDim.x) {
        const int r0 = (t / ng) * 4, c = t % ng;
        const int ra = min(r0, ng - 1) * lr, rb = min(r0 + 1, ng - 1) * lr, rc2 = min(r0 + 2, ng - 1) * lr, rd = min(r0 + 3, ng - 1) * lr;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        const float* Rc = R + c * rc;
        for (int s = 0; s < ng; ++s) {
            const float v = Rc[s * rs];
            a0 = fmaf(L[ra + s * ls], v, a0);
            a1 = fmaf(L[rb + s * ls], v, a1);
            a2 = fmaf(L[rc2 + s * ls], v, a2);
            a3 = fmaf(L[rd + s * ls], v, a3);
        }
        store(r0, c, a0);
        if (r0 + 1 < ng) store(r0 + 1, c, a1);
        if (r0 + 2 < ng) store(r0 + 2, c, a2);
        if (r0 + 3 < ng) store(r0 + 3, c, a3);
    }
}

// the real n x n corner of a plane -> LDS rows of stride ld
static __device__ __forceinline__ void pp_load_plane(float* S, int ld, const float* __restrict__ plane, int nmax, int ng) {
    for (int q = threadIdx.x; q < ng * ng; q += blockDim.x) {
        const int i = q / ng, j = q % ng;
        S[i * ld + j] = plane[(int64_t)i * nmax + j];
    }
}

// p[g, c] = a1[g, c] @ a2[g, c] on the real corner
static __global__ void ppgn_k_fwd_mm(const float* __restrict__ a12, const int32_t* __restrict__ n, int nmax, int C, float* __restrict__ p) {
    extern __shared__ float lds[];
    const int64_t g = blockIdx.x / C;
    const int c = (int)(blockIdx.x % C);
    const int ng = pp_nodes(n, g, nmax);
    const int ld = nmax | 1;
    const int64_t P = (int64_t)nmax * nmax;
    float* A1 = lds;
    float* A2 = lds + nmax * ld;
    pp_load_plane(A1, ld, a12 + (g * 2 * C + c) * P, nmax, ng);
    pp_load_plane(A2, ld, a12 + (g * 2 * C + C + c) * P, nmax, ng);
    __syncthreads();
    float* out = p + (g * C + c) * P;
    pp_mm(A1, ld, 1, A2, ld, 1, ng, [&](int i, int j, float v) { out[(int64_t)i * nmax + j] = v; });
}

// y[g, o] = relu(m (W3 [p ; x] + b3)) with zeros in the padding, and the readout of these channels
static __global__ void ppgn_k_fwd_c(const float* __restrict__ p, const float* __restrict__ x, const int32_t* __restrict__ n, int nmax,
                                    int Cin, int C, const float* __restrict__ w3, const float* __restrict__ b3, int readout,
                                    float* __restrict__ y, float* __restrict__ r, int nblk) {
    __shared__ __attribute__((aligned(16))) float wS[128 * PP_CB];
    __shared__ float bS[PP_CB];
    __shared__ float red[4][2 * PP_CB];
    const int64_t g = blockIdx.x / nblk;
    const int o0 = (int)(blockIdx.x % nblk) * PP_CB, K = C + Cin;
    const int ng = pp_nodes(n, g, nmax);
    const int64_t P = (int64_t)nmax * nmax;
    for (int t = threadIdx.x; t < K * PP_CB; t += blockDim.x) {
        const int k = t / PP_CB, o = o0 + t % PP_CB;
        wS[t] = o < C ? w3[o * K + k] : 0.f;
    }
    if (threadIdx.x < PP_CB) bS[threadIdx.x] = (b3 && o0 + (int)threadIdx.x < C) ? b3[o0 + threadIdx.x] : 0.f;
    __syncthreads();
    const float* pg = p + g * C * P;
    const float* xg = x + g * Cin * P;
    float* yg = y + g * C * P;
    float s0[PP_CB], s1[PP_CB];
#pragma unroll
    for (int u = 0; u < PP_CB; ++u) s0[u] = s1[u] = 0.f;
    for (int pix = threadIdx.x; pix < (int)P; pix += blockDim.x) {
        const int i = pix / nmax, j = pix % nmax;
        float acc[PP_CB];
        if (i < ng && j < ng) {
#pragma unroll
            for (int u = 0; u < PP_CB; ++u) acc[u] = bS[u];
            pp_acc(acc, pg + pix, C, P, wS);
            pp_acc(acc, xg + pix, Cin, P, wS + C * PP_CB);
#pragma unroll
            for (int u = 0; u < PP_CB; ++u) {
                acc[u] = fmaxf(acc[u], 0.f);
                if (i == j) s0[u] += acc[u]; else s1[u] += acc[u];
            }
        } else {
#pragma unroll
            for (int u = 0; u < PP_CB; ++u) acc[u] = 0.f;
        }
#pragma unroll
        for (int u = 0; u < PP_CB; ++u)
            if (o0 + u < C) yg[(int64_t)(o0 + u) * P + pix] = acc[u];
    }
    // lanes of a wave by xor butterflies (every lane ends with the same bits), then the waves in ascending order
#pragma unroll
    for (int u = 0; u < PP_CB; ++u)
        for (int d = 32; d >= 1; d >>= 1) {
            s0[u] += __shfl_xor(s0[u], d);
            s1[u] += __shfl_xor(s1[u], d);
        }
    const int wave = threadIdx.x / GML_WAVE, nw = blockDim.x / GML_WAVE;
    if (threadIdx.x % GML_WAVE == 0) {
#pragma unroll
        for (int u = 0; u < PP_CB; ++u) { red[wave][u] = s0[u]; red[wave][PP_CB + u] = s1[u]; }
    }
    __syncthreads();
    if (threadIdx.x < 2 * PP_CB) {
        const int u = threadIdx.x % PP_CB, which = threadIdx.x / PP_CB;
        float s = 0.f;
        for (int w = 0; w < nw; ++w) s += red[w][threadIdx.x];
        if (o0 + u < C) {
            if (readout == 1) s = s / (which == 0 ? (float)ng : (float)(ng * ng - ng));      // n = 1: 0 / 0 off the diagonal, kept
            if (readout == 2) { if (which == 0) r[g * C + o0 + u] = s; }
            else r[g * 2 * C + which * C + o0 + u] = s;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- backward
// dz3[g, co] = (dy + readout gradient) [y > 0];  dp[g, c] = sum_co W3[co, c] dz3[g, co]; this workgroup: 8 channels of both
static __global__ void ppgn_k_bwd_c(const float* __restrict__ y, const float* __restrict__ dy, const float* __restrict__ dr,
                                    const int32_t* __restrict__ n, int nmax, int Cin, int C, const float* __restrict__ w3, int readout,
                                    float* __restrict__ dz3, float* __restrict__ dp, int nblk) {
    __shared__ __attribute__((aligned(16))) float wS[64 * PP_CB];
    __shared__ float d0S[64], d1S[64];
    const int64_t g = blockIdx.x / nblk;
    const int o0 = (int)(blockIdx.x % nblk) * PP_CB, K = C + Cin;
    const int ng = pp_nodes(n, g, nmax);
    const int64_t P = (int64_t)nmax * nmax;
    for (int t = threadIdx.x; t < C * PP_CB; t += blockDim.x) {
        const int co = t / PP_CB, c = o0 + t % PP_CB;
        wS[t] = c < C ? w3[co * K + c] : 0.f;
    }
    for (int co = threadIdx.x; co < C; co += blockDim.x) {
        float d0 = 0.f, d1 = 0.f;
        if (dr) {
            if (readout == 2) d0 = dr[g * C + co];
            else { d0 = dr[g * 2 * C + co]; d1 = dr[g * 2 * C + C + co]; }
            if (readout == 1) { d0 = d0 / (float)ng; d1 = d1 / (float)(ng * ng - ng); }
        }
        d0S[co] = d0; d1S[co] = d1;
    }
    __syncthreads();
    const float* yg = y + g * C * P;
    const float* dyg = dy ? dy + g * C * P : nullptr;
    float* zg = dz3 + g * C * P;
    float* dpg = dp + g * C * P;
    for (int q = threadIdx.x; q < ng * ng; q += blockDim.x) {
        const int i = q / ng, j = q % ng;
        const int64_t pix = (int64_t)i * nmax + j;
        float acc[PP_CB];
#pragma unroll
        for (int u = 0; u < PP_CB; ++u) acc[u] = 0.f;
        for (int co = 0; co < C; ++co) {
            const float yv = yg[(int64_t)co * P + pix];
            const float gv = (dyg ? dyg[(int64_t)co * P + pix] : 0.f) + (i == j ? d0S[co] : d1S[co]);
            const float v = yv > 0.f ? gv : 0.f;
            if (co >= o0 && co < o0 + PP_CB) zg[(int64_t)co * P + pix] = v;
            const f32x4 wa = *reinterpret_cast<const f32x4*>(wS + co * PP_CB), wb = *reinterpret_cast<const f32x4*>(wS + co * PP_CB + 4);
            acc[0] = fmaf(wa.x, v, acc[0]); acc[1] = fmaf(wa.y, v, acc[1]); acc[2] = fmaf(wa.z, v, acc[2]); acc[3] = fmaf(wa.w, v, acc[3]);
            acc[4] = fmaf(wb.x, v, acc[4]); acc[5] = fmaf(wb.y, v, acc[5]); acc[6] = fmaf(wb.z, v, acc[6]); acc[7] = fmaf(wb.w, v, acc[7]);
        }
#pragma unroll
        for (int u = 0; u < PP_CB; ++u)
            if (o0 + u < C) dpg[(int64_t)(o0 + u) * P + pix] = acc[u];
    }
}

// dz12[g, c] = (dp_c @ a2_c^T) [a1_c > 0],  dz12[g, C + c] = (a1_c^T @ dp_c) [a2_c > 0]
static __global__ void ppgn_k_bwd_mm(const float* __restrict__ a12, const float* __restrict__ dp, const int32_t* __restrict__ n, int nmax,
                                     int C, float* __restrict__ dz12) {
    extern __shared__ float lds[];
    const int64_t g = blockIdx.x / C;
    const int c = (int)(blockIdx.x % C);
    const int ng = pp_nodes(n, g, nmax);
    const int ld = nmax | 1;
    const int64_t P = (int64_t)nmax * nmax;
    float* A1 = lds;
    float* A2 = lds + nmax * ld;
    float* DP = lds + 2 * nmax * ld;
    pp_load_plane(A1, ld, a12 + (g * 2 * C + c) * P, nmax, ng);
    pp_load_plane(A2, ld, a12 + (g * 2 * C + C + c) * P, nmax, ng);
    pp_load_plane(DP, ld, dp + (g * C + c) * P, nmax, ng);
    __syncthreads();
    float* z1 = dz12 + (g * 2 * C + c) * P;
    float* z2 = dz12 + (g * 2 * C + C + c) * P;
    // da1[i][k] = sum_j DP[i][j] A2[k][j]
    pp_mm(DP, ld, 1, A2, 1, ld, ng, [&](int i, int k, float v) { z1[(int64_t)i * nmax + k] = A1[i * ld + k] > 0.f ? v : 0.f; });
    // da2[k][j] = sum_i A1[i][k] DP[i][j]
    pp_mm(A1, 1, ld, DP, ld, 1, ng, [&](int k, int j, float v) { z2[(int64_t)k * nmax + j] = A2[k * ld + j] > 0.f ? v : 0.f; });
}

// dx[g, k] = sum_co W3[co, C + k] dz3[co] + W1[co, k] dz1[co] + W2[co, k] dz2[co], zeros in the padding
static __global__ void ppgn_k_bwd_x(const float* __restrict__ dz3, const float* __restrict__ dz12, const int32_t* __restrict__ n,
                                    int nmax, int Cin, int C, const float* __restrict__ w1, const float* __restrict__ w2,
                                    const float* __restrict__ w3, float* __restrict__ dx, int nblk) {
    __shared__ __attribute__((aligned(16))) float wS[192 * PP_CB];
    const int64_t g = blockIdx.x / nblk;
    const int k0 = (int)(blockIdx.x % nblk) * PP_CB, K3 = C + Cin;
    const int ng = pp_nodes(n, g, nmax);
    const int64_t P = (int64_t)nmax * nmax;
    for (int t = threadIdx.x; t < 3 * C * PP_CB; t += blockDim.x) {
        const int s = t / PP_CB, k = k0 + t % PP_CB;
        float w = 0.f;
        if (k < Cin) w = s < C ? w3[s * K3 + C + k] : (s < 2 * C ? w1[(s - C) * Cin + k] : w2[(s - 2 * C) * Cin + k]);
        wS[t] = w;
    }
    __syncthreads();
    const float* z3 = dz3 + g * C * P;
    const float* z12 = dz12 + g * 2 * C * P;
    float* dxg = dx + g * Cin * P;
    for (int pix = threadIdx.x; pix < (int)P; pix += blockDim.x) {
        const int i = pix / nmax, j = pix % nmax;
        float acc[PP_CB];
#pragma unroll
        for (int u = 0; u < PP_CB; ++u) acc[u] = 0.f;
        if (i < ng && j < ng) {
            pp_acc(acc, z3 + pix, C, P, wS);
            pp_acc(acc, z12 + pix, 2 * C, P, wS + C * PP_CB);
        }
#pragma unroll
        for (int u = 0; u < PP_CB; ++u)
            if (k0 + u < Cin) dxg[(int64_t)(k0 + u) * P + pix] = acc[u];
    }
}

// partial[job][wg][row, col] = sum over this workgroup's (graph, 32-pixel chunk) items, in ascending item order, of
//   job 0: dz3[row] * [p ; x ; 1][col]   (C x (C + Cin + 1))        job 1: dz12[row] * [x ; 1][col]   (2C x (Cin + 1))
static __global__ __launch_bounds__(256) void ppgn_k_dw(const float* __restrict__ dz3, const float* __restrict__ dz12,
                                                        const float* __restrict__ p, const float* __restrict__ x,
                                                        const int32_t* __restrict__ n, int64_t B, int nmax, int Cin, int C,
                                                        float* __restrict__ part, int nwg) {
    extern __shared__ float lds[];
    const int job = blockIdx.y, wg = blockIdx.x;
    const int Mr = job == 0 ? C : 2 * C, Nc = job == 0 ? C + Cin + 1 : Cin + 1;
    const int TM = (Mr + 15) / 16, TN = (Nc + 15) / 16, Mp = TM * 16, Np = TN * 16;
    const int64_t P = (int64_t)nmax * nmax;
    const int chunks = (int)((P + PP_CHUNK - 1) / PP_CHUNK);
    const int64_t items = B * chunks;
    float* rowsS = lds;
    float* colsS = lds + Mp * PP_LD;
    const int wave = threadIdx.x / GML_WAVE, lane = threadIdx.x % GML_WAVE;
    const int l16 = lane & 15, l4 = lane >> 4;
    f32x4 acc[PP_MAXT];
#pragma unroll
    for (int t = 0; t < PP_MAXT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int64_t item = wg; item < items; item += nwg) {
        const int64_t g = item / chunks;
        const int chunk = (int)(item % chunks);
        const int ng = pp_nodes(n, g, nmax);
        if (chunk * PP_CHUNK >= ng * ng) continue;                         // (the same answer in every thread of the workgroup)
        const float* rsrc = job == 0 ? dz3 + g * C * P : dz12 + g * 2 * C * P;
        const float* pg = p + g * C * P;
        const float* xg = x + g * Cin * P;
        for (int t = threadIdx.x; t < (Mp + Np) * PP_CHUNK; t += blockDim.x) {
            const int row = t / PP_CHUNK, q = chunk * PP_CHUNK + t % PP_CHUNK;
            float v = 0.f;
            if (q < ng * ng) {
                const int64_t pix = (int64_t)(q / ng) * nmax + q % ng;
                if (row < Mp) {
                    if (row < Mr) v = rsrc[(int64_t)row * P + pix];
                } else {
                    const int cidx = row - Mp;
                    if (job == 0) {
                        if (cidx < C) v = pg[(int64_t)cidx * P + pix];
                        else if (cidx < C + Cin) v = xg[(int64_t)(cidx - C) * P + pix];
                        else if (cidx == C + Cin) v = 1.f;
                    } else {
                        if (cidx < Cin) v = xg[(int64_t)cidx * P + pix];
                        else if (cidx == Cin) v = 1.f;
                    }
                }
            }
            lds[row * PP_LD + t % PP_CHUNK] = v;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < PP_MAXT; ++t) {
            const int tile = wave + 4 * t;
            if (tile < TM * TN) {
                const float* ar = rowsS + ((tile / TN) * 16 + l16) * PP_LD + l4;
                const float* br = colsS + ((tile % TN) * 16 + l16) * PP_LD + l4;
#pragma unroll
                for (int kk = 0; kk < PP_CHUNK / 4; ++kk) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[kk * 4], br[kk * 4], acc[t], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    const int64_t E0 = (int64_t)C * (C + Cin + 1);
    float* out = part + (job == 0 ? 0 : (int64_t)nwg * E0) + (int64_t)wg * Mr * Nc;
#pragma unroll
    for (int t = 0; t < PP_MAXT; ++t) {
        const int tile = wave + 4 * t;
        if (tile < TM * TN) {
            const int col = (tile % TN) * 16 + l16;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = (tile / TN) * 16 + 4 * l4 + r;
                if (row < Mr && col < Nc) out[(int64_t)row * Nc + col] = acc[t][r];
            }
        }
    }
}

// flat[e] = sum_w partial[job][w][e], w ascending
static __global__ void ppgn_k_fold(const float* __restrict__ part, int nwg, int64_t E0, int64_t E1, float* __restrict__ flat) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E0 + E1) return;
    const float* src = e < E0 ? part + e : part + (int64_t)nwg * E0 + (e - E0);
    const int64_t stride = e < E0 ? E0 : E1;
    float s = 0.f;
    for (int w = 0; w < nwg; ++w) s += src[(int64_t)w * stride];
    flat[e] = s;
}

// ---------------------------------------------------------------------------------------------------------------- host
static inline int pp_threads(int nmax) {
    const int P = nmax * nmax;
    return P >= 256 ? 256 : (P + 63) / 64 * 64;
}
static inline int pp_dw_wgs(int64_t B, int nmax) {
    const int64_t items = B * gml_cdiv((int64_t)nmax * nmax, PP_CHUNK);
    return (int)(items < PP_MAXWG ? items : PP_MAXWG);
}

extern "C" {

int gml_ppgn_supported(int32_t nmax, int32_t Cin, int32_t C) {
    return nmax >= 1 && nmax <= 64 && Cin >= 1 && Cin <= 64 && C >= 1 && C <= 64;
}

int gml_ppgn_inputs(const float* x, int64_t ldx, int32_t nfeat, const int64_t* edge_src, const int64_t* edge_dst, int64_t E,
                    const int32_t* ptr, const int64_t* batch, int64_t N, int64_t B, int32_t nmax, float* X2, float* M, int32_t* n,
                    gml_stream_t stream) {
    if (N < 0 || E < 0 || B < 0 || nmax < 1 || nfeat < 0 || ldx < nfeat) return GML_E_BADARG;
    if (B == 0) return GML_OK;
    if (!ptr || !X2 || !M || !n || (N && !batch) || (E && (!edge_src || !edge_dst)) || (nfeat && N && !x)) return GML_E_BADARG;
    int64_t T = N > E ? N : E;
    if (B > T) T = B;
    if (gml_cdiv(T, 256) > 0x7fffffff) return GML_E_UNSUPPORTED;
    hipLaunchKernelGGL(ppgn_k_inputs, dim3((unsigned)gml_cdiv(T, 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, nfeat, edge_src,
                       edge_dst, E, ptr, batch, N, B, nmax, X2, M, n);
    return gml_launch_status();
}

int gml_ppgn_fwd(const float* x, const int32_t* n, int64_t B, int32_t nmax, int32_t Cin, int32_t C, const float* w1, const float* b1,
                 const float* w2, const float* b2, const float* w3, const float* b3, int32_t readout, float* a12, float* p, float* y,
                 float* r, gml_stream_t stream) {
    if (B < 0 || readout < 0 || readout > 2) return GML_E_BADARG;
    if (!gml_ppgn_supported(nmax, Cin, C) || B * 16 > 0x7fffffff || B * C > 0x7fffffff) return GML_E_UNSUPPORTED;
    if (B == 0) return GML_OK;
    if (!x || !n || !w1 || !w2 || !w3 || !a12 || !p || !y || !r) return GML_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int bs = pp_threads(nmax);
    const int nba = (2 * C + PP_CB - 1) / PP_CB, nbc = (C + PP_CB - 1) / PP_CB;
    hipLaunchKernelGGL(ppgn_k_fwd_a, dim3((unsigned)(B * nba)), dim3(bs), 0, st, x, n, nmax, Cin, C, w1, b1, w2, b2, a12, nba);
    const size_t lds = (size_t)2 * nmax * (nmax | 1) * sizeof(float);
    hipLaunchKernelGGL(ppgn_k_fwd_mm, dim3((unsigned)(B * C)), dim3(bs), lds, st, a12, n, nmax, C, p);
    hipLaunchKernelGGL(ppgn_k_fwd_c, dim3((unsigned)(B * nbc)), dim3(bs), 0, st, p, x, n, nmax, Cin, C, w3, b3, readout, y, r, nbc);
    return gml_launch_status();
}

int64_t gml_ppgn_dw_floats(int32_t Cin, int32_t C) {
    return (int64_t)C * (C + Cin + 1) + (int64_t)2 * C * (Cin + 1);
}

size_t gml_ppgn_bwd_workspace_bytes(int64_t B, int32_t nmax, int32_t Cin, int32_t C) {
    if (B <= 0 || !gml_ppgn_supported(nmax, Cin, C)) return 0;
    const int64_t P = (int64_t)nmax * nmax;
    return (size_t)(4 * B * C * P + (int64_t)pp_dw_wgs(B, nmax) * gml_ppgn_dw_floats(Cin, C)) * sizeof(float);
}

int gml_ppgn_bwd(const float* x, const int32_t* n, int64_t B, int32_t nmax, int32_t Cin, int32_t C, const float* w1, const float* w2,
                 const float* w3, const float* a12, const float* p, const float* y, const float* dy, const float* dr, int32_t readout,
                 float* dx, float* dflat, void* ws, size_t ws_bytes, gml_stream_t stream) {
    if (B < 0 || readout < 0 || readout > 2) return GML_E_BADARG;
    if (!gml_ppgn_supported(nmax, Cin, C) || B * 16 > 0x7fffffff || B * C > 0x7fffffff) return GML_E_UNSUPPORTED;
    if (!dflat) return GML_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nflat = gml_ppgn_dw_floats(Cin, C);
    if (B == 0) { gml_zero_async(dflat, (size_t)nflat * sizeof(float), st); return gml_launch_status(); }
    if (!x || !n || !w1 || !w2 || !w3 || !a12 || !p || !y || (!dy && !dr)) return GML_E_BADARG;
    if (!ws || ws_bytes < gml_ppgn_bwd_workspace_bytes(B, nmax, Cin, C)) return GML_E_WORKSPACE;
    const int64_t P = (int64_t)nmax * nmax;
    float* dz3 = (float*)ws;
    float* dp = dz3 + B * C * P;
    float* dz12 = dp + B * C * P;
    float* part = dz12 + 2 * B * C * P;
    const int bs = pp_threads(nmax);
    const int nbc = (C + PP_CB - 1) / PP_CB, nbx = (Cin + PP_CB - 1) / PP_CB;
    hipLaunchKernelGGL(ppgn_k_bwd_c, dim3((unsigned)(B * nbc)), dim3(bs), 0, st, y, dy, dr, n, nmax, Cin, C, w3, readout, dz3, dp, nbc);
    const size_t lds = (size_t)3 * nmax * (nmax | 1) * sizeof(float);
    hipLaunchKernelGGL(ppgn_k_bwd_mm, dim3((unsigned)(B * C)), dim3(bs), lds, st, a12, dp, n, nmax, C, dz12);
    if (dx) hipLaunchKernelGGL(ppgn_k_bwd_x, dim3((unsigned)(B * nbx)), dim3(bs), 0, st, dz3, dz12, n, nmax, Cin, C, w1, w2, w3, dx, nbx);
    const int nwg = pp_dw_wgs(B, nmax);
    const int mp = (2 * C + 15) / 16 * 16, np = (C + Cin + 1 + 15) / 16 * 16;         // (the larger of the two jobs on each side)
    const size_t ldsw = (size_t)(mp + np) * PP_LD * sizeof(float);
    hipLaunchKernelGGL(ppgn_k_dw, dim3(nwg, 2), dim3(256), ldsw, st, dz3, dz12, p, x, n, B, nmax, Cin, C, part, nwg);
    const int64_t E0 = (int64_t)C * (C + Cin + 1), E1 = (int64_t)2 * C * (Cin + 1);
    hipLaunchKernelGGL(ppgn_k_fold, dim3((unsigned)gml_cdiv(E0 + E1, 256)), dim3(256), 0, st, part, nwg, E0, E1, dflat);
    return gml_launch_status();
}

}  // extern "C"
