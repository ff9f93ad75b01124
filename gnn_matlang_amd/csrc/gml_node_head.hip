// Node-level readout, masked squared loss and the sums of R^2 for the 2-D grid filtering experiment (filtering.py:268, :320-327):
//
//      pre[r]  = x[r] . w + b                                   (fc2: nin -> 1, nin <= 64)
//      loss    = sum_r (mask[r] (pre[r] - y[r]))^2              y[r] = y[r ldy + task]
//      ss_res  = sum_{mask == 1} (y - pre)^2,   ss_tot = sum_{mask == 1} (y - ybar)^2,   count = #{mask == 1}
//
// ybar is the mean of y over the same rows and is formed FIRST (a second pass over y): ss_tot is never the difference of two large
// sums.  r2 = 1 - ss_res / ss_tot is sklearn's r2_score.  One launch each way, one workgroup of 1024 threads (the experiment has 900
// rows; any N works, a workgroup walks it in strides), every sum a fixed-order tree: the same bits on every run, no atomics, no
// host read -- both launches can be captured.
//
// Backward: dpre[r] = g 2 mask[r]^2 (pre[r] - y[r]);  dx[r][f] = dpre[r] w[f];  dw[f] = sum_r dpre[r] x[r][f];  db = sum_r dpre[r].
// Thread (rg, f) of 16 x 64 walks the rows r = rg, rg + 16, ... for its feature (coalesced over f) and the 16 partial sums of a
// feature are added in ascending rg.
#include "gml_common.h"

#define NH_THREADS 1024

// sum over the workgroup in a fixed order (tree over LDS); every thread returns the total
__device__ __forceinline__ float nh_block_sum(float v, float* red) {
    const int tid = threadIdx.x;
    __syncthreads();                                         // (red may still be read from the previous sum)
    red[tid] = v;
    __syncthreads();
    for (int w = NH_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(NH_THREADS) void gml_k_node_head_fwd(const float* __restrict__ x, int64_t ldx, const float* __restrict__ w,
                                                                 const float* __restrict__ b, const float* __restrict__ y, int64_t ldy,
                                                                 const float* __restrict__ mask, int64_t ldm, int64_t N, int F,
                                                                 float* __restrict__ pre, float* __restrict__ loss,
                                                                 float* __restrict__ stats) {
    __shared__ float red[NH_THREADS];
    __shared__ float ws[64];
    const int tid = threadIdx.x;
    if (tid < 64) ws[tid] = tid < F ? w[tid] : 0.f;
    __syncthreads();
    const float bias = b != nullptr ? b[0] : 0.f;
    float l = 0.f, res = 0.f, sy = 0.f, cnt = 0.f;
    for (int64_t r = tid; r < N; r += NH_THREADS) {
        const float* xr = x + r * ldx;
        float a = bias;
        for (int f = 0; f < F; ++f) a = fmaf(xr[f], ws[f], a);
        pre[r] = a;
        const float m = mask[r * ldm], yy = y[r * ldy], d = a - yy;
        l = fmaf(m * d, m * d, l);
        if (m == 1.f) { res = fmaf(d, d, res); sy += yy; cnt += 1.f; }
    }
    l = nh_block_sum(l, red);
    res = nh_block_sum(res, red);
    sy = nh_block_sum(sy, red);
    cnt = nh_block_sum(cnt, red);
    const float ybar = cnt > 0.f ? sy / cnt : 0.f;
    float tot = 0.f;
    for (int64_t r = tid; r < N; r += NH_THREADS) {
        if (mask[r * ldm] == 1.f) { const float d = y[r * ldy] - ybar; tot = fmaf(d, d, tot); }
    }
    tot = nh_block_sum(tot, red);
    if (tid == 0) {
        loss[0] = l;
        if (stats != nullptr) { stats[0] = l; stats[1] = res; stats[2] = tot; stats[3] = cnt; }
    }
}

__global__ __launch_bounds__(NH_THREADS) void gml_k_node_head_bwd(const float* __restrict__ g, const float* __restrict__ x, int64_t ldx,
                                                                 const float* __restrict__ w, const float* __restrict__ pre,
                                                                 const float* __restrict__ y, int64_t ldy, const float* __restrict__ mask,
                                                                 int64_t ldm, int64_t N, int F, float* __restrict__ dx, int64_t lddx,
                                                                 float* __restrict__ dw, float* __restrict__ db) {
    __shared__ float part[16][65];
    const int tid = threadIdx.x, f = tid & 63, rg = tid >> 6;
    const float g2 = 2.f * g[0];
    const float wf = f < F ? w[f] : 0.f;
    float aw = 0.f, ab = 0.f;
    for (int64_t r = rg; r < N; r += 16) {
        const float m = mask[r * ldm];
        const float dp = g2 * m * m * (pre[r] - y[r * ldy]);
        ab += dp;
        if (f < F) {
            aw = fmaf(dp, x[r * ldx + f], aw);
            if (dx != nullptr) dx[r * lddx + f] = dp * wf;
        }
    }
    part[rg][f] = aw;
    if (f == 0) part[rg][64] = ab;
    __syncthreads();
    if (tid < 65) {
        float a = 0.f;
        for (int j = 0; j < 16; ++j) a += part[j][tid];
        if (tid < F) { if (dw != nullptr) dw[tid] = a; }
        else if (tid == 64 && db != nullptr) db[0] = a;
    }
}

extern "C" int gml_node_head_fwd(const float* x, int64_t ldx, const float* w, const float* b, const float* y, int64_t ldy,
                                 const float* mask, int64_t ldm, int64_t N, int32_t F, float* pre, float* loss, float* stats,
                                 void* stream) {
    if (x == nullptr || w == nullptr || y == nullptr || mask == nullptr || pre == nullptr || loss == nullptr || N < 0 || ldx < F ||
        ldy < 1 || ldm < 1)
        return GML_E_BADARG;
    if (F < 1 || F > 64) return GML_E_UNSUPPORTED;
    hipLaunchKernelGGL(gml_k_node_head_fwd, dim3(1), dim3(NH_THREADS), 0, (hipStream_t)stream, x, ldx, w, b, y, ldy, mask, ldm, N, F,
                       pre, loss, stats);
    return gml_launch_status();
}

extern "C" int gml_node_head_bwd(const float* g, const float* x, int64_t ldx, const float* w, const float* pre, const float* y,
                                 int64_t ldy, const float* mask, int64_t ldm, int64_t N, int32_t F, float* dx, int64_t lddx, float* dw,
                                 float* db, void* stream) {
    if (g == nullptr || x == nullptr || w == nullptr || pre == nullptr || y == nullptr || mask == nullptr || N < 0 || ldx < F ||
        ldy < 1 || ldm < 1 || (dx != nullptr && lddx < F))
        return GML_E_BADARG;
    if (F < 1 || F > 64) return GML_E_UNSUPPORTED;
    hipLaunchKernelGGL(gml_k_node_head_bwd, dim3(1), dim3(NH_THREADS), 0, (hipStream_t)stream, g, x, ldx, w, pre, y, ldy, mask, ldm, N,
                       F, dx, lddx, dw, db);
    return gml_launch_status();
}
