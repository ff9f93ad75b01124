// GIN: GINConv (torch_geometric 1.6.1) with its nn = Linear or Linear-ReLU-Linear fused behind the aggregation (include/gml.h:
// gml_gin_*).  Widths up to 64: a weight matrix is a [64][64] fp32 image in the LDS (16 KB, zero beyond its rows and columns).
//
//   forward   ONE launch.  A workgroup (4 waves) walks tiles of 32 target rows (tile = block, block + grid, ...; the weight images are
//             loaded once per workgroup).  Per tile:
//               h[i] = sum over the row's edges (j -> i) in CSR order of x[j], then + (1 + eps) x[i]      (eps read from DEVICE memory)
//                      one lane per (row, column); a wave serves 64 / max(4, pow2(Fin)) rows at once (at most its 8), the edge loop
//                      in chunks of 4 loads: any degree
//               depth 2: t = relu(W1 h + b1), y = act(W2 t + b2);  depth 1: y = act(W1 h + b1)
//                      lane = output column, a wave's 8 rows in registers, k ascending fmaf from the bias; the row operand is an LDS
//                      broadcast (float4 of k), the weight operand lane-contiguous (the image is stored transposed [k][o])
//             h and t go to global memory as well: the backward's inputs.
//   backward  THREE launches (TWO when dx is not wanted):
//             R  row pass.  Workgroup w owns the contiguous tiles [w tpw, (w + 1) tpw) and per tile forms g2 = dy act'(y), (depth 2)
//                g1 = (g2 W2) [t > 0], dh = g1 W1 -> workspace, and accumulates in registers, rows ascending,
//                dW2 += g2^T t, db2 += g2, dW1 += g1^T h, db1 += g1, deps += <dh[i], x[i]> (per thread, then the 256 threads in
//                ascending order); one partial [dW1 | db1 | dW2 | db2 | deps] per workgroup
//             S  source view: dx[j] = (1 + eps) dh[j], then + dh[i] over the edges (j -> i) in source-view CSR order
//             F  fold of the partials in ascending workgroup order -> dflat
// No atomics; every sum has one order.  Plain fp32 fmaf / tanhf.  Column indices outside [0, N) are skipped.
#include "gml_rowtile64.h"

// the sum of x[j] over the edges: every in-range j, a plain add
struct gin_edge {
    __device__ __forceinline__ bool keep(int64_t) const { return true; }
    __device__ __forceinline__ float weight(int64_t) const { return 1.f; }
    __device__ __forceinline__ float add(float acc, float, float v) const { return acc + v; }
};

static __global__ __launch_bounds__(256) void gin_k_fwd(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                        const float* __restrict__ x, int64_t ldx, int64_t N, int Fin, int gp,
                                                        const float* __restrict__ eps, const float* __restrict__ w1,
                                                        const float* __restrict__ b1, int Fh, const float* __restrict__ w2,
                                                        const float* __restrict__ b2, int Fout, int depth, int act,
                                                        float* __restrict__ h, int64_t ldh, float* __restrict__ t, int64_t ldt,
                                                        float* __restrict__ y, int64_t ldy, int64_t ntiles) {
    __shared__ __attribute__((aligned(16))) float w1s[GML_RT_W * GML_RT_W];       // [k][o]
    __shared__ __attribute__((aligned(16))) float w2s[GML_RT_W * GML_RT_W];       // [m][o]
    __shared__ __attribute__((aligned(16))) float hs[GML_RT_TR * GML_RT_W];
    __shared__ __attribute__((aligned(16))) float ts[GML_RT_TR * GML_RT_W];
    const int lane = threadIdx.x % GML_WAVE, wave = threadIdx.x / GML_WAVE;
    gml_rt_load_image<true>(w1s, w1, Fin, Fh, Fin);
    if (depth == 2) gml_rt_load_image<true>(w2s, w2, Fh, Fout, Fh);
    const float e1 = 1.f + eps[0];
    const int K1 = (Fin + 3) & ~3, K2 = (Fh + 3) & ~3;
    const float bias1 = (b1 && lane < Fh) ? b1[lane] : 0.f;
    const float bias2 = (depth == 2 && b2 && lane < Fout) ? b2[lane] : 0.f;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t r0 = tile * GML_RT_TR + wave * GML_RT_RPW;
        __syncthreads();                                                    // the images are in; the last tile's reads are over
        gml_rt_gather_rows(hs, r0, N, Fin, gp, wave, lane, true, [&](int64_t row, int c) {
            const float v = fmaf(e1, x[row * ldx + c], gml_rt_walk(rowptr, col, x, ldx, row, c, N, 0.f, gin_edge()));
            h[row * ldh + c] = v;
            return v;
        });
        __syncthreads();
        float acc[GML_RT_RPW];
#pragma unroll
        for (int r = 0; r < GML_RT_RPW; ++r) acc[r] = bias1;
        gml_rt_prod8(hs, w1s, K1, wave, lane, acc);
        if (depth == 2) {
#pragma unroll
            for (int r = 0; r < GML_RT_RPW; ++r) {
                const float v = lane < Fh ? fmaxf(acc[r], 0.f) : 0.f;
                ts[(wave * GML_RT_RPW + r) * GML_RT_W + lane] = v;
                if (lane < Fh && r0 + r < N) t[(r0 + r) * ldt + lane] = v;
                acc[r] = bias2;
            }
            __syncthreads();
            gml_rt_prod8(ts, w2s, K2, wave, lane, acc);
        }
        const int Fo = depth == 2 ? Fout : Fh;
        if (lane < Fo) {
#pragma unroll
            for (int r = 0; r < GML_RT_RPW; ++r)
                if (r0 + r < N) y[(r0 + r) * ldy + lane] = gml_rt_act(acc[r], act);
        }
    }
}

// partial layout = dflat layout: [dW1 Fh x Fin | db1 Fh | dW2 Fout x Fh | db2 Fout (depth 2) | deps]
static __global__ __launch_bounds__(256) void gin_k_bwd_r(const float* __restrict__ x, int64_t ldx, const float* __restrict__ h, int64_t ldh,
                                                          const float* __restrict__ t, int64_t ldt, const float* __restrict__ y,
                                                          int64_t ldy, const float* __restrict__ dy, int64_t lddy, int64_t N, int Fin,
                                                          const float* __restrict__ w1, int Fh, const float* __restrict__ w2, int Fout,
                                                          int depth, int act, float* __restrict__ dh, float* __restrict__ part,
                                                          int64_t P, int64_t ntiles, int64_t tpw) {
    __shared__ __attribute__((aligned(16))) float w1s[GML_RT_W * GML_RT_W];       // [o][k]
    __shared__ __attribute__((aligned(16))) float w2s[GML_RT_W * GML_RT_W];       // [o][m]
    __shared__ __attribute__((aligned(16))) float g2s[GML_RT_TR * GML_RT_W];
    __shared__ __attribute__((aligned(16))) float g1d[GML_RT_TR * GML_RT_W];
    __shared__ __attribute__((aligned(16))) float as[GML_RT_TR * GML_RT_W];       // t, then h
    const int lane = threadIdx.x % GML_WAVE, wave = threadIdx.x / GML_WAVE, tid = threadIdx.x;
    gml_rt_load_image<false>(w1s, w1, Fh, Fin, Fin);
    if (depth == 2) gml_rt_load_image<false>(w2s, w2, Fout, Fh, Fh);
    float* g1s = depth == 2 ? g1d : g2s;
    const int Fo = depth == 2 ? Fout : Fh;                                  // the width of y
    const int KO = (Fo + 3) & ~3, KH = (Fh + 3) & ~3;
    float aw1[16], aw2[16], ab = 0.f, aeps = 0.f;                           // thread (wave, lane): rows 16 wave .. + 15, column lane
#pragma unroll
    for (int u = 0; u < 16; ++u) aw1[u] = aw2[u] = 0.f;
    const int64_t t0 = (int64_t)blockIdx.x * tpw, t1 = t0 + tpw < ntiles ? t0 + tpw : ntiles;
    for (int64_t tile = t0; tile < t1; ++tile) {
        const int64_t r0 = tile * GML_RT_TR + wave * GML_RT_RPW;
        __syncthreads();
        gml_rt_load_g(g2s, dy, lddy, y, ldy, r0, N, Fo, act, wave, lane);
        if (depth == 2) gml_rt_load_rows(as, t, ldt, r0, N, Fh, wave, lane);
        else gml_rt_load_rows(as, h, ldh, r0, N, Fin, wave, lane);
        __syncthreads();
        if (depth == 2) {
            gml_rt_outer16(g2s, as, wave, lane, aw2);                           // dW2[o][m] += g2[r][o] t[r][m]
            if (tid >= 64 && tid < 128) gml_rt_colsum(g2s, lane, ab);
            float acc[GML_RT_RPW];
#pragma unroll
            for (int r = 0; r < GML_RT_RPW; ++r) acc[r] = 0.f;
            gml_rt_prod8(g2s, w2s, KO, wave, lane, acc);
#pragma unroll
            for (int r = 0; r < GML_RT_RPW; ++r)
                g1d[(wave * GML_RT_RPW + r) * GML_RT_W + lane] = as[(wave * GML_RT_RPW + r) * GML_RT_W + lane] > 0.f ? acc[r] : 0.f;
            __syncthreads();
            gml_rt_load_rows(as, h, ldh, r0, N, Fin, wave, lane);
            __syncthreads();
        }
        gml_rt_outer16(g1s, as, wave, lane, aw1);                               // dW1[o][k] += g1[r][o] h[r][k]
        if (tid < 64) gml_rt_colsum(g1s, lane, ab);
        float acc[GML_RT_RPW];
#pragma unroll
        for (int r = 0; r < GML_RT_RPW; ++r) acc[r] = 0.f;
        gml_rt_prod8(g1s, w1s, KH, wave, lane, acc);                           // dh[r][k] = sum_o g1[r][o] W1[o][k]
        if (lane < Fin) {
#pragma unroll
            for (int r = 0; r < GML_RT_RPW; ++r) {
                const int64_t row = r0 + r;
                if (row < N) {
                    if (dh) dh[row * Fin + lane] = acc[r];
                    aeps = fmaf(acc[r], x[row * ldx + lane], aeps);
                }
            }
        }
    }
    float* out = part + (int64_t)blockIdx.x * P;
    const int64_t o1 = (int64_t)Fh * Fin, o2 = o1 + Fh, o3 = o2 + (depth == 2 ? (int64_t)Fout * Fh : 0), o4 = o3 + (depth == 2 ? Fout : 0);
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int o = wave * 16 + u;
        if (o < Fh && lane < Fin) out[(int64_t)o * Fin + lane] = aw1[u];
        if (depth == 2 && o < Fout && lane < Fh) out[o2 + (int64_t)o * Fh + lane] = aw2[u];
    }
    if (tid < 64 && lane < Fh) out[o1 + lane] = ab;
    if (depth == 2 && tid >= 64 && tid < 128 && lane < Fout) out[o3 + lane] = ab;
    __syncthreads();
    g2s[tid] = aeps;
    __syncthreads();
    if (tid == 0) {
        float s = 0.f;
        for (int i = 0; i < 256; ++i) s += g2s[i];
        out[o4] = s;
    }
}

static __global__ __launch_bounds__(256) void gin_k_bwd_s(const int32_t* __restrict__ rowptr_t, const int32_t* __restrict__ col_t,
                                                          const float* __restrict__ dh, int64_t N, int Fin, int gp,
                                                          const float* __restrict__ eps, float* __restrict__ dx, int64_t lddx) {
    const int rpb = 256 / gp;
    const int sub = threadIdx.x / gp, c = threadIdx.x % gp;
    const int64_t row = (int64_t)blockIdx.x * rpb + sub;
    if (row >= N || c >= Fin) return;
    dx[row * lddx + c] = gml_rt_walk(rowptr_t, col_t, dh, Fin, row, c, N, (1.f + eps[0]) * dh[row * Fin + c], gin_edge());
}

extern "C" {

int gml_gin_supported(int32_t Fin, int32_t Fh, int32_t Fout, int32_t depth) {
    if (depth != 1 && depth != 2) return 0;
    if (Fin < 1 || Fin > GML_RT_W || Fh < 1 || Fh > GML_RT_W) return 0;
    return depth == 1 || (Fout >= 1 && Fout <= GML_RT_W);
}

int gml_gin_fwd(const int32_t* rowptr, const int32_t* col, const float* x, int64_t ldx, int64_t N, int64_t E, int32_t Fin, const float* eps,
                const float* w1, const float* b1, int32_t Fh, const float* w2, const float* b2, int32_t Fout, int32_t depth, int32_t act,
                float* h, int64_t ldh, float* t, int64_t ldt, float* y, int64_t ldy, gml_stream_t stream) {
    if (N < 0 || E < 0 || act < 0 || act > 2) return GML_E_BADARG;
    if (!gml_gin_supported(Fin, Fh, Fout, depth) || !gml_rt_range(N, E)) return GML_E_UNSUPPORTED;
    if (N == 0) return GML_OK;
    const int Fo = depth == 2 ? Fout : Fh;
    if (!rowptr || (E && !col) || !x || !eps || !w1 || !h || !y || ldx < Fin || ldh < Fin || ldy < Fo) return GML_E_BADARG;
    if (depth == 2 && (!w2 || !t || ldt < Fh)) return GML_E_BADARG;
    hipLaunchKernelGGL(gin_k_fwd, dim3(gml_rt_grid(N)), dim3(256), 0, (hipStream_t)stream, rowptr, col, x, ldx, N, (int)Fin, gml_rt_gp(Fin),
                       eps, w1, b1, (int)Fh, w2, b2, (int)Fout, (int)depth, (int)act, h, ldh, t, ldt, y, ldy, gml_rt_tiles(N));
    return gml_launch_status();
}

int64_t gml_gin_dflat_floats(int32_t Fin, int32_t Fh, int32_t Fout, int32_t depth) {
    if (!gml_gin_supported(Fin, Fh, Fout, depth)) return 0;
    return (int64_t)Fh * Fin + Fh + (depth == 2 ? (int64_t)Fout * Fh + Fout : 0) + 1;
}

size_t gml_gin_bwd_workspace_bytes(int64_t N, int32_t Fin, int32_t Fh, int32_t Fout, int32_t depth) {
    if (N <= 0 || N > 0x7fffffff || !gml_gin_supported(Fin, Fh, Fout, depth)) return 0;
    int64_t tpw;
    int nwg;
    gml_rt_row_plan(N, &tpw, &nwg);
    // dh [N, Fin] | partials [workgroups, dflat floats]
    return (size_t)(N * Fin + (int64_t)nwg * gml_gin_dflat_floats(Fin, Fh, Fout, depth)) * sizeof(float);
}

int gml_gin_bwd(const int32_t* rowptr_t, const int32_t* col_t, const float* x, int64_t ldx, const float* h, int64_t ldh, const float* t,
                int64_t ldt, const float* y, int64_t ldy, const float* dy, int64_t lddy, int64_t N, int64_t E, int32_t Fin, const float* eps,
                const float* w1, int32_t Fh, const float* w2, int32_t Fout, int32_t depth, int32_t act, float* dx, int64_t lddx,
                float* dflat, void* ws, size_t ws_bytes, gml_stream_t stream) {
    if (N < 0 || E < 0 || act < 0 || act > 2) return GML_E_BADARG;
    if (!gml_gin_supported(Fin, Fh, Fout, depth) || !gml_rt_range(N, E)) return GML_E_UNSUPPORTED;
    if (!dflat) return GML_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int64_t P = gml_gin_dflat_floats(Fin, Fh, Fout, depth);
    if (N == 0) {
        gml_zero_async(dflat, (size_t)P * sizeof(float), st);
        return gml_launch_status();
    }
    const int Fo = depth == 2 ? Fout : Fh;
    if (!x || !eps || !w1 || !h || !y || !dy || ldx < Fin || ldh < Fin || ldy < Fo || lddy < Fo) return GML_E_BADARG;
    if (depth == 2 && (!w2 || !t || ldt < Fh)) return GML_E_BADARG;
    if (dx && (!rowptr_t || (E && !col_t) || lddx < Fin)) return GML_E_BADARG;
    if (!ws || ((uintptr_t)ws & 3) || ws_bytes < gml_gin_bwd_workspace_bytes(N, Fin, Fh, Fout, depth)) return GML_E_WORKSPACE;
    int64_t tpw;
    int nwg;
    gml_rt_row_plan(N, &tpw, &nwg);
    float* dh = (float*)ws;
    float* part = dh + N * Fin;
    hipLaunchKernelGGL(gin_k_bwd_r, dim3(nwg), dim3(256), 0, st, x, ldx, h, ldh, t, ldt, y, ldy, dy, lddy, N, (int)Fin, w1, (int)Fh, w2,
                       (int)Fout, (int)depth, (int)act, dx ? dh : (float*)nullptr, part, P, gml_rt_tiles(N), tpw);
    if (dx) {
        const int gp = gml_rt_gp(Fin);
        hipLaunchKernelGGL(gin_k_bwd_s, dim3((unsigned)gml_cdiv(N, 256 / gp)), dim3(256), 0, st, rowptr_t, col_t, dh, N, (int)Fin, gp, eps,
                           dx, lddx);
    }
    gml_rt_fold(part, nwg, P, dflat, st);
    return gml_launch_status();
}

}  // extern "C"
