// ChebNet: ChebConv (torch_geometric 1.6.1, normalization 'sym') with the script's activation (include/gml.h: gml_cheb_*).  Widths up
// to 64, K up to 8: a weight matrix W_k [Fin][Fout] is a [64][64] fp32 image in the LDS (16 KB, zero beyond its rows and columns).
//
//   norm      ONE launch per batch: norm[i] = (dis[i], s[i]); dis = deg^-1/2 over the non-self edges of the SOURCE view (0 at deg 0),
//             s = 2 / lambda_max[batch[i]] (or 2 / the scalar).  Every layer of a model reads the same norm.
//   forward   K - 1 launches (ONE at K = 1).  A workgroup (4 waves) walks tiles of 32 target rows.  Launch k (1 <= k <= K - 1), per tile:
//               Tx_k[i] = sum over the row's edges (j -> i, j != i) in CSR order of fmaf(w, Tx_{k-1}[j], .), w = (-(s[i] dis[i])) dis[j],
//                         then fmaf(s[i] - 1, Tx_{k-1}[i], .); k >= 2: then fmaf(2, ., -Tx_{k-2}[i])
//                         one lane per (row, column); a wave serves 64 / max(4, pow2(Fin)) rows at once, the edge loop in chunks of 4
//               -> the tile in the LDS and T[:, (k - 1) Fin ..] in global memory (the backward's input; Tx_0 = x is not copied)
//               acc = (k == 1: bias, then x W_0) (k >= 2: the y of launch k - 1), then + Tx_k W_k: lane = output column, a wave's 8 rows
//                         in registers, input column ascending fmaf; the last launch writes act(acc), the others acc, to y
//             launch 1 holds W_0 and W_1 in the LDS, every other launch W_k alone.
//   backward  R  row pass.  Workgroup w owns the contiguous tiles [w tpw, (w + 1) tpw): g = dy act'(y), dW_k += Tx_k^T g (k ascending
//                inside a tile, rows ascending) and db += g in registers -> one partial [dW_0 .. dW_{K-1} | db] per workgroup;
//                g W_{K-1}^T -> dx at K = 1, else (dx wanted) the workspace: G_{K-1}
//             A  K - 1 adjoint launches over the SOURCE view, k = K - 2 .. 0 (dx wanted only):
//                G_k[j] = fmaf(c_k, a, g[j] W_k^T) - G_{k+2}[j],  a = sum over the row's edges (j -> i, i != j) in source-view CSR order
//                of fmaf(w, G_{k+1}[i], .) with the forward's w of that edge, then fmaf(s[j] - 1, G_{k+1}[j], .);  c_0 = 1, else 2
//                three rotating [N, Fin] buffers in the workspace; the last launch writes dx
//             F  fold of the partials in ascending workgroup order -> dflat
// No atomics; every sum has one order.  Plain fp32 fmaf / tanhf.  Column indices outside [0, N) are skipped, self loops dropped.
#include "gml_rowtile64.h"

#define CHEB_KMAX 8

// what an edge of `row` to column index j contributes (gml_rt_walk): self loops skipped, fmaf with the weight of the edge (j -> i),
// (-(s[i] dis[i])) dis[j], where `row` is i in the target view and j in the source view
template <bool TARGET_VIEW>
struct cheb_edge {
    const float* __restrict__ norm;
    int64_t row;
    float dr, ndr;                                                          // dis[row], -(s[row] dis[row])
    __device__ __forceinline__ bool keep(int64_t j) const { return j != row; }
    __device__ __forceinline__ float weight(int64_t j) const {
        return TARGET_VIEW ? ndr * norm[2 * j] : (-(norm[2 * j + 1] * norm[2 * j])) * dr;
    }
    __device__ __forceinline__ float add(float acc, float w, float v) const { return fmaf(w, v, acc); }
};
// one (row, column) of L^ src (TARGET_VIEW: the CSR lists the sources of the target `row`) or of L^T src (the CSR lists the targets
// of the source `row`): the edges in CSR order, then the diagonal
template <bool TARGET_VIEW>
static __device__ __forceinline__ float cheb_gather(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                    const float* __restrict__ norm, const float* src, int64_t ld, int64_t row, int c,
                                                    int64_t N) {
    const float dr = norm[2 * row], sr = norm[2 * row + 1];
    const float acc = gml_rt_walk(rowptr, col, src, ld, row, c, N, 0.f, cheb_edge<TARGET_VIEW>{norm, row, dr, -(sr * dr)});
    return fmaf(sr - 1.f, src[row * ld + c], acc);
}

static __global__ __launch_bounds__(256) void cheb_k_norm(const int32_t* __restrict__ rowptr_t, const int32_t* __restrict__ col_t,
                                                          const int32_t* __restrict__ batch, const float* __restrict__ lmax, int64_t B,
                                                          float lambda, int64_t N, float* __restrict__ norm) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    int deg = 0;
    for (int k = rowptr_t[i], k1 = rowptr_t[i + 1]; k < k1; ++k) {
        const int64_t t = col_t[k];
        deg += (t >= 0 && t < N && t != i) ? 1 : 0;
    }
    float lam = lambda;
    if (lmax) {
        const int64_t g = batch ? batch[i] : 0;
        lam = (g >= 0 && g < B) ? lmax[g] : 2.f;
    }
    norm[2 * i] = deg > 0 ? 1.f / sqrtf((float)deg) : 0.f;
    norm[2 * i + 1] = 2.f / lam;
}

#define CHEB_X0 1           // acc starts from the bias and x W_0 (launch 1, and the only launch of K = 1)
#define CHEB_GATHER 2       // Tx_k is formed from p (and q) and acc += Tx_k W_k
#define CHEB_LAST 4         // y = act(acc)

// p = Tx_{k-1} (rows of ldp), q = Tx_{k-2} (rows of ldq; NULL at k = 1), tk = where Tx_k goes (rows of ldt)
static __global__ __launch_bounds__(256) void cheb_k_step(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                          const float* __restrict__ norm, const float* __restrict__ x, int64_t ldx,
                                                          const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t N, int Fin,
                                                          int gp, const float* __restrict__ w0, const float* __restrict__ wk,
                                                          const float* __restrict__ bias, int Fout, int mode, int act, float* tk,
                                                          int64_t ldt, float* y, int64_t ldy, int64_t ntiles) {
    __shared__ __attribute__((aligned(16))) float w0s[GML_RT_W * GML_RT_W];     // [in][out]
    __shared__ __attribute__((aligned(16))) float wks[GML_RT_W * GML_RT_W];
    __shared__ __attribute__((aligned(16))) float xs[GML_RT_TR * GML_RT_W];
    __shared__ __attribute__((aligned(16))) float ts[GML_RT_TR * GML_RT_W];
    const int lane = threadIdx.x % GML_WAVE, wave = threadIdx.x / GML_WAVE;
    if (mode & CHEB_X0) gml_rt_load_image<false>(w0s, w0, Fin, Fout, Fout);
    if (mode & CHEB_GATHER) gml_rt_load_image<false>(wks, wk, Fin, Fout, Fout);
    const int K4 = (Fin + 3) & ~3;
    const float b = (bias && lane < Fout) ? bias[lane] : 0.f;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t r0 = tile * GML_RT_TR + wave * GML_RT_RPW;
        __syncthreads();                                                    // the images are in; the last tile's reads are over
        gml_rt_gather_rows(ts, r0, N, Fin, gp, wave, lane, (mode & CHEB_GATHER) != 0, [&](int64_t row, int c) {
            float v = cheb_gather<true>(rowptr, col, norm, p, ldp, row, c, N);
            if (q) v = fmaf(2.f, v, -q[row * ldq + c]);
            tk[row * ldt + c] = v;
            return v;
        });
        if (mode & CHEB_X0) gml_rt_load_rows(xs, x, ldx, r0, N, Fin, wave, lane);
        __syncthreads();
        float acc[GML_RT_RPW];
#pragma unroll
        for (int r = 0; r < GML_RT_RPW; ++r) {
            if (mode & CHEB_X0) acc[r] = b;
            else acc[r] = (lane < Fout && r0 + r < N) ? y[(r0 + r) * ldy + lane] : 0.f;
        }
        if (mode & CHEB_X0) gml_rt_prod8(xs, w0s, K4, wave, lane, acc);
        if (mode & CHEB_GATHER) gml_rt_prod8(ts, wks, K4, wave, lane, acc);
        if (lane < Fout) {
#pragma unroll
            for (int r = 0; r < GML_RT_RPW; ++r)
                if (r0 + r < N) y[(r0 + r) * ldy + lane] = (mode & CHEB_LAST) ? gml_rt_act(acc[r], act) : acc[r];
        }
    }
}

// partial layout = dflat layout: [dW_0 .. dW_{K-1}, each Fin x Fout | db Fout].  NK: the accumulator sets held (>= K).
// thread (wave, lane): input columns 16 wave .. + 15, output column lane.  gl: where g W_{K-1}^T goes (rows of ldgl), or NULL.
template <int NK>
static __global__ __launch_bounds__(256) void cheb_k_bwd_r(const float* __restrict__ x, int64_t ldx, const float* __restrict__ T, int64_t ldT,
                                                           const float* __restrict__ y, int64_t ldy, const float* __restrict__ dy,
                                                           int64_t lddy, int64_t N, int Fin, const float* __restrict__ w, int Fout, int K,
                                                           int act, float* __restrict__ gl, int64_t ldgl, float* __restrict__ part,
                                                           int64_t P, int64_t ntiles, int64_t tpw) {
    __shared__ __attribute__((aligned(16))) float wts[GML_RT_W * GML_RT_W];     // W_{K-1}^T: [out][in]
    __shared__ __attribute__((aligned(16))) float gs[GML_RT_TR * GML_RT_W];
    __shared__ __attribute__((aligned(16))) float as[GML_RT_TR * GML_RT_W];     // Tx_k
    const int lane = threadIdx.x % GML_WAVE, wave = threadIdx.x / GML_WAVE, tid = threadIdx.x;
    if (gl) gml_rt_load_image<true>(wts, w + (int64_t)(K - 1) * Fin * Fout, Fout, Fin, Fout);
    const int KO = (Fout + 3) & ~3;
    float aw[NK][16], ab = 0.f;
#pragma unroll
    for (int k = 0; k < NK; ++k)
#pragma unroll
        for (int u = 0; u < 16; ++u) aw[k][u] = 0.f;
    const int64_t t0 = (int64_t)blockIdx.x * tpw, t1 = t0 + tpw < ntiles ? t0 + tpw : ntiles;
    for (int64_t tile = t0; tile < t1; ++tile) {
        const int64_t r0 = tile * GML_RT_TR + wave * GML_RT_RPW;
        __syncthreads();
        gml_rt_load_g(gs, dy, lddy, y, ldy, r0, N, Fout, act, wave, lane);
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            if (k < K) {
                if (k) __syncthreads();                                     // the reads of Tx_{k-1}'s tile are over
                gml_rt_load_rows(as, k ? T + (int64_t)(k - 1) * Fin : x, k ? ldT : ldx, r0, N, Fin, wave, lane);
                __syncthreads();
                gml_rt_outer16(as, gs, wave, lane, aw[k]);                  // dW_k[i][o] += Tx_k[r][i] g[r][o]
            }
        }
        if (tid < 64) gml_rt_colsum(gs, lane, ab);
        if (gl) {
            float acc[GML_RT_RPW];
#pragma unroll
            for (int r = 0; r < GML_RT_RPW; ++r) acc[r] = 0.f;
            gml_rt_prod8(gs, wts, KO, wave, lane, acc);                       // sum_o g[r][o] W_{K-1}[i][o]
            if (lane < Fin) {
#pragma unroll
                for (int r = 0; r < GML_RT_RPW; ++r)
                    if (r0 + r < N) gl[(r0 + r) * ldgl + lane] = acc[r];
            }
        }
    }
    float* out = part + (int64_t)blockIdx.x * P;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        if (k < K) {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int i = wave * 16 + u;
                if (i < Fin && lane < Fout) out[((int64_t)k * Fin + i) * Fout + lane] = aw[k][u];
            }
        }
    }
    if (tid < 64 && lane < Fout) out[(int64_t)K * Fin * Fout + lane] = ab;
}

// one adjoint step: go[j] = fmaf(ck, (L^T g1)[j], g[j] W_k^T) - g2[j]   (g1 = G_{k+1}, g2 = G_{k+2} or NULL; g1, g2 rows of Fin)
static __global__ __launch_bounds__(256) void cheb_k_bwd_a(const int32_t* __restrict__ rowptr_t, const int32_t* __restrict__ col_t,
                                                           const float* __restrict__ norm, const float* __restrict__ y, int64_t ldy,
                                                           const float* __restrict__ dy, int64_t lddy, int64_t N, int Fin, int gp,
                                                           const float* __restrict__ wk, int Fout, int act, float ck,
                                                           const float* __restrict__ g1, const float* __restrict__ g2,
                                                           float* __restrict__ go, int64_t ldgo, int64_t ntiles) {
    __shared__ __attribute__((aligned(16))) float wts[GML_RT_W * GML_RT_W];     // W_k^T: [out][in]
    __shared__ __attribute__((aligned(16))) float gs[GML_RT_TR * GML_RT_W];
    __shared__ __attribute__((aligned(16))) float ts[GML_RT_TR * GML_RT_W];
    const int lane = threadIdx.x % GML_WAVE, wave = threadIdx.x / GML_WAVE;
    gml_rt_load_image<true>(wts, wk, Fout, Fin, Fout);
    const int KO = (Fout + 3) & ~3;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t r0 = tile * GML_RT_TR + wave * GML_RT_RPW;
        __syncthreads();
        gml_rt_load_g(gs, dy, lddy, y, ldy, r0, N, Fout, act, wave, lane);
        gml_rt_gather_rows(ts, r0, N, Fin, gp, wave, lane, true,
                           [&](int64_t row, int c) { return cheb_gather<false>(rowptr_t, col_t, norm, g1, Fin, row, c, N); });
        __syncthreads();
        float acc[GML_RT_RPW];
#pragma unroll
        for (int r = 0; r < GML_RT_RPW; ++r) acc[r] = 0.f;
        gml_rt_prod8(gs, wts, KO, wave, lane, acc);
        if (lane < Fin) {
#pragma unroll
            for (int r = 0; r < GML_RT_RPW; ++r) {
                const int64_t row = r0 + r;
                if (row < N) {
                    float v = fmaf(ck, ts[(wave * GML_RT_RPW + r) * GML_RT_W + lane], acc[r]);
                    if (g2) v -= g2[row * Fin + lane];
                    go[row * ldgo + lane] = v;
                }
            }
        }
    }
}

extern "C" {

int gml_cheb_supported(int32_t Fin, int32_t Fout, int32_t K) {
    return K >= 1 && K <= CHEB_KMAX && Fin >= 1 && Fin <= GML_RT_W && Fout >= 1 && Fout <= GML_RT_W;
}

int gml_cheb_norm(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* batch, const float* lmax, int64_t B, float lambda,
                  int64_t N, int64_t E, float* norm, gml_stream_t stream) {
    if (N < 0 || E < 0 || (lmax && B < 1)) return GML_E_BADARG;
    if (!gml_rt_range(N, E)) return GML_E_UNSUPPORTED;
    if (N == 0) return GML_OK;
    if (!rowptr_t || (E && !col_t) || !norm) return GML_E_BADARG;
    hipLaunchKernelGGL(cheb_k_norm, dim3((unsigned)gml_cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, rowptr_t, col_t, batch, lmax, B,
                       lambda, N, norm);
    return gml_launch_status();
}

int gml_cheb_fwd(const int32_t* rowptr, const int32_t* col, const float* norm, const float* x, int64_t ldx, int64_t N, int64_t E,
                 int32_t Fin, const float* w, const float* bias, int32_t Fout, int32_t K, int32_t act, float* T, int64_t ldT, float* y,
                 int64_t ldy, gml_stream_t stream) {
    if (N < 0 || E < 0 || act < 0 || act > 2) return GML_E_BADARG;
    if (!gml_cheb_supported(Fin, Fout, K) || !gml_rt_range(N, E)) return GML_E_UNSUPPORTED;
    if (N == 0) return GML_OK;
    if (!x || !w || !y || ldx < Fin || ldy < Fout) return GML_E_BADARG;
    if (K > 1 && (!rowptr || (E && !col) || !norm || !T || ldT < (int64_t)(K - 1) * Fin)) return GML_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nt = gml_rt_tiles(N);
    const unsigned grid = gml_rt_grid(N);
    const int gp = gml_rt_gp(Fin);
    const int64_t WS = (int64_t)Fin * Fout;
    if (K == 1) {
        hipLaunchKernelGGL(cheb_k_step, dim3(grid), dim3(256), 0, st, rowptr, col, norm, x, ldx, (const float*)nullptr, (int64_t)0,
                           (const float*)nullptr, (int64_t)0, N, (int)Fin, gp, w, (const float*)nullptr, bias, (int)Fout,
                           CHEB_X0 | CHEB_LAST, (int)act, (float*)nullptr, (int64_t)0, y, ldy, nt);
        return gml_launch_status();
    }
    for (int k = 1; k < K; ++k) {
        const float* p = k == 1 ? x : T + (int64_t)(k - 2) * Fin;
        const float* q = k == 1 ? nullptr : (k == 2 ? x : T + (int64_t)(k - 3) * Fin);
        const int mode = CHEB_GATHER | (k == 1 ? CHEB_X0 : 0) | (k == K - 1 ? CHEB_LAST : 0);
        hipLaunchKernelGGL(cheb_k_step, dim3(grid), dim3(256), 0, st, rowptr, col, norm, x, ldx, p, k == 1 ? ldx : ldT, q,
                           k == 2 ? ldx : ldT, N, (int)Fin, gp, w, w + k * WS, bias, (int)Fout, mode, (int)act,
                           T + (int64_t)(k - 1) * Fin, ldT, y, ldy, nt);
    }
    return gml_launch_status();
}

int64_t gml_cheb_dflat_floats(int32_t Fin, int32_t Fout, int32_t K) {
    if (!gml_cheb_supported(Fin, Fout, K)) return 0;
    return (int64_t)K * Fin * Fout + Fout;
}

size_t gml_cheb_bwd_workspace_bytes(int64_t N, int32_t Fin, int32_t Fout, int32_t K) {
    if (N <= 0 || N > 0x7fffffff || !gml_cheb_supported(Fin, Fout, K)) return 0;
    int64_t tpw;
    int nwg;
    gml_rt_row_plan(N, &tpw, &nwg);
    // three G buffers [N, Fin] (K >= 2) | partials [workgroups, dflat floats]
    return (size_t)((K > 1 ? 3 * N * Fin : 0) + (int64_t)nwg * gml_cheb_dflat_floats(Fin, Fout, K)) * sizeof(float);
}

int gml_cheb_bwd(const int32_t* rowptr_t, const int32_t* col_t, const float* norm, const float* x, int64_t ldx, const float* T, int64_t ldT,
                 const float* y, int64_t ldy, const float* dy, int64_t lddy, int64_t N, int64_t E, int32_t Fin, const float* w, int32_t Fout,
                 int32_t K, int32_t act, float* dx, int64_t lddx, float* dflat, void* ws, size_t ws_bytes, gml_stream_t stream) {
    if (N < 0 || E < 0 || act < 0 || act > 2) return GML_E_BADARG;
    if (!gml_cheb_supported(Fin, Fout, K) || !gml_rt_range(N, E)) return GML_E_UNSUPPORTED;
    if (!dflat) return GML_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int64_t P = gml_cheb_dflat_floats(Fin, Fout, K);
    if (N == 0) {
        gml_zero_async(dflat, (size_t)P * sizeof(float), st);
        return gml_launch_status();
    }
    if (!x || !w || !y || !dy || ldx < Fin || ldy < Fout || lddy < Fout) return GML_E_BADARG;
    if (K > 1 && (!T || ldT < (int64_t)(K - 1) * Fin)) return GML_E_BADARG;
    if (dx && lddx < Fin) return GML_E_BADARG;
    if (dx && K > 1 && (!rowptr_t || (E && !col_t) || !norm)) return GML_E_BADARG;
    if (!ws || ((uintptr_t)ws & 3) || ws_bytes < gml_cheb_bwd_workspace_bytes(N, Fin, Fout, K)) return GML_E_WORKSPACE;
    int64_t tpw;
    int nwg;
    gml_rt_row_plan(N, &tpw, &nwg);
    float* G[3] = {(float*)ws, (float*)ws + N * Fin, (float*)ws + 2 * N * Fin};
    float* part = (float*)ws + (K > 1 ? 3 * N * Fin : 0);
    const int64_t nt = gml_rt_tiles(N);
    float* gl = dx ? (K == 1 ? dx : G[0]) : (float*)nullptr;                // G_{K-1} lives in G[0]
    const int64_t ldgl = K == 1 ? lddx : Fin;
#define CHEB_ROW(NK)                                                                                                                   \
    hipLaunchKernelGGL(cheb_k_bwd_r<NK>, dim3(nwg), dim3(256), 0, st, x, ldx, T, ldT, y, ldy, dy, lddy, N, (int)Fin, w, (int)Fout, (int)K, \
                       (int)act, gl, ldgl, part, P, nt, tpw)
    if (K == 1) CHEB_ROW(1);
    else if (K == 2) CHEB_ROW(2);
    else if (K <= 4) CHEB_ROW(4);
    else CHEB_ROW(8);
#undef CHEB_ROW
    if (dx && K > 1) {
        const int gp = gml_rt_gp(Fin);
        const unsigned grid = gml_rt_grid(N);
        const int64_t WS = (int64_t)Fin * Fout;
        for (int k = K - 2; k >= 0; --k) {                                  // G_m lives in G[(K - 1 - m) % 3]
            const float* g1 = G[(K - 2 - k) % 3];
            const float* g2 = k + 2 <= K - 1 ? G[(K - 3 - k) % 3] : (const float*)nullptr;
            float* go = k == 0 ? dx : G[(K - 1 - k) % 3];
            hipLaunchKernelGGL(cheb_k_bwd_a, dim3(grid), dim3(256), 0, st, rowptr_t, col_t, norm, y, ldy, dy, lddy, N, (int)Fin, gp,
                               w + k * WS, (int)Fout, (int)act, k == 0 ? 1.f : 2.f, g1, g2, go, k == 0 ? lddx : (int64_t)Fin, nt);
        }
    }
    gml_rt_fold(part, nwg, P, dflat, st);
    return gml_launch_status();
}

}  // extern "C"
