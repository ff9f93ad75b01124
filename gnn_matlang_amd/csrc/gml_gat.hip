// GAT: the edge-softmax attention of GATConv (torch_geometric 1.6.1, concat=True, negative_slope 0.2) behind the projection
// xl = x W^T (include/gml.h: gml_gat_*).  H = 8 heads of C channels; a row of xl is H C floats, head h = columns [h C, (h + 1) C).
//
// One lane owns FOUR consecutive channels of one row (a float4; C % 4 == 0, so they lie in one head): a row takes G = 2 C lanes, padded
// to a power of two GP, and a wave serves 64 / GP rows at once (C = 8: four rows, 12 and 16: two, 32: one).  Every lane walks its row's
// edges, gathers its float4 of the neighbour's row and evaluates its head's logit itself (C / 4 lanes repeat one expf; no lane idles
// while others loop).  Lanes beyond G (C = 12: 8 of 32) mirror lane 0 of their row and store nothing.
//
//   logits    al[n, h] = <xl[n, h], att_l[h]>,  ar likewise                              one thread per (n, h), c ascending
//   forward   max over the row, then p = exp(e - m), z, sum p xl[j]; y = act(./(z + 1e-16) + bias); m, z out     self edge first
//   backward  T  target view: g = dy act'(y); d_e = <g[i, h], xl[j, h] - xl[i, h]> = dalpha_e - dalpha_self (the head's lanes summed in
//                lane order) -> da[k, h]; S = sum alpha d; dar = sum slope alpha d - S sum slope alpha; node record {ar, m,
//                1 / (z + 1e-16), S}
//             S  source view: ds_e = slope alpha (da[pos_t[k]] - S[i]); dal = sum ds; dxl = sum alpha g[i] + dal att_l + dar att_r
//             R  per-workgroup partials of datt_l, datt_r, dbias over contiguous row ranges, then one fold in workgroup order
// No atomics; every sum has one order.  Entries with col == row are skipped (the one self edge per node is implicit).
#include "gml_common.h"

#define GAT_H 8
#define GAT_SLOPE 0.2f
#define GAT_EPS 1e-16f
#define GAT_MAXWG 1024      // partials of the reduction

static __device__ __forceinline__ float gat_leaky(float s) { return s > 0.f ? s : GAT_SLOPE * s; }
static __device__ __forceinline__ float gat_slope(float s) { return s > 0.f ? 1.f : GAT_SLOPE; }

static __device__ __forceinline__ float gat_act(float v, int act) {
    if (act == 1) return fmaxf(v, 0.f);
    if (act == 2) return tanhf(v);
    if (act == 3) return v > 0.f ? v : expm1f(v);
    return v;
}
// act'(pre-activation) as a function of y = act(pre-activation)
static __device__ __forceinline__ float gat_dact(float y, int act) {
    if (act == 1) return y > 0.f ? 1.f : 0.f;
    if (act == 2) return 1.f - y * y;
    if (act == 3) return y > 0.f ? 1.f : y + 1.f;
    return 1.f;
}

template <int C>
struct GatMap {
    static constexpr int G = 2 * C;                                               // lanes of one row
    static constexpr int GP = G <= 8 ? 8 : (G <= 16 ? 16 : (G <= 32 ? 32 : 64));  // ... padded to a power of two
    static constexpr int RPW = 64 / GP;                                           // rows of one wave
    static constexpr int LPH = C / 4;                                             // lanes of one head
    static constexpr int HC = GAT_H * C;
};

static __global__ void gat_k_logits(const float* __restrict__ xl, int64_t ldxl, const float* __restrict__ att_l,
                                    const float* __restrict__ att_r, int64_t N, int C, float* __restrict__ al, float* __restrict__ ar) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N * GAT_H) return;
    const int64_t n = t / GAT_H;
    const int h = (int)(t % GAT_H);
    const float* x = xl + n * ldxl + h * C;
    float sl = 0.f, sr = 0.f;
    for (int c = 0; c < C; ++c) {
        const float v = x[c];
        sl = fmaf(v, att_l[h * C + c], sl);
        sr = fmaf(v, att_r[h * C + c], sr);
    }
    al[t] = sl;
    ar[t] = sr;
}

template <int C>
static __global__ __launch_bounds__(256) void gat_k_fwd(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                        const float* __restrict__ xl, int64_t ldxl, const float* __restrict__ al,
                                                        const float* __restrict__ ar, const float* __restrict__ bias, int64_t N, int act,
                                                        float* __restrict__ y, int64_t ldy, float* __restrict__ m, float* __restrict__ z) {
    typedef GatMap<C> M;
    const int lane = threadIdx.x % GML_WAVE, wave = threadIdx.x / GML_WAVE;
    const int q = lane % M::GP;
    const bool active = q < M::G;
    const int qq = active ? q : 0;
    const int64_t row = ((int64_t)blockIdx.x * 4 + wave) * M::RPW + lane / M::GP;
    if (row >= N) return;
    const int c0 = qq * 4, h = c0 / C;
    const int k0 = rowptr[row], k1 = rowptr[row + 1];
    const float ari = ar[row * GAT_H + h];
    const float eself = gat_leaky(al[row * GAT_H + h] + ari);
    float mx = eself;
    for (int k = k0; k < k1; ++k) {
        const int64_t j = col[k];
        if (j == row || j < 0 || j >= N) continue;
        mx = fmaxf(mx, gat_leaky(al[j * GAT_H + h] + ari));
    }
    float zz = expf(eself - mx);
    f32x4 v = *reinterpret_cast<const f32x4*>(xl + row * ldxl + c0);
    f32x4 acc = zz * v;
    for (int k = k0; k < k1; ++k) {
        const int64_t j = col[k];
        if (j == row || j < 0 || j >= N) continue;
        const float p = expf(gat_leaky(al[j * GAT_H + h] + ari) - mx);
        v = *reinterpret_cast<const f32x4*>(xl + j * ldxl + c0);
        zz += p;
        acc.x = fmaf(p, v.x, acc.x); acc.y = fmaf(p, v.y, acc.y); acc.z = fmaf(p, v.z, acc.z); acc.w = fmaf(p, v.w, acc.w);
    }
    if (!active) return;
    const float inv = 1.f / (zz + GAT_EPS);
    f32x4 b = f32x4{0.f, 0.f, 0.f, 0.f};
    if (bias) b = *reinterpret_cast<const f32x4*>(bias + c0);
    f32x4 o;
    o.x = gat_act(fmaf(acc.x, inv, b.x), act); o.y = gat_act(fmaf(acc.y, inv, b.y), act);
    o.z = gat_act(fmaf(acc.z, inv, b.z), act); o.w = gat_act(fmaf(acc.w, inv, b.w), act);
    *reinterpret_cast<f32x4*>(y + row * ldy + c0) = o;
    if (qq % M::LPH == 0) {
        m[row * GAT_H + h] = mx;
        z[row * GAT_H + h] = zz;
    }
}

// target view.  rec[i] = {ar[i, :], m[i, :], 1 / (z[i, :] + 1e-16), S[i, :]}: what the source view gathers per edge, one 128-byte record
template <int C>
static __global__ __launch_bounds__(256) void gat_k_bwd_t(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                          const float* __restrict__ xl, int64_t ldxl, const float* __restrict__ al,
                                                          const float* __restrict__ ar, const float* __restrict__ m,
                                                          const float* __restrict__ z, const float* __restrict__ y, int64_t ldy,
                                                          const float* __restrict__ dy, int64_t lddy, int64_t N, int act,
                                                          float* __restrict__ g, float* __restrict__ da, float* __restrict__ rec,
                                                          float* __restrict__ dar) {
    typedef GatMap<C> M;
    const int lane = threadIdx.x % GML_WAVE, wave = threadIdx.x / GML_WAVE;
    const int q = lane % M::GP;
    const bool active = q < M::G;
    const int qq = active ? q : 0;
    const int64_t row = ((int64_t)blockIdx.x * 4 + wave) * M::RPW + lane / M::GP;
    if (row >= N) return;
    const int c0 = qq * 4, h = c0 / C;
    const int hb = (lane / M::GP) * M::GP + h * M::LPH;                           // first lane of this head in the wave
    const bool lead = active && qq % M::LPH == 0;
    const f32x4 yv = *reinterpret_cast<const f32x4*>(y + row * ldy + c0);
    const f32x4 dv = *reinterpret_cast<const f32x4*>(dy + row * lddy + c0);
    f32x4 gv;
    gv.x = dv.x * gat_dact(yv.x, act); gv.y = dv.y * gat_dact(yv.y, act);
    gv.z = dv.z * gat_dact(yv.z, act); gv.w = dv.w * gat_dact(yv.w, act);
    if (active) *reinterpret_cast<f32x4*>(g + row * M::HC + c0) = gv;
    const int k0 = rowptr[row], k1 = rowptr[row + 1];
    const float ari = ar[row * GAT_H + h], mi = m[row * GAT_H + h];
    const float inv = 1.f / (z[row * GAT_H + h] + GAT_EPS);
    // <g[i, h], xl[j, h]>: four channels here, then the head's lanes in ascending lane order (every lane of the head: the same bits)
    auto headdot = [&](const f32x4& v) {
        const float d = fmaf(gv.w, v.w, fmaf(gv.z, v.z, fmaf(gv.y, v.y, gv.x * v.x)));
        float s = 0.f;
#pragma unroll
        for (int t = 0; t < M::LPH; ++t) s += __shfl(d, hb + t);
        return s;
    };
    // Everything about the row is taken RELATIVE to its self edge: d_e = <g[i, h], xl[j, h] - xl[i, h]> = dalpha_e - dalpha_self.  The
    // softmax gradient alpha (dalpha - sum alpha dalpha) does not change under a shift of dalpha, and the differences keep their digits
    // where neighbouring rows are alike (sum alpha dalpha and dalpha then agree to many places and would cancel).
    const f32x4 vs = *reinterpret_cast<const f32x4*>(xl + row * ldxl + c0);
    float S = 0.f, A1 = 0.f, A2;
    {
        const float s = al[row * GAT_H + h] + ari;
        A2 = gat_slope(s) * (expf(gat_leaky(s) - mi) * inv);                      // (the self edge: d = 0)
    }
    for (int k = k0; k < k1; ++k) {
        const int64_t j = col[k];
        if (j == row || j < 0 || j >= N) {                                        // (the same answer in every lane of the row)
            if (lead) da[(int64_t)k * GAT_H + h] = 0.f;
            continue;
        }
        const float s = al[j * GAT_H + h] + ari;
        const float a = expf(gat_leaky(s) - mi) * inv;
        const f32x4 v = *reinterpret_cast<const f32x4*>(xl + j * ldxl + c0);
        const float d = headdot(v - vs);
        const float sa = gat_slope(s) * a;
        S = fmaf(a, d, S); A1 = fmaf(sa, d, A1); A2 += sa;
        if (lead) da[(int64_t)k * GAT_H + h] = d;
    }
    if (lead) {
        float* r = rec + row * (4 * GAT_H) + h;
        r[0] = ari; r[GAT_H] = mi; r[2 * GAT_H] = inv; r[3 * GAT_H] = S;
        dar[row * GAT_H + h] = fmaf(-S, A2, A1);
    }
}

// source view
template <int C>
static __global__ __launch_bounds__(256) void gat_k_bwd_s(const int32_t* __restrict__ rowptr_t, const int32_t* __restrict__ col_t,
                                                          const int32_t* __restrict__ pos_t, const float* __restrict__ al,
                                                          const float* __restrict__ g, const float* __restrict__ da,
                                                          const float* __restrict__ rec, const float* __restrict__ dar,
                                                          const float* __restrict__ att_l, const float* __restrict__ att_r, int64_t N,
                                                          int64_t E, float* __restrict__ dxl, int64_t lddxl, float* __restrict__ dal) {
    typedef GatMap<C> M;
    const int lane = threadIdx.x % GML_WAVE, wave = threadIdx.x / GML_WAVE;
    const int q = lane % M::GP;
    const bool active = q < M::G;
    const int qq = active ? q : 0;
    const int64_t row = ((int64_t)blockIdx.x * 4 + wave) * M::RPW + lane / M::GP;
    if (row >= N) return;
    const int c0 = qq * 4, h = c0 / C;
    const int k0 = rowptr_t[row], k1 = rowptr_t[row + 1];
    const float alj = al[row * GAT_H + h];
    float dsum;
    f32x4 acc;
    {
        const float* r = rec + row * (4 * GAT_H) + h;
        const float s = alj + r[0];
        const float a = expf(gat_leaky(s) - r[GAT_H]) * r[2 * GAT_H];
        dsum = gat_slope(s) * a * (0.f - r[3 * GAT_H]);                            // (the self edge: d = 0)
        acc = a * *reinterpret_cast<const f32x4*>(g + row * M::HC + c0);
    }
    for (int k = k0; k < k1; ++k) {
        const int64_t i = col_t[k];
        const int64_t kk = pos_t[k];
        if (i == row || i < 0 || i >= N || kk < 0 || kk >= E) continue;
        const float* r = rec + i * (4 * GAT_H) + h;
        const float s = alj + r[0];
        const float a = expf(gat_leaky(s) - r[GAT_H]) * r[2 * GAT_H];
        dsum = fmaf(gat_slope(s) * a, da[kk * GAT_H + h] - r[3 * GAT_H], dsum);
        const f32x4 v = *reinterpret_cast<const f32x4*>(g + i * M::HC + c0);
        acc.x = fmaf(a, v.x, acc.x); acc.y = fmaf(a, v.y, acc.y); acc.z = fmaf(a, v.z, acc.z); acc.w = fmaf(a, v.w, acc.w);
    }
    if (!active) return;
    const f32x4 wl = *reinterpret_cast<const f32x4*>(att_l + c0), wr = *reinterpret_cast<const f32x4*>(att_r + c0);
    const float dr = dar[row * GAT_H + h];
    f32x4 o;
    o.x = fmaf(dr, wr.x, fmaf(dsum, wl.x, acc.x)); o.y = fmaf(dr, wr.y, fmaf(dsum, wl.y, acc.y));
    o.z = fmaf(dr, wr.z, fmaf(dsum, wl.z, acc.z)); o.w = fmaf(dr, wr.w, fmaf(dsum, wl.w, acc.w));
    *reinterpret_cast<f32x4*>(dxl + row * lddxl + c0) = o;
    if (qq % M::LPH == 0) dal[row * GAT_H + h] = dsum;
}

// part[wg][0 | 1 | 2][t] = sum over the rows [wg rpw, (wg + 1) rpw) of dal[n, h] xl[n, t] | dar[n, h] xl[n, t] | g[n, t], n ascending
static __global__ void gat_k_red(const float* __restrict__ xl, int64_t ldxl, const float* __restrict__ g, const float* __restrict__ dal,
                                 const float* __restrict__ dar, int64_t N, int C, int64_t rpw, float* __restrict__ part) {
    const int t = threadIdx.x, HC = GAT_H * C;
    if (t >= HC) return;
    const int h = t / C;
    const int64_t r0 = (int64_t)blockIdx.x * rpw, r1 = r0 + rpw < N ? r0 + rpw : N;
    float sl = 0.f, sr = 0.f, sb = 0.f;
    for (int64_t n = r0; n < r1; ++n) {
        const float x = xl[n * ldxl + t];
        sl = fmaf(dal[n * GAT_H + h], x, sl);
        sr = fmaf(dar[n * GAT_H + h], x, sr);
        sb += g[n * HC + t];
    }
    float* out = part + (int64_t)blockIdx.x * 3 * HC + t;
    out[0] = sl; out[HC] = sr; out[2 * HC] = sb;
}

// workgroups in ascending order
static __global__ void gat_k_fold(const float* __restrict__ part, int nwg, int HC, float* __restrict__ datt_l, float* __restrict__ datt_r,
                                  float* __restrict__ dbias) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 3 * HC) return;
    float* dst = e < HC ? datt_l : (e < 2 * HC ? datt_r : dbias);
    if (!dst) return;
    float s = 0.f;
    for (int w = 0; w < nwg; ++w) s += part[(int64_t)w * 3 * HC + e];
    dst[e % HC] = s;
}

// ---------------------------------------------------------------------------------------------------------------- host
static inline bool gat_rows4(const void* p, int64_t ld, int HC) { return ((uintptr_t)p & 15) == 0 && ld % 4 == 0 && ld >= HC; }
static inline int gat_red_wgs(int64_t N) {
    const int64_t w = gml_cdiv(N, 64);
    return (int)(w < 1 ? 1 : (w > GAT_MAXWG ? GAT_MAXWG : w));
}
template <int C>
static inline unsigned gat_blocks(int64_t N) { return (unsigned)gml_cdiv(N, 4 * GatMap<C>::RPW); }

#define GAT_DISPATCH(C, CALL) \
    switch (C) {              \
    case 4: CALL(4); break;   \
    case 8: CALL(8); break;   \
    case 12: CALL(12); break; \
    case 16: CALL(16); break; \
    default: CALL(32); break; \
    }

extern "C" {

int gml_gat_supported(int32_t H, int32_t C) { return H == GAT_H && (C == 4 || C == 8 || C == 12 || C == 16 || C == 32); }

int gml_gat_logits(const float* xl, int64_t ldxl, const float* att_l, const float* att_r, int64_t N, int32_t H, int32_t C, float* al,
                   float* ar, gml_stream_t stream) {
    if (N < 0) return GML_E_BADARG;
    if (!gml_gat_supported(H, C) || N > 0x7fffffff / (4 * GAT_H)) return GML_E_UNSUPPORTED;
    if (N == 0) return GML_OK;
    if (!xl || !att_l || !att_r || !al || !ar || ldxl < H * C) return GML_E_BADARG;
    hipLaunchKernelGGL(gat_k_logits, dim3((unsigned)gml_cdiv(N * GAT_H, 256)), dim3(256), 0, (hipStream_t)stream, xl, ldxl, att_l, att_r, N,
                       (int)C, al, ar);
    return gml_launch_status();
}

int gml_gat_fwd(const int32_t* rowptr, const int32_t* col, const float* xl, int64_t ldxl, const float* al, const float* ar,
                const float* bias, int64_t N, int64_t E, int32_t H, int32_t C, int32_t act, float* y, int64_t ldy, float* m, float* z,
                gml_stream_t stream) {
    if (N < 0 || E < 0 || act < 0 || act > 3) return GML_E_BADARG;
    if (!gml_gat_supported(H, C) || N > 0x7fffffff / (4 * GAT_H) || E > 0x7fffffff / GAT_H) return GML_E_UNSUPPORTED;
    if (N == 0) return GML_OK;
    if (!rowptr || (E && !col) || !xl || !al || !ar || !y || !m || !z) return GML_E_BADARG;
    const int HC = H * C;
    if (!gat_rows4(xl, ldxl, HC) || !gat_rows4(y, ldy, HC) || (bias && ((uintptr_t)bias & 15))) return GML_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
#define GAT_FWD(CC) hipLaunchKernelGGL(gat_k_fwd<CC>, dim3(gat_blocks<CC>(N)), dim3(256), 0, st, rowptr, col, xl, ldxl, al, ar, bias, N, \
                                       (int)act, y, ldy, m, z)
    GAT_DISPATCH(C, GAT_FWD)
#undef GAT_FWD
    return gml_launch_status();
}

size_t gml_gat_bwd_workspace_bytes(int64_t N, int64_t E, int32_t H, int32_t C) {
    if (N <= 0 || E < 0 || !gml_gat_supported(H, C)) return 0;
    const int64_t HC = (int64_t)H * C;
    // g [N, HC] | rec [N, 4 H] | dar, dal [N, H] each | da [E, H] | partials [wgs, 3, HC]
    return (size_t)(N * HC + N * 6 * GAT_H + E * GAT_H + (int64_t)gat_red_wgs(N) * 3 * HC) * sizeof(float);
}

int gml_gat_bwd(const int32_t* rowptr, const int32_t* col, const int32_t* rowptr_t, const int32_t* col_t, const int32_t* pos_t,
                const float* xl, int64_t ldxl, const float* al, const float* ar, const float* m, const float* z, const float* y,
                int64_t ldy, const float* dy, int64_t lddy, const float* att_l, const float* att_r, int64_t N, int64_t E, int32_t H,
                int32_t C, int32_t act, float* dxl, int64_t lddxl, float* datt_l, float* datt_r, float* dbias, void* ws,
                size_t ws_bytes, gml_stream_t stream) {
    if (N < 0 || E < 0 || act < 0 || act > 3) return GML_E_BADARG;
    if (!gml_gat_supported(H, C) || N > 0x7fffffff / (4 * GAT_H) || E > 0x7fffffff / GAT_H) return GML_E_UNSUPPORTED;
    if (!datt_l || !datt_r) return GML_E_BADARG;
    const int HC = H * C;
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {
        gml_zero_async(datt_l, (size_t)HC * sizeof(float), st);
        gml_zero_async(datt_r, (size_t)HC * sizeof(float), st);
        if (dbias) gml_zero_async(dbias, (size_t)HC * sizeof(float), st);
        return gml_launch_status();
    }
    if (!rowptr || !rowptr_t || (E && (!col || !col_t || !pos_t)) || !xl || !al || !ar || !m || !z || !y || !dy || !att_l || !att_r || !dxl)
        return GML_E_BADARG;
    if (!gat_rows4(xl, ldxl, HC) || !gat_rows4(y, ldy, HC) || !gat_rows4(dy, lddy, HC) || !gat_rows4(dxl, lddxl, HC) ||
        ((uintptr_t)att_l & 15) || ((uintptr_t)att_r & 15))
        return GML_E_UNSUPPORTED;
    if (!ws || ((uintptr_t)ws & 15) || ws_bytes < gml_gat_bwd_workspace_bytes(N, E, H, C)) return GML_E_WORKSPACE;
    float* g = (float*)ws;
    float* rec = g + N * HC;
    float* dar = rec + N * 4 * GAT_H;
    float* dal = dar + N * GAT_H;
    float* da = dal + N * GAT_H;
    float* part = da + E * GAT_H;
    const int nwg = gat_red_wgs(N);
    const int64_t rpw = gml_cdiv(N, nwg);
#define GAT_BWD(CC)                                                                                                                     \
    do {                                                                                                                                \
        hipLaunchKernelGGL(gat_k_bwd_t<CC>, dim3(gat_blocks<CC>(N)), dim3(256), 0, st, rowptr, col, xl, ldxl, al, ar, m, z, y, ldy, dy, \
                           lddy, N, (int)act, g, da, rec, dar);                                                                         \
        hipLaunchKernelGGL(gat_k_bwd_s<CC>, dim3(gat_blocks<CC>(N)), dim3(256), 0, st, rowptr_t, col_t, pos_t, al, g, da, rec, dar,     \
                           att_l, att_r, N, E, dxl, lddxl, dal);                                                                        \
    } while (0)
    GAT_DISPATCH(C, GAT_BWD)
#undef GAT_BWD
    hipLaunchKernelGGL(gat_k_red, dim3(nwg), dim3((HC + 63) / 64 * 64), 0, st, xl, ldxl, g, dal, dar, N, (int)C, rpw, part);
    hipLaunchKernelGGL(gat_k_fold, dim3((3 * HC + 255) / 256), dim3(256), 0, st, part, nwg, HC, datt_l, datt_r, dbias);
    return gml_launch_status();
}

}  // extern "C"
