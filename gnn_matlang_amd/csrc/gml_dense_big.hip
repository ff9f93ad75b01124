// Dense support product for ONE large graph (96 < n <= 1024 nodes, F <= 64 features, any S): the 2-D grid filtering experiment
// (filtering.py: one 30 x 30 grid, recfield = 5 -> a mask that is 40 % full, S = 11).  The sparse road gives such a batch 15
// workgroups; as dense blocks the layer [S n, n] x [n, F] cuts into (support, row block, K slice) items that fill the machine.
//
//      out[r ldo + s so + f]  (=, or summed over s when sum_s)   sum_k  D[s][r][k] . act[k lda + s sa + f]
//
//   forward :  D = the stored blocks (row = target node), act = X (sa = 0), out = Hcat [n, S Fin] (so = Fin);
//   adjoint :  D = the transposed blocks, act = d Hcat (sa = Fin), sum_s = 1 -> d X.
//
// Images as in gml_dense.hip: bf16 (hi, lo) [S][2][n][KP], KP = 32 ceil(n / 32), columns >= n zero (gml_dense_big_pack).
// Machine mapping: a workgroup of 4 waves owns (support s, 64 rows, K slice kc); a wave owns 16 rows.  A lane's support operand
// (its row, 8 consecutive k) is one 16-byte load from HBM / L2, issued for a whole K chunk (128 k) before the chunk's activation
// rows are staged, so that the loads fly during the staging.  The activation panel does not fit LDS at n = 1024 (1024 x 64 fp32
// as hi and lo images = 256 KB): K is walked in chunks of 128 rows, each staged as fp32 -> (hi, lo) row-major images [k][f] and
// read back transposed by ds_read_b64_tr_b16 (the operand layout of gml_k_dense_support_mm).  Rows k >= n of act do not exist:
// they are never read, their image rows are zeros.  bf16x3 (hi.hi + lo.hi + hi.lo) in fp32 accumulators.
//
// Without a K split and without the sum over s an item writes its tile of out itself.  Otherwise it writes a partial tile
// ws[s nks + kc][n][F] and gml_k_dense_big_fold adds the partials of an output element in ascending (s, kc) order: no float
// atomics, the same bits on every run.
#include "gml_common.h"

#define DB_ROWS 64                                           // rows per workgroup (4 waves x 16)
#define DB_CH 4                                              // K = 32 steps per staged chunk
#define DB_MAXN 1024
#define DB_MAXF 64

struct GmlDenseBigParams {
    const uint16_t* dimg;
    const float* act;
    float* out;                                              // direct: out; otherwise the partial tiles
    int64_t lda, ldo;                                        // (partials: ldo = F, so = 0)
    int32_t sa, so, S, n, KP, F, nrb, nks, direct, vec_in, vec_out;
};

__device__ __forceinline__ uint32_t db_pack2(float a, float b) {             // v_cvt_pk_bf16_f32 (RNE)
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{a, b}, bf16x2));
}
#define DB_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)
// image row pitch in bytes: 32 bytes per 16-feature tile + 16 (gml_dense.hip: dn_pitch)
__host__ __device__ constexpr int db_pitch(int nft) { return 32 * nft + (nft == 1 ? 0 : 16); }

template <int NFT>
__global__ __launch_bounds__(256) void gml_k_dense_big_mm(GmlDenseBigParams p) {
    constexpr int PA = db_pitch(NFT);
    constexpr int NCH = 4 * NFT;                             // 8-byte chunks (4 features) per image row
    constexpr int CK = 32 * DB_CH;                           // staged k rows
    __shared__ __attribute__((aligned(16))) unsigned char img_h[CK * PA];
    __shared__ __attribute__((aligned(16))) unsigned char img_l[CK * PA];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t16 = lane & 15, kq = lane >> 4;
    const int n = p.n, KP = p.KP, KS = KP >> 5, F = p.F;
    const int item = blockIdx.x;
    const int kc = item % p.nks, rb = (item / p.nks) % p.nrb, s = item / (p.nks * p.nrb);
    const int ks0 = (int)((int64_t)kc * KS / p.nks), ks1 = (int)((int64_t)(kc + 1) * KS / p.nks);
    const int row = rb * DB_ROWS + wave * 16 + t16;          // this lane's support row (the column of the transposed product)
    const int rowc = row < n ? row : n - 1;
    const float* a = p.act + (int64_t)s * p.sa;
    const uint16_t* dh = p.dimg + ((int64_t)s * 2 * n + rowc) * KP + 8 * kq;
    const uint16_t* dl = dh + (int64_t)n * KP;
    // transposing-read addresses: lane (t, kq) passes row 8 kq + (t >> 2) (+ 4 for the second read), 8-byte chunk (t & 3)
    const int aoff = (8 * kq + (t16 >> 2)) * PA + 8 * (t16 & 3);

    f32x4 acc[NFT];
#pragma unroll
    for (int ft = 0; ft < NFT; ++ft) acc[ft] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int kb = ks0; kb < ks1; kb += DB_CH) {
        // support operand of this lane for the chunk: row rowc, k = 32 ks + 8 kq .. + 7 of the hi and the lo image
        u32x4 bh[DB_CH], bl[DB_CH];
#pragma unroll
        for (int j = 0; j < DB_CH; ++j) {
            const int ks = kb + j < ks1 ? kb + j : ks1 - 1;  // (clamped: the loads stay unconditional, the product skips them)
            bh[j] = *reinterpret_cast<const u32x4*>(dh + 32 * ks);
            bl[j] = *reinterpret_cast<const u32x4*>(dl + 32 * ks);
        }
        if (kb > ks0) __syncthreads();                       // every wave is done with the previous chunk
        const int kbase = 32 * kb, krows = 32 * min(DB_CH, ks1 - kb);
        for (int idx = tid; idx < krows * NCH; idx += 256) { // act[k][s sa : s sa + F] -> (hi, lo) images [k][f]
            const int kl = idx / NCH, ch = idx % NCH, k = kbase + kl;
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (k < n && 4 * ch < F) {
                const float* q = a + (int64_t)k * p.lda + 4 * ch;
                if (p.vec_in) v = *reinterpret_cast<const f32x4*>(q);
                else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) if (4 * ch + j < F) v[j] = q[j];
                }
            }
            const uint32_t h0 = db_pack2(v[0], v[1]), h1 = db_pack2(v[2], v[3]);
            const uint32_t l0 = db_pack2(v[0] - __uint_as_float(h0 << 16), v[1] - __uint_as_float(h0 & 0xffff0000u));
            const uint32_t l1 = db_pack2(v[2] - __uint_as_float(h1 << 16), v[3] - __uint_as_float(h1 & 0xffff0000u));
            *reinterpret_cast<uint2*>(img_h + kl * PA + 8 * ch) = uint2{h0, h1};
            *reinterpret_cast<uint2*>(img_l + kl * PA + 8 * ch) = uint2{l0, l1};
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < DB_CH; ++j) {
            if (kb + j < ks1) {
                const bf16x8 Bh = __builtin_bit_cast(bf16x8, bh[j]), Bl = __builtin_bit_cast(bf16x8, bl[j]);
                const unsigned char* ah = img_h + 32 * j * PA + aoff;
                const unsigned char* al = img_l + 32 * j * PA + aoff;
#pragma unroll
                for (int ft = 0; ft < NFT; ++ft) {
                    const bf16x8 Ah = gml_tr_frag(ah + 32 * ft, ah + 32 * ft + 4 * PA);
                    const bf16x8 Al = gml_tr_frag(al + 32 * ft, al + 32 * ft + 4 * PA);
                    acc[ft] = DB_MFMA(Al, Bh, acc[ft]);
                    acc[ft] = DB_MFMA(Ah, Bl, acc[ft]);
                    acc[ft] = DB_MFMA(Ah, Bh, acc[ft]);
                }
            }
        }
    }
    if (row >= n) return;
    // the lane holds features 16 ft + 4 kq .. + 3 of its own row
    float* o = p.direct ? p.out + (int64_t)row * p.ldo + (int64_t)s * p.so + 4 * kq
                        : p.out + ((int64_t)(s * p.nks + kc) * n + row) * F + 4 * kq;
#pragma unroll
    for (int ft = 0; ft < NFT; ++ft) {
        const int f0 = 16 * ft + 4 * kq;
        if (f0 >= F) continue;
        if (p.vec_out) *reinterpret_cast<f32x4*>(o + 16 * ft) = acc[ft];
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (f0 + j < F) o[16 * ft + j] = acc[ft][j];
        }
    }
}

// out[r ldo + g so + f] = sum of the partial tiles part[(g npg + q)][r][f], q = 0 .. npg - 1 ascending; groups g = supports
// (npg = nks) or one group of all S nks tiles (sum_s)
__global__ __launch_bounds__(256) void gml_k_dense_big_fold(const float* __restrict__ part, float* __restrict__ out, int64_t ldo,
                                                            int so, int ngroups, int npg, int n, int F) {
    const int64_t total = (int64_t)ngroups * n * F;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int f = (int)(i % F), r = (int)((i / F) % n), g = (int)(i / ((int64_t)F * n));
    const float* q = part + ((int64_t)g * npg * n + r) * F + f;
    float a = 0.f;
    for (int j = 0; j < npg; ++j) a += q[(int64_t)j * n * F];
    out[(int64_t)r * ldo + (int64_t)g * so + f] = a;
}

// K slices per (support, row block): the forward writes its tiles itself once (support, row block) items alone fill half the
// machine; the adjoint folds anyway (the sum over s), so it is cut until about two items per CU exist.  A slice keeps >= 2 steps.
static int db_nks(int S, int n, int KP, int sum_s) {
    const int64_t base = (int64_t)S * gml_cdiv(n, DB_ROWS);
    const int KS = KP / 32;
    if (!sum_s && base >= GML_NUM_CU / 2) return 1;
    int64_t nks = gml_cdiv(2 * GML_NUM_CU, base);
    if (nks > KS / 2) nks = KS / 2;
    return nks < 1 ? 1 : (int)nks;
}

static int db_supported(int S, int n, int KP, int F) {
    return n > 96 && n <= DB_MAXN && KP % 32 == 0 && KP >= n && KP < n + 32 && F >= 1 && F <= DB_MAXF && S >= 1;
}

extern "C" size_t gml_dense_big_workspace_bytes(int32_t S, int32_t n, int32_t F, int32_t sum_s) {
    const int KP = (n + 31) / 32 * 32;
    if (!db_supported(S, n, KP, F)) return 0;
    const int nks = db_nks(S, n, KP, sum_s);
    if (nks == 1 && !sum_s) return 0;
    return (size_t)S * nks * n * F * sizeof(float);
}

__global__ __launch_bounds__(256) void gml_k_dense_big_pack(const float* __restrict__ blocks, uint16_t* __restrict__ img,
                                                            int64_t nblocks, int n, int KP, int transpose) {
    const int64_t total = nblocks * n * KP;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int k = (int)(i % KP);
        const int r = (int)((i / KP) % n);
        const int64_t blk = i / ((int64_t)KP * n);
        float v = 0.f;
        if (k < n) v = blocks[blk * n * n + (transpose ? (int64_t)k * n + r : (int64_t)r * n + k)];
        const uint32_t h = db_pack2(v, 0.f) & 0xffffu;
        const uint32_t l = db_pack2(v - __uint_as_float(h << 16), 0.f) & 0xffffu;
        img[(blk * 2) * n * KP + (int64_t)r * KP + k] = (uint16_t)h;
        img[(blk * 2 + 1) * n * KP + (int64_t)r * KP + k] = (uint16_t)l;
    }
}

extern "C" int gml_dense_big_pack(const float* blocks, uint16_t* img, int64_t nblocks, int32_t n, int32_t KP, int32_t transpose,
                                  void* stream) {
    if (blocks == nullptr || img == nullptr) return GML_E_BADARG;
    if (!db_supported(1, n, KP, 1) || nblocks < 0) return GML_E_UNSUPPORTED;
    if (nblocks == 0) return GML_OK;
    int64_t grid = gml_cdiv(nblocks * n * KP, 256);
    if (grid > 64 * GML_NUM_CU) grid = 64 * GML_NUM_CU;
    hipLaunchKernelGGL(gml_k_dense_big_pack, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, blocks, img, nblocks, n, KP,
                       transpose);
    return gml_launch_status();
}

extern "C" int gml_dense_big_support_mm(const uint16_t* dimg, const float* act, int64_t lda, int32_t sa, float* out, int64_t ldo,
                                        int32_t so, int32_t sum_s, int32_t S, int32_t n, int32_t KP, int32_t F, void* ws,
                                        size_t ws_bytes, void* stream) {
    if (dimg == nullptr || act == nullptr || out == nullptr || lda < F || ldo < F || sa < 0 || so < 0) return GML_E_BADARG;
    if (!db_supported(S, n, KP, F)) return GML_E_UNSUPPORTED;
    if (lda < (int64_t)(S - 1) * sa + F || (!sum_s && ldo < (int64_t)(S - 1) * so + F)) return GML_E_BADARG;
    GmlDenseBigParams p;
    p.nks = db_nks(S, n, KP, sum_s);
    p.direct = (p.nks == 1 && !sum_s) ? 1 : 0;
    const size_t need = p.direct ? 0 : (size_t)S * p.nks * n * F * sizeof(float);
    if (need > 0 && (ws == nullptr || ws_bytes < need || ((uintptr_t)ws & 15) != 0)) return GML_E_WORKSPACE;
    p.dimg = dimg; p.act = act; p.lda = lda; p.sa = sa; p.S = S; p.n = n; p.KP = KP; p.F = F;
    p.nrb = (int)gml_cdiv(n, DB_ROWS);
    p.vec_in = (F % 4 == 0 && lda % 4 == 0 && sa % 4 == 0 && ((uintptr_t)act & 15) == 0) ? 1 : 0;
    if (p.direct) {
        p.out = out; p.ldo = ldo; p.so = so;
        p.vec_out = (F % 4 == 0 && ldo % 4 == 0 && so % 4 == 0 && ((uintptr_t)out & 15) == 0) ? 1 : 0;
    } else {
        p.out = (float*)ws; p.ldo = F; p.so = 0;
        p.vec_out = F % 4 == 0 ? 1 : 0;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(S * p.nrb * p.nks));
    const int nft = (F + 15) / 16;
    if (nft <= 1) hipLaunchKernelGGL(gml_k_dense_big_mm<1>, grid, dim3(256), 0, st, p);
    else if (nft == 2) hipLaunchKernelGGL(gml_k_dense_big_mm<2>, grid, dim3(256), 0, st, p);
    else if (nft == 3) hipLaunchKernelGGL(gml_k_dense_big_mm<3>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(gml_k_dense_big_mm<4>, grid, dim3(256), 0, st, p);
    int rc = gml_launch_status();
    if (rc != GML_OK || p.direct) return rc;
    const int ngroups = sum_s ? 1 : S, npg = sum_s ? S * p.nks : p.nks;
    hipLaunchKernelGGL(gml_k_dense_big_fold, dim3((unsigned)gml_cdiv((int64_t)ngroups * n * F, 256)), dim3(256), 0, st,
                       (const float*)ws, out, ldo, sum_s ? 0 : so, ngroups, npg, n, F);
    return gml_launch_status();
}
