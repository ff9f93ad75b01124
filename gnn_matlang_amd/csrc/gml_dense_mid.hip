// Dense support product for a BATCH of equal-size graphs of 96 < n <= 256 nodes (F <= 128 features, any S): the size class between
// gml_dense.hip (B graphs of n <= 96, one workgroup per graph) and gml_dense_big.hip (ONE graph of up to 1024 nodes).  freqclass.py
// trains GNNML3 on graphs of 200 nodes whose 2-hop masks are 6-8 % full (S = 6, layers 66 -> 64 + 2).
//
//      out[(b n + r) ldo + s so + f]  (=, or summed over s when sum_s)   sum_{k < n}  D[g_b][s][r][k] . act[(b n + k) lda + s sa + f]
//      g_b = gid ? gid[b] : b          (the graph's slot in the bank of G graphs)
//
//   forward :  D = the stored blocks (row = target node), act = X (sa = 0), out = Hcat [B n, S Fin] (so = Fin);
//   adjoint :  D = the transposed blocks, act = d Hcat (sa = Fin), sum_s = 1 -> d X.
//
// Images as gml_dense_big_pack writes them: bf16 (hi, lo) [G][S][2][n][KP], KP = 32 ceil(n / 32), columns >= n zero.
// Machine mapping (gml_k_dense_big_mm without its K split): a workgroup of 4 waves owns (graph b, 64 rows, support s) -- or, with sum_s,
// (graph b, 64 rows) and walks the supports in ascending order into the same accumulators; a wave owns 16 rows.  KP <= 256 is at most
// 8 K steps: one workgroup forms the whole K sum, so there is no partial tile, no fold launch, no workspace and no atomic, and every
// output element is the same sequence of MFMAs on every run.  A lane's support operand (its row, 8 consecutive k) is one 16-byte load,
// issued for a whole chunk of 128 k before the chunk's activation rows are staged as fp32 -> (hi, lo) row-major images [k][f] in LDS;
// the images are read back transposed by ds_read_b64_tr_b16.  F <= 128 is up to 8 feature tiles of 16 in ONE pass (the support
// operands are read once): two images of 128 rows at the 8-tile pitch of 272 bytes are 69,632 bytes of LDS, two workgroups per CU.
// Rows k >= n of a graph belong to the next graph (or do not exist): they are never read, their image rows are zeros.
// bf16x3 (hi.hi + lo.hi + hi.lo) in fp32 accumulators.
#include "gml_common.h"

#define DM_ROWS 64                                           // rows per workgroup (4 waves x 16)
#define DM_CH 4                                              // K = 32 steps per staged chunk
#define DM_MAXN 256
#define DM_MAXF 128

struct GmlDenseMidParams {
    const uint16_t* dimg;
    const int32_t* gid;
    const float* act;
    float* out;
    int64_t lda, ldo;
    int32_t sa, so, S, n, KP, F, nrb, sum_s, vec_in, vec_out;
};

__device__ __forceinline__ uint32_t dm_pack2(float a, float b) {             // v_cvt_pk_bf16_f32 (RNE)
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{a, b}, bf16x2));
}
#define DM_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)
// image row pitch in bytes: 32 bytes per 16-feature tile + 16 (gml_dense.hip: dn_pitch)
__host__ __device__ constexpr int dm_pitch(int nft) { return 32 * nft + (nft == 1 ? 0 : 16); }

template <int NFT>
__global__ __launch_bounds__(256) void gml_k_dense_mid_mm(GmlDenseMidParams p) {
    constexpr int PA = dm_pitch(NFT);
    constexpr int NCH = 4 * NFT;                             // 8-byte chunks (4 features) per image row
    constexpr int CK = 32 * DM_CH;                           // staged k rows
    __shared__ __attribute__((aligned(16))) unsigned char img_h[CK * PA];
    __shared__ __attribute__((aligned(16))) unsigned char img_l[CK * PA];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t16 = lane & 15, kq = lane >> 4;
    const int n = p.n, KP = p.KP, KS = KP >> 5, F = p.F, S = p.S;
    const int item = blockIdx.x;
    const int rb = item % p.nrb, rest = item / p.nrb;
    const int b = p.sum_s ? rest : rest / S;
    const int s0 = p.sum_s ? 0 : rest % S, s1 = p.sum_s ? S : s0 + 1;
    const int g = p.gid ? p.gid[b] : b;
    const int row = rb * DM_ROWS + wave * 16 + t16;          // this lane's support row (the column of the transposed product)
    const int rowc = row < n ? row : n - 1;
    const float* abase = p.act + (int64_t)b * n * p.lda;
    // transposing-read addresses: lane (t, kq) passes row 8 kq + (t >> 2) (+ 4 for the second read), 8-byte chunk (t & 3)
    const int aoff = (8 * kq + (t16 >> 2)) * PA + 8 * (t16 & 3);

    f32x4 acc[NFT];
#pragma unroll
    for (int ft = 0; ft < NFT; ++ft) acc[ft] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int s = s0; s < s1; ++s) {
        const float* a = abase + (int64_t)s * p.sa;
        const uint16_t* dh = p.dimg + (((int64_t)g * S + s) * 2 * n + rowc) * KP + 8 * kq;
        const uint16_t* dl = dh + (int64_t)n * KP;
        for (int kb = 0; kb < KS; kb += DM_CH) {
            // support operand of this lane for the chunk: row rowc, k = 32 ks + 8 kq .. + 7 of the hi and the lo image
            u32x4 bh[DM_CH], bl[DM_CH];
#pragma unroll
            for (int j = 0; j < DM_CH; ++j) {
                const int ks = kb + j < KS ? kb + j : KS - 1;    // (clamped: the loads stay unconditional, the product skips them)
                bh[j] = *reinterpret_cast<const u32x4*>(dh + 32 * ks);
                bl[j] = *reinterpret_cast<const u32x4*>(dl + 32 * ks);
            }
            if (s > s0 || kb > 0) __syncthreads();               // every wave is done with the previous chunk
            const int kbase = 32 * kb, krows = 32 * min(DM_CH, KS - kb);
            for (int idx = tid; idx < krows * NCH; idx += 256) { // act[b n + k][s sa : s sa + F] -> (hi, lo) images [k][f]
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
                const uint32_t h0 = dm_pack2(v[0], v[1]), h1 = dm_pack2(v[2], v[3]);
                const uint32_t l0 = dm_pack2(v[0] - __uint_as_float(h0 << 16), v[1] - __uint_as_float(h0 & 0xffff0000u));
                const uint32_t l1 = dm_pack2(v[2] - __uint_as_float(h1 << 16), v[3] - __uint_as_float(h1 & 0xffff0000u));
                *reinterpret_cast<uint2*>(img_h + kl * PA + 8 * ch) = uint2{h0, h1};
                *reinterpret_cast<uint2*>(img_l + kl * PA + 8 * ch) = uint2{l0, l1};
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < DM_CH; ++j) {
                if (kb + j < KS) {
                    const bf16x8 Bh = __builtin_bit_cast(bf16x8, bh[j]), Bl = __builtin_bit_cast(bf16x8, bl[j]);
                    const unsigned char* ah = img_h + 32 * j * PA + aoff;
                    const unsigned char* al = img_l + 32 * j * PA + aoff;
#pragma unroll
                    for (int ft = 0; ft < NFT; ++ft) {
                        const bf16x8 Ah = gml_tr_frag(ah + 32 * ft, ah + 32 * ft + 4 * PA);
                        const bf16x8 Al = gml_tr_frag(al + 32 * ft, al + 32 * ft + 4 * PA);
                        acc[ft] = DM_MFMA(Al, Bh, acc[ft]);
                        acc[ft] = DM_MFMA(Ah, Bl, acc[ft]);
                        acc[ft] = DM_MFMA(Ah, Bh, acc[ft]);
                    }
                }
            }
        }
    }
    if (row >= n) return;
    // the lane holds features 16 ft + 4 kq .. + 3 of its own row
    float* o = p.out + ((int64_t)b * n + row) * p.ldo + (p.sum_s ? 0 : (int64_t)s0 * p.so) + 4 * kq;
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

template <int NFT>
static void dm_launch(const GmlDenseMidParams& p, unsigned grid, hipStream_t st) {
    hipLaunchKernelGGL(gml_k_dense_mid_mm<NFT>, dim3(grid), dim3(256), 0, st, p);
}

extern "C" int gml_dense_mid_support_mm(const uint16_t* dimg, const int32_t* gid, const float* act, int64_t lda, int32_t sa, float* out,
                                        int64_t ldo, int32_t so, int32_t sum_s, int32_t B, int32_t G, int32_t S, int32_t n, int32_t KP,
                                        int32_t F, void* stream) {
    if (dimg == nullptr || act == nullptr || out == nullptr || ((uintptr_t)dimg & 15) != 0 || sa < 0 || so < 0) return GML_E_BADARG;
    if (n <= 96 || n > DM_MAXN || KP != (n + 31) / 32 * 32 || F < 1 || F > DM_MAXF || S < 1 || B < 1 || G < 1) return GML_E_UNSUPPORTED;
    if (gid == nullptr && B > G) return GML_E_BADARG;
    if (lda < (int64_t)(S - 1) * sa + F || ldo < (sum_s ? (int64_t)F : (int64_t)(S - 1) * so + F)) return GML_E_BADARG;
    GmlDenseMidParams p;
    p.dimg = dimg; p.gid = gid; p.act = act; p.out = out; p.lda = lda; p.ldo = ldo; p.sa = sa; p.so = so;
    p.S = S; p.n = n; p.KP = KP; p.F = F; p.sum_s = sum_s ? 1 : 0;
    p.nrb = (int)gml_cdiv(n, DM_ROWS);
    const int64_t items = (int64_t)B * p.nrb * (p.sum_s ? 1 : S);
    if (items > 0x7fffffffLL) return GML_E_UNSUPPORTED;
    p.vec_in = (F % 4 == 0 && lda % 4 == 0 && sa % 4 == 0 && ((uintptr_t)act & 15) == 0) ? 1 : 0;
    p.vec_out = (F % 4 == 0 && ldo % 4 == 0 && (p.sum_s || so % 4 == 0) && ((uintptr_t)out & 15) == 0) ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)items;
    switch ((F + 15) / 16) {
        case 1: dm_launch<1>(p, grid, st); break;
        case 2: dm_launch<2>(p, grid, st); break;
        case 3: dm_launch<3>(p, grid, st); break;
        case 4: dm_launch<4>(p, grid, st); break;
        case 5: dm_launch<5>(p, grid, st); break;
        case 6: dm_launch<6>(p, grid, st); break;
        case 7: dm_launch<7>(p, grid, st); break;
        default: dm_launch<8>(p, grid, st); break;
    }
    return gml_launch_status();
}
