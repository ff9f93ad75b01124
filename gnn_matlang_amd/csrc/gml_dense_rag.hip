// Dense-block SpectConv for batches of graphs of DIFFERENT sizes (n <= NP = 128) with near-dense masks and dropout on the
// support entries (the TF GNNML3 of enzymes_contfeats_gnnml3_tf.py: libs/layers_tf.py:276-298 evaluates the layer as
// matmul(dropout(support[:, i]), x) on blocks padded to the largest graph; recfield = 5 fills the ENZYMES masks to 97 %).
//
//      out[(ptr[b] + r) ldo + s so + f]  (=, or summed over s)
//          = scale . sum_{k < n_b}  keep(b, s, r, k) . D[gid[b]][s][r][k] . act[(ptr[b] + k) lda + s sa + f]
//
// gml_dense.hip's batched support product with three differences.  (1) The node rows are COMPACT (ptr = row offsets, no padding
// rows anywhere) and the supports live in a per-data-set bank of bf16 (hi, lo) images [G][S][2][NP][NP] addressed through gid, so a
// shuffled batch copies nothing; a graph touches only its own ceil(n / 16) row tiles and ceil(n / 32) K steps of its slot.
// (2) Up to 256 features: 128-column blocks on the grid's second dimension, each with its own activation tile (<= 68 KB of LDS).
// (3) Optional keep bits (gml_dense_rag_mask: one bit per support entry, both orientations) zero the dropped bf16 halves of the
// lane's 16-byte operand before the MFMA; scale multiplies the accumulators once at the end.
// Mapping as there: one wave per 16 rows, a lane's operand = one 16-byte load from the image, the activation tile through LDS
// as bf16 (hi, lo) images read back with the transposing reads, bf16x3 on mfma_f32_16x16x32_bf16, fp32 accumulators, no atomics.
#include "gml_common.h"

#define RG_NP 128

struct GmlRagParams {
    const uint16_t* dimg;
    const uint32_t* mask;
    const int32_t* gid;
    const int32_t* ptr;
    const float* act;
    float* out;
    int64_t lda, ldo;
    float scale;
    int32_t sa, so, B, S, G, F, vec_in, vec_out;
};

__device__ __forceinline__ uint32_t rg_pack2(float a, float b) {             // v_cvt_pk_bf16_f32 (RNE)
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{a, b}, bf16x2));
}
#define RG_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)

// image row pitch in bytes (gml_dense.hip: 32 bytes per 16-feature tile + 16, so the transposing reads fall on distinct banks)
__host__ __device__ __forceinline__ int rg_pitch(int nft) { return 32 * nft + (nft == 1 ? 0 : 16); }

// 8 keep bits (bit j = k-slot j) -> the operand's 4 dwords with the dropped bf16 halves zeroed
__device__ __forceinline__ u32x4 rg_apply_keep(u32x4 v, uint32_t bits) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint32_t m = ((0u - ((bits >> (2 * d)) & 1u)) & 0x0000ffffu) | ((0u - ((bits >> (2 * d + 1)) & 1u)) & 0xffff0000u);
        v[d] &= m;
    }
    return v;
}

template <bool ACC, bool MASK>
__global__ __launch_bounds__(512) void gml_k_dense_rag_support_mm(GmlRagParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rg_lds[];
    constexpr int NFT = 8, KSMAX = 4;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t16 = lane & 15, kq = lane >> 4;
    const int b = blockIdx.x;
    const int r0 = p.ptr[b], n = p.ptr[b + 1] - r0;
    const int slot = p.gid != nullptr ? p.gid[b] : b;
    if (n < 1 || n > RG_NP || slot < 0 || slot >= p.G) return;    // (uniform per workgroup, before any barrier)
    const int c0 = RG_NP * blockIdx.y;                            // first feature of this column block
    const int Fc = min(p.F - c0, RG_NP);
    const int nft = (Fc + 15) >> 4;                               // 16-feature tiles in use
    const int PA = rg_pitch(nft), NCH = 4 * nft;
    const int KS = (n + 31) >> 5, KP = KS << 5;
    unsigned char* img_h = rg_lds;
    unsigned char* img_l = rg_lds + KP * PA;
    const int row = wave * 16 + t16;                              // this lane's support row (< NP: the image has it, zero beyond n)
    const bool active = wave * 16 < n;                            // waves without rows only stage
    const float* actb = p.act + (int64_t)r0 * p.lda + c0;
    float* outr = p.out + ((int64_t)r0 + row) * p.ldo + c0;

    auto stage = [&](int s) {                                     // act[:, s sa + c0 : + Fc] of this graph -> (hi, lo) images [k][f]
        const float* a = actb + s * p.sa;
        for (int idx = tid; idx < KP * NCH; idx += 512) {
            const int k = idx / NCH, ch = idx - k * NCH;
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (k < n && 4 * ch < Fc) {
                const float* q = a + (int64_t)k * p.lda + 4 * ch;
                if (p.vec_in) v = *reinterpret_cast<const f32x4*>(q);
                else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) if (4 * ch + j < Fc) v[j] = q[j];
                }
            }
            const uint32_t h0 = rg_pack2(v[0], v[1]), h1 = rg_pack2(v[2], v[3]);
            const uint32_t l0 = rg_pack2(v[0] - __uint_as_float(h0 << 16), v[1] - __uint_as_float(h0 & 0xffff0000u));
            const uint32_t l1 = rg_pack2(v[2] - __uint_as_float(h1 << 16), v[3] - __uint_as_float(h1 & 0xffff0000u));
            *reinterpret_cast<uint2*>(img_h + k * PA + 8 * ch) = uint2{h0, h1};
            *reinterpret_cast<uint2*>(img_l + k * PA + 8 * ch) = uint2{l0, l1};
        }
    };
    // support operand of this lane for support s: row `row`, k = 32 ks + 8 kq .. + 7 of the hi and the lo image; its keep bits: row
    // `row` of the bit tile = 4 words, byte kq of word ks
    u32x4 bh[KSMAX], bl[KSMAX], mw = u32x4{~0u, ~0u, ~0u, ~0u};
    auto load_rows = [&](int s) {
        const uint16_t* base = p.dimg + (((int64_t)slot * p.S + s) * 2 * RG_NP + row) * RG_NP + 8 * kq;
#pragma unroll
        for (int ks = 0; ks < KSMAX; ++ks) {
            const int kc = ks < KS ? ks : KS - 1;                 // (clamped: the loads stay unconditional, the product skips ks >= KS)
            bh[ks] = *reinterpret_cast<const u32x4*>(base + 32 * kc);
            bl[ks] = *reinterpret_cast<const u32x4*>(base + RG_NP * RG_NP + 32 * kc);
        }
        if constexpr (MASK) mw = *reinterpret_cast<const u32x4*>(p.mask + (((int64_t)b * p.S + s) * RG_NP + row) * 4);
    };
    // transposing-read addresses: lane (t, kq) passes row 8 kq + (t >> 2) (+ 4 for the second read), 8-byte chunk (t & 3)
    const int aoff = (8 * kq + (t16 >> 2)) * PA + 8 * (t16 & 3);

    f32x4 acc[NFT];
#pragma unroll
    for (int ft = 0; ft < NFT; ++ft) acc[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto store = [&](int s) {
        if (row >= n) return;
        float* o = outr + s * p.so + 4 * kq;
#pragma unroll
        for (int ft = 0; ft < NFT; ++ft) {
            const int f0 = 16 * ft + 4 * kq;
            if (f0 >= Fc) continue;
            f32x4 v = acc[ft];
            if constexpr (MASK) v *= p.scale;
            if (p.vec_out) *reinterpret_cast<f32x4*>(o + 16 * ft) = v;
            else {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (f0 + j < Fc) o[16 * ft + j] = v[j];
            }
        }
    };

    if (active) load_rows(0);
    for (int s = 0; s < p.S; ++s) {
        if (s == 0 || p.sa != 0) {
            if (s > 0) __syncthreads();                           // every wave is done with the previous tile
            stage(s);
            __syncthreads();
        }
        if (!active) continue;                                    // (wave-uniform; the barriers above are reached by every wave)
        u32x4 ch[KSMAX], cl[KSMAX];
        const u32x4 cm = mw;
#pragma unroll
        for (int ks = 0; ks < KSMAX; ++ks) { ch[ks] = bh[ks]; cl[ks] = bl[ks]; }
        if (s + 1 < p.S) load_rows(s + 1);                        // next support's rows in flight during this product
#pragma unroll
        for (int ks = 0; ks < KSMAX; ++ks) {
            if (ks < KS) {
                u32x4 vh = ch[ks], vl = cl[ks];
                if constexpr (MASK) {
                    const uint32_t bits = (cm[ks] >> (8 * kq)) & 0xffu;
                    vh = rg_apply_keep(vh, bits);
                    vl = rg_apply_keep(vl, bits);
                }
                const bf16x8 Bh = __builtin_bit_cast(bf16x8, vh), Bl = __builtin_bit_cast(bf16x8, vl);
                const unsigned char* ah = img_h + 32 * ks * PA + aoff;
                const unsigned char* al = img_l + 32 * ks * PA + aoff;
#pragma unroll
                for (int ft = 0; ft < NFT; ++ft) {
                    if (ft < nft) {
                        const bf16x8 Ah = gml_tr_frag(ah + 32 * ft, ah + 32 * ft + 4 * PA);
                        const bf16x8 Al = gml_tr_frag(al + 32 * ft, al + 32 * ft + 4 * PA);
                        acc[ft] = RG_MFMA(Al, Bh, acc[ft]);
                        acc[ft] = RG_MFMA(Ah, Bl, acc[ft]);
                        acc[ft] = RG_MFMA(Ah, Bh, acc[ft]);
                    }
                }
            }
        }
        if constexpr (!ACC) {
            store(s);
#pragma unroll
            for (int ft = 0; ft < NFT; ++ft) acc[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    if constexpr (ACC) {
        if (active) store(0);
    }
}

template <bool ACC, bool MASK>
static int rg_launch(const GmlRagParams& p, hipStream_t st) {
    const int ncb = (p.F + RG_NP - 1) / RG_NP;
    const int nft = ((p.F < RG_NP ? p.F : RG_NP) + 15) / 16;
    const size_t lds = (size_t)2 * RG_NP * rg_pitch(nft);
    GML_ALLOW_BIG_LDS(rc, (gml_k_dense_rag_support_mm<ACC, MASK>), 2 * RG_NP * rg_pitch(8));
    if (rc != hipSuccess) return (int)rc;
    hipLaunchKernelGGL((gml_k_dense_rag_support_mm<ACC, MASK>), dim3((unsigned)p.B, (unsigned)ncb), dim3(512), lds, st, p);
    return gml_launch_status();
}

extern "C" int gml_dense_rag_support_mm(const uint16_t* dimg, const uint32_t* mask, float scale, const int32_t* gid, const int32_t* ptr,
                                        const float* act, int64_t lda, int32_t sa, float* out, int64_t ldo, int32_t so, int32_t sum_s,
                                        int32_t B, int32_t S, int32_t G, int32_t F, void* stream) {
    if (dimg == nullptr || ptr == nullptr || act == nullptr || out == nullptr) return GML_E_BADARG;
    if (F < 1 || F > 2 * RG_NP || S < 1 || B < 0 || G < 1 || sa < 0 || so < 0) return GML_E_UNSUPPORTED;
    if (((uintptr_t)dimg & 15) || ((uintptr_t)mask & 15) || ((uintptr_t)gid & 3) || ((uintptr_t)ptr & 3) || ((uintptr_t)act & 3) ||
        ((uintptr_t)out & 3))
        return GML_E_BADARG;
    if (lda < (int64_t)(S - 1) * sa + F || ldo < (sum_s ? (int64_t)F : (int64_t)(S - 1) * so + F)) return GML_E_BADARG;
    if (gid == nullptr && B > G) return GML_E_BADARG;
    if (B == 0) return GML_OK;
    GmlRagParams p;
    p.dimg = dimg; p.mask = mask; p.gid = gid; p.ptr = ptr; p.act = act; p.out = out; p.lda = lda; p.ldo = ldo;
    p.scale = mask != nullptr ? scale : 1.f;
    p.sa = sa; p.so = so; p.B = B; p.S = S; p.G = G; p.F = F;
    p.vec_in = (F % 4 == 0 && lda % 4 == 0 && sa % 4 == 0 && ((uintptr_t)act & 15) == 0) ? 1 : 0;
    p.vec_out = (F % 4 == 0 && ldo % 4 == 0 && so % 4 == 0 && ((uintptr_t)out & 15) == 0) ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    if (mask != nullptr) return sum_s ? rg_launch<true, true>(p, st) : rg_launch<false, true>(p, st);
    return sum_s ? rg_launch<true, false>(p, st) : rg_launch<false, false>(p, st);
}

// ---------------------------------------------------------------------------------------------------------------------
// Keep bits of one dropout site for a batch of B graphs, both orientations.  The decision of support entry (b, s, r, k) is the
// dropout contract of gml_dropout.hip on the logical element e = ((b S + s) NP + r) NP + k: Philox4x32-10 keyed by the seed, counter
// block (j lo, j hi, site, counter lo), j = e >> 2, word e & 3, keep iff draw >= t.  One workgroup per (b, s); a thread draws the
// 8 Philox blocks of one 32-bit word of the forward tile (row r, k = 32 w .. + 31), the tile is assembled in LDS and read back
// transposed, so both orientations come out of one pass and every draw is computed once.  Bits with r >= n_b or k >= n_b are 0.
__device__ __forceinline__ u32x4 rg_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return u32x4{c0, c1, c2, c3};
}

__global__ __launch_bounds__(256) void gml_k_dense_rag_mask(const int32_t* __restrict__ ptr, uint32_t* __restrict__ mask_fwd,
                                                           uint32_t* __restrict__ mask_bwd, int S, uint64_t t,
                                                           const int64_t* __restrict__ state, uint32_t site) {
    __shared__ uint32_t tile[RG_NP * 4];
    const int bs = blockIdx.x, b = bs / S, tid = threadIdx.x;
    int n = ptr[b + 1] - ptr[b];
    n = n < 0 ? 0 : (n > RG_NP ? RG_NP : n);
    const uint64_t seed = (uint64_t)state[0], ctr = (uint64_t)state[1];
    for (int i = tid; i < RG_NP * 4; i += 256) {
        const int r = i >> 2, w = i & 3;
        uint32_t bits = 0;
        if (r < n && 32 * w < n) {
            const int64_t j0 = (((int64_t)bs * RG_NP + r) * RG_NP + 32 * w) >> 2;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                if (32 * w + 4 * q < n) {
                    const int64_t j = j0 + q;
                    const u32x4 u = rg_philox4x32_10((uint32_t)j, (uint32_t)((uint64_t)j >> 32), site, (uint32_t)ctr, (uint32_t)seed,
                                                     (uint32_t)(seed >> 32));
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if ((uint64_t)u[c] >= t && 32 * w + 4 * q + c < n) bits |= 1u << (4 * q + c);
                }
            }
        }
        tile[i] = bits;
        mask_fwd[(int64_t)bs * RG_NP * 4 + i] = bits;
    }
    if (mask_bwd == nullptr) return;
    __syncthreads();
    for (int i = tid; i < RG_NP * 4; i += 256) {
        const int k = i >> 2, w = i & 3;                          // transposed word: row k, bits r = 32 w .. + 31
        uint32_t bits = 0;
        if (k < n && 32 * w < n) {
#pragma unroll 8
            for (int rr = 0; rr < 32; ++rr) bits |= ((tile[(32 * w + rr) * 4 + (k >> 5)] >> (k & 31)) & 1u) << rr;
        }
        mask_bwd[(int64_t)bs * RG_NP * 4 + i] = bits;
    }
}

extern "C" int gml_dense_rag_mask(const int32_t* ptr, uint32_t* mask_fwd, uint32_t* mask_bwd, int32_t B, int32_t S, uint64_t t,
                                  const int64_t* state, uint32_t site, void* stream) {
    if (B < 0 || S < 1 || t > (1ull << 32)) return GML_E_BADARG;
    if (B == 0) return GML_OK;
    if (ptr == nullptr || mask_fwd == nullptr || state == nullptr) return GML_E_BADARG;
    if (((uintptr_t)ptr & 3) || ((uintptr_t)mask_fwd & 15) || ((uintptr_t)mask_bwd & 15) || ((uintptr_t)state & 7)) return GML_E_BADARG;
    hipLaunchKernelGGL(gml_k_dense_rag_mask, dim3((unsigned)((int64_t)B * S)), dim3(256), 0, (hipStream_t)stream, ptr, mask_fwd, mask_bwd,
                       S, t, state, site);
    return gml_launch_status();
}

// ---------------------------------------------------------------------------------------------------------------------
// The bank of a whole data set from its collated COO supports: img_fwd[g][s][hi | lo][j - ptr[g]][i - ptr[g]] = edge_attr2[e][s] for
// edge e = (i -> j) (the orientation of dense_supports: row = target node), img_bwd the transposes; hi + lo as gml_dense_pack.
// Both images are zero-filled first (by a kernel: gml_common.h), then one thread per (edge, support) writes its four halves -- the
// mask lists every (i, j) once, so no two threads write the same entry.  Edges outside their graph's NP x NP block are skipped.
__global__ __launch_bounds__(256) void gml_k_dense_rag_pack(const int64_t* __restrict__ ei, const float* __restrict__ ea,
                                                           const int64_t* __restrict__ batch, const int32_t* __restrict__ ptr,
                                                           uint16_t* __restrict__ img_fwd, uint16_t* __restrict__ img_bwd, int64_t E,
                                                           int64_t N, int G, int S) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= E * S) return;
    const int64_t e = idx / S;
    const int s = (int)(idx - e * S);
    const int64_t i = ei[e], j = ei[E + e];
    if (i < 0 || i >= N || j < 0 || j >= N) return;
    const int64_t g = batch[i];
    if (g < 0 || g >= G) return;
    const int64_t li = i - ptr[g], lj = j - ptr[g];
    if (li < 0 || li >= RG_NP || lj < 0 || lj >= RG_NP) return;
    const float v = ea[idx];
    const uint32_t h = rg_pack2(v, 0.f) & 0xffffu;
    const uint32_t l = rg_pack2(v - __uint_as_float(h << 16), 0.f) & 0xffffu;
    const int64_t blk = (g * S + s) * 2 * RG_NP * RG_NP;
    img_fwd[blk + lj * RG_NP + li] = (uint16_t)h;
    img_fwd[blk + RG_NP * RG_NP + lj * RG_NP + li] = (uint16_t)l;
    img_bwd[blk + li * RG_NP + lj] = (uint16_t)h;
    img_bwd[blk + RG_NP * RG_NP + li * RG_NP + lj] = (uint16_t)l;
}

extern "C" int gml_dense_rag_pack(const int64_t* edge_index2, const float* edge_attr2, const int64_t* batch, const int32_t* ptr,
                                  uint16_t* img_fwd, uint16_t* img_bwd, int64_t E, int64_t N, int32_t G, int32_t S, void* stream) {
    if (E < 0 || N < 0 || G < 0 || S < 1) return GML_E_BADARG;
    if (G == 0) return GML_OK;
    if (img_fwd == nullptr || img_bwd == nullptr || ptr == nullptr || ((uintptr_t)img_fwd & 15) || ((uintptr_t)img_bwd & 15)) return GML_E_BADARG;
    if (E > 0 && (edge_index2 == nullptr || edge_attr2 == nullptr || batch == nullptr)) return GML_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const size_t nbytes = (size_t)G * S * 2 * RG_NP * RG_NP * sizeof(uint16_t);
    gml_zero_async(img_fwd, nbytes, st);
    gml_zero_async(img_bwd, nbytes, st);
    if (E > 0)
        hipLaunchKernelGGL(gml_k_dense_rag_pack, dim3((unsigned)gml_cdiv(E * S, 256)), dim3(256), 0, st, edge_index2, edge_attr2, batch, ptr,
                           img_fwd, img_bwd, E, N, G, S);
    return gml_launch_status();
}
