// Pairwise distinguishability of graph embeddings: the isomorphism tests of sr25.py:281-300, graph8c.py:282-302 and
// exp_iso.py:284-304.  For a pair (i, j) of rows of E [G, D] the test is
//     d = sum_k |E[i, k] - E[j, k]|   (float32, numpy's summation order)      separated  <=>  d > tol   (float32 compare)
// and a bitmap accumulates "separated at least once" over seeds.  Layout and contract: include/gml.h, DESIGN s4.11.
//
// Summation order of numpy's float32 sum(axis=-1) over a contiguous axis of length D <= 128 (pairwise_sum):
//   D < 8 : s = 0; s += x[0]; s += x[1]; ...
//   D >= 8: r[m] = x[m], then r[m] += x[8 b + m] for the full 8-blocks b = 1 .. D / 8 - 1,
//           s = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then s += x[k] for the tail k = 8 (D / 8) .. D - 1.
// There is no multiply anywhere, so no FMA contraction can occur, and clang does not reassociate without fast-math.
#include "gml_common.h"
#include <algorithm>

#define GML_PAIR_TILE_I 256     // rows of an all-pairs tile: one lane per row i, 4 waves
#define GML_PAIR_SEG 1024       // bitmap words per segment of the count / list kernels (4 per lane)

// d(a, b) in numpy's order.  a: the row in registers (zero beyond D); b(k): element k of the other row.  EXACT: D == DMAX
// is known at compile time; otherwise D <= DMAX is uniform over the launch and the branches on it are scalar.
template <int DMAX, bool EXACT, typename BF>
__device__ __forceinline__ float gml_pair_l1(const float (&a)[DMAX], BF b, int Drt) {
    const int D = EXACT ? DMAX : Drt;
    if constexpr (DMAX < 8) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < DMAX; ++k)
            if (k < D) s += fabsf(a[k] - b(k));
        return s;
    }
    if (!EXACT && D < 8) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 7; ++k)
            if (k < D) s += fabsf(a[k] - b(k));
        return s;
    }
    const int nb = D >> 3;
    float r[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) r[m] = fabsf(a[m] - b(m));
#pragma unroll
    for (int blk = 1; blk < DMAX / 8; ++blk)
        if (blk < nb) {
#pragma unroll
            for (int m = 0; m < 8; ++m) r[m] += fabsf(a[8 * blk + m] - b(8 * blk + m));
        }
    float s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
    for (int k = 8; k < DMAX; ++k)
        if (k >= 8 * nb && k < D) s += fabsf(a[k] - b(k));
    return s;
}

// bits [lo, hi) of a word, 0 <= lo, hi <= 64
__device__ __forceinline__ uint64_t gml_bit_range(int lo, int hi) {
    if (hi <= lo) return 0ull;
    const uint64_t m = (hi - lo == 64) ? ~0ull : ((1ull << (hi - lo)) - 1ull);
    return m << lo;
}

// the valid bits of bitmap word q: all-pairs (W words per row i, bit b of word w = column j = 64 w + b, valid for i < j < G)
// or a pair list (bit p & 63 of word p >> 6, valid for p < P)
__device__ __forceinline__ uint64_t gml_pair_valid(int64_t q, int G, int64_t W, int64_t P, bool all) {
    if (!all) return gml_bit_range(0, (int)min<int64_t>(64, max<int64_t>(0, P - 64 * q)));
    const int64_t i = q / W, j0 = 64 * (q - i * W);
    const int lo = (int)min<int64_t>(64, max<int64_t>(0, i + 1 - j0));
    const int hi = (int)min<int64_t>(64, max<int64_t>(0, (int64_t)G - j0));
    return gml_bit_range(lo, hi);
}

// All pairs.  Tile (bi, tj) = rows [256 bi, 256 bi + 256) x columns [64 tj, 64 tj + 64); the tiles with some j > i are
// tj = 4 bi .. W - 1, so i-block bi owns W - 4 bi tiles starting at linear id start(bi) = bi W - 2 bi (bi - 1).
// The 64 column rows are staged in LDS (the inner loop reads one address per wave: a broadcast); each lane keeps its row i in
// registers and builds the 64-bit word (i, tj) in registers.  Every word belongs to exactly one lane: plain read-OR-write.
template <int DMAX, bool EXACT>
__global__ void __launch_bounds__(GML_PAIR_TILE_I) gml_k_pair_distinct_all(const float* __restrict__ E, int64_t ldE, int G, int Drt,
                                                                        float tol, uint64_t* __restrict__ bits, int W, int NB) {
    __shared__ float sj[64 * DMAX];
    const int D = EXACT ? DMAX : Drt;
    const int t = blockIdx.x;
    int lo = 0, hi = NB - 1;                   // largest bi with start(bi) <= t (uniform)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int64_t)mid * W - 2ll * mid * (mid - 1) <= t) lo = mid; else hi = mid - 1;
    }
    const int bi = lo;
    const int tj = 4 * bi + (int)(t - ((int64_t)bi * W - 2ll * bi * (bi - 1)));
    const int j0 = 64 * tj;
    for (int idx = threadIdx.x; idx < 64 * DMAX; idx += GML_PAIR_TILE_I) {
        const int r = idx / DMAX, k = idx - r * DMAX;
        sj[idx] = (k < D && j0 + r < G) ? E[(int64_t)(j0 + r) * ldE + k] : 0.f;
    }
    __syncthreads();
    const int i = GML_PAIR_TILE_I * bi + threadIdx.x;
    const uint64_t valid = gml_pair_valid((int64_t)i * W + tj, G, W, 0, true);
    if (i >= G || valid == 0) return;
    float a[DMAX];
#pragma unroll
    for (int k = 0; k < DMAX; ++k) a[k] = k < D ? E[(int64_t)i * ldE + k] : 0.f;
    uint64_t word = 0;
    for (int jj = 0; jj < 64; ++jj) {
        const float* b = sj + jj * DMAX;
        const float d = gml_pair_l1<DMAX, EXACT>(a, [&](int k) { return b[k]; }, D);
        word |= (uint64_t)(d > tol) << jj;             // NaN compares false: never separates
    }
    word &= valid;
    if (word) bits[(int64_t)i * W + tj] |= word;
}

// A pair list: lane p tests pairs[p] and the wave's ballot is word p >> 6.  A pair with an index outside [0, G) is not read
// and stays clear.
template <int DMAX, bool EXACT>
__global__ void __launch_bounds__(256) gml_k_pair_distinct_list(const float* __restrict__ E, int64_t ldE, int G, const int32_t* __restrict__ pairs,
                                                                int64_t P, int Drt, float tol, uint64_t* __restrict__ bits) {
    const int D = EXACT ? DMAX : Drt;
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool sep = false;
    if (p < P) {
        const int i = pairs[2 * p], j = pairs[2 * p + 1];
        if (i >= 0 && i < G && j >= 0 && j < G) {
            float a[DMAX];
#pragma unroll
            for (int k = 0; k < DMAX; ++k) a[k] = k < D ? E[(int64_t)i * ldE + k] : 0.f;
            const float* b = E + (int64_t)j * ldE;
            sep = gml_pair_l1<DMAX, EXACT>(a, [&](int k) { return b[k]; }, D) > tol;
        }
    }
    const uint64_t word = __ballot(sep);
    if ((threadIdx.x & 63) == 0 && p < P && word) bits[p >> 6] |= word;
}

// count += never-separated valid bits of the words [grid-stride]; a word with no valid bit is not read
__global__ void __launch_bounds__(256) gml_k_pair_count(const uint64_t* __restrict__ bits, int G, int64_t W, int64_t P, bool all,
                                                        int64_t nwords, unsigned long long* __restrict__ count) {
    __shared__ unsigned long long part[4];
    unsigned long long c = 0;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nwords; q += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t v = gml_pair_valid(q, G, W, P, all);
        if (v) c += __popcll(v & ~bits[q]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += (unsigned long long)__shfl_xor((long long)c, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long s = part[0] + part[1] + part[2] + part[3];
        if (s) atomicAdd(count, s);
    }
}

// never-separated bits of the 4 words of lane t of segment s: words 4 t .. 4 t + 3 of the segment
__device__ __forceinline__ void gml_pair_seg_words(const uint64_t* __restrict__ bits, int G, int64_t W, int64_t P, bool all, int64_t nwords,
                                                   int64_t q0, uint64_t (&m)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t q = q0 + u;
        const uint64_t v = q < nwords ? gml_pair_valid(q, G, W, P, all) : 0ull;
        m[u] = v ? (v & ~bits[q]) : 0ull;
    }
}

// block-wide exclusive scan of one int64 per lane (256 lanes); returns the lane's prefix, *total = the block's sum
__device__ __forceinline__ int64_t gml_block_scan256(int64_t v, int64_t* sh, int64_t* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) sh[w] = x;
    __syncthreads();
    int64_t base = 0, tot = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (u < w) base += sh[u];
        tot += sh[u];
    }
    *total = tot;
    return base + x - v;
}

// pass 1: ws[s] = never-separated count of segment s
__global__ void __launch_bounds__(256) gml_k_pair_seg_count(const uint64_t* __restrict__ bits, int G, int64_t W, int64_t P, bool all,
                                                            int64_t nwords, int64_t* __restrict__ ws) {
    __shared__ int64_t sh[4];
    uint64_t m[4];
    gml_pair_seg_words(bits, G, W, P, all, nwords, (int64_t)blockIdx.x * GML_PAIR_SEG + 4 * threadIdx.x, m);
    const int64_t c = __popcll(m[0]) + __popcll(m[1]) + __popcll(m[2]) + __popcll(m[3]);
    int64_t tot;
    gml_block_scan256(c, sh, &tot);
    if (threadIdx.x == 0) ws[blockIdx.x] = tot;
}

// pass 2 (one workgroup): ws <- exclusive prefix of ws, *count = the total
__global__ void __launch_bounds__(256) gml_k_pair_seg_scan(int64_t* __restrict__ ws, int64_t nseg, int64_t* __restrict__ count) {
    __shared__ int64_t sh[4];
    const int64_t per = (nseg + 255) / 256;
    const int64_t s0 = per * threadIdx.x, s1 = min(nseg, s0 + per);
    int64_t v = 0;
    for (int64_t s = s0; s < s1; ++s) v += ws[s];
    int64_t tot;
    int64_t run = gml_block_scan256(v, sh, &tot);
    for (int64_t s = s0; s < s1; ++s) {
        const int64_t c = ws[s];
        ws[s] = run;
        run += c;
    }
    if (threadIdx.x == 0) *count = tot;
}

// pass 3: each never-separated bit at its rank: out[rank] = (i, j), ascending bitmap order = ascending (i, j) for all pairs,
// list order for a pair list; ranks >= cap are not written
__global__ void __launch_bounds__(256) gml_k_pair_seg_emit(const uint64_t* __restrict__ bits, int G, int64_t W, const int32_t* __restrict__ pairs,
                                                           int64_t P, bool all, int64_t nwords, const int64_t* __restrict__ ws,
                                                           int64_t* __restrict__ out, int64_t cap) {
    __shared__ int64_t sh[4];
    uint64_t m[4];
    const int64_t q0 = (int64_t)blockIdx.x * GML_PAIR_SEG + 4 * threadIdx.x;
    gml_pair_seg_words(bits, G, W, P, all, nwords, q0, m);
    const int64_t c = __popcll(m[0]) + __popcll(m[1]) + __popcll(m[2]) + __popcll(m[3]);
    int64_t tot;
    int64_t r = ws[blockIdx.x] + gml_block_scan256(c, sh, &tot);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        uint64_t x = m[u];
        while (x && r < cap) {
            const int b = __ffsll((unsigned long long)x) - 1;
            x &= x - 1;
            const int64_t q = q0 + u;
            int64_t i, j;
            if (all) {
                i = q / W;
                j = 64 * (q - i * W) + b;
            } else {
                const int64_t p = 64 * q + b;
                i = pairs[2 * p];
                j = pairs[2 * p + 1];
            }
            out[2 * r] = i;
            out[2 * r + 1] = j;
            ++r;
        }
    }
}

#define GML_PAIR_MAX_G 65536

template <int DMAX, bool EXACT>
static void gml_pair_launch_all(const float* E, int64_t ldE, int G, int D, float tol, uint64_t* bits, hipStream_t st) {
    const int W = (int)gml_cdiv(G, 64), NB = (int)gml_cdiv(G, GML_PAIR_TILE_I);
    const int64_t ntiles = (int64_t)NB * W - 2ll * NB * (NB - 1);
    hipLaunchKernelGGL((gml_k_pair_distinct_all<DMAX, EXACT>), dim3((unsigned)ntiles), dim3(GML_PAIR_TILE_I), 0, st, E, ldE, G, D, tol, bits, W, NB);
}

template <int DMAX, bool EXACT>
static void gml_pair_launch_list(const float* E, int64_t ldE, int G, const int32_t* pairs, int64_t P, int D, float tol, uint64_t* bits,
                                 hipStream_t st) {
    hipLaunchKernelGGL((gml_k_pair_distinct_list<DMAX, EXACT>), dim3((unsigned)gml_cdiv(P, 256)), dim3(256), 0, st, E, ldE, G, pairs, P, D, tol, bits);
}

// exact kernels for D <= 16 (the scripts' heads: D = 10), D-bucketed ones above
#define GML_PAIR_DISPATCH(LAUNCH, ...)                                                                                            \
    switch (D) {                                                                                                                  \
        case 1: LAUNCH<1, true>(__VA_ARGS__); break;   case 2: LAUNCH<2, true>(__VA_ARGS__); break;                               \
        case 3: LAUNCH<3, true>(__VA_ARGS__); break;   case 4: LAUNCH<4, true>(__VA_ARGS__); break;                               \
        case 5: LAUNCH<5, true>(__VA_ARGS__); break;   case 6: LAUNCH<6, true>(__VA_ARGS__); break;                               \
        case 7: LAUNCH<7, true>(__VA_ARGS__); break;   case 8: LAUNCH<8, true>(__VA_ARGS__); break;                               \
        case 9: LAUNCH<9, true>(__VA_ARGS__); break;   case 10: LAUNCH<10, true>(__VA_ARGS__); break;                             \
        case 11: LAUNCH<11, true>(__VA_ARGS__); break; case 12: LAUNCH<12, true>(__VA_ARGS__); break;                             \
        case 13: LAUNCH<13, true>(__VA_ARGS__); break; case 14: LAUNCH<14, true>(__VA_ARGS__); break;                             \
        case 15: LAUNCH<15, true>(__VA_ARGS__); break; case 16: LAUNCH<16, true>(__VA_ARGS__); break;                             \
        default:                                                                                                                  \
            if (D <= 32) LAUNCH<32, false>(__VA_ARGS__);                                                                          \
            else if (D <= 64) LAUNCH<64, false>(__VA_ARGS__);                                                                     \
            else LAUNCH<128, false>(__VA_ARGS__);                                                                                 \
    }

static inline bool gml_pair_args_ok(const float* E, int64_t ldE, int64_t G, int32_t D, const uint64_t* bits) {
    return E && bits && D >= 1 && D <= 128 && ldE >= D && G >= 0 && G <= GML_PAIR_MAX_G && (uintptr_t)E % 4 == 0 &&
           (uintptr_t)bits % 8 == 0;
}

extern "C" int64_t gml_pair_bitmap_words(int64_t G, int64_t P) {
    if (G < 0 || G > GML_PAIR_MAX_G) return -1;
    return P < 0 ? G * gml_cdiv(G, (int64_t)64) : gml_cdiv(P, (int64_t)64);
}

extern "C" int gml_pair_distinct_all(const float* E, int64_t ldE, int64_t G, int32_t D, float tol, uint64_t* bits, gml_stream_t stream) {
    if (!gml_pair_args_ok(E, ldE, G, D, bits)) return GML_E_BADARG;
    if (G < 2) return GML_OK;
    GML_PAIR_DISPATCH(gml_pair_launch_all, E, ldE, (int)G, D, tol, bits, (hipStream_t)stream)
    return gml_launch_status();
}

extern "C" int gml_pair_distinct_list(const float* E, int64_t ldE, int64_t G, const int32_t* pairs, int64_t P, int32_t D, float tol,
                                      uint64_t* bits, gml_stream_t stream) {
    if (!gml_pair_args_ok(E, ldE, G, D, bits) || P < 0 || P > (int64_t)INT32_MAX || (P > 0 && !pairs) ||
        (uintptr_t)pairs % 4)
        return GML_E_BADARG;
    if (P == 0) return GML_OK;
    GML_PAIR_DISPATCH(gml_pair_launch_list, E, ldE, (int)G, pairs, P, D, tol, bits, (hipStream_t)stream)
    return gml_launch_status();
}

extern "C" int gml_pair_count_similar(const uint64_t* bits, int64_t G, const int32_t* pairs, int64_t P, int64_t* count,
                                      gml_stream_t stream) {
    const bool all = pairs == nullptr;
    const int64_t nwords = gml_pair_bitmap_words(G, all ? -1 : P);
    if (nwords < 0 || !count || (nwords > 0 && !bits) || (uintptr_t)bits % 8 || (uintptr_t)count % 8 || (!all && P < 0)) return GML_E_BADARG;
    hipError_t e = hipMemsetAsync(count, 0, sizeof(int64_t), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    if (nwords == 0) return GML_OK;
    const unsigned grid = (unsigned)std::min<int64_t>(gml_cdiv(nwords, (int64_t)256), 4096);
    hipLaunchKernelGGL(gml_k_pair_count, dim3(grid), dim3(256), 0, (hipStream_t)stream, bits, (int)G, gml_cdiv(G, (int64_t)64), P, all,
                       nwords, (unsigned long long*)count);
    return gml_launch_status();
}

extern "C" size_t gml_pair_list_workspace_bytes(int64_t G, int64_t P) {
    const int64_t nwords = gml_pair_bitmap_words(G, P);
    return nwords <= 0 ? 0 : (size_t)gml_cdiv(nwords, (int64_t)GML_PAIR_SEG) * sizeof(int64_t);
}

extern "C" int gml_pair_list_similar(const uint64_t* bits, int64_t G, const int32_t* pairs, int64_t P, int64_t* out, int64_t cap,
                                     int64_t* count, void* ws, size_t ws_bytes, gml_stream_t stream) {
    const bool all = pairs == nullptr;
    const int64_t nwords = gml_pair_bitmap_words(G, all ? -1 : P);
    if (nwords < 0 || !count || cap < 0 || (cap > 0 && !out) || (nwords > 0 && !bits) || (!all && P < 0) || (uintptr_t)bits % 8 ||
        (uintptr_t)count % 8 || (uintptr_t)out % 8 || (uintptr_t)ws % 8 || (uintptr_t)pairs % 4)
        return GML_E_BADARG;
    if (nwords == 0) {
        hipError_t e = hipMemsetAsync(count, 0, sizeof(int64_t), (hipStream_t)stream);
        return e == hipSuccess ? GML_OK : (int)e;
    }
    const int64_t nseg = gml_cdiv(nwords, (int64_t)GML_PAIR_SEG);
    if (!ws || ws_bytes < (size_t)nseg * sizeof(int64_t)) return GML_E_WORKSPACE;
    const int64_t W = gml_cdiv(G, (int64_t)64);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gml_k_pair_seg_count, dim3((unsigned)nseg), dim3(256), 0, st, bits, (int)G, W, P, all, nwords, (int64_t*)ws);
    hipLaunchKernelGGL(gml_k_pair_seg_scan, dim3(1), dim3(256), 0, st, (int64_t*)ws, nseg, count);
    hipLaunchKernelGGL(gml_k_pair_seg_emit, dim3((unsigned)nseg), dim3(256), 0, st, bits, (int)G, W, pairs, P, all, nwords,
                       (const int64_t*)ws, out, cap);
    return gml_launch_status();
}
