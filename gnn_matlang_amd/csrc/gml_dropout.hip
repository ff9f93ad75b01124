// Dropout with a counter-based mask (F.dropout in front of every layer of ptc.py:349-358, enzymes.py:372-381,
// proteins.py:282-285, mnist75.py:299-317).  The keep decision of logical element e = r C + c is a pure function of
// (seed, counter, site, e): Philox4x32-10 (Salmon et al., SC'11) keyed by the seed, counter block
// (j lo, j hi, site, counter lo) with j = e >> 2, word e & 3.  Nothing depends on the launch geometry, the strides or the
// device, so tests restate it on the CPU and a captured step replays the same masks as the same step run eagerly.
// One lane = 4 consecutive elements = one Philox call; 8 consecutive lanes own one 32-bit word of the packed mask.
#include "gml_common.h"

__device__ __forceinline__ u32x4 gml_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
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

// (row, column) of the first element of lane j: 32-bit division while every element index fits (the uniform branch is taken
// the same way by the whole grid)
__device__ __forceinline__ void gml_dropout_rc(int64_t e0, int C, bool small, int64_t& r, int& c) {
    if (small) {
        const uint32_t q = (uint32_t)e0 / (uint32_t)C;
        r = q;
        c = (int)((uint32_t)e0 - q * (uint32_t)C);
    } else {
        r = e0 / C;
        c = (int)(e0 - r * C);
    }
}

// VEC: C % 4 == 0 and float4-addressable rows of x and y -- the 4 elements of a lane are one aligned float4 of one row
template <bool VEC>
__global__ void __launch_bounds__(256) gml_k_dropout_fwd(const float* __restrict__ x, int64_t ldx, float* __restrict__ y, int64_t ldy,
                                                         uint32_t* __restrict__ mask, int64_t N, int C, int64_t nlanes, uint64_t t, float scale,
                                                         const int64_t* __restrict__ state, uint32_t site, bool small) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t seed = (uint64_t)state[0], ctr = (uint64_t)state[1];
    uint32_t nib = 0;
    if (j < nlanes) {
        const u32x4 u = gml_philox4x32_10((uint32_t)j, (uint32_t)((uint64_t)j >> 32), site, (uint32_t)ctr, (uint32_t)seed,
                                          (uint32_t)(seed >> 32));
        const int64_t e0 = j * 4;
        int64_t r;
        int c;
        gml_dropout_rc(e0, C, small, r, c);
        if (VEC) {
            const f32x4 v = *(const f32x4*)(x + r * ldx + c);
            f32x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool keep = (uint64_t)u[k] >= t;
                o[k] = keep ? v[k] * scale : 0.f;
                nib |= (uint32_t)keep << k;
            }
            *(f32x4*)(y + r * ldy + c) = o;
        } else {
            const int64_t NC = N * C;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (e0 + k < NC) {
                    const bool keep = (uint64_t)u[k] >= t;
                    const float v = x[r * ldx + c];
                    y[r * ldy + c] = keep ? v * scale : 0.f;
                    nib |= (uint32_t)keep << k;
                }
                if (++c == C) { c = 0; ++r; }
            }
        }
    }
    // lanes 8w .. 8w+7 (one wave, blocks are whole multiples of 8 lanes) hold the 8 nibbles of mask word w
    uint32_t w = nib << ((j & 7) * 4);
    w |= (uint32_t)__shfl_xor((int)w, 1);
    w |= (uint32_t)__shfl_xor((int)w, 2);
    w |= (uint32_t)__shfl_xor((int)w, 4);
    if ((j & 7) == 0 && j < nlanes) mask[j >> 3] = w;
}

template <bool VEC>
__global__ void __launch_bounds__(256) gml_k_dropout_bwd(const float* __restrict__ g, int64_t ldg, const uint32_t* __restrict__ mask,
                                                         float* __restrict__ dx, int64_t lddx, int64_t N, int C, int64_t nlanes, float scale,
                                                         bool small) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nlanes) return;
    const uint32_t nib = (mask[j >> 3] >> ((j & 7) * 4)) & 15u;
    const int64_t e0 = j * 4;
    int64_t r;
    int c;
    gml_dropout_rc(e0, C, small, r, c);
    if (VEC) {
        const f32x4 v = *(const f32x4*)(g + r * ldg + c);
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = ((nib >> k) & 1u) ? v[k] * scale : 0.f;
        *(f32x4*)(dx + r * lddx + c) = o;
    } else {
        const int64_t NC = N * C;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (e0 + k < NC) dx[r * lddx + c] = ((nib >> k) & 1u) ? g[r * ldg + c] * scale : 0.f;
            if (++c == C) { c = 0; ++r; }
        }
    }
}

static inline bool gml_dropout_vec(const void* a, int64_t lda, const void* b, int64_t ldb, int C) {
    return C % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 && (uintptr_t)a % 16 == 0 && (uintptr_t)b % 16 == 0;
}

extern "C" int gml_dropout_fwd(const float* x, int64_t ldx, float* y, int64_t ldy, uint32_t* mask, int64_t num_rows, int32_t C,
                               uint64_t t, float scale, const int64_t* state, uint32_t site, gml_stream_t stream) {
    if (num_rows < 0 || C < 0 || t > (1ull << 32)) return GML_E_BADARG;
    if (num_rows == 0 || C == 0) return GML_OK;
    if (ldx < C || ldy < C || !x || !y || !mask || !state) return GML_E_BADARG;
    if ((uintptr_t)x % 4 || (uintptr_t)y % 4 || (uintptr_t)mask % 4 || (uintptr_t)state % 8) return GML_E_BADARG;
    const int64_t nlanes = gml_cdiv(num_rows * C, 4);
    const bool small = num_rows * C + 4 <= (int64_t)UINT32_MAX;
    const dim3 grid((unsigned)gml_cdiv(nlanes, 256)), block(256);
    if (gml_dropout_vec(x, ldx, y, ldy, C))
        hipLaunchKernelGGL(gml_k_dropout_fwd<true>, grid, block, 0, (hipStream_t)stream, x, ldx, y, ldy, mask, num_rows, C, nlanes, t, scale,
                           state, site, small);
    else
        hipLaunchKernelGGL(gml_k_dropout_fwd<false>, grid, block, 0, (hipStream_t)stream, x, ldx, y, ldy, mask, num_rows, C, nlanes, t, scale,
                           state, site, small);
    return gml_launch_status();
}

extern "C" int gml_dropout_bwd(const float* g, int64_t ldg, const uint32_t* mask, float* dx, int64_t lddx, int64_t num_rows, int32_t C,
                               float scale, gml_stream_t stream) {
    if (num_rows < 0 || C < 0) return GML_E_BADARG;
    if (num_rows == 0 || C == 0) return GML_OK;
    if (ldg < C || lddx < C || !g || !mask || !dx) return GML_E_BADARG;
    if ((uintptr_t)g % 4 || (uintptr_t)dx % 4 || (uintptr_t)mask % 4) return GML_E_BADARG;
    const int64_t nlanes = gml_cdiv(num_rows * C, 4);
    const bool small = num_rows * C + 4 <= (int64_t)UINT32_MAX;
    const dim3 grid((unsigned)gml_cdiv(nlanes, 256)), block(256);
    if (gml_dropout_vec(g, ldg, dx, lddx, C))
        hipLaunchKernelGGL(gml_k_dropout_bwd<true>, grid, block, 0, (hipStream_t)stream, g, ldg, mask, dx, lddx, num_rows, C, nlanes, scale, small);
    else
        hipLaunchKernelGGL(gml_k_dropout_bwd<false>, grid, block, 0, (hipStream_t)stream, g, ldg, mask, dx, lddx, num_rows, C, nlanes, scale, small);
    return gml_launch_status();
}
