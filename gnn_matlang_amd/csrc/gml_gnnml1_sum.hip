// GNNML1 block in the sum-and-factors form of enzymes_contfeat.py:284-346 (block mode 4 of DESIGN s4.15):
//
//   a = fc_i1(x)   c = conv_i1(x) = (A^T x) Wc + bc   f2 = fc_i2(x)   f3 = fc_i3(x)
//   out [N, n1 + n3] = [ act(a) + act(c) | act(f2) * act(f3) ]            n1 == n2 <= 128, n3 <= 64, Fin <= 192
//
// At Fin = 192 with parts 128 / 128 / 64 / 64 the one-image layout of gml_gnnml1_impl.h is 24 blocks x 48 x 64 floats = 294,912 bytes:
// it does not fit, so the image is SPLIT over blockIdx.y and every workgroup holds at most 8 column blocks (GS_GB of each of two
// matrices) of it:
//   group g < ceil(nb1 / 4):  columns 64 g .. 64 g + 63 of fc_i1 AND of conv_i1 (their sum is formed in registers)
//   the last group:           fc_i2 and fc_i3 (their product is formed in registers; no aggregation)
//   LDS = 8 FPL 64 floats = 16,384 / 49,152 / 98,304 bytes at FPL = 8 / 24 / 48 (Fin <= 32 / 96 / 192).
// A lane keeps its x slice and its aggregate slice (FPL registers each) across the group's 2 x 4 MFMA chains, which run interleaved
// (8 independent accumulators per j).  Arithmetic as in gml_gnnml1_impl.h: exact fp32 products on v_mfma_f32_16x16x4_f32, one
// ascending chain per output, VALU aggregation in the CSR's edge order, no atomics: repeat runs are bitwise equal.
//
// Backward.  Phase 1 writes
//   g4 [N, 16 (2 nb1 + 2 nb3)] = [da | dc | df2 | df3],   da = g_sum act'(a), dc = g_sum act'(c), df2 = g_p act(f3) act'(f2), df3 likewise.
// The sum act(a) + act(c) does not tell the two activation patterns apart.  relu: the forward RECORDS them, one byte per 4 columns (bit u:
// a > 0, bit 4 + u: c > 0 of column 4 j + u; 32 bytes per row at n1 = 128), and gml_k_gnnml1s_pat forms da, dc from gout and that byte --
// per row 32 threads of a few dozen instructions and no weight image, against 768 MFMAs per 16-row tile, as many LDS reads and the
// aggregation gather twice for recomputing a and c.  tanh needs both VALUES, not bits: there (and wherever no pattern is handed in) phase 1 is the forward kernel
// again with another epilogue (BWD = true) over all groups.  f2 and f3 are always recomputed, by the last group alone (no aggregation).
// Then q = A dc (gml_k_gnnml1s_q: a plain gather over the source-keyed view), dx = [da | q | df2 | df3] [W1; Wc^T; W2; W3]
// (gml_k_gnnml1s_dx: the transposed image split over blockIdx.y by input-feature blocks, 4 of 12 per workgroup, <= 98,304 bytes), and the
// weight gradients in one pass + one ordered fold (gml_k_gnnml1s_dw: 12 x blocks by 24 g4 blocks).
#include "gml_gnnml1_rows.h"

#define GS_GB 4                                         // 16-column blocks per matrix and workgroup

struct GmlGsParams : GmlG1Params {
    uint8_t* pat; int64_t ldp;                          // the recorded relu patterns [N, ldp >= 4 nb1] (NULL: none)
    int32_t g0;                                         // first column group of the launch (phase 1 with a pattern: the last group only)
};

template <int FPL>
__device__ __forceinline__ void gs_fill(float* dst, const float* w, int n, int Fin, bool conv, int sb0, int tid, int nt) {
    // blocks sb0 .. sb0 + GS_GB of one matrix in the forward form of g1_fill_fwd; zeros past n and past Fin
    for (int i = tid; i < GS_GB * FPL * 64; i += nt) {
        const int lane = i & 63, j = (i >> 6) % FPL, nb = (i >> 6) / FPL;
        const int c = 16 * (sb0 + nb) + (lane & 15), f = (lane >> 4) * FPL + j;
        dst[i] = (c < n && f < Fin) ? (conv ? w[(int64_t)f * n + c] : w[(int64_t)c * Fin + f]) : 0.f;
    }
}

// The lane's slice of one row, xp = the row's base + kq FPL, nf = how many of its FPL features exist (0 for a row past the end).
// g1_load_row's two paths with the choice made ONCE per kernel (vec: 16-byte rows AND Fin % 4 == 0, so a chunk is whole or absent):
// written per element as there, FPL = 48 keeps 48 column indices and their masks alive across the edge loop and spills.
template <int FPL>
__device__ __forceinline__ void gs_load_row(const float* xp, int nf, bool vec, float (&xr)[FPL]) {
    if (vec) {
#pragma unroll
        for (int j4 = 0; j4 < FPL / 4; ++j4) {
            f32x4 t = f32x4{0.f, 0.f, 0.f, 0.f};
            if (4 * j4 < nf) t = *reinterpret_cast<const f32x4*>(xp + 4 * j4);
            xr[4 * j4] = t.x; xr[4 * j4 + 1] = t.y; xr[4 * j4 + 2] = t.z; xr[4 * j4 + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < FPL; ++j) xr[j] = j < nf ? xp[j] : 0.f;
    }
}

// activation value and derivative at a pre-activation
__device__ __forceinline__ void gs_act_d(float v, int act, float& y, float& d) {
    if (act == 0) gml_tanh_d(v, y, d);
    else { y = fmaxf(v, 0.f); d = v > 0.f ? 1.f : 0.f; }
}

// ------------------------------------------------------------------------------------------- forward, and phase 1 of the backward
template <int FPL, bool BWD>
__global__ __launch_bounds__(64 * G1_NW) void gml_k_gnnml1s_main(const GmlGsParams p) {
    extern __shared__ __attribute__((aligned(16))) float wl[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, kq = lane >> 4;
    const int nb1 = (p.n1 + 15) / 16, nb3 = (p.n3 + 15) / 16, nsg = (nb1 + GS_GB - 1) / GS_GB;
    const int g = blockIdx.y + p.g0;
    const bool fac = g >= nsg;                                                       // the fc_i2 / fc_i3 group
    const int b0 = fac ? 0 : GS_GB * g;
    float* wa = wl;
    float* wb = wl + GS_GB * FPL * 64;
    if (fac) {
        gs_fill<FPL>(wa, p.w2, p.n3, p.Fin, false, 0, tid, blockDim.x);
        gs_fill<FPL>(wb, p.w3, p.n3, p.Fin, false, 0, tid, blockDim.x);
    } else {
        gs_fill<FPL>(wa, p.w1, p.n1, p.Fin, false, b0, tid, blockDim.x);
        gs_fill<FPL>(wb, p.wc, p.n2, p.Fin, true, b0, tid, blockDim.x);
    }
    __syncthreads();
    const float* ba = fac ? p.b2 : p.b1;
    const float* bb = fac ? p.b3 : p.bc;
    const int n = fac ? p.n3 : p.n1, ocol = fac ? p.n1 : 0;                           // part width; its column base in out / gout
    const int gA = fac ? 32 * nb1 : 0, gB = fac ? 32 * nb1 + 16 * nb3 : 16 * nb1, gn = 16 * (fac ? nb3 : nb1);   // g4: column bases, part width
    const bool vec = p.ldx % 4 == 0 && p.Fin % 4 == 0 && (reinterpret_cast<uintptr_t>(p.x) & 15) == 0;
    const int nfl = min(max(p.Fin - kq * FPL, 0), FPL);                              // features of the lane's slice
    for (int t = blockIdx.x * G1_NW + wave; t < p.ntiles; t += gridDim.x * G1_NW) {
        const int64_t row = (int64_t)t * 16 + r16;
        const bool valid = row < p.nrows;
        float xr[FPL], hr[FPL];
        if (!fac) {
#pragma unroll
            for (int j = 0; j < FPL; ++j) hr[j] = 0.f;
            const int e0 = valid ? p.rowptr[row] : 0, e1 = valid ? p.rowptr[row + 1] : 0;
#pragma unroll 1
            for (int e = e0; e < e1; ++e) {                                        // the reference's per-target summation order
                const int c = p.col[e];
                const float v = p.val ? p.val[e] : 1.f;
                float xn[FPL];
                gs_load_row<FPL>(p.x + (int64_t)c * p.ldx + kq * FPL, nfl, vec, xn);
#pragma unroll
                for (int j = 0; j < FPL; ++j) hr[j] = fmaf(v, xn[j], hr[j]);
            }
        }
        gs_load_row<FPL>(p.x + row * p.ldx + kq * FPL, valid ? nfl : 0, vec, xr);                 // (after the edge loop: not live across it)
        if (fac) {
#pragma unroll
            for (int j = 0; j < FPL; ++j) hr[j] = xr[j];
        }
        f32x4 A[GS_GB], B[GS_GB];
#pragma unroll
        for (int nb = 0; nb < GS_GB; ++nb) A[nb] = B[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
        // the 8 fragments of step j + 1 are read while the 8 MFMAs of step j issue; the scheduling barrier keeps the compiler from
        // hoisting every LDS read of the tile in front of the first MFMA (8 FPL live registers: scratch at FPL >= 24)
        // (two lane bases, each with immediate offsets below 64 KB: folded into one base the compiler precomputes an address register
        // per 64 KB-crossing fragment outside the tile loop.  The pinned values are LDS-typed 32-bit addresses: pinning generic
        // pointers hides the address space and every fragment read becomes a flat load)
        typedef __attribute__((address_space(3))) const float gs_ldsf;
        gs_ldsf* wal = (gs_ldsf*)(wa + lane);
        gs_ldsf* wbl = (gs_ldsf*)(wb + lane);
        asm volatile("" : "+v"(wal), "+v"(wbl));
        float wn[2 * GS_GB];
#pragma unroll
        for (int nb = 0; nb < GS_GB; ++nb) { wn[nb] = wal[nb * FPL * 64]; wn[GS_GB + nb] = wbl[nb * FPL * 64]; }
#pragma unroll
        for (int j = 0; j < FPL; ++j) {
            float wc[2 * GS_GB];
#pragma unroll
            for (int i = 0; i < 2 * GS_GB; ++i) wc[i] = wn[i];
            if (j + 1 < FPL) {
#pragma unroll
                for (int nb = 0; nb < GS_GB; ++nb) { wn[nb] = wal[(nb * FPL + j + 1) * 64]; wn[GS_GB + nb] = wbl[(nb * FPL + j + 1) * 64]; }
            }
#pragma unroll
            for (int nb = 0; nb < GS_GB; ++nb) {
                A[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[nb], xr[j], A[nb], 0, 0, 0);
                B[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[GS_GB + nb], hr[j], B[nb], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int nb = 0; nb < GS_GB; ++nb) {
            if (16 * (b0 + nb) >= n) break;
            const int c0 = 16 * (b0 + nb) + 4 * kq;
            const f32x4 va = A[nb] + g1_bias4(ba, c0, n), vb = B[nb] + g1_bias4(bb, c0, n);
            if constexpr (!BWD) {
                f32x4 y;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float ya = g1_act(va[u], p.act), yb = g1_act(vb[u], p.act);
                    y[u] = fac ? ya * yb : ya + yb;
                }
                g1_store4(p.out + ocol, p.ldo, row, c0, n, valid, y);
                if (!fac && p.pat && valid) {
                    unsigned bits = 0;
#pragma unroll
                    for (int u = 0; u < 4; ++u) bits |= (va[u] > 0.f ? 1u << u : 0u) | (vb[u] > 0.f ? 16u << u : 0u);
                    p.pat[row * p.ldp + (c0 >> 2)] = (uint8_t)bits;
                }
            } else {
                const f32x4 go = g1_load4(p.gout + ocol, p.ldgo, row, c0, n, valid);
                f32x4 dA, dB;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    float ya, ea, yb, eb;
                    gs_act_d(va[u], p.act, ya, ea);
                    gs_act_d(vb[u], p.act, yb, eb);
                    dA[u] = fac ? go[u] * yb * ea : go[u] * ea;
                    dB[u] = fac ? go[u] * ya * eb : go[u] * eb;
                }
                g1_store4(p.g4 + gA, p.ldg4, row, c0, gn, valid, dA);
                g1_store4(p.g4 + gB, p.ldg4, row, c0, gn, valid, dB);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------- da, dc from the recorded pattern
// one thread per (row, 4 columns): da = gout . [a > 0], dc = gout . [c > 0] (relu), written into the da and dc parts of g4
__global__ __launch_bounds__(256) void gml_k_gnnml1s_pat(const GmlGsParams p) {
    const int nc4 = 4 * ((p.n1 + 15) / 16);
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = idx / nc4;
    const int c4 = (int)(idx - row * nc4);
    if (row >= p.nrows) return;
    const f32x4 go = g1_load4(p.gout, p.ldgo, row, 4 * c4, p.n1, true);
    const unsigned bits = p.pat[row * p.ldp + c4];
    f32x4 da, dc;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        da[u] = go[u] * ((bits >> u) & 1u ? 1.f : 0.f);
        dc[u] = go[u] * ((bits >> (4 + u)) & 1u ? 1.f : 0.f);
    }
    float* g = p.g4 + row * p.ldg4 + 4 * c4;
    *reinterpret_cast<f32x4*>(g) = da;
    *reinterpret_cast<f32x4*>(g + 4 * nc4) = dc;
}

// ------------------------------------------------------------------------------------------------------------- q = A dc
// one thread per (row, 4 columns): q[row] = sum over the row's OUT-edges (source-keyed view) of val * dc[destination], in edge order
__global__ __launch_bounds__(256) void gml_k_gnnml1s_q(const GmlGsParams p) {
    const int nc4 = 4 * ((p.n1 + 15) / 16);
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = idx / nc4;
    const int c4 = (int)(idx - row * nc4);
    if (row >= p.nrows) return;
    const float* dcb = p.g4 + 4 * nc4 + 4 * c4;                                        // the dc part follows the da part
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    const int e0 = p.rowptr[row], e1 = p.rowptr[row + 1];
    for (int e = e0; e < e1; ++e) {
        const int64_t d = p.col[e];
        const float v = p.val ? p.val[e] : 1.f;
        const f32x4 dn = *reinterpret_cast<const f32x4*>(dcb + d * p.ldg4);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = fmaf(v, dn[u], acc[u]);
    }
    *reinterpret_cast<f32x4*>(p.q + row * p.ldq + 4 * c4) = acc;
}

// ------------------------------------------------------------------------------------------------------------------ dx
// dx[r] = da[r] W1 + q[r] Wc^T + df2[r] W2 + df3[r] W3: K blocks in the order of g4 (the dc part replaced by q), the transposed
// image [fb < GS_GB][K block][4][64] of the workgroup's GS_GB input-feature blocks (gml_gnnml1_impl.h: fill_tr); GS_GB chains run
// interleaved, each ascending in k.
__global__ __launch_bounds__(64 * G1_NW) void gml_k_gnnml1s_dx(const GmlGsParams p) {
    extern __shared__ __attribute__((aligned(16))) float wl[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, kq = lane >> 4;
    const int nb1 = (p.n1 + 15) / 16, nb3 = (p.n3 + 15) / 16, nkb = 2 * nb1 + 2 * nb3;
    const int fb0 = GS_GB * blockIdx.y;
    for (int i = tid; i < GS_GB * nkb * 256; i += blockDim.x) {
        const int ln = i & 63, reg = (i >> 6) & 3, kb = (i >> 8) % nkb, fbl = (i >> 8) / nkb;
        const int f = 16 * (fb0 + fbl) + (ln & 15);
        const float* w;
        int n, nb;
        if (kb < nb1) { w = p.w1; n = p.n1; nb = kb; }
        else if (kb < 2 * nb1) { w = p.wc; n = p.n2; nb = kb - nb1; }
        else if (kb < 2 * nb1 + nb3) { w = p.w2; n = p.n3; nb = kb - 2 * nb1; }
        else { w = p.w3; n = p.n3; nb = kb - 2 * nb1 - nb3; }
        const bool conv = kb >= nb1 && kb < 2 * nb1;
        const int c = 16 * nb + 4 * (ln >> 4) + reg;
        wl[i] = (c < n && f < p.Fin) ? (conv ? w[(int64_t)f * n + c] : w[(int64_t)c * p.Fin + f]) : 0.f;
    }
    __syncthreads();
    for (int t = blockIdx.x * G1_NW + wave; t < p.ntiles; t += gridDim.x * G1_NW) {
        const int64_t row = (int64_t)t * 16 + r16;
        const bool valid = row < p.nrows;
        f32x4 acc[GS_GB];
#pragma unroll
        for (int fbl = 0; fbl < GS_GB; ++fbl) acc[fbl] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kb = 0; kb < nkb; ++kb) {
            const bool isq = kb >= nb1 && kb < 2 * nb1;
            const f32x4 d = isq ? g1_load4(p.q, p.ldq, row, 16 * (kb - nb1) + 4 * kq, 16 * nb1, valid)
                                : g1_load4(p.g4, p.ldg4, row, 16 * kb + 4 * kq, 16 * nkb, valid);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg)
#pragma unroll
                for (int fbl = 0; fbl < GS_GB; ++fbl)
                    acc[fbl] = __builtin_amdgcn_mfma_f32_16x16x4f32(wl[((fbl * nkb + kb) * 4 + reg) * 64 + lane], d[reg], acc[fbl], 0, 0, 0);
        }
#pragma unroll
        for (int fbl = 0; fbl < GS_GB; ++fbl)
            if (16 * (fb0 + fbl) < p.Fin) g1_store4(p.dx, p.lddx, row, 16 * (fb0 + fbl) + 4 * kq, p.Fin, valid, acc[fbl]);
    }
}

// ------------------------------------------------------------------------------------------------------- weight gradients
// As gml_k_gnnml1w_dw (gml_gnnml1_impl.h), for 12 x blocks by 24 g4 blocks: wave w owns the g4 blocks w, w + 8, w + 16 and walks the rows
// of the workgroup's chunk once for them against the GS_NXB x blocks of blockIdx.y (3 x 6 accumulator tiles); then the waves below
// GS_NXB form their x block of dWc = x^T q against all (<= 8) q blocks.  One partial per blockIdx.x, laid out as the flat result
// [dW1 | dW2 | dW3 | dWc | sums] (the two halves of blockIdx.y write disjoint elements of it), folded in order by gml_fold_many.
struct GmlGsDwParams {
    const float* x; int64_t ldx; const float* g4; int64_t ldg4; const float* q; int64_t ldq;
    int64_t nrows; int32_t Fin, n1, n3;
    float* part; int64_t nflat; int32_t rows_per_wg;
};
#define GS_NXB 6
#define GS_NGW 3

__global__ __launch_bounds__(64 * G1_NW) void gml_k_gnnml1s_dw(const GmlGsDwParams p) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), c16 = lane & 15, k4 = lane >> 4;
    const int nb1 = (p.n1 + 15) / 16, nb3 = (p.n3 + 15) / 16, nfb = (p.Fin + 15) / 16;
    const int ngb = 2 * nb1 + 2 * nb3;                                   // 16-column blocks of g4 (<= 24)
    const int xb0 = GS_NXB * blockIdx.y;
    const int64_t r_begin = (int64_t)blockIdx.x * p.rows_per_wg;
    const int64_t r_end = min(r_begin + (int64_t)p.rows_per_wg, p.nrows);
    float* out = p.part + (int64_t)blockIdx.x * p.nflat;
    const int64_t o_w1 = 0, o_w2 = (int64_t)p.n1 * p.Fin, o_w3 = o_w2 + (int64_t)p.n3 * p.Fin, o_wc = o_w3 + (int64_t)p.n3 * p.Fin,
                  o_s = o_wc + (int64_t)p.Fin * p.n1;
    constexpr int U = 4;
    {
        int na = 0;
#pragma unroll
        for (int i = 0; i < GS_NGW; ++i) na += (wave + G1_NW * i < ngb) ? 1 : 0;
        f32x4 acc[GS_NGW][GS_NXB];
        float bsum[GS_NGW];
#pragma unroll
        for (int i = 0; i < GS_NGW; ++i) {
            bsum[i] = 0.f;
#pragma unroll
            for (int b = 0; b < GS_NXB; ++b) acc[i][b] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if (na > 0) {
            for (int64_t r = r_begin; r < r_end; r += 4 * U) {
                float av[U][GS_NGW], bv[U][GS_NXB];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int64_t row = r + 4 * u + k4;
                    const bool rv = row < r_end;
#pragma unroll
                    for (int i = 0; i < GS_NGW; ++i) av[u][i] = (i < na && rv) ? p.g4[row * p.ldg4 + 16 * (wave + G1_NW * i) + c16] : 0.f;
#pragma unroll
                    for (int b = 0; b < GS_NXB; ++b)
                        bv[u][b] = (rv && 16 * (xb0 + b) + c16 < p.Fin) ? p.x[row * p.ldx + 16 * (xb0 + b) + c16] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int i = 0; i < GS_NGW; ++i) {
                        bsum[i] += av[u][i];
#pragma unroll
                        for (int b = 0; b < GS_NXB; ++b) acc[i][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][i], bv[u][b], acc[i][b], 0, 0, 0);
                    }
            }
        }
#pragma unroll
        for (int i = 0; i < GS_NGW; ++i) {
            const int grp = wave + G1_NW * i;
            if (grp >= ngb) continue;
            // g4 block `grp` belongs to [da nb1 | dc nb1 | df2 nb3 | df3 nb3]; the dc blocks have no Linear weight: their sums only
            const bool isdc = grp >= nb1 && grp < 2 * nb1;
            if (!isdc) {
                const int g2 = grp - 2 * nb1;
                const int m = grp < nb1 ? 0 : (g2 < nb3 ? 1 : 2), nb = grp < nb1 ? grp : (g2 < nb3 ? g2 : g2 - nb3);
                const int n = m == 0 ? p.n1 : p.n3;
                float* w = out + (m == 0 ? o_w1 : (m == 1 ? o_w2 : o_w3));
#pragma unroll
                for (int b = 0; b < GS_NXB; ++b) {
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {                   // D[i = g4 column 4 k4 + reg][j = x column c16]
                        const int c = 16 * nb + 4 * k4 + reg, f = 16 * (xb0 + b) + c16;
                        if (c < n && f < p.Fin) w[(int64_t)c * p.Fin + f] = acc[i][b][reg];
                    }
                }
            }
            if (blockIdx.y == 0) {
                float t = bsum[i];
                t += __shfl_xor(t, 16);
                t += __shfl_xor(t, 32);
                if (k4 == 0) out[o_s + 16 * grp + c16] = t;
            }
        }
    }
    // dWc = x^T q: x block xb0 + wave against all q blocks
    const int fb = xb0 + wave;
    if (wave < GS_NXB && fb < nfb) {
        f32x4 acc[8];
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int64_t r = r_begin; r < r_end; r += 4 * U) {
            float av[U], bv[U][8];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t row = r + 4 * u + k4;
                const bool rv = row < r_end;
                av[u] = (rv && 16 * fb + c16 < p.Fin) ? p.x[row * p.ldx + 16 * fb + c16] : 0.f;
#pragma unroll
                for (int b = 0; b < 8; ++b) bv[u][b] = (b < nb1 && rv) ? p.q[row * p.ldq + 16 * b + c16] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int b = 0; b < 8; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u][b], acc[b], 0, 0, 0);
        }
#pragma unroll
        for (int b = 0; b < 8; ++b) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int f = 16 * fb + 4 * k4 + reg, c = 16 * b + c16;
                if (f < p.Fin && c < p.n1) out[o_wc + (int64_t)f * p.n1 + c] = acc[b][reg];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ entry points
static int gs_fpl(int Fin) { return Fin <= 32 ? 8 : (Fin <= 96 ? 24 : 48); }

extern "C" int gml_gnnml1_sum_supported(int32_t Fin, int32_t n1, int32_t n2, int32_t n3) {
    return (Fin > 0 && n1 > 0 && n3 > 0 && n1 == n2 && Fin <= 192 && n1 <= 128 && n3 <= 64) ? 1 : 0;
}

static int gs_check(const GmlGsParams& p) {
    if (p.nrows < 0 || p.Fin <= 0 || p.n1 <= 0 || p.n2 <= 0 || p.n3 <= 0 || p.n1 != p.n2 || p.act < 0 || p.act > 1) return GML_E_BADARG;
    if (!gml_gnnml1_sum_supported(p.Fin, p.n1, p.n2, p.n3)) return GML_E_UNSUPPORTED;
    if (!p.rowptr || !p.col || !p.x || !p.w1 || !p.wc || !p.w2 || !p.w3 || p.ldx < p.Fin) return GML_E_BADARG;
    return GML_OK;
}

// workgroups along x: one 16-row tile per wave and trip; all groups together fill the device once (twice while two images fit a CU)
static unsigned gs_grid_x(int ntiles, size_t lds, int ny) {
    int64_t gx = gml_cdiv(ntiles, G1_NW);
    const int64_t cap = (lds > 80 * 1024 ? 1 : 2) * GML_NUM_CU / ny;
    return (unsigned)(gx > cap ? cap : gx);
}

template <int FPL, bool BWD>
static int gs_main_t(const GmlGsParams& p, hipStream_t st) {
    const size_t lds = (size_t)2 * GS_GB * FPL * 64 * sizeof(float);
    const int ny = ((p.n1 + 15) / 16 + GS_GB - 1) / GS_GB + 1 - p.g0;
    GML_ALLOW_BIG_LDS(rc_big, (&gml_k_gnnml1s_main<FPL, BWD>), 160 * 1024)
    if (rc_big != hipSuccess) return (int)rc_big;
    hipLaunchKernelGGL((gml_k_gnnml1s_main<FPL, BWD>), dim3(gs_grid_x(p.ntiles, lds, ny), (unsigned)ny), dim3(64 * G1_NW), lds, st, p);
    return gml_launch_status();
}

template <bool BWD>
static int gs_main(const GmlGsParams& p, hipStream_t st) {
    switch (gs_fpl(p.Fin)) {
        case 8: return gs_main_t<8, BWD>(p, st);
        case 24: return gs_main_t<24, BWD>(p, st);
        default: return gs_main_t<48, BWD>(p, st);
    }
}

extern "C" int gml_gnnml1_sum_fwd(const int32_t* rowptr, const int32_t* col, const float* val, const float* x, int64_t ldx, int64_t num_rows,
                                  int32_t Fin, const float* w1, const float* b1, int32_t n1, const float* wc, const float* bc, int32_t n2,
                                  const float* w2, const float* b2, const float* w3, const float* b3, int32_t n3, int32_t act,
                                  float* out, int64_t ldo, uint8_t* pattern, int64_t ldp, gml_stream_t stream) {
    GmlGsParams p = {};
    p.pat = pattern; p.ldp = ldp;
    p.rowptr = rowptr; p.col = col; p.val = val; p.x = x; p.ldx = ldx; p.w1 = w1; p.b1 = b1; p.wc = wc; p.bc = bc; p.w2 = w2; p.b2 = b2;
    p.w3 = w3; p.b3 = b3; p.out = out; p.ldo = ldo; p.nrows = num_rows; p.Fin = Fin; p.n1 = n1; p.n2 = n2; p.n3 = n3; p.mode = 4; p.act = act;
    const int rc = gs_check(p);
    if (rc != GML_OK) return rc;
    if (!out || ldo < n1 + n3 || (pattern && ldp < 4 * ((n1 + 15) / 16))) return GML_E_BADARG;
    if (num_rows == 0) return GML_OK;
    p.ntiles = (int)gml_cdiv(num_rows, 16);
    return gs_main<false>(p, (hipStream_t)stream);
}

extern "C" int gml_gnnml1_sum_g4_cols(int32_t n1, int32_t n2, int32_t n3) {
    return 16 * ((n1 + 15) / 16 + (n2 + 15) / 16 + 2 * ((n3 + 15) / 16));
}

extern "C" int gml_gnnml1_sum_bwd(const int32_t* rowptr, const int32_t* col, const float* val, const int32_t* rowptr_t, const int32_t* col_t,
                                  const float* val_t, const float* x, int64_t ldx, const float* gout, int64_t ldgo, int64_t num_rows,
                                  int32_t Fin, const float* w1, const float* b1, int32_t n1, const float* wc, const float* bc, int32_t n2,
                                  const float* w2, const float* b2, const float* w3, const float* b3, int32_t n3, int32_t act,
                                  const uint8_t* pattern, int64_t ldp, float* dx, int64_t lddx, float* g4, int64_t ldg4, float* q, int64_t ldq,
                                  gml_stream_t stream) {
    GmlGsParams p = {};
    p.pat = const_cast<uint8_t*>(pattern); p.ldp = ldp;
    p.rowptr = rowptr; p.col = col; p.val = val; p.x = x; p.ldx = ldx; p.w1 = w1; p.b1 = b1; p.wc = wc; p.bc = bc; p.w2 = w2; p.b2 = b2;
    p.w3 = w3; p.b3 = b3; p.gout = gout; p.ldgo = ldgo; p.dx = dx; p.lddx = lddx; p.g4 = g4; p.ldg4 = ldg4; p.q = q; p.ldq = ldq;
    p.nrows = num_rows; p.Fin = Fin; p.n1 = n1; p.n2 = n2; p.n3 = n3; p.mode = 4; p.act = act;
    const int rc = gs_check(p);
    if (rc != GML_OK) return rc;
    if (!rowptr_t || !col_t || !gout || !g4 || !q || ldgo < n1 + n3 || (dx && lddx < Fin)) return GML_E_BADARG;
    const int nb1 = (n1 + 15) / 16, nb3 = (n3 + 15) / 16;
    if (pattern && (act != 1 || ldp < 4 * nb1)) return GML_E_BADARG;      // (bits are relu's derivative only)
    if (ldg4 < gml_gnnml1_sum_g4_cols(n1, n2, n3) || ldg4 % 4 != 0 || ldq < 16 * nb1 || ldq % 4 != 0) return GML_E_BADARG;
    if (((uintptr_t)g4 & 15) != 0 || ((uintptr_t)q & 15) != 0) return GML_E_BADARG;
    if (num_rows == 0) return GML_OK;
    p.ntiles = (int)gml_cdiv(num_rows, 16);
    hipStream_t st = (hipStream_t)stream;
    if (pattern) {                                                           // da, dc from the pattern; df2, df3 by the last group alone
        hipLaunchKernelGGL(gml_k_gnnml1s_pat, dim3((unsigned)gml_cdiv(num_rows * 4 * nb1, 256)), dim3(256), 0, st, p);
        p.g0 = (nb1 + GS_GB - 1) / GS_GB;
    }
    const int rc1 = gs_main<true>(p, st);                                   // g4 (all of it without a pattern: the target-keyed view)
    if (rc1 != GML_OK) return rc1;
    p.g0 = 0;
    p.rowptr = rowptr_t; p.col = col_t; p.val = val_t;                       // q and dx: the source-keyed view
    hipLaunchKernelGGL(gml_k_gnnml1s_q, dim3((unsigned)gml_cdiv(num_rows * 4 * nb1, 256)), dim3(256), 0, st, p);
    if (dx) {
        const size_t lds = (size_t)GS_GB * (2 * nb1 + 2 * nb3) * 256 * sizeof(float);
        const int ny = (int)gml_cdiv(gml_cdiv(Fin, 16), GS_GB);
        GML_ALLOW_BIG_LDS(rc_big, (&gml_k_gnnml1s_dx), 160 * 1024)
        if (rc_big != hipSuccess) return (int)rc_big;
        hipLaunchKernelGGL(gml_k_gnnml1s_dx, dim3(gs_grid_x(p.ntiles, lds, ny), (unsigned)ny), dim3(64 * G1_NW), lds, st, p);
    }
    return gml_launch_status();
}

// floats of the flat result [dW1 (n1 x Fin) | dW2 (n3 x Fin) | dW3 (n3 x Fin) | dWc (Fin x n2) | column sums of g4]
extern "C" int64_t gml_gnnml1_sum_dw_floats(int32_t Fin, int32_t n1, int32_t n2, int32_t n3) {
    return (int64_t)n1 * Fin + 2 * (int64_t)n3 * Fin + (int64_t)Fin * n2 + gml_gnnml1_sum_g4_cols(n1, n2, n3);
}

static int gs_dw_grid(int64_t n) {
    int64_t g = gml_cdiv(n, 128);
    if (g > GML_NUM_CU) g = GML_NUM_CU;
    return g < 1 ? 1 : (int)g;
}

extern "C" size_t gml_gnnml1_sum_dw_workspace_bytes(int64_t num_rows, int32_t Fin, int32_t n1, int32_t n2, int32_t n3) {
    return (size_t)gs_dw_grid(num_rows) * (size_t)gml_gnnml1_sum_dw_floats(Fin, n1, n2, n3) * sizeof(float);
}

extern "C" int gml_gnnml1_sum_dw(const float* x, int64_t ldx, const float* g4, int64_t ldg4, const float* q, int64_t ldq, int64_t num_rows,
                                 int32_t Fin, int32_t n1, int32_t n2, int32_t n3, float* out_flat, void* ws, size_t ws_bytes,
                                 gml_stream_t stream) {
    if (Fin <= 0 || n1 <= 0 || n2 <= 0 || n3 <= 0 || n1 != n2) return GML_E_BADARG;
    if (!gml_gnnml1_sum_supported(Fin, n1, n2, n3)) return GML_E_UNSUPPORTED;
    if (num_rows < 0 || !x || !g4 || !q || !out_flat || ldx < Fin || ldg4 < gml_gnnml1_sum_g4_cols(n1, n2, n3) || ldq < 16 * ((n1 + 15) / 16))
        return GML_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nflat = gml_gnnml1_sum_dw_floats(Fin, n1, n2, n3);
    if (num_rows == 0) { gml_zero_async(out_flat, sizeof(float) * nflat, st); return gml_launch_status(); }
    if (!ws || ws_bytes < gml_gnnml1_sum_dw_workspace_bytes(num_rows, Fin, n1, n2, n3)) return GML_E_WORKSPACE;
    GmlGsDwParams p;
    p.x = x; p.ldx = ldx; p.g4 = g4; p.ldg4 = ldg4; p.q = q; p.ldq = ldq; p.nrows = num_rows; p.Fin = Fin; p.n1 = n1; p.n3 = n3;
    p.part = (float*)ws; p.nflat = nflat;
    const int grid = gs_dw_grid(num_rows);
    p.rows_per_wg = (int)((gml_cdiv(num_rows, grid) + 3) / 4 * 4);
    gml_zero_async(ws, (size_t)grid * nflat * sizeof(float), st);       // (a workgroup whose row chunk is empty still leaves a defined partial)
    const int ny = (int)gml_cdiv(gml_cdiv(Fin, 16), GS_NXB);
    hipLaunchKernelGGL(gml_k_gnnml1s_dw, dim3((unsigned)grid, (unsigned)ny), dim3(64 * G1_NW), 0, st, p);
    const int rc = gml_launch_status();
    if (rc != GML_OK) return rc;
    gml_fold_job job = {};
    job.partial = (const float*)ws; job.nparts = grid; job.n = nflat; job.dst[0] = out_flat; job.ndst[0] = nflat;
    return gml_fold_many(&job, 1, stream);
}
