// Readout head + sum binary cross-entropy on logits + number of correct predictions of the EXP classification experiment
// (reference: exp_classify.py:293-295 GNNML3 head, :260-262 GNNML1 head, :328-329 loss, :334 accuracy)
//
//   h = act(W1 p + b1),   z = w2 . h + b2,   l = y softplus(-z) + (1 - y) softplus(z)   (each softplus capped at 100)
//   loss = sum_r valid[r] l_r,   ok = sum_r valid[r] [(z_r > 0) == (y_r == 1)],   n = #{r: valid[r] != 0}       r < rows_loss
//
// one pass forward and one pass backward for ANY number of rows and any widths nin, nh <= 64 (the experiment's are 48 -> 10 with relu
// and 64 -> 10 without: neither is a multiple of 4, so gml_head.hip serves neither).  A workgroup of 256 threads owns slabs of up to 256
// rows held in LDS, laid out as in gml_head.hip with every LDS row padded with zeros to a multiple of 4 floats (16-byte LDS reads,
// scalar global accesses: no alignment asked of the caller).  One slab: every result is written by that launch.  More slabs: a
// workgroup adds its slabs (ascending) into ONE record  dW1 | db1 | dw2 | db2 | loss | ok | n  in the caller's workspace and a second
// small launch adds the records in ascending workgroup order.  No atomics, every sum in a fixed order: bitwise repeatable.
#include "gml_common.h"

#define HBCE_ROWS 256                /* rows per slab = threads per workgroup */
#define HBCE_MAX_W 64
#define HBCE_MAX_GRID GML_NUM_CU     /* workgroups (= partial records) of a launch */

struct GmlHeadBceParams {
    const float* p; int64_t ldp;
    const float* y; const float* valid;                       // [Rl]; valid may be NULL (all ones)
    const float* w1; const float* b1; const float* w2; const float* b2;   // [nh, nin], [nh], [1, nh], [1]
    int64_t R, Rl;                                             // pooled rows, rows that enter the loss (<= R)
    int32_t nin, nh, act;                                      // act: 1 = relu, 0 = identity
    int64_t nslabs;
    float* part;                                               // NULL: one workgroup writes the results itself; else [grid][npart] records
    float* loss; float* pre; float* stats;                     // forward
    const float* gscale;                                       // backward: upstream gradient of the loss (device scalar; NULL = 1)
    float* gp; int64_t ldgp;
    float* dw1; float* db1; float* dw2; float* db2;
};

__host__ __device__ __forceinline__ int hbce_up4(int n) { return (n + 3) & ~3; }
__host__ __device__ __forceinline__ int hbce_npart(int nin, int nh) { return nh * nin + 2 * nh + 1 + 3; }

__device__ __forceinline__ float hbce_dot4(const f32x4 a, const f32x4 b, float acc) {
    acc = fmaf(a.x, b.x, acc); acc = fmaf(a.y, b.y, acc); acc = fmaf(a.z, b.z, acc); return fmaf(a.w, b.w, acc);
}

// LDS regions (floats), every one 16-byte aligned
struct HbceLds {
    float *ps, *hs, *w1s, *w2s, *b1s, *pre, *sg, *red;
    int n4, h4;
    __device__ HbceLds(float* sm, int nin, int nh, int slab_rows) {
        n4 = hbce_up4(nin); h4 = hbce_up4(nh);
        ps = sm; hs = ps + slab_rows * n4; w1s = hs + slab_rows * h4; w2s = w1s + nh * n4; b1s = w2s + h4;
        pre = b1s + h4; sg = pre + HBCE_ROWS; red = sg + HBCE_ROWS;
    }
};
static size_t hbce_lds_floats(int nin, int nh, int slab_rows) {
    const int n4 = hbce_up4(nin), h4 = hbce_up4(nh);
    return (size_t)slab_rows * n4 + (size_t)slab_rows * h4 + (size_t)nh * n4 + 2 * (size_t)h4 + 2 * HBCE_ROWS + 3 * HBCE_ROWS;
}

// W1 rows, w2 and b1 into LDS, the padding columns zero
__device__ __forceinline__ void hbce_load_weights(const GmlHeadBceParams& q, const HbceLds& L) {
    const int tid = threadIdx.x;
    for (int i = tid; i < q.nh * L.n4; i += HBCE_ROWS) {
        const int j = i / L.n4, k = i % L.n4;
        L.w1s[i] = k < q.nin ? q.w1[j * q.nin + k] : 0.f;
    }
    for (int j = tid; j < L.h4; j += HBCE_ROWS) {
        L.w2s[j] = j < q.nh ? q.w2[j] : 0.f;
        L.b1s[j] = (j < q.nh && q.b1) ? q.b1[j] : 0.f;
    }
}

// the slab's rows [r0, r0 + nr): ps, hs = act(W1 p + b1) (padding columns zero), pre = w2 . h + b2
__device__ __forceinline__ void hbce_forward(const GmlHeadBceParams& q, const HbceLds& L, int64_t r0, int nr) {
    const int tid = threadIdx.x;
    const int n4 = L.n4, h4 = L.h4;
    for (int i = tid; i < nr * n4; i += HBCE_ROWS) {
        const int r = i / n4, k = i % n4;
        L.ps[i] = k < q.nin ? q.p[(r0 + r) * q.ldp + k] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < nr * h4; i += HBCE_ROWS) {
        const int r = i / h4, j = i % h4;
        float a = 0.f;
        if (j < q.nh) {
            a = L.b1s[j];
#pragma unroll 8
            for (int k = 0; k < n4 / 4; ++k)
                a = hbce_dot4(*reinterpret_cast<const f32x4*>(L.w1s + j * n4 + 4 * k), *reinterpret_cast<const f32x4*>(L.ps + r * n4 + 4 * k), a);
            if (q.act) a = fmaxf(a, 0.f);
        }
        L.hs[i] = a;
    }
    __syncthreads();
    for (int r = tid; r < nr; r += HBCE_ROWS) {
        float a = q.b2 ? q.b2[0] : 0.f;
#pragma unroll 8
        for (int j = 0; j < h4 / 4; ++j)
            a = hbce_dot4(*reinterpret_cast<const f32x4*>(L.w2s + 4 * j), *reinterpret_cast<const f32x4*>(L.hs + r * h4 + 4 * j), a);
        L.pre[r] = a;
    }
    __syncthreads();
}

// e = exp(-|z|) serves both: softplus(t) = max(t, 0) + log1p(e) for t = +-z, sigmoid(|z|) = 1 / (1 + e), sigmoid(-|z|) = e / (1 + e)
__device__ __forceinline__ float hbce_loss(float z, float y) {
    const float l1p = log1pf(expf(-fabsf(z)));
    const float sp_pos = fminf(fmaxf(z, 0.f) + l1p, 100.f), sp_neg = fminf(fmaxf(-z, 0.f) + l1p, 100.f);   // softplus(z), softplus(-z)
    return y * sp_neg + (1.f - y) * sp_pos;
}
__device__ __forceinline__ float hbce_sigmoid(float t) {
    const float e = expf(-fabsf(t));
    return (t >= 0.f ? 1.f : e) / (1.f + e);
}
// sigmoid(z) - y without the cancellation at a saturated logit of the right class (y = 1: -(1 - sigmoid(z)) = -sigmoid(-z))
__device__ __forceinline__ float hbce_dz(float z, float y) {
    return y == 1.f ? -hbce_sigmoid(-z) : (y == 0.f ? hbce_sigmoid(z) : hbce_sigmoid(z) - y);
}

// fixed-order tree over the 256 threads' three partial sums; the totals are valid for thread 0
__device__ __forceinline__ void hbce_reduce3(float* red, float& a, float& b, float& c) {
    const int tid = threadIdx.x;
    red[tid] = a; red[HBCE_ROWS + tid] = b; red[2 * HBCE_ROWS + tid] = c;
    __syncthreads();
    for (int s = HBCE_ROWS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red[tid] += red[tid + s]; red[HBCE_ROWS + tid] += red[HBCE_ROWS + tid + s]; red[2 * HBCE_ROWS + tid] += red[2 * HBCE_ROWS + tid + s];
        }
        __syncthreads();
    }
    a = red[0]; b = red[HBCE_ROWS]; c = red[2 * HBCE_ROWS];
    __syncthreads();
}

// the slab's loss, correct predictions and valid rows (thread 0 holds the totals)
__device__ __forceinline__ void hbce_slab_loss(const GmlHeadBceParams& q, const HbceLds& L, int64_t r0, int nr, float& l, float& ok, float& n) {
    l = 0.f; ok = 0.f; n = 0.f;
    const int r = threadIdx.x;
    if (r < nr && r0 + r < q.Rl) {
        const float z = L.pre[r], y = q.y[r0 + r], v = q.valid ? q.valid[r0 + r] : 1.f;
        l = v * hbce_loss(z, y);
        ok = ((z > 0.f) == (y == 1.f)) ? v : 0.f;
        n = v != 0.f ? 1.f : 0.f;
    }
    hbce_reduce3(L.red, l, ok, n);
}

__global__ __launch_bounds__(HBCE_ROWS) void gml_k_head_bce_fwd(const GmlHeadBceParams q, int slab_rows) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const HbceLds L(sm, q.nin, q.nh, slab_rows);
    hbce_load_weights(q, L);
    float al = 0.f, aok = 0.f, an = 0.f;                       // (thread 0: this workgroup's slabs in ascending order)
    for (int64_t s = blockIdx.x; s < q.nslabs; s += gridDim.x) {
        const int64_t r0 = s * HBCE_ROWS;
        const int nr = (int)min((int64_t)HBCE_ROWS, q.R - r0);
        hbce_forward(q, L, r0, nr);
        if (q.pre && (int)threadIdx.x < nr) q.pre[r0 + threadIdx.x] = L.pre[threadIdx.x];
        float l, ok, n;
        hbce_slab_loss(q, L, r0, nr, l, ok, n);
        al += l; aok += ok; an += n;
    }
    if (threadIdx.x != 0) return;
    if (q.part) {
        float* P = q.part + (int64_t)blockIdx.x * hbce_npart(q.nin, q.nh) + q.nh * q.nin + 2 * q.nh + 1;
        P[0] = al; P[1] = aok; P[2] = an;
    } else {
        q.loss[0] = al;
        if (q.stats) { q.stats[0] += al; q.stats[1] += aok; q.stats[2] += an; }
    }
}

__global__ __launch_bounds__(HBCE_ROWS) void gml_k_head_bce_bwd(const GmlHeadBceParams q, int slab_rows) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const HbceLds L(sm, q.nin, q.nh, slab_rows);
    const int tid = threadIdx.x, n4 = L.n4, h4 = L.h4, nk = n4 / 4;
    hbce_load_weights(q, L);
    const float gs = q.gscale ? q.gscale[0] : 1.f;
    // this workgroup's sums over its slabs: thread <-> dW1 items (unit j, 4 consecutive inputs) tid, tid + 256, ... (<= 64 * 16 = 4 x 256);
    // threads j < nh: db1[j], dw2[j]; the last thread: db2
    f32x4 aw[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) aw[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    float ab1 = 0.f, aw2 = 0.f, ab2 = 0.f;
    for (int64_t s = blockIdx.x; s < q.nslabs; s += gridDim.x) {
        const int64_t r0 = s * HBCE_ROWS;
        const int nr = (int)min((int64_t)HBCE_ROWS, q.R - r0);
        hbce_forward(q, L, r0, nr);
        if (tid < nr) {
            float d = 0.f;
            if (r0 + tid < q.Rl) d = gs * (q.valid ? q.valid[r0 + tid] : 1.f) * hbce_dz(L.pre[tid], q.y[r0 + tid]);
            L.sg[tid] = d;
        }
        __syncthreads();
        // d loss / d p: thread <-> (row, 4 consecutive inputs); dh[r][j] = sg[r] w2[j] [h > 0 under relu].  A row outside the loss gets exact zeros.
        for (int i = tid; i < nr * nk; i += HBCE_ROWS) {
            const int r = i / nk, k = 4 * (i % nk);
            const float sgr = L.sg[r];
            f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
            if (sgr != 0.f) {
#pragma unroll 8
                for (int j = 0; j < q.nh; ++j) {
                    const float d = (q.act && !(L.hs[r * h4 + j] > 0.f)) ? 0.f : sgr * L.w2s[j];
                    a += d * *reinterpret_cast<const f32x4*>(L.w1s + j * n4 + k);
                }
            }
            float* dst = q.gp + (r0 + r) * q.ldgp + k;
            dst[0] = a.x;
            if (k + 1 < q.nin) dst[1] = a.y;
            if (k + 2 < q.nin) dst[2] = a.z;
            if (k + 3 < q.nin) dst[3] = a.w;
        }
        // dW1[j][k] += sum_r dh[r][j] p[r][k];  db1[j] += sum_r dh[r][j];  dw2[j] += sum_r sg[r] h[r][j];  db2 += sum_r sg[r]  (ascending r)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = tid + u * HBCE_ROWS;
            if (i < q.nh * nk) {
                const int j = i / nk, k = 4 * (i % nk);
                const float w2j = L.w2s[j];
                f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
                for (int r = 0; r < nr; ++r) {
                    const float d = (q.act && !(L.hs[r * h4 + j] > 0.f)) ? 0.f : L.sg[r] * w2j;
                    a += d * *reinterpret_cast<const f32x4*>(L.ps + r * n4 + k);
                }
                aw[u] += a;
            }
        }
        if (tid < q.nh) {
            const float w2j = L.w2s[tid];
            float a = 0.f, b = 0.f;
#pragma unroll 4
            for (int r = 0; r < nr; ++r) {
                const float h = L.hs[r * h4 + tid];
                a += (q.act && !(h > 0.f)) ? 0.f : L.sg[r] * w2j;
                b = fmaf(L.sg[r], h, b);
            }
            ab1 += a; aw2 += b;
        }
        if (tid == HBCE_ROWS - 1) {
            float a = 0.f;
            for (int r = 0; r < nr; ++r) a += L.sg[r];
            ab2 += a;
        }
        __syncthreads();                                       // (the next slab overwrites ps / hs / sg)
    }
    // results: the caller's gradients (one workgroup) or this workgroup's record
    const int nw = q.nh * q.nin;
    float* W = q.part ? q.part + (int64_t)blockIdx.x * hbce_npart(q.nin, q.nh) : q.dw1;
    float* B1 = q.part ? W + nw : q.db1;
    float* W2 = q.part ? W + nw + q.nh : q.dw2;
    float* B2 = q.part ? W + nw + 2 * q.nh : q.db2;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = tid + u * HBCE_ROWS;
        if (i < q.nh * nk) {
            const int j = i / nk, k = 4 * (i % nk);
            float* dst = W + j * q.nin + k;
            dst[0] = aw[u].x;
            if (k + 1 < q.nin) dst[1] = aw[u].y;
            if (k + 2 < q.nin) dst[2] = aw[u].z;
            if (k + 3 < q.nin) dst[3] = aw[u].w;
        }
    }
    if (tid < q.nh) {
        if (B1) B1[tid] = ab1;
        W2[tid] = aw2;
    }
    if (tid == HBCE_ROWS - 1 && B2) B2[0] = ab2;
}

// columns [c0, npart) of the records added in ascending record order: thread <-> column.  The last three columns go to loss / stats
// (forward: c0 = npart - 3), the others to dw1 | db1 | dw2 | db2 (backward: c0 = 0, the last three columns are not its own)
__global__ __launch_bounds__(256) void gml_k_head_bce_fold(const float* __restrict__ part, int nparts, int nin, int nh, int c0, int c1,
                                                           float* __restrict__ dw1, float* __restrict__ db1, float* __restrict__ dw2,
                                                           float* __restrict__ db2, float* __restrict__ loss, float* __restrict__ stats) {
    const int np = hbce_npart(nin, nh), nw = nh * nin;
    const int j = c0 + blockIdx.x * 256 + threadIdx.x;
    if (j >= c1) return;
    float a = 0.f;
    for (int w = 0; w < nparts; ++w) a += part[(int64_t)w * np + j];
    if (j < nw) dw1[j] = a;
    else if (j < nw + nh) { if (db1) db1[j - nw] = a; }
    else if (j < nw + 2 * nh) dw2[j - nw - nh] = a;
    else if (j == nw + 2 * nh) { if (db2) db2[0] = a; }
    else {
        const int k = j - (nw + 2 * nh + 1);                   // 0 loss, 1 ok, 2 n
        if (k == 0) loss[0] = a;
        if (stats) stats[k] += a;
    }
}

static int hbce_grid(int64_t rows) {
    const int64_t ns = gml_cdiv(rows, HBCE_ROWS);
    return (int)(ns < HBCE_MAX_GRID ? ns : HBCE_MAX_GRID);
}

static int hbce_check(const GmlHeadBceParams& q) {
    if (q.R <= 0 || q.Rl < 0 || q.Rl > q.R || q.nin <= 0 || q.nh <= 0 || q.ldp < q.nin) return GML_E_BADARG;
    if (q.nin > HBCE_MAX_W || q.nh > HBCE_MAX_W || (q.act != 0 && q.act != 1)) return GML_E_UNSUPPORTED;
    if (!q.p || (!q.y && q.Rl > 0) || !q.w1 || !q.w2) return GML_E_BADARG;
    return GML_OK;
}

// floats of workspace gml_head_bce_fwd / _bwd need: 0 for rows <= 256 (one workgroup, no workspace) and for shapes not served
extern "C" size_t gml_head_bce_workspace_floats(int64_t rows, int32_t nin, int32_t nh) {
    if (rows <= HBCE_ROWS || nin <= 0 || nh <= 0 || nin > HBCE_MAX_W || nh > HBCE_MAX_W) return 0;
    return (size_t)hbce_grid(rows) * hbce_npart(nin, nh);
}

static GmlHeadBceParams hbce_params(const float* p, int64_t ldp, const float* y, const float* valid, const float* w1, const float* b1,
                                    const float* w2, const float* b2, int64_t rows, int64_t rows_loss, int32_t nin, int32_t nh, int32_t act) {
    GmlHeadBceParams q = {};
    q.p = p; q.ldp = ldp; q.y = y; q.valid = valid; q.w1 = w1; q.b1 = b1; q.w2 = w2; q.b2 = b2;
    q.R = rows; q.Rl = rows_loss; q.nin = nin; q.nh = nh; q.act = act; q.nslabs = rows > 0 ? gml_cdiv(rows, HBCE_ROWS) : 0;
    return q;
}

extern "C" int gml_head_bce_fwd(const float* p, int64_t ldp, const float* y, const float* valid, const float* w1, const float* b1,
                                const float* w2, const float* b2, int64_t rows, int64_t rows_loss, int32_t nin, int32_t nh, int32_t act,
                                float* loss, float* pre, float* stats, void* ws, size_t ws_floats, gml_stream_t stream) {
    GmlHeadBceParams q = hbce_params(p, ldp, y, valid, w1, b1, w2, b2, rows, rows_loss, nin, nh, act);
    const int rc = hbce_check(q);
    if (rc != GML_OK) return rc;
    if (!loss) return GML_E_BADARG;
    q.loss = loss; q.pre = pre; q.stats = stats;
    const int grid = hbce_grid(rows);
    if (q.nslabs > 1) {
        if (!ws || ws_floats < (size_t)grid * hbce_npart(nin, nh)) return GML_E_WORKSPACE;
        q.part = (float*)ws;
    }
    const int slab_rows = (int)(rows < HBCE_ROWS ? rows : HBCE_ROWS);
    const size_t lds = sizeof(float) * hbce_lds_floats(nin, nh, slab_rows);
    GML_ALLOW_BIG_LDS(rca, (&gml_k_head_bce_fwd), 160 * 1024)
    if (rca != hipSuccess) return (int)rca;
    hipLaunchKernelGGL(gml_k_head_bce_fwd, dim3(grid), dim3(HBCE_ROWS), lds, (hipStream_t)stream, q, slab_rows);
    int st = gml_launch_status();
    if (st != GML_OK || !q.part) return st;
    const int np = hbce_npart(nin, nh);
    hipLaunchKernelGGL(gml_k_head_bce_fold, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)ws, grid, nin, nh, np - 3, np,
                       (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr, loss, stats);
    return gml_launch_status();
}

extern "C" int gml_head_bce_bwd(const float* p, int64_t ldp, const float* y, const float* valid, const float* w1, const float* b1,
                                const float* w2, const float* b2, int64_t rows, int64_t rows_loss, int32_t nin, int32_t nh, int32_t act,
                                const float* gscale, float* gp, int64_t ldgp, float* dw1, float* db1, float* dw2, float* db2,
                                void* ws, size_t ws_floats, gml_stream_t stream) {
    GmlHeadBceParams q = hbce_params(p, ldp, y, valid, w1, b1, w2, b2, rows, rows_loss, nin, nh, act);
    const int rc = hbce_check(q);
    if (rc != GML_OK) return rc;
    if (!gp || !dw1 || !dw2 || ldgp < nin) return GML_E_BADARG;
    q.gscale = gscale; q.gp = gp; q.ldgp = ldgp; q.dw1 = dw1; q.db1 = db1; q.dw2 = dw2; q.db2 = db2;
    const int grid = hbce_grid(rows);
    if (q.nslabs > 1) {
        if (!ws || ws_floats < (size_t)grid * hbce_npart(nin, nh)) return GML_E_WORKSPACE;
        q.part = (float*)ws;
    }
    const int slab_rows = (int)(rows < HBCE_ROWS ? rows : HBCE_ROWS);
    const size_t lds = sizeof(float) * hbce_lds_floats(nin, nh, slab_rows);
    GML_ALLOW_BIG_LDS(rca, (&gml_k_head_bce_bwd), 160 * 1024)
    if (rca != hipSuccess) return (int)rca;
    hipLaunchKernelGGL(gml_k_head_bce_bwd, dim3(grid), dim3(HBCE_ROWS), lds, (hipStream_t)stream, q, slab_rows);
    int st = gml_launch_status();
    if (st != GML_OK || !q.part) return st;
    const int np = hbce_npart(nin, nh);
    hipLaunchKernelGGL(gml_k_head_bce_fold, dim3((unsigned)gml_cdiv(np - 3, 256)), dim3(256), 0, (hipStream_t)stream, (const float*)ws, grid,
                       nin, nh, 0, np - 3, dw1, db1, dw2, db2, (float*)nullptr, (float*)nullptr);
    return gml_launch_status();
}
