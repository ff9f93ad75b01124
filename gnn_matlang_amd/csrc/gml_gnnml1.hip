// GNNML1 block: the C entry points, and the kernels of inputs up to 64 wide in modes 0 .. 2 (device code: gml_gnnml1_impl.h).
// Wider inputs and mode 3 are instantiated in gml_gnnml1_wide.hip, so that this file's device code stays what rounds 5-6 measured
// (tools/isa_same.py <commit> gml_gnnml1.hip).
#include "gml_gnnml1_impl.h"

// this file's instantiations; 0: the launch goes to gml_gnnml1_wide.hip (Fin > 64, or mode 3)
static int g1_fpl(int Fin, int mode) { return mode == 3 ? 0 : (Fin <= 16 ? 4 : (Fin <= 64 ? 16 : 0)); }

static int g1_check(const GmlG1Params& p) {
    if (p.nrows < 0 || p.Fin <= 0 || p.n1 <= 0 || p.n2 <= 0 || p.n3 <= 0 || p.mode < 0 || p.mode > 3 || p.act < 0 || p.act > 1) return GML_E_BADARG;
    if (p.Fin > 144 || p.n1 > 64 || p.n2 > 64 || p.n3 > 64) return GML_E_UNSUPPORTED;
    if (p.mode == 0 && (p.n1 != p.n2 || p.n1 != p.n3)) return GML_E_BADARG;
    if (!p.rowptr || !p.col || !p.x || !p.w1 || !p.wc || !p.w2 || !p.w3 || !p.out) return GML_E_BADARG;
    return GML_OK;
}

// 1 when gml_gnnml1_fwd / _bwd serve these widths: inputs up to 144 (the LDS limit at 64 | 64 | 64), parts up to 64, modes 0 .. 3
extern "C" int gml_gnnml1_supported(int32_t Fin, int32_t n1, int32_t n2, int32_t n3, int32_t mode) {
    if (Fin <= 0 || n1 <= 0 || n2 <= 0 || n3 <= 0 || Fin > 144 || n1 > 64 || n2 > 64 || n3 > 64 || mode < 0 || mode > 3) return 0;
    return (mode != 0 || (n1 == n2 && n1 == n3)) ? 1 : 0;
}

extern "C" int gml_gnnml1_fwd(const int32_t* rowptr, const int32_t* col, const float* val, const float* x, int64_t ldx, int64_t num_rows,
                              int32_t Fin, const float* w1, const float* b1, int32_t n1, const float* wc, const float* bc, int32_t n2,
                              const float* w2, const float* b2, const float* w3, const float* b3, int32_t n3, int32_t mode, int32_t act,
                              float* out, int64_t ldo, gml_stream_t stream) {
    GmlG1Params p = {};
    p.rowptr = rowptr; p.col = col; p.val = val; p.x = x; p.ldx = ldx; p.w1 = w1; p.b1 = b1; p.wc = wc; p.bc = bc; p.w2 = w2; p.b2 = b2;
    p.w3 = w3; p.b3 = b3; p.out = out; p.ldo = ldo; p.nrows = num_rows; p.Fin = Fin; p.n1 = n1; p.n2 = n2; p.n3 = n3; p.mode = mode; p.act = act;
    const int rc = g1_check(p);
    if (rc != GML_OK) return rc;
    if (ldx < Fin || ldo < (mode == 0 ? n1 : n1 + n2 + n3)) return GML_E_BADARG;
    if (num_rows == 0) return GML_OK;
    p.ntiles = (int)gml_cdiv(num_rows, 16);
    const int fpl = g1_fpl(Fin, mode);
    if (fpl == 0) return gml_g1w_fwd(p, (hipStream_t)stream);
    const int nblk = (n1 + 15) / 16 + (n2 + 15) / 16 + 2 * ((n3 + 15) / 16);
    hipStream_t st = (hipStream_t)stream;
    int64_t grid = gml_cdiv(p.ntiles, G1_NW);
    if (grid > 2 * GML_NUM_CU) grid = 2 * GML_NUM_CU;
    if (fpl == 4) {
        const size_t lds = (size_t)GmlG1Cfg<4>::fwd_floats(nblk) * 4;
        GML_ALLOW_BIG_LDS(rc4, (&gml_k_gnnml1_fwd<4>), 160 * 1024)
        if (rc4 != hipSuccess) return (int)rc4;
        hipLaunchKernelGGL((gml_k_gnnml1_fwd<4>), dim3((unsigned)grid), dim3(64 * G1_NW), lds, st, p);
    } else {
        const size_t lds = (size_t)GmlG1Cfg<16>::fwd_floats(nblk) * 4;
        GML_ALLOW_BIG_LDS(rc16, (&gml_k_gnnml1_fwd<16>), 160 * 1024)
        if (rc16 != hipSuccess) return (int)rc16;
        if (lds > 64 * 1024 && grid > GML_NUM_CU) grid = GML_NUM_CU;
        hipLaunchKernelGGL((gml_k_gnnml1_fwd<16>), dim3((unsigned)grid), dim3(64 * G1_NW), lds, st, p);
    }
    return gml_launch_status();
}

// columns of g4: gml_gnnml1_g4_cols(n1, n2, n3, mode); q: [N, 16 ceil(n2 / 16)]
extern "C" int gml_gnnml1_g4_cols(int32_t n1, int32_t n2, int32_t n3, int32_t mode) {
    return 16 * ((n1 + 15) / 16 + (mode == 0 ? 0 : (n2 + 15) / 16) + 2 * ((n3 + 15) / 16));
}

extern "C" int gml_gnnml1_bwd(const int32_t* rowptr_t, const int32_t* col_t, const float* val_t, const float* x, int64_t ldx,
                              const float* out, int64_t ldo, const float* gout, int64_t ldgo, int64_t num_rows, int32_t Fin,
                              const float* w1, int32_t n1, const float* wc, int32_t n2, const float* w2, const float* b2, const float* w3,
                              const float* b3, int32_t n3, int32_t mode, int32_t act, float* dx, int64_t lddx, float* g4, int64_t ldg4,
                              float* q, int64_t ldq, gml_stream_t stream) {
    GmlG1Params p = {};
    p.rowptr = rowptr_t; p.col = col_t; p.val = val_t; p.x = x; p.ldx = ldx; p.w1 = w1; p.wc = wc; p.w2 = w2; p.b2 = b2; p.w3 = w3; p.b3 = b3;
    p.out = const_cast<float*>(out); p.ldo = ldo; p.gout = gout; p.ldgo = ldgo; p.dx = dx; p.lddx = lddx; p.g4 = g4; p.ldg4 = ldg4; p.q = q; p.ldq = ldq;
    p.nrows = num_rows; p.Fin = Fin; p.n1 = n1; p.n2 = n2; p.n3 = n3; p.mode = mode; p.act = act;
    const int rc = g1_check(p);
    if (rc != GML_OK) return rc;
    const int C = mode == 0 ? n1 : n1 + n2 + n3;
    if (!gout || !g4 || !q || ldx < Fin || ldo < C || ldgo < C || (dx && lddx < Fin)) return GML_E_BADARG;
    if (ldg4 < gml_gnnml1_g4_cols(n1, n2, n3, mode) || ldg4 % 4 != 0 || ldq < 16 * ((n2 + 15) / 16) || ldq % 4 != 0) return GML_E_BADARG;
    if (num_rows == 0) return GML_OK;
    p.ntiles = (int)gml_cdiv(num_rows, 16);
    const int fpl = g1_fpl(Fin, mode);
    if (fpl == 0) return gml_g1w_bwd(p, (hipStream_t)stream);
    const int nb1 = (n1 + 15) / 16, nb2 = (n2 + 15) / 16, nb3 = (n3 + 15) / 16;
    hipStream_t st = (hipStream_t)stream;
    int64_t grid = gml_cdiv(p.ntiles, G1_NW);
    if (grid > 2 * GML_NUM_CU) grid = 2 * GML_NUM_CU;
    if (fpl == 4) {
        const size_t lds1 = (size_t)GmlG1Cfg<4>::fwd_floats(2 * nb3) * 4, lds2 = dx ? (size_t)GmlG1Cfg<4>::tr_floats(nb1 + 2 * nb3 + nb2) * 4 : 0;
        if (lds1 > 160 * 1024 || lds2 > 160 * 1024) return GML_E_UNSUPPORTED;
        GML_ALLOW_BIG_LDS(rc4a, (&gml_k_gnnml1_bwd<4, 1>), 160 * 1024)
        if (rc4a != hipSuccess) return (int)rc4a;
        GML_ALLOW_BIG_LDS(rc4, (&gml_k_gnnml1_bwd<4, 2>), 160 * 1024)
        if (rc4 != hipSuccess) return (int)rc4;
        hipLaunchKernelGGL((gml_k_gnnml1_bwd<4, 1>), dim3((unsigned)grid), dim3(64 * G1_NW), lds1, st, p);
        hipLaunchKernelGGL((gml_k_gnnml1_bwd<4, 2>), dim3((unsigned)grid), dim3(64 * G1_NW), lds2, st, p);
    } else {
        const size_t lds1 = (size_t)GmlG1Cfg<16>::fwd_floats(2 * nb3) * 4, lds2 = dx ? (size_t)GmlG1Cfg<16>::tr_floats(nb1 + 2 * nb3 + nb2) * 4 : 0;
        if (lds1 > 160 * 1024 || lds2 > 160 * 1024) return GML_E_UNSUPPORTED;
        GML_ALLOW_BIG_LDS(rc16a, (&gml_k_gnnml1_bwd<16, 1>), 160 * 1024)
        if (rc16a != hipSuccess) return (int)rc16a;
        GML_ALLOW_BIG_LDS(rc16, (&gml_k_gnnml1_bwd<16, 2>), 160 * 1024)
        if (rc16 != hipSuccess) return (int)rc16;
        hipLaunchKernelGGL((gml_k_gnnml1_bwd<16, 1>), dim3((unsigned)grid), dim3(64 * G1_NW), lds1, st, p);
        hipLaunchKernelGGL((gml_k_gnnml1_bwd<16, 2>), dim3((unsigned)grid), dim3(64 * G1_NW), lds2, st, p);
    }
    return gml_launch_status();
}

// floats of the flat result [dW1 (n1 x Fin) | dW2 (n3 x Fin) | dW3 (n3 x Fin) | dWc (Fin x n2) | column sums of g4 (gml_gnnml1_g4_cols)]
extern "C" int64_t gml_gnnml1_dw_floats(int32_t Fin, int32_t n1, int32_t n2, int32_t n3, int32_t mode) {
    return (int64_t)n1 * Fin + 2 * (int64_t)n3 * Fin + (int64_t)Fin * n2 + gml_gnnml1_g4_cols(n1, n2, n3, mode);
}

static int g1_dw_grid(int64_t n) {
    int64_t g = gml_cdiv(n, 128);
    if (g > 2 * GML_NUM_CU) g = 2 * GML_NUM_CU;
    return g < 1 ? 1 : (int)g;
}

extern "C" size_t gml_gnnml1_dw_workspace_bytes(int64_t num_rows, int32_t Fin, int32_t n1, int32_t n2, int32_t n3, int32_t mode) {
    return (size_t)g1_dw_grid(num_rows) * (size_t)gml_gnnml1_dw_floats(Fin, n1, n2, n3, mode) * sizeof(float);
}

extern "C" int gml_gnnml1_dw(const float* x, int64_t ldx, const float* g4, int64_t ldg4, const float* q, int64_t ldq, int64_t num_rows,
                             int32_t Fin, int32_t n1, int32_t n2, int32_t n3, int32_t mode, float* out_flat, void* ws, size_t ws_bytes,
                             gml_stream_t stream) {
    if (!gml_gnnml1_supported(Fin, n1, n2, n3, mode)) return GML_E_UNSUPPORTED;
    if (num_rows < 0 || !x || !g4 || !q || !out_flat || ldx < Fin || ldg4 < gml_gnnml1_g4_cols(n1, n2, n3, mode) || ldq < 16 * ((n2 + 15) / 16))
        return GML_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nflat = gml_gnnml1_dw_floats(Fin, n1, n2, n3, mode);
    if (num_rows == 0) { gml_zero_async(out_flat, sizeof(float) * nflat, st); return gml_launch_status(); }
    if (!ws || ws_bytes < gml_gnnml1_dw_workspace_bytes(num_rows, Fin, n1, n2, n3, mode)) return GML_E_WORKSPACE;
    GmlG1DwParams p;
    p.x = x; p.ldx = ldx; p.g4 = g4; p.ldg4 = ldg4; p.q = q; p.ldq = ldq; p.nrows = num_rows; p.Fin = Fin; p.n1 = n1; p.n2 = n2; p.n3 = n3;
    p.mode = mode; p.part = (float*)ws; p.nflat = nflat;
    const int grid = g1_dw_grid(num_rows);
    p.rows_per_wg = (int)((gml_cdiv(num_rows, grid) + 3) / 4 * 4);
    gml_zero_async(ws, (size_t)grid * nflat * sizeof(float), st);       // (elements outside the written blocks: the dc block has no weight)
    int rc;
    if (Fin > 64) rc = gml_g1w_dw(p, grid, st);                         // (more than 4 x blocks: the 9-block instantiation)
    else { hipLaunchKernelGGL(gml_k_gnnml1_dw, dim3((unsigned)grid), dim3(64 * G1_NW), 0, st, p); rc = gml_launch_status(); }
    if (rc != GML_OK) return rc;
    gml_fold_job job = {};
    job.partial = (const float*)ws; job.nparts = grid; job.n = nflat; job.dst[0] = out_flat; job.ndst[0] = nflat;
    return gml_fold_many(&job, 1, stream);
}
