// GNNML1 block as the sum of three activated parts (block mode 5 of DESIGN s4.18) -- filtering.py:246-248, the script's concat = False:
//
//   a = fc_i1(x)   c = conv_i1(x) = (A^T x) Wc + bc   f2 = fc_i2(x)   f3 = fc_i3(x)
//   out [N, n] = act(a) + act(c) + act(f2 * f3)                n1 == n2 == n3 == n <= 64, Fin <= 144, act = relu
//
// The device code is gml_gnnml1_impl.h compiled a third time (G1_M5 = 1, kernels gml_k_gnnml1a_*): the one-image forward with mode 5's
// epilogue, the same exact fp32 products on v_mfma_f32_16x16x4_f32, VALU aggregation in the CSR's edge order, no atomics -- repeat runs
// are bitwise equal.  gml_gnnml1.hip and gml_gnnml1_wide.hip compile the header with G1_M5 = 0: their device code is what it was.
//
// The sum does not tell the relu patterns of a and c apart, so the forward RECORDS them in the layout of mode 4 (gml_gnnml1_sum.hip): one
// byte per 4 columns, bit u = a > 0, bit 4 + u = c > 0 of column 4 j + u; the lane (row, kq) that owns columns 16 nb + 4 kq .. + 3
// writes byte 4 nb + kq.  The sign of f2 f3 is not recorded: phase 1 of the backward recomputes f2 and f3 for df2 / df3 anyway.
// relu'(0) = 0.  Phase 1 writes g4 = [da | dc | df2 | df3] from gout, the byte and the recomputed factors; `out` is neither read nor
// saved.  That is the four-block layout of mode 1 with n1 = n2 = n3, and neither phase 2 (q = A dc, dx) nor the weight-gradient pass
// reads anything else of the forward, so both run as mode 1: phase 2 from this unit's instantiation, gml_gnnml1_dw(mode = 1) as it is.
//
// act = tanh needs the VALUES of a and c, not bits, and no script uses it in this form: it is GML_E_UNSUPPORTED here and the caller
// runs the composition.
#include "gml_gnnml1_rows.h"

struct GmlG1aParams : GmlG1Params {
    uint8_t* pat; int64_t ldp;                          // the relu patterns of a and c [N, ldp >= 4 ceil(n / 16)] (fwd: written, NULL: none)
};

#define G1_M5 1
#define G1_M3 0
#define G1_NXB 4
#define G1_P GmlG1aParams
#define G1_K(stem) gml_k_gnnml1a_##stem
#include "gml_gnnml1_impl.h"

static int g1a_fpl(int Fin) { return Fin <= 16 ? 4 : (Fin <= 64 ? 16 : (Fin <= 96 ? 24 : (Fin <= 112 ? 28 : 36))); }

// workgroups: one 16-row tile per wave and trip; two workgroups per CU while two LDS images fit into its 160 KB
static int64_t g1a_grid(int ntiles, size_t lds) {
    int64_t grid = gml_cdiv(ntiles, G1_NW);
    const int64_t cap = (lds > 80 * 1024 ? 1 : 2) * GML_NUM_CU;
    return grid > cap ? cap : grid;
}

template <int FPL>
static int g1a_fwd_t(const GmlG1aParams& p, hipStream_t st) {
    const size_t lds = (size_t)GmlG1Cfg<FPL>::fwd_floats(4 * ((p.n1 + 15) / 16)) * 4;
    if (lds > 160 * 1024) return GML_E_UNSUPPORTED;
    G1_LAUNCH(gml_k_gnnml1a_fwd<FPL>, g1a_grid(p.ntiles, lds), lds, st, p)
    return gml_launch_status();
}

template <int FPL>
static int g1a_bwd_t(const GmlG1aParams& p, hipStream_t st) {
    const int nb = (p.n1 + 15) / 16;
    const size_t lds1 = (size_t)GmlG1Cfg<FPL>::fwd_floats(2 * nb) * 4;
    const size_t lds2 = p.dx ? (size_t)GmlG1Cfg<FPL>::tr_floats(4 * nb) * 4 : 0;
    if (lds1 > 160 * 1024 || lds2 > 160 * 1024) return GML_E_UNSUPPORTED;
    G1_LAUNCH((gml_k_gnnml1a_bwd<FPL, 1>), g1a_grid(p.ntiles, lds1), lds1, st, p)
    GmlG1aParams p2 = p;
    p2.mode = 1;                                        // g4 is mode 1's [da | dc | df2 | df3]: q and dx as there
    G1_LAUNCH((gml_k_gnnml1a_bwd<FPL, 2>), g1a_grid(p.ntiles, lds2), lds2, st, p2)
    return gml_launch_status();
}

// 1 when gml_gnnml1_actsum_fwd / _bwd serve these widths and this activation (relu only: tanh needs the values of a and c)
extern "C" int gml_gnnml1_actsum_supported(int32_t Fin, int32_t n1, int32_t n2, int32_t n3, int32_t act) {
    return (Fin > 0 && n1 > 0 && n1 == n2 && n2 == n3 && Fin <= 144 && n1 <= 64 && act == 1) ? 1 : 0;
}

static int g1a_check(const GmlG1aParams& p) {
    if (p.nrows < 0 || p.Fin <= 0 || p.n1 <= 0 || p.n2 <= 0 || p.n3 <= 0 || p.n1 != p.n2 || p.n2 != p.n3 || p.act < 0 || p.act > 1) return GML_E_BADARG;
    if (!gml_gnnml1_actsum_supported(p.Fin, p.n1, p.n2, p.n3, p.act)) return GML_E_UNSUPPORTED;
    if (!p.rowptr || !p.col || !p.x || !p.w1 || !p.wc || !p.w2 || !p.w3 || p.ldx < p.Fin) return GML_E_BADARG;
    return GML_OK;
}

extern "C" int gml_gnnml1_actsum_fwd(const int32_t* rowptr, const int32_t* col, const float* val, const float* x, int64_t ldx, int64_t num_rows,
                                     int32_t Fin, const float* w1, const float* b1, int32_t n1, const float* wc, const float* bc, int32_t n2,
                                     const float* w2, const float* b2, const float* w3, const float* b3, int32_t n3, int32_t act,
                                     float* out, int64_t ldo, uint8_t* pattern, int64_t ldp, gml_stream_t stream) {
    GmlG1aParams p = {};
    p.pat = pattern; p.ldp = ldp;
    p.rowptr = rowptr; p.col = col; p.val = val; p.x = x; p.ldx = ldx; p.w1 = w1; p.b1 = b1; p.wc = wc; p.bc = bc; p.w2 = w2; p.b2 = b2;
    p.w3 = w3; p.b3 = b3; p.out = out; p.ldo = ldo; p.nrows = num_rows; p.Fin = Fin; p.n1 = n1; p.n2 = n2; p.n3 = n3; p.mode = 5; p.act = act;
    const int rc = g1a_check(p);
    if (rc != GML_OK) return rc;
    if (!out || ldo < n1 || (pattern && ldp < 4 * ((n1 + 15) / 16))) return GML_E_BADARG;
    if (num_rows == 0) return GML_OK;
    p.ntiles = (int)gml_cdiv(num_rows, 16);
    hipStream_t st = (hipStream_t)stream;
    switch (g1a_fpl(Fin)) {
        case 4: return g1a_fwd_t<4>(p, st);
        case 16: return g1a_fwd_t<16>(p, st);
        case 24: return g1a_fwd_t<24>(p, st);
        case 28: return g1a_fwd_t<28>(p, st);
        default: return g1a_fwd_t<36>(p, st);
    }
}

extern "C" int gml_gnnml1_actsum_bwd(const int32_t* rowptr_t, const int32_t* col_t, const float* val_t, const float* x, int64_t ldx,
                                     const float* gout, int64_t ldgo, int64_t num_rows, int32_t Fin, const float* w1, int32_t n1,
                                     const float* wc, int32_t n2, const float* w2, const float* b2, const float* w3, const float* b3,
                                     int32_t n3, int32_t act, const uint8_t* pattern, int64_t ldp, float* dx, int64_t lddx,
                                     float* g4, int64_t ldg4, float* q, int64_t ldq, gml_stream_t stream) {
    GmlG1aParams p = {};
    p.pat = const_cast<uint8_t*>(pattern); p.ldp = ldp;
    p.rowptr = rowptr_t; p.col = col_t; p.val = val_t; p.x = x; p.ldx = ldx; p.w1 = w1; p.wc = wc; p.w2 = w2; p.b2 = b2; p.w3 = w3; p.b3 = b3;
    p.gout = gout; p.ldgo = ldgo; p.dx = dx; p.lddx = lddx; p.g4 = g4; p.ldg4 = ldg4; p.q = q; p.ldq = ldq;
    p.nrows = num_rows; p.Fin = Fin; p.n1 = n1; p.n2 = n2; p.n3 = n3; p.mode = 5; p.act = act;
    const int rc = g1a_check(p);
    if (rc != GML_OK) return rc;
    const int nb = (n1 + 15) / 16;
    if (!pattern || ldp < 4 * nb || !gout || !g4 || !q || ldgo < n1 || (dx && lddx < Fin)) return GML_E_BADARG;
    if (ldg4 < 64 * nb || ldg4 % 4 != 0 || ldq < 16 * nb || ldq % 4 != 0) return GML_E_BADARG;   // (64 nb = gml_gnnml1_g4_cols(n, n, n, 1))
    if (num_rows == 0) return GML_OK;
    p.ntiles = (int)gml_cdiv(num_rows, 16);
    hipStream_t st = (hipStream_t)stream;
    switch (g1a_fpl(Fin)) {
        case 4: return g1a_bwd_t<4>(p, st);
        case 16: return g1a_bwd_t<16>(p, st);
        case 24: return g1a_bwd_t<24>(p, st);
        case 28: return g1a_bwd_t<28>(p, st);
        default: return g1a_bwd_t<36>(p, st);
    }
}
