// GNNML1 block for inputs wider than 64 features, and the tanh-factor form (mode 3) at any width -- the blocks after the first of
// Zinc12k.py / counting.py / freqclass.py / ptc.py / enzymes.py / proteins.py read a concatenation 48 / 96 / 96 / 98 / 48 / 144 wide.
//
// The SAME device code as gml_gnnml1.hip (gml_gnnml1_impl.h) at a wider per-lane slice: lane (r16, kq) owns FPL = 24 / 28 / 36
// features of its row (FP = 4 FPL = 96 / 112 / 144 >= Fin), so that every product stays ONE ascending-k fmaf chain per output and
// the aggregation stays in the CSR's edge order -- the results do not depend on which instantiation serves a width.  (Walking the
// input in 64-feature chunks of FPL = 16 gives the same chains; it would keep the x / aggregate registers at 48 but needs the
// aggregate of every chunk alive until the last chunk's products, i.e. the same 3 FPL registers, plus a chunk loop around the
// edge loop or a second pass over the edges.  Registers are not the limit here -- see DESIGN s4.14 -- so the plain form was kept.)
//
// LDS: forward image nblk FPL 64 floats, phase-2 image (FP / 16) nblk 4 64 floats, nblk = nb1 + nb2 + 2 nb3 <= 16: 147,456 bytes at
// FP = 144 with three 64-wide parts -- under the 160 KB of GML_ALLOW_BIG_LDS, which is why 144 is the widest input.
#define G1_M3 1
#define G1_NXB 9
#define G1_K(stem) gml_k_gnnml1w_##stem
#include "gml_gnnml1_impl.h"

static int g1w_fpl(int Fin) { return Fin <= 16 ? 4 : (Fin <= 64 ? 16 : (Fin <= 96 ? 24 : (Fin <= 112 ? 28 : 36))); }

// workgroups: one 16-row tile per wave and trip; two workgroups per CU while two LDS images fit into its 160 KB
static int64_t g1w_grid(int ntiles, size_t lds) {
    int64_t grid = gml_cdiv(ntiles, G1_NW);
    const int64_t cap = (lds > 80 * 1024 ? 1 : 2) * GML_NUM_CU;
    return grid > cap ? cap : grid;
}

template <int FPL>
static int g1w_fwd_t(const GmlG1Params& p, hipStream_t st) {
    const int nblk = (p.n1 + 15) / 16 + (p.n2 + 15) / 16 + 2 * ((p.n3 + 15) / 16);
    const size_t lds = (size_t)GmlG1Cfg<FPL>::fwd_floats(nblk) * 4;
    if (lds > 160 * 1024) return GML_E_UNSUPPORTED;
    G1_LAUNCH(gml_k_gnnml1w_fwd<FPL>, g1w_grid(p.ntiles, lds), lds, st, p)
    return gml_launch_status();
}

template <int FPL>
static int g1w_bwd_t(const GmlG1Params& p, hipStream_t st) {
    const int nb1 = (p.n1 + 15) / 16, nb2 = (p.n2 + 15) / 16, nb3 = (p.n3 + 15) / 16;
    const size_t lds1 = (size_t)GmlG1Cfg<FPL>::fwd_floats(2 * nb3) * 4;
    const size_t lds2 = p.dx ? (size_t)GmlG1Cfg<FPL>::tr_floats(nb1 + 2 * nb3 + nb2) * 4 : 0;
    if (lds1 > 160 * 1024 || lds2 > 160 * 1024) return GML_E_UNSUPPORTED;
    G1_LAUNCH((gml_k_gnnml1w_bwd<FPL, 1>), g1w_grid(p.ntiles, lds1), lds1, st, p)
    G1_LAUNCH((gml_k_gnnml1w_bwd<FPL, 2>), g1w_grid(p.ntiles, lds2), lds2, st, p)
    return gml_launch_status();
}

int gml_g1w_fwd(const GmlG1Params& p, hipStream_t st) {
    switch (g1w_fpl(p.Fin)) {
        case 4: return g1w_fwd_t<4>(p, st);
        case 16: return g1w_fwd_t<16>(p, st);
        case 24: return g1w_fwd_t<24>(p, st);
        case 28: return g1w_fwd_t<28>(p, st);
        default: return g1w_fwd_t<36>(p, st);
    }
}

int gml_g1w_bwd(const GmlG1Params& p, hipStream_t st) {
    switch (g1w_fpl(p.Fin)) {
        case 4: return g1w_bwd_t<4>(p, st);
        case 16: return g1w_bwd_t<16>(p, st);
        case 24: return g1w_bwd_t<24>(p, st);
        case 28: return g1w_bwd_t<28>(p, st);
        default: return g1w_bwd_t<36>(p, st);
    }
}

int gml_g1w_dw(const GmlG1DwParams& p, int grid, hipStream_t st) {
    hipLaunchKernelGGL(gml_k_gnnml1w_dw, dim3((unsigned)grid), dim3(64 * G1_NW), 0, st, p);
    return gml_launch_status();
}
