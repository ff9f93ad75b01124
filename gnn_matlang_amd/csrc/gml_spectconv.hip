// Dispatch of the fused forward kernel families + the unfused SpMM / SDDMM kernels.
//
// Which kernel serves a conv forward is decided in plan_fwd / fwd_kernel below and nowhere else:
//   64-row family (gml_spectconv_impl.h): any shape, exact fp32 or bf16x3, 64-row records -- all that the 128-row kernels do not take.
//   fwd3 (gml_spectconv_fwd3_impl.h): S in {4, 8}, Fin, Fout <= 32, the ZINC-class default.  An LDS-DMA landing ring, hence its three
//       conditions: float4-addressable x rows, no accumulate mode, 32-bit byte offsets into x.  Has the ConCat / depthwise epilogues
//       and the fused Hadamard branch; groups beyond its staging gather from global memory.
//   fwd2 (gml_spectconv_fwd2_impl.h): S in {4, 8, 12}, Fin, Fout <= 32, register-staged.  S = 12 (counting.py) always; S in {4, 8} when
//       a call misses one of fwd3's conditions.  NOB = 0 is the stand-alone SpMM.
//   fwd4 (gml_spectconv_fwd4_impl.h): the ring kernel walking a group in edge chunks.  The only 128-row kernel for 6 supports and for
//       33 .. 48 input features (sr25.py, mutag.py); serves fwd3's shapes when the caller sets GML_FWD_CHUNKED.  fwd3's conditions, no
//       Hadamard branch, and a bound on the column window (gml_spectconv_fwd_stage_window): it has no global-gather road.
#include "gml_spectconv_impl.h"
#include "gml_spectconv_fwd2_impl.h"
#include "gml_spectconv_fwd3_impl.h"
#include "gml_spectconv_fwd4_impl.h"
#include "gml_spmm3_impl.h"

#define GML_DECL_FWD2(S, B) template <> int gml_launch_fwd2<S, B>(const GmlFwdParams&, dim3, hipStream_t, bool, bool);
#define GML_DECL_SPMM2(S) GML_DECL_FWD2(S, 0)
#define GML_DECL_FWD3(S, B) template <> int gml_launch_fwd3<S, B>(const GmlFwdParams&, dim3, hipStream_t, bool);
#define GML_DECL_FWD4(S, FB, B) template <> int gml_launch_fwd4<S, FB, B>(const GmlFwdParams&, dim3, hipStream_t);
#define GML_DECL_FAM(SC, FPL) template <> int gml_launch_fwd_family<SC, FPL>(const GmlFwdParams&, int, bool, bool, dim3, size_t, hipStream_t);
GML_FWD2_SHAPES(GML_DECL_FWD2)
GML_SPMM2_SHAPES(GML_DECL_SPMM2)
GML_FWD3_SHAPES(GML_DECL_FWD3)
GML_FWD4_SHAPES(GML_DECL_FWD4)
GML_FWD_FAMILY_SHAPES(GML_DECL_FAM)

#if defined(GML_FWD2_TIMING) || (GML_F4DBG & (8 | 64))
/* GmlFwdParams::prof of the measuring builds: 256 bytes of counters.  -DGML_FWD2_TIMING: [0,16) fwd2, [16,32) fwd3 phase cycles */
static unsigned long long* prof_buf() {
    static unsigned long long* b = [] { unsigned long long* q = nullptr; (void)hipMalloc(&q, 256); (void)hipMemset(q, 0, 256); return q; }();
    return b;
}
static int prof_read(unsigned long long* out, size_t bytes, int reset) {
    hipError_t e = hipMemcpy(out, prof_buf(), bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess && reset) e = hipMemset(prof_buf(), 0, bytes);
    return (int)e;
}
#ifdef GML_FWD2_TIMING
extern "C" int gml_debug_fwd2_prof(unsigned long long* out, int reset) { return prof_read(out, 256, reset); }
#else
extern "C" int gml_debug_f4_counts(unsigned long long* out, int reset) { return prof_read(out, 64, reset); }
#endif
#endif

enum FwdKernel { FWD_FAMILY64, FWD2, FWD3, FWD4, FWD_UNSUPPORTED };

/* the shape class of a conv forward: a function of (S, Fin, Fout, flags) alone */
struct FwdPlan {
    int rows;            /* group records the shape's kernels read: 128 (fwd2 / fwd3 / fwd4) or 64 (the 64-row family) */
    bool staged;         /* fwd2 is compiled for it; with S in {4, 8} (ring) fwd3 is too */
    bool ring;
    bool chunked_only;   /* 6 supports and / or 33 .. 48 input features: only fwd4 serves it on 128-row records */
    bool chunked;        /* fwd4 is asked for: chunked_only, or the caller set GML_FWD_CHUNKED */
    int fb, nob;         /* fwd4's feature blocks beyond 32 (0 / 1); 16-wide output blocks (1 / 2) */
};

static FwdPlan plan_fwd(int S, int Fin, int Fout, uint32_t flags) {
    FwdPlan pl = {};
    const bool bf = (flags & GML_F32_MFMA) == 0 && Fout <= 32;
    /* S % 4 == 0: fwd2's register-staged value rows are float4 (other S keep the 64-row kernel, which stages any S) */
    pl.staged = bf && (S == 4 || S == 8 || S == 12) && Fin <= 32;
    pl.ring = pl.staged && S != 12;
    pl.chunked_only = bf && ((S == 6 && Fin <= 48) || (S == 4 && Fin > 32 && Fin <= 48));
    pl.rows = (pl.staged || pl.chunked_only) ? 128 : 64;
    pl.chunked = pl.chunked_only || (pl.rows == 128 && (flags & GML_FWD_CHUNKED));
    pl.fb = Fin > 32 ? 1 : 0;
    pl.nob = Fout > 16 ? 2 : 1;
    return pl;
}

static bool x_float4(const float* x, int64_t ldx) { return (ldx % 4 == 0) && (((uintptr_t)x & 15) == 0); }

/* the kernel that serves ONE call on 128-row records: what only a launch knows added to the plan.  mix: the Hadamard branch rides
   along (gml_ml3_fwd); epilogue: gml_spectconv_fwd_epi (fwd3 has the only epilogues). */
static FwdKernel fwd_kernel(const FwdPlan& pl, int S, const float* x, int64_t ldx, int64_t num_rows, uint32_t flags, bool mix, bool epilogue) {
    if (pl.rows != 128) return FWD_FAMILY64;
    /* the ring kernels: LDS-DMA of float4-addressable x rows, no accumulate mode, 32-bit buffer offsets
       (value rows beyond 4 GB are handled inside the kernels: they read the edge count themselves) */
    const bool ring_ok = x_float4(x, ldx) && !(flags & GML_ACCUM) && (num_rows + 16) * ldx * 4 < (int64_t)INT32_MAX;
    if (pl.chunked && !epilogue) {
        bool have4 = false;
#define GML_FWD4_HAVE(SV, FBV, B) have4 = have4 || (S == SV && pl.fb == FBV);
        GML_FWD4_SHAPES(GML_FWD4_HAVE)
        if (have4 && ring_ok && !mix) return FWD4;
        if (pl.chunked_only) return FWD_UNSUPPORTED;         /* (unaligned x rows, accumulate mode: the caller takes the 64-row family) */
    }
    if (pl.ring && ring_ok) return FWD3;
    return (pl.staged && !epilogue) ? FWD2 : FWD_UNSUPPORTED;
}

extern "C" int32_t gml_spectconv_fwd_group_rows(int32_t S, int32_t Fin, int32_t Fout, uint32_t flags) { return plan_fwd(S, Fin, Fout, flags).rows; }

// edges of one 128-row group the ring kernel of this shape keeps in LDS at once (one work item); 0: the shape is on no ring kernel
extern "C" int32_t gml_spectconv_fwd_stage_edges(int32_t S, int32_t Fin, int32_t Fout, uint32_t flags) {
    const FwdPlan pl = plan_fwd(S, Fin, Fout, flags);
    /* one work item of the chunked ring kernel (its gathering form: the smaller one) */
#define GML_FWD4_ECAP(SV, FBV, B) if (pl.chunked_only && S == SV && pl.fb == FBV) return GmlFwd4Cfg<SV, FBV, true>::ECAP - 3;
    GML_FWD4_SHAPES(GML_FWD4_ECAP)
#define GML_FWD3_ECAP(SV, B) if (pl.ring && S == SV) return GmlFwd3Cfg<SV>::ECAP - 3;
    GML_FWD3_SHAPES(GML_FWD3_ECAP)
    return 0;
}

// widest column window (int 3 of a 128-row group record) the chunked ring kernel serves; 0 = no bound (fwd4 is not asked for).
// Non-zero without GML_FWD_CHUNKED exactly for the shapes only the chunked kernel serves (functional.fwd_groups relies on it).
extern "C" int32_t gml_spectconv_fwd_stage_window(int32_t S, int32_t Fin, int32_t Fout, uint32_t flags) {
    const FwdPlan pl = plan_fwd(S, Fin, Fout, flags);
    if (!pl.chunked) return 0;
    return pl.fb ? GmlFwd4Cfg<4, 1, false>::XCAP - 15 : GmlFwd4Cfg<4, 0, false>::XCAP - 7;
}

/* persistent workgroups, each a contiguous range of groups: at most `wgs` of them; returns the grid */
static int persistent_grid(int ngroups, int wgs, int32_t* groups_per_wg) {
    const int grid = ngroups < wgs ? ngroups : wgs;
    *groups_per_wg = (int)gml_cdiv(ngroups, grid);
    return (int)gml_cdiv(ngroups, *groups_per_wg);
}

/* the fields every forward launch fills the same way: graph, x, weights, output, shape, one pass over all supports */
static GmlFwdParams fwd_params(const int32_t* rowptr, const int32_t* col, const int32_t* ginfo, const int32_t* epos, const float* val,
                               const float* x, int64_t ldx, const float* w, int64_t w_ss, int64_t w_si, int64_t w_so, const float* bias,
                               float* out, int64_t ldo, int64_t num_rows, int32_t S, int32_t Fin, int32_t Fout, uint32_t flags) {
    GmlFwdParams p = {};
    p.rowptr = rowptr; p.col = col; p.ginfo = ginfo; p.epos = epos; p.val = val; p.x = x; p.ldx = ldx;
    p.w = w; p.w_ss = w_ss; p.w_si = w_si; p.w_so = w_so; p.bias = bias; p.out = out; p.ldo = ldo;
    p.nrows = num_rows; p.S = S; p.Fin = Fin; p.Fout = Fout; p.flags = flags; p.npass = 1; p.nchunks = 1; p.val_vec = 1;
    return p;
}

/* one launch of the 128-row kernel `k` (one 8-wave workgroup per CU) */
static int launch128(FwdKernel k, const FwdPlan& pl, GmlFwdParams& p, bool mix, hipStream_t st) {
    const int S = p.S;
    const bool xv = x_float4(p.x, p.ldx);
    p.ngroups = (int)gml_cdiv(p.nrows, 128);
    const dim3 grid(persistent_grid(p.ngroups, GML_NUM_CU, &p.groups_per_wg));
#define GML_FWD4_GO(SV, FBV, B) if (k == FWD4 && S == SV && pl.fb == FBV) return gml_launch_fwd4<SV, FBV, B>(p, grid, st);
    GML_FWD4_SHAPES(GML_FWD4_GO)
#define GML_FWD3_GO(SV, B) if (k == FWD3 && S == SV && pl.nob == B) return gml_launch_fwd3<SV, B>(p, grid, st, mix);
    GML_FWD3_SHAPES(GML_FWD3_GO)
#define GML_FWD2_GO(SV, B) if (k == FWD2 && S == SV && pl.nob == B) return gml_launch_fwd2<SV, B>(p, grid, st, xv, mix);
    GML_FWD2_SHAPES(GML_FWD2_GO)
    return GML_E_UNSUPPORTED;
}

// conv (+ optionally the Hadamard branch of the same rows, F2 > 0) on 128-row group records
static int launch_fwd2(const int32_t* rowptr, const int32_t* col, const int32_t* ginfo, const int32_t* epos, const float* val, const float* x,
                       int64_t ldx, const float* w, int64_t w_ss, int64_t w_si, int64_t w_so, const float* bias,
                       const float* w11, const float* b11, const float* w12, const float* b12, float* out, int64_t ldo,
                       int64_t num_rows, int32_t S, int32_t Fin, int32_t Fout, int32_t F2, uint32_t flags, hipStream_t st) {
    const FwdPlan pl = plan_fwd(S, Fin, Fout, flags);
    GmlFwdParams p = fwd_params(rowptr, col, ginfo, epos, val, x, ldx, w, w_ss, w_si, w_so, bias, out, ldo, num_rows, S, Fin, Fout, flags);
    p.w11 = w11; p.b11 = b11; p.w12 = w12; p.b12 = b12; p.F2 = F2; p.mix_col = Fout;
#if defined(GML_FWD2_TIMING) || (GML_F4DBG & (8 | 64))
    p.prof = prof_buf();
#endif
#if GML_F4DBG & 256
    { const char* e = getenv("GML_F4_HOUT"); p.hout = e ? (float*)(uintptr_t)strtoull(e, nullptr, 0) : nullptr; }
#endif
    return launch128(fwd_kernel(pl, S, x, ldx, num_rows, flags, F2 > 0, false), pl, p, F2 > 0, st);
}

// SpectConCatConv (epilogue 1) / depthwise SpectConv (2) forward on fwd3's epilogues (gml.h; GmlFwdParams::epl).  GML_E_UNSUPPORTED
// wherever fwd3 does not serve the call: the caller then uses the weight-transform mapping onto gml_spectconv_fwd.
extern "C" int gml_spectconv_fwd_epi(const int32_t* rowptr, const int32_t* col, const int32_t* ginfo128, const float* val,
                                     const float* x, int64_t ldx, const float* w, int64_t w_ss, int64_t w_si, int64_t w_so,
                                     const float* bias, float* out, int64_t ldo, int64_t num_rows, int32_t S, int32_t Fin,
                                     int32_t Fout, uint32_t flags, int32_t epilogue, const float* ds, int32_t self_term,
                                     gml_stream_t stream) {
    if (num_rows < 0 || S <= 0 || Fin <= 0 || Fout <= 0 || ldx < Fin) return GML_E_BADARG;
    if (epilogue != 1 && epilogue != 2) return GML_E_BADARG;
    if (epilogue == 2 && ds == nullptr) return GML_E_BADARG;
    if (ldo < (epilogue == 1 ? (int64_t)(S + (self_term ? 1 : 0)) * Fout : Fout)) return GML_E_BADARG;
    if (num_rows == 0) return GML_OK;
    if (!rowptr || !ginfo128 || !x || !w || !out) return GML_E_BADARG;
    const FwdPlan pl = plan_fwd(S, Fin, Fout, flags);
    if (fwd_kernel(pl, S, x, ldx, num_rows, flags, false, true) != FWD3 || (((uintptr_t)val & 15) != 0)) return GML_E_UNSUPPORTED;
    GmlFwdParams p = fwd_params(rowptr, col, ginfo128, nullptr, val, x, ldx, w, w_ss, w_si, w_so, bias, out, ldo, num_rows, S, Fin, Fout, flags);
    p.epl = epilogue; p.ds = ds; p.ds_self = self_term ? 1 : 0; p.cc_off = self_term ? 1 : 0;
    return launch128(FWD3, pl, p, false, (hipStream_t)stream);
}

static int launch_family(int SC, int FPL, const GmlFwdParams& p, int NB, bool xvec, bool bf, dim3 grid, size_t lds, hipStream_t st) {
#define GML_FAM(SCV, FPLV) if (SC == SCV && FPL == FPLV) return gml_launch_fwd_family<SCV, FPLV>(p, NB, xvec, bf, grid, lds, st);
    GML_FWD_FAMILY_SHAPES(GML_FAM)
    return GML_E_UNSUPPORTED;
}

static const int kSC8[] = {8, 6, 4, 3, 2, 1};
static const int kSC4[] = {16, 12, 8, 6, 4, 3, 2, 1};

extern "C" int gml_spectconv_fwd(const int32_t* rowptr, const int32_t* col, const int32_t* ginfo, const int32_t* epos,
                                 const float* val, const float* x, int64_t ldx,
                                 const float* w, int64_t w_ss, int64_t w_si, int64_t w_so,
                                 const float* bias, float* out, int64_t ldo,
                                 int64_t num_rows, int32_t S, int32_t Fin, int32_t Fout,
                                 uint32_t flags, gml_stream_t stream) {
    if (num_rows < 0 || S <= 0 || Fin <= 0 || Fout <= 0 || ldx < Fin || ldo < Fout) return GML_E_BADARG;
    if (num_rows == 0) return GML_OK;
    if (!rowptr || !ginfo || !x || !w || !out) return GML_E_BADARG;   /* col/val may be null when there are no edges */
    if (num_rows > (int64_t)INT32_MAX - 16) return GML_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;

    if (flags & GML_GROUPS128) {
        // the 128-row kernels: the caller passes 128-row group records (gml_spectconv_fwd_group_rows said 128)
        if (plan_fwd(S, Fin, Fout, flags).rows != 128 || (((uintptr_t)val & (S % 4 == 0 ? 15 : 7)) != 0)) return GML_E_BADARG;
        return launch_fwd2(rowptr, col, ginfo, epos, val, x, ldx, w, w_ss, w_si, w_so, bias, nullptr, nullptr, nullptr, nullptr,
                           out, ldo, num_rows, S, Fin, Fout, 0, flags, st);
    }

    // features per lane per chunk: 8 unless 4 pads the contraction less.  The bf16x3 projection needs 8, so outside the exact-fp32
    // mode the wider padding is taken beyond Fin = 32 (Fin = 48: sr25 / mutag forward -22 % / -15 %); Fin <= 16 keeps 4 per lane =
    // exact products (so few terms per output do not average the split's 2^-17: mutag GNNML1's gradients left the 1e-4 bar)
    const int pad8 = (Fin + 31) / 32 * 32, pad4 = (Fin + 15) / 16 * 16;
    const int FPL = (pad4 < pad8 && ((flags & GML_F32_MFMA) || Fin <= 32)) ? 4 : 8;
    const int CH = 4 * FPL;
    const int nchunks = (Fin + CH - 1) / CH;
    const bool xvec = (Fin % 4 == 0) && (ldx % 4 == 0) && (((uintptr_t)x & 15) == 0);
    const bool val_ok = (((uintptr_t)val & 15) == 0);
    if (!val_ok) return GML_E_BADARG;

    // support passes: one launch if S = npass * SC for a compiled SC, else a greedy split with accumulation
    const int* scs = (FPL == 8) ? kSC8 : kSC4;
    const int nscs = (FPL == 8) ? 6 : 8;
    struct Part { int s0, count, sc; } parts[32];
    int nparts = 0;
    for (int i = 0; i < nscs && nparts == 0; ++i)
        if (S % scs[i] == 0 && (scs[i] >= 4 || scs[i] == S)) { parts[0] = {0, S, scs[i]}; nparts = 1; }
    if (nparts == 0) {
        int s0 = 0;
        while (s0 < S) {
            int sc = 1;
            for (int i = 0; i < nscs; ++i) if (scs[i] <= S - s0) { sc = scs[i]; break; }
            if (nparts == 32) return GML_E_UNSUPPORTED;
            parts[nparts++] = {s0, sc, sc};
            s0 += sc;
        }
    }

    // persistent workgroups, each a contiguous range of 64-row groups; 2 resident per CU (LDS bound)
    const int ngroups = (int)gml_cdiv(num_rows, GML_GROUP);
    int32_t groups_per_wg;
    const int grid = persistent_grid(ngroups, GML_NUM_CU * 2, &groups_per_wg);

    for (int ip = 0; ip < nparts; ++ip) {
        const int SC = parts[ip].sc;
        const int colgrp = (SC * FPL > 32) ? 64 : 128;   // keep one W block <= 64 KiB of LDS
        for (int o0 = 0; o0 < Fout; o0 += colgrp) {
            const int fo = (Fout - o0 < colgrp) ? Fout - o0 : colgrp;
            const int nb16 = (fo + 15) / 16;
            const int NB = nb16 <= 1 ? 1 : (nb16 <= 2 ? 2 : (nb16 <= 4 ? 4 : 8));
            const bool last = (ip == nparts - 1), first = (ip == 0);
            GmlFwdParams p = fwd_params(rowptr, col, ginfo, epos, val, x, ldx, w + (int64_t)o0 * w_so, w_ss, w_si, w_so,
                                        (last && bias) ? bias + o0 : nullptr, out + o0, ldo, num_rows, S, Fin, fo, 0);
            p.s0 = parts[ip].s0; p.npass = parts[ip].count / SC; p.nchunks = nchunks;
            p.ngroups = ngroups; p.groups_per_wg = groups_per_wg;
            p.flags = (first ? (flags & GML_ACCUM) : GML_ACCUM) | (last ? (flags & GML_RELU) : 0u) | (flags & 0xff00u);
            const size_t wblk = (size_t)SC * FPL * NB * 64 * sizeof(float);
            const size_t all = wblk * p.npass * nchunks;
            const int ecap = SC == 6 ? 2 * GML_ECAP : GML_ECAP;                  /* = GmlStage<SC, FPL>::ECAP */
            const size_t stage = (size_t)(76 + ecap + ecap * SC + GML_XCAP * (4 * FPL + 4)) * sizeof(float);
            p.allw = all + stage <= 80 * 1024;           // two workgroups per CU
            const int va = (SC % 4 == 0) ? 4 : ((SC % 2 == 0) ? 2 : 1);
            p.val_vec = (S % va == 0) && (p.s0 % va == 0);
            p.wfloats = (int)((p.allw ? all : wblk) / sizeof(float));
            const size_t lds = (size_t)p.wfloats * sizeof(float) + stage;
            int rc = launch_family(SC, FPL, p, NB, xvec && FPL >= 4, (flags & GML_F32_MFMA) == 0, dim3(grid), lds, st);
            if (rc != GML_OK) return rc;
        }
    }
    return GML_OK;
}

// ML3Layer forward (libs/spect_conv.py:204-212) minus the edge branch: out[:, :nout1] = relu?(conv(x)) and
// out[:, nout1:nout1+F2] = tanh(fc11 x) * tanh(fc12 x); one launch on the 8-wave kernel when it applies (F2 <= 8).
extern "C" int gml_ml3_fwd(const int32_t* rowptr, const int32_t* col, const int32_t* ginfo, const int32_t* epos,
                           const float* val, const float* x, int64_t ldx, const float* w, int64_t w_ss, int64_t w_si, int64_t w_so,
                           const float* bias, const float* w11, const float* b11, const float* w12, const float* b12,
                           float* out, int64_t ldo, int64_t num_rows, int32_t S, int32_t Fin, int32_t nout1,
                           int32_t F2, uint32_t flags, gml_stream_t stream) {
    if (F2 < 0 || ldo < nout1 + F2 || (F2 > 0 && (!w11 || !w12))) return GML_E_BADARG;
    const FwdPlan pl = plan_fwd(S, Fin, nout1, flags);
    /* fused: fwd3 / fwd2 carry the Hadamard branch (the chunked kernel does not) */
    if (num_rows > 0 && F2 > 0 && F2 <= 8 && (flags & GML_GROUPS128) && pl.rows == 128 && !pl.chunked &&
        (((uintptr_t)val & 15) == 0) && !(flags & GML_ACCUM)) {
        if (!rowptr || !ginfo || !x || !w || !out) return GML_E_BADARG;
        return launch_fwd2(rowptr, col, ginfo, epos, val, x, ldx, w, w_ss, w_si, w_so, bias, w11, b11, w12, b12, out, ldo,
                           num_rows, S, Fin, nout1, F2, flags, (hipStream_t)stream);
    }
    int rc = gml_spectconv_fwd(rowptr, col, ginfo, epos, val, x, ldx, w, w_ss, w_si, w_so, bias, out, ldo, num_rows, S,
                               Fin, nout1, flags, stream);
    if (rc != GML_OK || F2 == 0) return rc;
    return gml_node_mix_fwd(x, ldx, w11, b11, w12, b12, out + nout1, ldo, num_rows, Fin, F2, stream);
}

// =============================================================================================
// Unfused SpMM: H[r, s, :] = sum_k val[pos(k), s] * x[col[k], :]   (materialises H; used for dW)
// GW lanes share one row (lane <-> feature, coalesced X rows), 64/GW rows per wave.
// =============================================================================================
template <int SC, int GW>
__global__ __launch_bounds__(256) void gml_k_spmm(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                 const int32_t* __restrict__ epos, const float* __restrict__ val,
                                                 const float* __restrict__ x, int64_t ldx, float* __restrict__ h,
                                                 int64_t nrows, int S, int s0, int Fin) {
    constexpr int RPW = 64 / GW;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t row = wave * RPW + lane / GW;
    const int lr = lane % GW;
    if (row >= nrows) return;
    const int kbeg = rowptr[row], kend = rowptr[row + 1];
    for (int f = lr; f < Fin; f += GW) {
        float acc[SC];
#pragma unroll
        for (int s = 0; s < SC; ++s) acc[s] = 0.f;
        for (int k = kbeg; k < kend; ++k) {
            const int64_t pk = epos ? (int64_t)epos[k] : (int64_t)k;
            const float xv = x[(int64_t)col[k] * ldx + f];
            const float* vr = val + pk * S + s0;
#pragma unroll
            for (int s = 0; s < SC; ++s) acc[s] = fmaf(vr[s], xv, acc[s]);
        }
#pragma unroll
        for (int s = 0; s < SC; ++s) h[(row * S + s0 + s) * Fin + f] = acc[s];
    }
}

template <int SC>
static int launch_spmm(const int32_t* rowptr, const int32_t* col, const int32_t* epos, const float* val,
                       const float* x, int64_t ldx, float* h, int64_t nrows, int S, int s0, int Fin, hipStream_t st) {
    const int GW = Fin <= 16 ? 16 : (Fin <= 32 ? 32 : 64);
    const int64_t waves = gml_cdiv(nrows, 64 / GW);
    const dim3 grid((unsigned)gml_cdiv(waves, 4));
    if (GW == 16) hipLaunchKernelGGL((gml_k_spmm<SC, 16>), grid, dim3(256), 0, st, rowptr, col, epos, val, x, ldx, h, nrows, S, s0, Fin);
    else if (GW == 32) hipLaunchKernelGGL((gml_k_spmm<SC, 32>), grid, dim3(256), 0, st, rowptr, col, epos, val, x, ldx, h, nrows, S, s0, Fin);
    else hipLaunchKernelGGL((gml_k_spmm<SC, 64>), grid, dim3(256), 0, st, rowptr, col, epos, val, x, ldx, h, nrows, S, s0, Fin);
    return gml_launch_status();
}

extern "C" int gml_spmm_fwd(const int32_t* rowptr, const int32_t* col, const int32_t* ginfo128, const int32_t* epos,
                            const float* val, const float* x, int64_t ldx, float* h, int64_t num_rows, int32_t S,
                            int32_t Fin, gml_stream_t stream) {
    return gml_spmm_fwd_ex(rowptr, col, ginfo128, epos, val, x, ldx, h, num_rows, S, Fin, -1, stream);
}

extern "C" int gml_spmm_fwd_ex(const int32_t* rowptr, const int32_t* col, const int32_t* ginfo128, const int32_t* epos,
                               const float* val, const float* x, int64_t ldx, float* h, int64_t num_rows, int32_t S,
                               int32_t Fin, int32_t max_group_edges, gml_stream_t stream) {
    if (num_rows < 0 || S <= 0 || Fin <= 0 || ldx < Fin) return GML_E_BADARG;
    if (num_rows == 0) return GML_OK;
    if (!rowptr || !x || !h) return GML_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    // ring kernel (gml_spmm3_impl.h): any S (chunks of 4, 2, 1 supports), any Fin (chunks of 32 features), degrees up to ~16 per
    // row on average staged in LDS.  Shapes of the conv's 128-row class (plan_fwd) keep fwd2's NOB = 0 form, or the loop below, while
    // every group fits fwd2's 1024-edge staging (ZINC: 0.65 vs 0.61 of the roof at 131,072 graphs) or the group sizes are unknown (< 0)
    const FwdPlan pl = plan_fwd(S, Fin, 16, 0);
    const bool rows128 = pl.rows == 128;
    const bool fwd2_fits = rows128 && (((uintptr_t)val & 15) == 0) && (max_group_edges < 0 || max_group_edges <= GML_FWD2_ECAP);
    if (!fwd2_fits && ginfo128 != nullptr && epos == nullptr && (ldx % 4 == 0) && (((uintptr_t)x & 15) == 0) && Fin % 4 == 0 &&
        (((uintptr_t)h & 15) == 0) && (((uintptr_t)val & 3) == 0) && (num_rows + 16) * ldx * 4 < (int64_t)INT32_MAX &&
        (int64_t)128 * S * Fin * 4 < (int64_t)INT32_MAX && (int64_t)S * 4 * 24 <= GmlSpmm3Cfg::VAL_BYTES) {
        GmlSpmm3Params q = {};
        q.rowptr = rowptr; q.col = col; q.ginfo = ginfo128; q.val = val; q.ldx = ldx; q.h = h; q.nrows = num_rows; q.S = S; q.hs = Fin;
        q.ngroups = (int)gml_cdiv(num_rows, 128);
        const int grid = persistent_grid(q.ngroups, GML_NUM_CU, &q.groups_per_wg);
        for (int f0 = 0; f0 < Fin;) {                           // feature chunks: separate launches, the value rows are read again
            const int left = Fin - f0;
            // a remainder of 36 .. 48 features is ONE launch of the 192-byte-row form (sr25 / mutag hidden width 48); else chunks of 32
            const bool w48 = left > 32 && left <= 48 && (int64_t)S * 4 * 24 <= GmlSpmm3CfgT<true>::VAL_BYTES;
            q.x = x + f0; q.Fin = w48 ? left : (left < 32 ? left : 32); q.hf0 = f0;
            int rc;
            if (w48) rc = (S % 4 == 0) ? gml_launch_spmm3<4, true>(q, dim3(grid), st)
                          : ((S % 2 == 0) ? gml_launch_spmm3<2, true>(q, dim3(grid), st) : gml_launch_spmm3<1, true>(q, dim3(grid), st));
            else rc = (S % 4 == 0) ? gml_launch_spmm3<4>(q, dim3(grid), st)
                      : ((S % 2 == 0) ? gml_launch_spmm3<2>(q, dim3(grid), st) : gml_launch_spmm3<1>(q, dim3(grid), st));
            if (rc != GML_OK) return rc;
            f0 += q.Fin;
        }
        return GML_OK;
    }
    if (ginfo128 != nullptr && epos == nullptr && pl.staged && (((uintptr_t)val & 15) == 0) && (((uintptr_t)h & 15) == 0)) {
        // the 8-wave kernel's staged, degree-ranked aggregation; H written straight from the accumulators.  pl.staged, not rows128:
        // a lane of fwd2 holds features 8 kq .. 8 kq + 7 < 32, so S = 4 with 33 .. 48 features (128-row class through fwd4 alone)
        // would leave H[:, :, 32:] unwritten on the S = 4 instantiation
        GmlFwdParams p = fwd_params(rowptr, col, ginfo128, nullptr, val, x, ldx, nullptr, 0, 0, 0, nullptr, nullptr, 0, num_rows, S, Fin, 16, 0);
        p.hout = h;
        p.ngroups = (int)gml_cdiv(num_rows, GML_FWD2_ROWS);
        const dim3 grid(persistent_grid(p.ngroups, GML_NUM_CU, &p.groups_per_wg));
#define GML_SPMM2_GO(SV) if (S == SV) return gml_launch_fwd2<SV, 0>(p, grid, st, x_float4(x, ldx), false);
        GML_SPMM2_SHAPES(GML_SPMM2_GO)
        /* (the shapes only the chunked conv kernel serves have no NOB = 0 instantiation: the loop below) */
    }
    int s0 = 0;
    while (s0 < S) {
        const int rem = S - s0;
        int rc;
        if (rem >= 8) { rc = launch_spmm<8>(rowptr, col, epos, val, x, ldx, h, num_rows, S, s0, Fin, st); s0 += 8; }
        else if (rem >= 4) { rc = launch_spmm<4>(rowptr, col, epos, val, x, ldx, h, num_rows, S, s0, Fin, st); s0 += 4; }
        else if (rem >= 2) { rc = launch_spmm<2>(rowptr, col, epos, val, x, ldx, h, num_rows, S, s0, Fin, st); s0 += 2; }
        else { rc = launch_spmm<1>(rowptr, col, epos, val, x, ldx, h, num_rows, S, s0, Fin, st); s0 += 1; }
        if (rc != GML_OK) return rc;
    }
    return GML_OK;
}

// =============================================================================================
// SDDMM: dval[pos(k), s] = < x[col[k], :], gw[r, s, :] >   (gradient of message() w.r.t. norm)
// GW lanes share one row; each lane keeps its slice of gw[r] in registers; width-GW shuffle tree.
// =============================================================================================
template <int SC, int GW, int NFC>
__global__ __launch_bounds__(256) void gml_k_sddmm(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                  const int32_t* __restrict__ epos, const float* __restrict__ x,
                                                  int64_t ldx, const float* __restrict__ gw, float* __restrict__ dval,
                                                  int64_t nrows, int S, int s0, int Fin) {
    constexpr int RPW = 64 / GW;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t row = wave * RPW + lane / GW;
    const int lr = lane % GW;
    const bool valid = row < nrows;
    const int kbeg = valid ? rowptr[row] : 0, kend = valid ? rowptr[row + 1] : 0;
    float g[SC][NFC];
#pragma unroll
    for (int s = 0; s < SC; ++s)
#pragma unroll
        for (int c = 0; c < NFC; ++c) {
            const int f = lr + c * GW;
            g[s][c] = (valid && f < Fin) ? gw[(row * S + s0 + s) * Fin + f] : 0.f;
        }
    // all lanes of a wave must run the same trip count for the shuffles
    int n = kend - kbeg;
#pragma unroll
    for (int off = 32; off >= GW; off >>= 1) n = max(n, __shfl_xor(n, off));
    for (int i = 0; i < n; ++i) {
        const int k = kbeg + i;
        const bool kv = k < kend;
        float part[SC];
#pragma unroll
        for (int s = 0; s < SC; ++s) part[s] = 0.f;
        if (kv) {
            const float* xr = x + (int64_t)col[k] * ldx;
#pragma unroll
            for (int c = 0; c < NFC; ++c) {
                const int f = lr + c * GW;
                const float xv = (f < Fin) ? xr[f] : 0.f;
#pragma unroll
                for (int s = 0; s < SC; ++s) part[s] = fmaf(xv, g[s][c], part[s]);
            }
        }
#pragma unroll
        for (int s = 0; s < SC; ++s)
#pragma unroll
            for (int off = GW / 2; off >= 1; off >>= 1) part[s] += __shfl_xor(part[s], off);
        if (kv && lr == 0) {
            const int64_t pk = epos ? (int64_t)epos[k] : (int64_t)k;
#pragma unroll
            for (int s = 0; s < SC; ++s) dval[pk * S + s0 + s] = part[s];
        }
    }
}

template <int SC>
static int launch_sddmm(const int32_t* rowptr, const int32_t* col, const int32_t* epos, const float* x, int64_t ldx,
                        const float* gw, float* dval, int64_t nrows, int S, int s0, int Fin, hipStream_t st) {
    const int GW = Fin <= 16 ? 16 : (Fin <= 32 ? 32 : 64);
    const int64_t waves = gml_cdiv(nrows, 64 / GW);
    const dim3 grid((unsigned)gml_cdiv(waves, 4));
#define GML_SDDMM(GWV, NFCV) \
    hipLaunchKernelGGL((gml_k_sddmm<SC, GWV, NFCV>), grid, dim3(256), 0, st, rowptr, col, epos, x, ldx, gw, dval, nrows, S, s0, Fin)
    if (GW == 16) GML_SDDMM(16, 1);
    else if (GW == 32) GML_SDDMM(32, 1);
    else if (Fin <= 64) GML_SDDMM(64, 1);
    else if (Fin <= 128) GML_SDDMM(64, 2);
    else if (Fin <= 256) GML_SDDMM(64, 4);
    else return GML_E_UNSUPPORTED;
    return gml_launch_status();
}

extern "C" int gml_sddmm(const int32_t* rowptr, const int32_t* col, const int32_t* epos, const float* x, int64_t ldx,
                         const float* gw, float* dval, int64_t num_rows, int32_t S, int32_t Fin, gml_stream_t stream) {
    if (num_rows < 0 || S <= 0 || Fin <= 0 || ldx < Fin) return GML_E_BADARG;
    if (num_rows == 0) return GML_OK;
    if (!rowptr || !x || !gw) return GML_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    int s0 = 0;
    while (s0 < S) {
        const int rem = S - s0;
        int rc;
        if (rem >= 8) { rc = launch_sddmm<8>(rowptr, col, epos, x, ldx, gw, dval, num_rows, S, s0, Fin, st); s0 += 8; }
        else if (rem >= 4) { rc = launch_sddmm<4>(rowptr, col, epos, x, ldx, gw, dval, num_rows, S, s0, Fin, st); s0 += 4; }
        else if (rem >= 2) { rc = launch_sddmm<2>(rowptr, col, epos, x, ldx, gw, dval, num_rows, S, s0, Fin, st); s0 += 2; }
        else { rc = launch_sddmm<1>(rowptr, col, epos, x, ldx, gw, dval, num_rows, S, s0, Fin, st); s0 += 1; }
        if (rc != GML_OK) return rc;
    }
    return GML_OK;
}
