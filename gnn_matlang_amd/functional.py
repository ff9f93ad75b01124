"""Autograd functions over the C ABI of libgml_hip.so.

Forward of one SpectConv (libs/spect_conv.py:64-96) is ONE fused launch (gml_spectconv_fwd / gml_ml3_fwd); backward is ONE
fused launch organised by source rows (gml_spectconv_bwd*: dX = sum_s A_s (G W_s^T), dval[e, s] = <X[src] W_s, G[dst]>,
dW_s = X^T (A_s G), no atomics) plus the one-pass output stage (gml_ml3_split_bwd*: relu mask, bias sums, Hadamard branch).
Only shapes outside every compiled kernel class take the unfused composition (_conv_backward: transposed forward + SpMM +
SDDMM + two GEMMs; GML_VERBOSE=1 shows which road a call took).
Every tensor handed to the library is fp32, contiguous and on the current CUDA(HIP) device; the
launches go to torch's current stream, so they order with the surrounding torch ops and are
captured by torch.cuda.graphs like any other kernel.
"""
import ctypes

import torch

from . import _lib
from .graph import _ptr, _stream, _require_cuda


# ---------------------------------------------------------------------------- live kernel timing
# bench.py sets PROFILE = {} for one profiled block: every tagged launch is then bracketed by two HIP
# events recorded on the stream the kernel runs on, with its algorithmic bytes / flops.
PROFILE = None

# Projection arithmetic of the fused kernels: default = bf16x3 split on the bf16 matrix cores (fp32-class,
# ~1e-6 of the output scale); F32_MFMA = True (or env GML_F32_MFMA=1) = f32-input MFMA, bit-identical to fmaf.
import os as _os
import collections as _collections
import weakref as _weakref
_linear = torch.nn.functional.linear
F32_MFMA = _os.environ.get('GML_F32_MFMA', '0') not in ('0', '')


import threading as _threading
_TLS = _threading.local()


# Diagnostic switches (tools/precision_diag.py): EXACT_ONLY = None or a set of kernel families ('edge', 'conv') -- exact products are then
# taken only by those families; FORCE_BWD_EXACT = None / True / False overrides the arithmetic a backward inherits from its forward.
EXACT_ONLY = None
FORCE_BWD_EXACT = None


def _bwd_exact(ctx):
    return ctx.exact if FORCE_BWD_EXACT is None else bool(FORCE_BWD_EXACT)


def exact_mode(family='conv'):
    """True when the launches of THIS thread run on exact f32 products: the process-wide default F32_MFMA (environment, tests,
    bench) or an exact_products() scope of this thread.  The scope is thread-local: autograd runs a layer's backward on its own
    worker thread, and a scope entered there (ctx.exact) must not flip the arithmetic of a forward another thread is in the
    middle of."""
    on = bool(F32_MFMA) or getattr(_TLS, 'exact', 0) > 0
    return on and (EXACT_ONLY is None or family in EXACT_ONLY)


class exact_products(object):
    """``with exact_products():`` -- the launches of this thread inside the scope run on exact f32 products (a layer whose gradients
    a BatchNorm backward amplifies: models.GNNML3(bn=True) runs its FIRST layer so; the layer's backward re-enters the scope through
    ctx.exact).  Nestable; per thread."""

    def __init__(self, on=True):
        self.on = bool(on)

    def __enter__(self):
        if self.on:
            _TLS.exact = getattr(_TLS, 'exact', 0) + 1

    def __exit__(self, *a):
        if self.on:
            _TLS.exact -= 1


_FOLDS = None                      # the open deferred_folds scope's job list (process-wide: autograd runs backward on its own threads)
_FOLDS_LOCK = _threading.Lock()


class deferred_folds(object):
    """``with deferred_folds(model.parameters()): loss.backward()`` -- every weight-gradient kernel launched inside leaves its
    per-workgroup partial sums unfolded (include/gml.h "Deferred folds") and ONE launch folds them all when the scope closes
    (bit-identical sums: the same order).  For the reference's batch size, where a step is a chain of tiny launches (twelve folds at
    ZINC's four layers).  The gradient tensors autograd hands to the parameters are FILLED AT SCOPE EXIT: read .grad (optimizer,
    all-reduce) after the ``with`` block, never inside it.

    REQUIREMENT: every parameter's ``.grad`` is None when the backward runs (``zero_grad(set_to_none=True)``), so that autograd ADOPTS
    the not-yet-filled tensor as ``.grad``.  With an existing ``.grad`` (``zero_grad(set_to_none=False)``, micro-batch accumulation)
    AccumulateGrad would add the unfilled memory into it inside the scope and the fold would never reach it.  Pass the
    parameters the backward reaches: if any of them already holds a gradient the scope is INERT -- the folds run undeferred, launch by
    launch, and accumulation behaves as without the scope.  ``deferred_folds(None)`` = the caller vouches for the requirement.
    The scope is process-wide (the backward runs on autograd's worker threads, not on the thread that opened it): one at a time, one
    device, not nestable."""

    def __init__(self, params):
        self.active = params is None or all(p.grad is None for p in params)

    def __enter__(self):
        global _FOLDS
        if not self.active:
            return self
        with _FOLDS_LOCK:
            assert _FOLDS is None, 'deferred_folds scopes do not nest / overlap'
            _FOLDS = []
        return self

    def __exit__(self, exc_type, *a):
        global _FOLDS
        if not self.active:
            return
        with _FOLDS_LOCK:
            jobs, _FOLDS = _FOLDS, None
        if exc_type is None:
            flush_folds(jobs)


class _FoldQueue(object):
    def __init__(self, jobs):
        self.jobs = jobs

    def append(self, job):
        with _FOLDS_LOCK:
            self.jobs.append(job)


def _fold_queue():
    jobs = _FOLDS
    return _FoldQueue(jobs) if jobs is not None else None


def flush_folds(jobs):
    """jobs: [(partial tensor, nparts, n, [(dst tensor or None, count), ...])] -> gml_fold_many in chunks of 16"""
    if not jobs:
        return
    dev = jobs[0][0].device
    with torch.cuda.device(dev):
        for c0 in range(0, len(jobs), _lib.GML_FOLD_MAX_JOBS):
            chunk = jobs[c0:c0 + _lib.GML_FOLD_MAX_JOBS]
            arr = (_lib.FoldJob * len(chunk))()
            for a, (part, nparts, n, dsts) in zip(arr, chunk):
                a.partial, a.nparts, a.n = part.data_ptr(), int(nparts), int(n)
                for k in range(5):
                    t, c = dsts[k] if k < len(dsts) else (None, 0)
                    a.dst[k] = t.data_ptr() if t is not None else None
                    a.ndst[k] = int(c)
            with _Timed('fold'):
                _lib.call('gml_fold_many', ctypes.addressof(arr), len(chunk), _stream(dev))


EDGE_VALU = None               # GML_EDGE_VALU=1 as the LIBRARY read it (it decides: csrc/gml_edge_plan.h); filled by _edge_arith


# GML_VERBOSE=1: count which kernel family every layer call takes (shapes off the compiled set degrade in SPEED, never in
# results -- this is how a caller sees it).  PATHS maps e.g. 'conv_bwd: fused bf16x3 (S=8 Fin=32 Fout=30)' -> calls;
# printed at exit, read by tools/bench_configs.py to assert "no unfused fallback on any BASELINE config".
VERBOSE = _os.environ.get('GML_VERBOSE', '0') not in ('0', '')
PATHS = {}


def _path(kind, what, S=None, Fin=None, Fout=None):
    if VERBOSE:
        key = '%s: %s' % (kind, what) + ((' (S=%s Fin=%s Fout=%s)' % (S, Fin, Fout)) if S is not None else '')
        PATHS[key] = PATHS.get(key, 0) + 1


if VERBOSE:
    import atexit as _atexit
    import sys as _sys
    _atexit.register(lambda: [print('[gml path] %5d x %s' % (n, k), file=_sys.stderr) for k, n in sorted(PATHS.items())])


class _Timed(object):
    """q: algorithmic bytes of the launch as this design runs it; q2 (default q): the COMPULSORY bytes -- without arrays the design
    writes for itself (the dense block's Hcat): what an honest roofline is priced against."""
    __slots__ = ('tag', 'q', 'f', 'q2', 'e0')

    def __init__(self, tag, q=0, f=0, q2=None):
        self.tag, self.q, self.f, self.q2 = tag, q, f, (q if q2 is None else q2)

    def __enter__(self):
        if PROFILE is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *a):
        if PROFILE is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            PROFILE.setdefault(self.tag, []).append((self.e0, e1, self.q, self.f, self.q2))


def profile_summary(prof):
    """tag -> dict(launches, ms (mean per launch), bytes, flops, bytes_compulsory (means per launch))."""
    out = {}
    for tag, recs in prof.items():
        ms = [r[0].elapsed_time(r[1]) for r in recs]
        out[tag] = dict(launches=len(recs), ms=sum(ms) / len(ms), bytes=sum(r[2] for r in recs) / len(recs),
                        flops=sum(r[3] for r in recs) / len(recs), bytes_compulsory=sum(r[4] for r in recs) / len(recs))
    return out


def conv_cost(N, E, S, Fin, Fout):
    """fusion-agnostic compulsory traffic / flops of one SpectConv forward, fp32:
       Q = 4 (E S + N Fin + N Fout + S Fin Fout + Fout) + 4 (E + N + 1);  F = 2 E S Fin + 2 N S Fin Fout."""
    q = 4 * (E * S + N * Fin + N * Fout + S * Fin * Fout + Fout) + 4 * (E + N + 1)
    f = 2 * E * S * Fin + 2 * N * S * Fin * Fout
    return q, f


def conv_cost_bwd(N, E, S, Fin, Fout, need_x=True, need_val=True):
    """compulsory traffic / flops of one SpectConv backward incl. d/dval:
       Q = 4 (2 E S + 2 N Fin + N Fout + 2 S Fin Fout + Fout) + 4 (E + N + 1);  F = 6 E S Fin + 4 N S Fin Fout.
    A launch that produces no dX (the first layer: its input is data) is charged one N Fin (x is still read for dW and
    dval), one that produces no dval one E S: the bytes it actually has to move."""
    q = 4 * ((2 if need_val else 1) * E * S + (2 if need_x else 1) * N * Fin + N * Fout + 2 * S * Fin * Fout + Fout) + 4 * (E + N + 1)
    f = (6 if need_val else 4) * E * S * Fin + (4 if need_x else 2) * N * S * Fin * Fout
    return q, f


def _off(t, elems):
    return ctypes.c_void_p(t.data_ptr() + 4 * int(elems))


def _f32c(t, name):
    _require_cuda(t, name)
    if t.dtype != torch.float32:
        raise TypeError('%s must be float32, got %s' % (name, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


def _f32rows(t, name):
    """x as the kernels take it: float32 rows with unit column stride -- a row-strided view (a data set that hands out
    float4-addressable rows: dataset.DeviceDataset.batch_assembled) passes as it is, like the padded copy rows4 makes"""
    _require_cuda(t, name)
    if t.dtype != torch.float32:
        raise TypeError('%s must be float32, got %s' % (name, t.dtype))
    return t if (t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.size(1)) else t.contiguous()


# rows of x as the 8-wave kernels want them: float4-addressable (leading dimension a multiple of 4 floats, 16-byte aligned
# base), which is what the LDS-DMA landing ring of the forward (csrc/gml_spectconv_fwd3_impl.h) and the vector paths of the
# backward kernels copy.  Zinc12k.py's 21 + 4 = 25 input features (libs/utils.py:253-259) are not: the first layer's input is
# copied once into a zero-padded [N, 28] buffer; for a tensor that carries no gradient (per-batch data) the copy is kept per
# tensor object, so a batch that is stepped on repeatedly, or a data set that hands out padded rows itself, pays it once.
_ROWS4_CACHE = _collections.OrderedDict()


def rows4(x):
    if x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0:
        return x
    # While a HIP graph is being captured the copy must be RECORDED: a cache hit would leave it out of the graph, and every
    # replay after `static_x.copy_(new)` would read the padded copy of the warm-up data; the cached buffer could
    # also be evicted and freed while the graph still holds its address.  So: no lookup, no insert under capture.
    capturing = x.is_cuda and torch.cuda.is_current_stream_capturing()
    key = id(x)
    ent = None if capturing else _ROWS4_CACHE.get(key)
    if ent is not None and ent[0]() is x and ent[1] == x._version:
        _ROWS4_CACHE.move_to_end(key)
        return ent[2]
    F = int(x.size(1))
    buf = torch.zeros(x.size(0), (F + 3) // 4 * 4, dtype=x.dtype, device=x.device)
    buf[:, :F] = x
    v = buf[:, :F]
    if not x.requires_grad and not capturing:
        _ROWS4_CACHE[key] = (_weakref.ref(x), x._version, v)
        while len(_ROWS4_CACHE) > 4:
            _ROWS4_CACHE.popitem(last=False)
    return v


# The FORWARD projection of the 8-wave kernels (fwd3: every ML3Layer of the ZINC config; fwd2: counting.py's 12 supports; fwd4: sr25's / mutag's
# 48-wide layers) on f16 (hi, lo) pieces under power-of-two scales
# (GML_F16X3, csrc/gml_common.h "f16x3": residual 2^-24 per operand instead of 2^-17, same matrix-pipe instruction count) -- the
# default since round 6; GML_FWD_F16=0 restores the bf16 pairs.  With the three-piece edge forward (EDGE_FWD6) this makes the whole
# forward pass fp32-class, which is what trained-state gradients need (profiles/r06_precision_diag.jsonl); the backward kernels
# keep bf16x3 (measured not to matter).
FWD_F16 = _os.environ.get('GML_FWD_F16', '1') not in ('0', '')


def _fwd_arith_flags():
    return _lib.GML_F32_MFMA if exact_mode() else (_lib.GML_F16X3 if FWD_F16 else 0)


# ---------------------------------------------------------------------------- raw launches
def fused_conv(rowptr, col, ginfo, epos, val, x, ldx, w, w_strides, bias, out, ldo, nrows, S, Fin, Fout, flags=0,
               out_off=0, tag='spectconv_fwd'):
    q, f = conv_cost(int(nrows), int(val.size(0)), int(S), int(Fin), int(Fout)) if PROFILE is not None else (0, 0)
    with _Timed(tag, q + (4 * int(val.size(0)) if epos is not None else 0), f):
        _fused_conv(rowptr, col, ginfo, epos, val, x, ldx, w, w_strides, bias, out, ldo, nrows, S, Fin, Fout, flags,
                    out_off)


def _fused_conv(rowptr, col, ginfo, epos, val, x, ldx, w, w_strides, bias, out, ldo, nrows, S, Fin, Fout, flags,
                out_off):
    _lib.call('gml_spectconv_fwd', _ptr(rowptr), _ptr(col), _ptr(ginfo), _ptr(epos), _ptr(val), _ptr(x), int(ldx),
              _ptr(w), int(w_strides[0]), int(w_strides[1]), int(w_strides[2]), _ptr(bias),
              _off(out, out_off), int(ldo), int(nrows), int(S), int(Fin), int(Fout),
              int(flags) | _fwd_arith_flags(), _stream(x.device))


def conv_epilogue_applies(S, Fin, Fout):
    """shape class of gml_spectconv_fwd_epi (the ring kernel's ConCat / depthwise epilogues)"""
    return (not exact_mode()) and S in (4, 8) and Fin <= 32 and Fout <= 32


def conv_epilogue(csr, x, val, w, bias, S, epilogue, ds, self_term, ncols):
    """one launch of gml_spectconv_fwd_epi: epilogue 1 = ConCat column blocks, 2 = depthwise; returns out [N, ncols] or None when
    the library reports the shape unsupported.  x: float4-addressable rows (rows4), val: target-sorted supports [E, S]."""
    Fin, Fout = int(w.size(-2)), int(w.size(-1))
    N = csr.N
    out = torch.empty(N, int(ncols), dtype=torch.float32, device=x.device)
    w = w.contiguous()
    b = _f32c(bias.detach(), 'bias') if bias is not None else None
    rc = _lib.lib().gml_spectconv_fwd_epi(_ptr(csr.rowptr), _ptr(csr.col), _ptr(csr.ginfo128), _ptr(val), _ptr(x), int(x.stride(0)),
                                          _ptr(w), Fin * Fout, Fout, 1, _ptr(b), _ptr(out), int(ncols), N, int(S), Fin, Fout, 0,
                                          int(epilogue), _ptr(ds), 1 if self_term else 0, _stream(x.device))
    if rc == _lib.GML_E_UNSUPPORTED:
        return None
    _lib.check(rc)
    _path('conv_fwd', 'ring kernel, %s epilogue' % ('ConCat' if epilogue == 1 else 'depthwise'), S, Fin, Fout)
    return out


# Groups with more edges than one work item of the ring kernels stage at once (sr25.py: 13 entries per row) are walked in edge chunks
# on gml_k_spectconv_fwd4 (2-3 x the 64-row family's speed).  Opt-in through most of round 4 -- the chunked road differed from itself in
# ~1 launch of 200 in fresh processes -- until the cause was found (one v_pk_fma_f32 operand form, csrc/gml_spectconv_fwd4_impl.h `fma`,
# DESIGN s4.1c): 0 of 1536 since.  GML_FWD_CHUNKS=0 keeps such batches on the 64-row family.
FWD_CHUNKS = _os.environ.get('GML_FWD_CHUNKS', '1') not in ('0', '')


# How one conv forward runs (decided once, by _conv_fwd_road): rows = the group records it walks (128: the 8-wave kernels, 64: the 4-wave
# family), flags = what the launch adds to the caller's, label = its GML_VERBOSE text; gathers = the SHAPE is one of the 8-wave kernel's
# (whatever this batch then runs on): a training ML3Layer then keeps its edge branch in source order and the conv gathers the rows
ConvFwdRoad = _collections.namedtuple('ConvFwdRoad', 'rows flags label gathers')


def _conv_fwd_road(S, Fin, Fout, exact, gmax, N, stride, ptr16, chunks):
    """ConvFwdRoad from plain values only (no tensor, no launch)"""
    # gmax: (edges, column window) of the largest 128-row group of the target view, None when unknown; N, stride, ptr16: rows of x, their
    # stride in floats, x's address % 16; chunks: the FWD_CHUNKS switch
    flags = _lib.GML_F32_MFMA if exact else 0
    L = _lib.lib()
    shape = (int(S), int(Fin), int(Fout))
    rows = int(L.gml_spectconv_fwd_group_rows(*shape, flags))
    road = lambda rows_, fl, label: ConvFwdRoad(rows_, fl, label, rows == 128)
    if rows == 128:
        # a window bound without GML_FWD_CHUNKED: only the chunked ring kernel (fwd4) serves the shape on 128-row records
        win4 = int(L.gml_spectconv_fwd_stage_window(*shape, flags))
        cap = int(L.gml_spectconv_fwd_stage_edges(*shape, flags))      # edges of one work item of the ring kernel
        gm_e, gm_w = gmax if gmax is not None else (0, 0)
        # the chunked ring kernel (fwd4) addresses x with 32-bit byte offsets, reads float4 rows and needs the real group maxima to check
        # its window: without any of them, the 64-row family (any size, global gathers where a group does not fit) -- ADVICE r04
        ring_ok = stride % 4 == 0 and ptr16 == 0 and (int(N) + 16) * int(stride) * 4 < 2 ** 31
        if win4 and (not (gmax is not None and ring_ok) or gm_w > win4 or (gm_e > cap and not chunks)):
            pass                                  # fwd4 alone serves the shape and cannot serve this batch: the 64-row family
        elif win4 and gm_e > cap:
            # 48 features: one staged X window instead of two -> twice the edges per chunk (sr25: 2 chunks per group instead of 4)
            onewin = _lib.GML_FWD_ONEWIN if Fin > 32 else 0
            return road(128, _lib.GML_GROUPS128 | onewin, 'fused 8-wave bf16x3, edge chunks%s' % (', one X window' if onewin else ''))
        elif (not win4 and cap > 0 and gm_e > cap and chunks and ring_ok
              and gm_w <= int(L.gml_spectconv_fwd_stage_window(*shape, flags | _lib.GML_FWD_CHUNKED))):
            # a group beyond what the default ring kernel stages at once: its chunked form instead of global gathers
            return road(128, _lib.GML_GROUPS128 | _lib.GML_FWD_CHUNKED, 'fused 8-wave bf16x3, edge chunks')
        else:
            return road(128, _lib.GML_GROUPS128, 'fused 8-wave bf16x3')
    return road(64, 0, 'fused 4-wave (%s)' % ('f32 MFMA' if (exact or Fin <= 16 or Fout > 32) else 'bf16x3'))


# (group records, extra flags) of a ConvFwdRoad; records its GML_VERBOSE label
def _conv_fwd_records(csr, road, S, Fin, Fout):
    _path('conv_fwd', road.label, S, Fin, Fout)
    return (csr.ginfo128 if road.rows == 128 else csr.ginfo), road.flags


def fwd_groups(csr, x, S, Fin, Fout):
    """(group records, extra flags) the forward kernel wants for this shape and this x (the tensor properties _conv_fwd_road decides on)"""
    return _conv_fwd_records(csr, _conv_fwd_road(S, Fin, Fout, bool(exact_mode()), getattr(csr, 'gmax128', None), csr.N, int(x.stride(0)),
                                                 x.data_ptr() % 16, FWD_CHUNKS), S, Fin, Fout)


def fwd_gathers(S, Fin, Fout):
    """True when the forward of this shape runs on the 8-wave kernel, which can take its value rows through a position map."""
    return _conv_fwd_road(S, Fin, Fout, bool(exact_mode()), None, 0, 4, 0, FWD_CHUNKS).gathers


def ml3_edge_in_source_order(csr, S, Fin, Fout):
    """True when a training ML3Layer of this shape runs its edge branch in source order (fused backward + gathering forward)."""
    return fused_bwd_available(csr, S, Fin, Fout) and fwd_gathers(S, Fin, Fout)


def spmm(csr, val, x, S, Fin):
    h = torch.empty(csr.N, S * Fin, dtype=torch.float32, device=x.device)
    # hint for the kernel choice: the largest 128-row group (of the source view -- SpectralDesign's masks are symmetric, so of
    # this view too; only the choice depends on it)
    gm = csr.gmax_t128[0] if getattr(csr, 'gmax_t128', None) is not None else -1
    _lib.call('gml_spmm_fwd_ex', _ptr(csr.rowptr), _ptr(csr.col), _ptr(csr.ginfo128), _ptr(None), _ptr(val), _ptr(x), int(x.stride(0)),
              _ptr(h), csr.N, int(S), int(Fin), int(gm), _stream(x.device))
    return h


def sddmm(csr, x, gw, S, Fin):
    dval = torch.empty(csr.E, S, dtype=torch.float32, device=x.device)
    _lib.call('gml_sddmm', _ptr(csr.rowptr), _ptr(csr.col), _ptr(None), _ptr(x), int(x.stride(0)), _ptr(gw),
              _ptr(dval), csr.N, int(S), int(Fin), _stream(x.device))
    return dval


def relu_bwd(gy, gy_off, ldgy, y, ldy, nrows, F):
    """[nrows, F] view of a buffer whose rows are zero-padded to a multiple of 4 floats (float4-readable)."""
    ld = (F + 3) // 4 * 4
    g = torch.empty(nrows, ld, dtype=torch.float32, device=gy.device)
    _lib.call('gml_relu_bwd', _off(gy, gy_off), int(ldgy), _ptr(y), int(ldy), _ptr(g), ld, int(nrows), int(F),
              _stream(gy.device))
    return g[:, :F]


def edge_presplit(ea):
    """bf16 hi | lo image of the rows of ea for the matrix-core edge kernels (32 bytes per edge for S <= 8, 64 bytes for
    8 < S <= 16); None when not applicable."""
    E, S = ea.shape
    if S > 16 or E == 0:
        return None
    es = torch.empty(E, 8 if S <= 8 else 16, dtype=torch.int32, device=ea.device)
    _lib.call('gml_edge_presplit', _ptr(ea), _ptr(es), int(E), int(S), _stream(ea.device))
    return es


def _edge_mlp_pad(ea, w1, w2, w3, w4):
    """nedgeoutput != nedgeinput (spect_conv.py:66-71 allows it, no reference script uses it): the kernels are compiled
    for square shapes, and zero-padded operands of size P = max(S, Sout) give the identical result — a padded hidden
    unit is relu(0) = 0 resp. tanh(0)^2 = 0, a padded output column is dropped."""
    S, So = ea.size(1), w4.size(0)
    P = max(S, So)

    def pad_in(w):
        z = w.new_zeros(2 * P, P)
        z[:2 * S, :S] = w
        return z
    w4p = w4.new_zeros(P, 4 * P)
    w4p[:So, :2 * S] = w4[:, :2 * S]
    w4p[:So, 2 * P:2 * P + 2 * S] = w4[:, 2 * S:]
    return torch.nn.functional.pad(ea, (0, P - S)), pad_in(w1), pad_in(w2), pad_in(w3), w4p, P


def _edge_branch_torch(ea, w1, w2, w3, w4):
    """libs/spect_conv.py:205-207 as library calls (fc1_4 on the two halves of its input: no [E, 4S] concatenation)."""
    h1, h23 = torch.relu(_linear(ea, w1)), torch.tanh(_linear(ea, w2)) * torch.tanh(_linear(ea, w3))
    return torch.relu(torch.addmm(h1 @ w4[:, :h1.size(1)].t(), h23, w4[:, h1.size(1):].t()))


EDGE_WIDE_BWD_LIB = _os.environ.get('GML_EDGE_WIDE_BWD_LIB', '0') not in ('0', '')     # A/B: the round-5 library recompute


class EdgeBranchWide(torch.autograd.Function):
    """ML3Layer edge branch for 16 < max(S, Sout) <= 48: forward = ONE launch (gml_edge_mlp_wide_fwd: weights in LDS, exact fp32
    products, no intermediate in HBM -- the library road writes ~30 GB of them at S = 48 on 13 M edges); backward (round 6) = ONE launch
    for the per-edge part (gml_edge_mlp_wide_bwd: masked output gradient, hidden activations and the three pre-activation gradients,
    exact fp32) + the four weight gradients as tall contractions on the matrix cores (gml_xty_wide); the supports' own gradient, when
    asked for, is three library GEMMs.  GML_EDGE_WIDE_BWD_LIB=1: the library expression recomputed under autograd (rounds 1-5)."""

    @staticmethod
    def forward(ctx, ea, w1, w2, w3, w4):
        ea = _f32c(ea, 'edge_attr')
        ws = [_f32c(w.detach(), 'edge weight') for w in (w1, w2, w3, w4)]
        E, S = ea.shape
        So = int(w4.size(0))
        out = torch.empty(E, So, dtype=torch.float32, device=ea.device)
        with torch.cuda.device(ea.device):
            _lib.call('gml_edge_mlp_wide_fwd', _ptr(ea), _ptr(ws[0]), _ptr(ws[1]), _ptr(ws[2]), _ptr(ws[3]), _ptr(out), int(E), int(S), So,
                      _stream(ea.device))
        ctx.save_for_backward(ea, w1, w2, w3, w4, out)
        return out

    @staticmethod
    def backward(ctx, g):
        ea, w1, w2, w3, w4, out = ctx.saved_tensors
        need = ctx.needs_input_grad
        E, S = ea.shape
        So = int(w4.size(0))
        if not EDGE_WIDE_BWD_LIB and not exact_mode('edge') and E > 0:
            dev = ea.device
            ws = [_f32c(w.detach(), 'edge weight') for w in (w1, w2, w3, w4)]
            g = _f32c(g, 'grad_output')
            H2 = 2 * S
            H2R = int(_lib.lib().gml_edge_mlp_wide_bwd_h2r(int(S)))
            with torch.cuda.device(dev):
                go = torch.empty(E, So, dtype=torch.float32, device=dev)
                hid = torch.empty(E, 2 * H2R, dtype=torch.float32, device=dev)
                gz = torch.empty(E, 3 * H2R, dtype=torch.float32, device=dev)
                _lib.call('gml_edge_mlp_wide_bwd', _ptr(ea), _ptr(ws[0]), _ptr(ws[1]), _ptr(ws[2]), _ptr(ws[3]), _ptr(out), _ptr(g), _ptr(go),
                          _ptr(hid), _ptr(gz), int(E), int(S), So, _stream(dev))
                dws = [xty_wide(gz[:, m * H2R:m * H2R + H2], ea) for m in range(3)]           # dW_m = gz_m^T e   [2S, S]
                d4 = [xty_wide(hid[:, b * H2R:b * H2R + H2], go) for b in range(2)]           # (hid_b^T go)^T    [So, 2S] each
                if all(t is not None for t in dws + d4):
                    dw4 = torch.cat([d4[0].t(), d4[1].t()], 1).contiguous()
                    gin = None
                    if need[0]:                            # d e = sum_m gz_m W_m (no reference script trains the raw supports)
                        gin = gz[:, :H2] @ ws[0]
                        gin.addmm_(gz[:, H2R:H2R + H2], ws[1]).addmm_(gz[:, 2 * H2R:2 * H2R + H2], ws[2])
                    return gin, dws[0], dws[1], dws[2], dw4
        with torch.enable_grad():
            ins = [t.detach().requires_grad_(n) for t, n in zip((ea, w1, w2, w3, w4), need)]
            o2 = _edge_branch_torch(*ins)
            wanted = [t for t, n in zip(ins, need) if n]
            gs = iter(torch.autograd.grad(o2, wanted, g) if wanted else ())
        return tuple(next(gs) if n else None for n in need)


def _edge_arith():
    """the arithmetic flag of gml_edge_mlp_plan for a forward call under the current switches"""
    global EDGE_VALU
    if EDGE_VALU is None:
        EDGE_VALU = int(_lib.lib().gml_edge_mlp_plan(_lib.GML_EDGE_FWD, 2, 2, 0, _lib.GML_EDGE_TWO_PIECE)) == _lib.GML_EDGE_FAM_VALU
    if exact_mode('edge'):
        return _lib.GML_EDGE_EXACT
    return _lib.GML_EDGE_THREE_PIECE if (EDGE_FWD6 and not EDGE_VALU) else _lib.GML_EDGE_TWO_PIECE


# GML_VERBOSE labels of the families gml_edge_mlp_plan answers (tools/bench_configs.py lists 'VALU kernels' as a slow path)
_EDGE_LABEL = {_lib.GML_EDGE_FAM_VALU: 'VALU kernels (one edge per lane, fp32)', _lib.GML_EDGE_FAM_CHAIN: 'matrix-core chain, two-piece',
               _lib.GML_EDGE_FAM_CHAIN16: 'matrix-core chain16, two-piece', _lib.GML_EDGE_FAM_CHAIN6: 'matrix-core chain, three-piece',
               _lib.GML_EDGE_FAM_CHAIN16X6: 'matrix-core chain16, three-piece', _lib.GML_EDGE_FAM_SYM6: 'matrix-core chain, three-piece, unique rows',
               _lib.GML_EDGE_FAM_SYM16X6: 'matrix-core chain16, three-piece, unique rows'}


def _edge_path(fam, arith, S, L=0):
    if VERBOSE:
        what = 'exact family (one edge per lane, fp32)' if arith == _lib.GML_EDGE_EXACT else _EDGE_LABEL[fam]
        _path('edge', ('stack of %d layers in one pass, ' % L if L > 1 else '') + what, S, '-', S)


# family (include/gml.h GML_EDGE_FAM_*), the arithmetic it runs on and the entry point of one edge-branch forward; entry None: no kernel
EdgeFwd = _collections.namedtuple('EdgeFwd', 'family arith entry')


def _edge_fwd_family(S, So, L, arith, has_split, dual, pairs):
    """EdgeFwd of L layers' edge branches in one pass (L = 1: one layer); every gml_edge_mlp_plan query of the forward is made here."""
    # has_split / dual: the pre-split rows are there / the scattered second copy is wanted; pairs: the batch has a unique-row list.
    # Unique rows where the plan has them, else the stacked kernel (L > 1; exact: none) or the single-layer entry of `arith`.
    NONE = _lib.GML_EDGE_FAM_NONE
    plan = lambda n, ar, fl: int(_lib.lib().gml_edge_mlp_plan(_lib.GML_EDGE_FWD, int(S), int(So), n, ar | fl))
    flags = (_lib.GML_EDGE_HAS_SPLIT if has_split else 0) | (_lib.GML_EDGE_DUAL if dual and L == 1 else 0)
    # the unique support rows only (gml_edge_chain_sym_impl.h): every output row is written, by its own entry or by its mirror's
    fam = plan(L, arith, _lib.GML_EDGE_UNIQUE) if pairs else NONE
    if fam != NONE:
        return EdgeFwd(fam, arith, 'gml_edge_mlp_fwd_stack6_sym')
    if L > 1:
        fam = plan(L, arith, flags)
        return EdgeFwd(fam, arith, {NONE: None, _lib.GML_EDGE_FAM_CHAIN6: 'gml_edge_mlp_fwd_stack6'}.get(fam, 'gml_edge_mlp_fwd_stack'))
    fam = plan(0, arith, flags)
    if fam == NONE and arith == _lib.GML_EDGE_THREE_PIECE:      # S = 1 has no three-piece form: the default entry
        arith = _lib.GML_EDGE_TWO_PIECE
        fam = plan(0, arith, flags)
    # exact arithmetic covers the edge branch too (round 5: it did not); the three-piece entry (fp32-class) reads the fp32 rows itself
    return EdgeFwd(fam, arith, None if fam == NONE else ('gml_edge_mlp_fwd', 'gml_edge_mlp_fwd6', 'gml_edge_mlp_fwd_exact')[arith])


def edge_mlp_fwd(ea, w1, w2, w3, w4, tpos=None, ea_split=None, fam=None):
    """returns out (same edge order as ea) and, when tpos is given, the same rows at out_t[tpos[e]]; fam: the caller's EdgeFwd, if any"""
    E, S = ea.shape
    So = w4.size(0)
    if So != S:
        eap, w1p, w2p, w3p, w4p, _ = _edge_mlp_pad(ea, w1, w2, w3, w4)
        out, out_t = edge_mlp_fwd(eap, w1p, w2p, w3p, w4p, tpos, edge_presplit(eap))
        return out[:, :So].contiguous(), (out_t[:, :So].contiguous() if out_t is not None else None)
    out = torch.empty(E, So, dtype=torch.float32, device=ea.device)
    out_t = torch.empty(E, So, dtype=torch.float32, device=ea.device) if tpos is not None else None
    fam = fam or _edge_fwd_family(S, So, 1, _edge_arith(), ea_split is not None, tpos is not None, False)
    if fam.entry is None:
        _lib.check(_lib.GML_E_UNSUPPORTED)
    _edge_path(fam.family, fam.arith, S)
    _lib.call(fam.entry, _ptr(ea), *((_ptr(ea_split),) if fam.arith == _lib.GML_EDGE_TWO_PIECE else ()), _ptr(w1), _ptr(w2), _ptr(w3), _ptr(w4),
              _ptr(out), _ptr(tpos), _ptr(out_t), int(E), int(S), int(So), _stream(ea.device))
    return out, out_t


EDGE_STACK = not _os.environ.get('GML_NO_EDGE_STACK')     # A/B switch: edge branches of stacked layers in one launch
# The edge-branch FORWARD on three-piece products ("bf16x6", csrc/gml_edge_chain6_impl.h: fp32-class learned supports) -- the default
# since round 6; GML_EDGE_FWD6=0 restores the two-piece chain (bf16x3: ~5e-7 rms on the supports, which after training moved
# parameter gradients to 1e-3 .. 1e-2 of their term sums: profiles/r06_precision_diag.jsonl).
EDGE_FWD6 = _os.environ.get('GML_EDGE_FWD6', '1') not in ('0', '')
# The edge branch over a batch's UNIQUE support rows (csrc/gml_edge_chain_sym_impl.h: an edge and its mirror mostly carry bitwise the
# same row -- the supports sample symmetric matrices -- and then get the same output; exact, no tolerance): GML_EDGE_SYM=0 turns it off.
EDGE_SYM = _os.environ.get('GML_EDGE_SYM', '1') not in ('0', '')


def edge_mlp_fwd_stack(ea, ea_split, weights, sym=None, fam=None):
    """The edge branches of several layers on the SAME supports in one pass (gml_edge_mlp_fwd_stack): weights = [(w1, w2, w3, w4)]
    per layer; returns the list of outputs [E, S] (edge order of ea), or None when the library has no stacked kernel for the shape."""
    # sym: the batch's unique-row list; fam: the EdgeFwd the caller resolved for this call (default: asked here)
    E, S = ea.shape
    L = len(weights)
    if fam is None and not any(w[3].size(0) != S or w[0].size(1) != S for w in weights):
        fam = _edge_fwd_family(S, S, L, _edge_arith(), ea_split is not None, False, sym is not None and EDGE_SYM)
    if fam is None or 'stack' not in (fam.entry or ''):
        return None
    _edge_path(fam.family, fam.arith, S, L)
    outs = [torch.empty(E, S, dtype=torch.float32, device=ea.device) for _ in range(L)]
    arr = lambda ts: (ctypes.c_void_p * L)(*[t.data_ptr() for t in ts])
    tail = [arr([w[i] for w in weights]) for i in range(4)] + [arr(outs), int(E), int(S), int(S), _stream(ea.device)]
    if fam.entry == 'gml_edge_mlp_fwd_stack6_sym':
        # (uid, mir, count): the entry count lives on the device (an assembled batch)
        _lib.call(fam.entry + '_dev' if len(sym) == 3 else fam.entry, _ptr(ea), *[_ptr(t) for t in sym], int(sym[0].numel()), L, *tail)
    else:
        _lib.call(fam.entry, _ptr(ea if fam.entry == 'gml_edge_mlp_fwd_stack6' else ea_split), L, *tail)
    return outs


def _edge_dw_flat(fq, ws, nparts, S, So, w1, w2, w3, w4):
    """Queue the deferred fold of the partial rows in ws and return dw1 .. dw4 as views of its ONE flat destination: autograd takes
    a view over as .grad without a copy, and the flat tensor (held by the queue until the fold has run) cannot be freed under the
    fold's feet -- separate tensors referenced by the queue would be CLONED by AccumulateGrad (a second owner), before the fold
    has filled them."""
    n1, n4 = 2 * S * S, 4 * S * So
    flat = torch.empty(3 * n1 + n4, dtype=torch.float32, device=ws.device)
    fq.append((ws, nparts, 3 * n1 + n4, [(flat, 3 * n1 + n4)]))
    return flat[:n1].view_as(w1), flat[n1:2 * n1].view_as(w2), flat[2 * n1:3 * n1].view_as(w3), flat[3 * n1:].view_as(w4)


def edge_mlp_bwd(ea, w1, w2, w3, w4, gout, need_gin, ea_split=None, sym=None):
    E, S = ea.shape
    So = w4.size(0)
    dev = ea.device
    if So != S:
        eap, w1p, w2p, w3p, w4p, P = _edge_mlp_pad(ea, w1, w2, w3, w4)
        gin, d1, d2, d3, d4 = edge_mlp_bwd(eap, w1p, w2p, w3p, w4p, torch.nn.functional.pad(gout, (0, P - So)), need_gin,
                                           edge_presplit(eap))
        return (gin[:, :S].contiguous() if gin is not None else None, d1[:2 * S, :S].contiguous(),
                d2[:2 * S, :S].contiguous(), d3[:2 * S, :S].contiguous(),
                torch.cat([d4[:So, :2 * S], d4[:So, 2 * P:2 * P + 2 * S]], 1))
    nbytes = int(_lib.lib().gml_edge_mlp_bwd_workspace_bytes(int(E), int(S), int(So)))
    ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
    gin = torch.empty_like(ea) if need_gin else None
    dw1, dw2, dw3, dw4 = torch.empty_like(w1), torch.empty_like(w2), torch.empty_like(w3), torch.empty_like(w4)
    wsa = (int(E), int(S), int(So), _ptr(ws), ws.numel(), _stream(dev))
    if exact_mode('edge'):
        _lib.call('gml_edge_mlp_bwd_exact', _ptr(ea), _ptr(w1), _ptr(w2), _ptr(w3), _ptr(w4), _ptr(gout), _ptr(gin),
                  _ptr(dw1), _ptr(dw2), _ptr(dw3), _ptr(dw4), *wsa)
        return gin, dw1, dw2, dw3, dw4
    _edge_arith()                                         # (fills EDGE_VALU)
    fq = _fold_queue() if E > 0 else None                 # deferred fold: no destinations, the partial rows stay in ws
    d = [_ptr(None)] * 4 if fq is not None else [_ptr(dw1), _ptr(dw2), _ptr(dw3), _ptr(dw4)]
    flags = (_lib.GML_EDGE_HAS_SPLIT if ea_split is not None else 0) | (_lib.GML_EDGE_WANT_GIN if need_gin else 0)
    unique = sym is not None and EDGE_SYM and not EDGE_VALU and E > 0
    if unique and int(_lib.lib().gml_edge_mlp_plan(_lib.GML_EDGE_BWD, int(S), int(So), 0, flags | _lib.GML_EDGE_UNIQUE)) != _lib.GML_EDGE_FAM_NONE:
        # unique support rows only: entry u runs the chain once on gout[uid[u]] + gout[mir[u]]
        U = int(sym[0].numel())
        if len(sym) == 3:                                 # (uid, mir, count): U is the capacity, the count lives on the device
            _lib.call('gml_edge_mlp_bwd_sym_dev', _ptr(ea_split), _ptr(sym[0]), _ptr(sym[1]), _ptr(sym[2]), U, _ptr(w1), _ptr(w2), _ptr(w3),
                      _ptr(w4), _ptr(gout), *d, *wsa)
        else:
            _lib.call('gml_edge_mlp_bwd_sym', _ptr(ea_split), _ptr(sym[0]), _ptr(sym[1]), U, _ptr(w1), _ptr(w2), _ptr(w3), _ptr(w4), _ptr(gout),
                      *d, *wsa)
        nparts = int(_lib.lib().gml_edge_mlp_bwd_sym_parts(U, int(S))) if fq is not None else 0
        gin = None
    else:
        _lib.call('gml_edge_mlp_bwd', _ptr(ea), _ptr(ea_split), _ptr(w1), _ptr(w2), _ptr(w3), _ptr(w4), _ptr(gout), _ptr(gin), *d, *wsa)
        nparts = int(_lib.lib().gml_edge_mlp_bwd_parts(int(E), int(S), int(So), 1 if ea_split is not None else 0, 1 if need_gin else 0)) if fq is not None else 0
    if fq is not None:
        dw1, dw2, dw3, dw4 = _edge_dw_flat(fq, ws, nparts, S, So, w1, w2, w3, w4)
    return gin, dw1, dw2, dw3, dw4


def node_mix_native(Fin, F2):
    """True when the Hadamard branch tanh(fc11 x) * tanh(fc12 x) of this shape runs on the fused HIP kernels."""
    return int(_lib.lib().gml_node_mix_bwd_workspace_bytes(1, int(Fin), int(F2))) != 0


def ml3_split_bwd(gy, y, nout1, x=None, w11=None, b11=None, w12=None, b12=None, need_dx=False, need_dcb=False, dz_out=False,
                  gy_seg=None, premasked=False):
    """One pass over the rows for the backward of  cat[relu(conv), tanh(fc11 x) * tanh(fc12 x)]  (or of a plain
    relu(conv) when w11 is None): returns G [N, nout1] (view of a zero-padded buffer), dx (Hadamard-branch part
    only, or None), dcb, dw11, db11, dw12, db12.  dz_out (2 nout2 <= 4): the second result is dz [N, 4] = (dz11 | dz12)
    instead of dx = dz [w11; w12] (the operand of fused_conv_bwd(..., mix=)).  gy_seg (int32 [N]): gy has one row per
    segment and row r reads gy[gy_seg[r]] (the un-expanded gradient of a global add pool that follows the layer).
    premasked: gy[:, :nout1] already carries this layer's relu mask (the consumer layer's conv backward applied it,
    fused_conv_bwd(..., relu_cols=)): y is not read, no G is written -- the returned G is a view of gy."""
    N = y.size(0)
    F2 = 0 if w11 is None else int(w11.size(0))
    Fin = int(x.size(1)) if F2 else 0
    dev = gy.device
    nbytes = int(_lib.lib().gml_ml3_split_bwd_workspace_bytes(int(N), Fin, int(nout1), F2))
    if nbytes == 0 and N > 0:
        return None
    ld = (nout1 + 3) // 4 * 4                                # zero padded: float4-readable rows
    assert not premasked or (gy_seg is None and _rows4_ok(*_rows_of(gy), nout1)), 'a pre-masked gradient is handed on as G: float4-readable rows'
    G = gy if premasked else torch.empty(N, ld, dtype=torch.float32, device=dev)
    ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
    dx = torch.empty(N, Fin, dtype=torch.float32, device=dev) if (need_dx and F2 and not dz_out) else None
    dz = torch.empty(N, 4, dtype=torch.float32, device=dev) if (dz_out and F2) else None
    dcb = torch.empty(nout1, dtype=torch.float32, device=dev) if need_dcb else None
    dw11 = torch.empty_like(w11) if F2 else None
    dw12 = torch.empty_like(w12) if F2 else None
    db11 = torch.empty_like(b11) if (F2 and b11 is not None) else None
    db12 = torch.empty_like(b12) if (F2 and b12 is not None) else None
    fq = _fold_queue()
    kd = (dcb, dw11, db11, dw12, db12)                       # what the kernel's own fold writes
    if fq is not None and N > 0 and any(t is not None for t in kd):
        # deferred: no destinations -> the entry point skips its fold; the partial rows [dw11 | dw12 | db11 | db12 | dcb] stay in ws
        npart = 2 * F2 * Fin + 2 * F2 + int(nout1)
        flat = torch.empty(npart, dtype=torch.float32, device=dev)                 # (views of it go to autograd: see edge_mlp_bwd)
        fq.append((ws, nbytes // (4 * npart), npart, [(flat, npart)]))
        o = 0
        if F2:
            dw11, dw12 = flat[:F2 * Fin].view_as(w11), flat[F2 * Fin:2 * F2 * Fin].view_as(w12)
            o = 2 * F2 * Fin
            db11 = flat[o:o + F2] if db11 is not None else None
            db12 = flat[o + F2:o + 2 * F2] if db12 is not None else None
            o += 2 * F2
        dcb = flat[o:o + int(nout1)] if dcb is not None else None
        kd = (None,) * 5
    kcb, k11, kb11, k12, kb12 = kd
    with _Timed('ml3_split_bwd', 4 * N * ((1 if premasked else 3) * (nout1 + F2) + (2 * Fin if dx is not None else Fin) + (4 if dz is not None else 0))):
        if dz is not None or gy_seg is not None or premasked:
            _lib.call('gml_ml3_split_bwd_ex', _ptr(gy), int(gy.stride(0)), _ptr(gy_seg), _ptr(None if premasked else y), int(y.stride(0)), _ptr(x),
                      int(x.stride(0)) if F2 else 0, _ptr(w11), _ptr(b11), _ptr(w12), _ptr(b12), _ptr(None if premasked else G), ld, _ptr(dx), Fin,
                      _ptr(dz), _ptr(kcb), _ptr(k11), _ptr(kb11), _ptr(k12), _ptr(kb12), int(N), Fin, int(nout1), F2,
                      _ptr(ws), ws.numel(), _stream(dev))
        else:
            _lib.call('gml_ml3_split_bwd', _ptr(gy), int(gy.stride(0)), _ptr(y), int(y.stride(0)), _ptr(x),
                      int(x.stride(0)) if F2 else 0, _ptr(w11), _ptr(b11), _ptr(w12), _ptr(b12), _ptr(G), ld, _ptr(dx), Fin,
                      _ptr(kcb), _ptr(k11), _ptr(kb11), _ptr(k12), _ptr(kb12), int(N), Fin, int(nout1), F2, _ptr(ws),
                      ws.numel(), _stream(dev))
    return G[:, :nout1], (dz if dz is not None else dx), dcb, dw11, db11, dw12, db12


def xty(a, b):
    """a^T b for two tall matrices with <= 64 columns each ([n,p], [n,q] -> [p,q]); None if outside the kernel range."""
    n, p, q = int(a.size(0)), int(a.size(1)), int(b.size(1))
    nbytes = int(_lib.lib().gml_xty_workspace_bytes(n, p, q))
    if nbytes == 0 and n > 0:
        return None
    out = torch.empty(p, q, dtype=torch.float32, device=a.device)
    ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=a.device)
    with _Timed('xty'):
        _lib.call('gml_xty', _ptr(a), int(a.stride(0)), _ptr(b), int(b.stride(0)), _ptr(out), n, p, q, _ptr(ws), ws.numel(),
                  _stream(a.device))
    return out


def gnnml1_block_supported(x, Fin, n1, n2, n3, mode, act=1):
    """the fused block (GNNML1BlockFunction) serves this input.  Modes 0..3: inputs up to 144 wide, parts up to 64; mode 4 (its own
    kernel family): n1 = n2 <= 128, n3 <= 64, Fin <= 192; mode 5: three equal parts up to 64, inputs up to 144, and act = 1 (relu)
    only -- the one mode whose answer depends on the activation (tanh there runs on the composition)"""
    if not (x.is_cuda and x.dtype == torch.float32) or _os.environ.get('GML_NO_GNNML1_FUSED'):
        return False
    if int(mode) == 5:
        return bool(_lib.lib().gml_gnnml1_actsum_supported(int(Fin), int(n1), int(n2), int(n3), int(act)))
    if int(mode) == 4:
        return bool(_lib.lib().gml_gnnml1_sum_supported(int(Fin), int(n1), int(n2), int(n3)))
    return bool(_lib.lib().gml_gnnml1_supported(int(Fin), int(n1), int(n2), int(n3), int(mode)))


class GNNML1BlockFunction(torch.autograd.Function):
    """One GNNML1 block (sr25.py:231-240, mnist75.py:296-318, mutag.py:253-262, enzymes_contfeat.py:284-346) as ONE launch forward;
    backward = one launch (g4, q = A dc, dx only when x needs it) and one weight-gradient pass + fold.  a = fc_i1 x, c = conv_i1 x
    (SpectConv K = 1), f2 = fc_i2 x, f3 = fc_i3 x;
    mode 0: act(a + c + f2 f3); 1: [act a | act c | act(f2 f3)]; 2: [act a | act c | act f2 . act f3]; 3: [act a | act c | tanh f2 . tanh f3]
    (ptc.py:311); 4: [act a + act c | act f2 . act f3] with n1 = n2; 5: act a + act c + act(f2 f3) with n1 = n2 = n3 (filtering.py:246);
    act 0 tanh / 1 relu.  Modes 0..3 (csrc/gml_gnnml1.hip): inputs up
    to 144 wide, parts up to 64; mode 4 (csrc/gml_gnnml1_sum.hip): inputs up to 192 wide, n1 <= 128, n3 <= 64
    (gnnml1_block_supported); rows of any stride.  Mode 4 differs in three places: its entry points, the pattern buffer and what is
    saved.  With relu its forward records the two activation patterns of the sum (one byte per 4 columns, saved for backward instead of
    `out`) and phase 1 reads them; tanh, or record=False: phase 1 recomputes a and c (the same bits).  record has no effect in modes
    0..3.  Mode 5 (csrc/gml_gnnml1_act.hip; relu only, inputs up to 144 wide, parts up to 64) always records the patterns of a and c
    in mode 4's byte layout, saves them instead of `out`, and its phase 1 forms g4 from gout, the bytes and the recomputed f2, f3; the g4
    it writes is mode 1's, so the weight-gradient pass runs as mode 1.  tanh in mode 5 is not served (TypeError here; the module
    composes it).  val: per-edge values in TARGET order ([E] / [E, 1]) or None for ones (the scripts pass torch.ones); they carry no gradient
    here (the module takes the unfused road when edge_attr requires one).  Exact fp32 products."""

    @staticmethod
    def forward(ctx, x, csr, val, w1, b1, wc, bc, w2, b2, w3, b3, mode, act, record=True):
        x = _f32rows(x, 'x')
        mode, act = int(mode), int(act)
        N, Fin = int(x.size(0)), int(x.size(1))
        n1, n2, n3 = int(w1.size(0)), int(wc.size(-1)), int(w2.size(0))
        w1, w2, w3, wc = _f32c(w1, 'fc1.weight'), _f32c(w2, 'fc2.weight'), _f32c(w3, 'fc3.weight'), _f32c(wc, 'conv.weight')
        C = n1 if mode in (0, 5) else (n1 + n3 if mode == 4 else n1 + n2 + n3)
        if mode == 5 and act != 1:
            raise TypeError('GNNML1 block mode 5 is fused for relu only (gnnml1_block_supported)')
        dev = x.device
        if val is not None:
            val = _f32c(val.reshape(-1), 'edge_attr')
        nbytes = 4 * (N * (Fin + C) + csr.E + N + Fin * (n1 + n2 + 2 * n3)) if PROFILE is not None else 0
        head = (_ptr(csr.rowptr), _ptr(csr.col), _ptr(val), _ptr(x), int(x.stride(0)), N, Fin,
                _ptr(w1), _ptr(b1), n1, _ptr(wc), _ptr(bc), n2, _ptr(w2), _ptr(b2), _ptr(w3), _ptr(b3), n3)
        with torch.cuda.device(dev):
            out = torch.empty(N, C, dtype=torch.float32, device=dev)
            if mode == 4:
                npat = (n1 + 15) // 16 * 4
                pat = torch.empty(N, npat, dtype=torch.uint8, device=dev) if (act == 1 and record) else None
                with _Timed('gnnml1_sum_fwd', nbytes, 0):
                    _lib.call('gml_gnnml1_sum_fwd', *head, act, _ptr(out), C, _ptr(pat), npat, _stream(dev))
            elif mode == 5:
                npat = (n1 + 15) // 16 * 4
                pat = torch.empty(N, npat, dtype=torch.uint8, device=dev)
                with _Timed('gnnml1_actsum_fwd', nbytes + N * npat if PROFILE is not None else 0, 0):
                    _lib.call('gml_gnnml1_actsum_fwd', *head, act, _ptr(out), C, _ptr(pat), npat, _stream(dev))
                _path('gnnml1_block', 'fused act_sum (Fin=%d n=%d)' % (Fin, n1))
            else:
                with _Timed('gnnml1_fwd', nbytes, 0):
                    _lib.call('gml_gnnml1_fwd', *head, mode, act, _ptr(out), C, _stream(dev))
        ctx.csr, ctx.mode, ctx.act, ctx.dims = csr, mode, act, (N, Fin, n1, n2, n3, C)
        ctx.has_b = (b1 is not None, bc is not None, b2 is not None, b3 is not None)
        # mode 4 recomputes a and c from the biases (or reads the pattern) and never reads `out`; mode 5 reads the pattern; modes 0..3
        # read `out`
        ctx.save_for_backward(x, val, w1, wc, w2, b2, w3, b3, *((b1, bc, pat) if mode == 4 else ((pat,) if mode == 5 else (out,))))
        return out

    @staticmethod
    def backward(ctx, gout):
        x, val, w1, wc, w2, b2, w3, b3, *rest = ctx.saved_tensors
        N, Fin, n1, n2, n3, C = ctx.dims
        csr, mode, act = ctx.csr, ctx.mode, ctx.act
        dev = x.device
        gout = _f32rows(gout, 'grad_output')
        L = _lib.lib()
        # the entry points of mode 4 take no mode argument; mode 5 writes mode 1's g4: the shared pass runs as mode 1
        sfx, m = ('_sum', ()) if mode == 4 else ('', (1 if mode == 5 else mode,))
        ng4 = int(getattr(L, 'gml_gnnml1%s_g4_cols' % sfx)(n1, n2, n3, *m))
        p1, p2, p3 = (n1 + 15) // 16 * 16, (n2 + 15) // 16 * 16, (n3 + 15) // 16 * 16
        need_x = ctx.needs_input_grad[0]
        with torch.cuda.device(dev):
            val_t = csr.to_source_order(val.view(-1, 1)).view(-1) if val is not None else None
            g4 = torch.empty(N, ng4, dtype=torch.float32, device=dev)
            q = torch.empty(N, p2, dtype=torch.float32, device=dev)                   # (mode 4: p2 == p1)
            dx = torch.empty(N, Fin, dtype=torch.float32, device=dev) if need_x else None
            if mode == 4:
                b1, bc, pat = rest
                with _Timed('gnnml1_sum_bwd', 4 * (N * (Fin + C + (Fin if need_x else 0) + ng4 + p1) + 2 * (csr.E + N)) if PROFILE is not None else 0, 0):
                    _lib.call('gml_gnnml1_sum_bwd', _ptr(csr.rowptr), _ptr(csr.col), _ptr(val), _ptr(csr.rowptr_t), _ptr(csr.col_t), _ptr(val_t),
                              _ptr(x), int(x.stride(0)), _ptr(gout), int(gout.stride(0)), N, Fin, _ptr(w1), _ptr(b1), n1, _ptr(wc), _ptr(bc), n2,
                              _ptr(w2), _ptr(b2), _ptr(w3), _ptr(b3), n3, act, _ptr(pat), p1 // 4, _ptr(dx), Fin, _ptr(g4), ng4, _ptr(q), p1,
                              _stream(dev))
            elif mode == 5:
                pat, = rest
                with _Timed('gnnml1_actsum_bwd', 4 * (N * (Fin + C + (Fin if need_x else 0) + ng4 + p2) + csr.E + N) + N * p1 // 4 if PROFILE is not None else 0, 0):
                    _lib.call('gml_gnnml1_actsum_bwd', _ptr(csr.rowptr_t), _ptr(csr.col_t), _ptr(val_t), _ptr(x), int(x.stride(0)), _ptr(gout),
                              int(gout.stride(0)), N, Fin, _ptr(w1), n1, _ptr(wc), n2, _ptr(w2), _ptr(b2), _ptr(w3), _ptr(b3), n3, act,
                              _ptr(pat), p1 // 4, _ptr(dx), Fin, _ptr(g4), ng4, _ptr(q), p2, _stream(dev))
            else:
                out, = rest
                with _Timed('gnnml1_bwd', 4 * (N * (Fin + 2 * C + (Fin if need_x else 0) + ng4 + p2) + csr.E + N) if PROFILE is not None else 0, 0):
                    _lib.call('gml_gnnml1_bwd', _ptr(csr.rowptr_t), _ptr(csr.col_t), _ptr(val_t), _ptr(x), int(x.stride(0)), _ptr(out), C,
                              _ptr(gout), int(gout.stride(0)), N, Fin, _ptr(w1), n1, _ptr(wc), n2, _ptr(w2), _ptr(b2), _ptr(w3), _ptr(b3), n3,
                              mode, act, _ptr(dx), Fin, _ptr(g4), ng4, _ptr(q), p2, _stream(dev))
            with _Timed('gnnml1_actsum_dw' if mode == 5 else 'gnnml1%s_dw' % sfx):
                nflat = int(getattr(L, 'gml_gnnml1%s_dw_floats' % sfx)(Fin, n1, n2, n3, *m))
                nws = int(getattr(L, 'gml_gnnml1%s_dw_workspace_bytes' % sfx)(N, Fin, n1, n2, n3, *m))
                flat = torch.empty(nflat, dtype=torch.float32, device=dev)
                ws = torch.empty(max(nws, 4), dtype=torch.uint8, device=dev)
                _lib.call('gml_gnnml1%s_dw' % sfx, _ptr(x), int(x.stride(0)), _ptr(g4), ng4, _ptr(q), p2, N, Fin, n1, n2, n3, *m, _ptr(flat),
                          _ptr(ws), ws.numel(), _stream(dev))
                e1, e2, e3, e4 = n1 * Fin, n1 * Fin + n3 * Fin, n1 * Fin + 2 * n3 * Fin, n1 * Fin + 2 * n3 * Fin + Fin * n2
                dw1, dw2, dw3, dwc = flat[:e1].view(n1, Fin), flat[e1:e2].view(n3, Fin), flat[e2:e3].view(n3, Fin), flat[e3:e4].view(Fin, n2)
                sums = flat[e4:]                                      # column sums of g4: mode 0 [da = dc | df2 | df3], else [da | dc | df2 | df3]
        oa, oc = 0, p1
        o2 = p1 if mode == 0 else p1 + p2
        o3 = o2 + p3
        hb1, hbc, hb2, hb3 = ctx.has_b
        db1 = sums[oa:oa + n1] if hb1 else None
        # mode 0: fc_i1's and conv_i1's biases receive the SAME column sums -- as two tensors with their own memory (autograd adopts a
        # returned gradient as .grad; two parameters sharing one buffer would double every in-place op on the gradients: ADVICE r05)
        dbc = ((sums[oa:oa + n2].clone() if hb1 else sums[oa:oa + n2]) if mode == 0 else sums[oc:oc + n2]) if hbc else None
        db2 = sums[o2:o2 + n3] if hb2 else None
        db3 = sums[o3:o3 + n3] if hb3 else None
        return dx, None, None, dw1, db1, dwc.view(1, Fin, n2), dbc, dw2, db2, dw3, db3, None, None, None


def xty_wide(a, b):
    """a^T b for a tall wide a [n, p <= 4096] and b [n, q <= 128] on the bf16 matrix cores (bf16x3 products; gml_xty_wide): the dense
    block's dW = Hcat^T g; None if outside the kernel range."""
    n, p, q = int(a.size(0)), int(a.size(1)), int(b.size(1))
    L = _lib.lib()
    if not L.gml_xty_wide_supported(n, p, q) or exact_mode() or a.stride(1) != 1 or b.stride(1) != 1:
        return None
    nbytes = int(L.gml_xty_wide_workspace_bytes(n, p, q))
    out = torch.empty(p, q, dtype=torch.float32, device=a.device)
    ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=a.device)
    _lib.call('gml_xty_wide', _ptr(a), int(a.stride(0)), _ptr(b), int(b.stride(0)), _ptr(out), n, p, q, _ptr(ws), ws.numel(),
              _stream(a.device))
    return out


class BatchNormFunction(torch.autograd.Function):
    """torch.nn.BatchNorm1d in training mode on the HIP kernels of csrc/gml_bn.hip (mutag.py:272-288: BatchNorm between the layers).
    Returns (y, batch mean, biased batch variance); raises NotImplementedError for shapes the kernels do not take (the module then
    uses torch's implementation)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        N, C = int(x.size(0)), int(x.size(1))
        dev = x.device
        L = _lib.lib()
        with torch.cuda.device(dev):
            st = _stream(dev)
            stats = torch.empty(3, C, dtype=torch.float32, device=dev)
            ws = torch.empty(max(int(L.gml_bn_workspace_bytes(N)), 4), dtype=torch.uint8, device=dev)
            with _Timed('bn_fwd'):
                rc = L.gml_bn_stats(_ptr(x), int(x.stride(0)), N, C, float(eps), _ptr(stats[0]), _ptr(stats[1]), _ptr(stats[2]), _ptr(ws), ws.numel(), st)
            if rc == _lib.GML_E_UNSUPPORTED:
                raise NotImplementedError('shape')
            _lib.check(rc)
            y = torch.empty(N, C, dtype=torch.float32, device=dev)
            with _Timed('bn_fwd'):
                _lib.call('gml_bn_apply', _ptr(x), int(x.stride(0)), N, C, _ptr(stats[0]), _ptr(stats[2]), _ptr(weight), _ptr(bias), _ptr(y), C, st)
        ctx.save_for_backward(x, weight, stats)
        ctx.has_bias = bias is not None
        ctx.mark_non_differentiable(stats)
        return y, stats

    @staticmethod
    def backward(ctx, dy, _ds):
        x, weight, stats = ctx.saved_tensors
        N, C = int(x.size(0)), int(x.size(1))
        dev = x.device
        dy = dy if (dy.stride(1) == 1 and dy.stride(0) % 4 == 0 and dy.data_ptr() % 16 == 0) else dy.contiguous()
        with torch.cuda.device(dev):
            st = _stream(dev)
            sums = torch.empty(2, C, dtype=torch.float32, device=dev)
            ws = torch.empty(max(int(_lib.lib().gml_bn_workspace_bytes(N)), 4), dtype=torch.uint8, device=dev)
            with _Timed('bn_bwd'):
                _lib.call('gml_bn_bwd_sums', _ptr(dy), int(dy.stride(0)), _ptr(x), int(x.stride(0)), N, C, _ptr(stats[0]), _ptr(stats[2]),
                          _ptr(sums[0]), _ptr(sums[1]), _ptr(ws), ws.numel(), st)
            dx = None
            if ctx.needs_input_grad[0]:
                dx = torch.empty(N, C, dtype=torch.float32, device=dev)
                with _Timed('bn_bwd'):
                    _lib.call('gml_bn_bwd_apply', _ptr(dy), int(dy.stride(0)), _ptr(x), int(x.stride(0)), N, C, _ptr(stats[0]), _ptr(stats[2]),
                              _ptr(weight), _ptr(sums[0]), _ptr(sums[1]), _ptr(dx), C, st)
        return dx, (sums[1] if weight is not None else None), (sums[0] if ctx.has_bias else None), None


class MaskedBatchNormFunction(torch.autograd.Function):
    """BatchNormFunction over the VALID rows of a padded batch (csrc/gml_bn.hip gml_bn_masked_*): row r takes part iff valid[r] != 0
    (float32 [N] on the device).  Returns (y, stats [3, C] = batch mean / biased variance / rstd, count [1] = number of valid rows, on
    the device); y and dx are exact zeros on the other rows.  No host read: capturable.  Raises NotImplementedError for shapes the
    kernels do not take (there is no unmasked fallback that would be right)."""

    @staticmethod
    def forward(ctx, x, valid, weight, bias, eps):
        N, C = int(x.size(0)), int(x.size(1))
        dev = x.device
        L = _lib.lib()
        with torch.cuda.device(dev):
            st = _stream(dev)
            stats = torch.empty(3, C, dtype=torch.float32, device=dev)
            count = torch.empty(1, dtype=torch.float32, device=dev)
            ws = torch.empty(max(int(L.gml_bn_masked_workspace_bytes(N)), 4), dtype=torch.uint8, device=dev)
            with _Timed('bn_fwd'):
                rc = L.gml_bn_masked_stats(_ptr(x), int(x.stride(0)), _ptr(valid), N, C, float(eps), _ptr(stats[0]), _ptr(stats[1]),
                                           _ptr(stats[2]), _ptr(count), _ptr(ws), ws.numel(), st)
            if rc == _lib.GML_E_UNSUPPORTED:
                raise NotImplementedError('masked BatchNorm: C <= 64, C % 4 == 0, float4-addressable rows')
            _lib.check(rc)
            y = torch.empty(N, C, dtype=torch.float32, device=dev)
            with _Timed('bn_fwd'):
                _lib.call('gml_bn_masked_apply', _ptr(x), int(x.stride(0)), _ptr(valid), N, C, _ptr(stats[0]), _ptr(stats[2]), _ptr(weight),
                          _ptr(bias), _ptr(y), C, st)
        ctx.save_for_backward(x, valid, weight, stats, count)
        ctx.has_bias = bias is not None
        ctx.mark_non_differentiable(stats, count)
        return y, stats, count

    @staticmethod
    def backward(ctx, dy, _ds, _dc):
        x, valid, weight, stats, count = ctx.saved_tensors
        N, C = int(x.size(0)), int(x.size(1))
        dev = x.device
        dy = dy if (dy.stride(1) == 1 and dy.stride(0) % 4 == 0 and dy.data_ptr() % 16 == 0) else dy.contiguous()
        with torch.cuda.device(dev):
            st = _stream(dev)
            sums = torch.empty(2, C, dtype=torch.float32, device=dev)
            ws = torch.empty(max(int(_lib.lib().gml_bn_masked_workspace_bytes(N)), 4), dtype=torch.uint8, device=dev)
            with _Timed('bn_bwd'):
                _lib.call('gml_bn_masked_bwd_sums', _ptr(dy), int(dy.stride(0)), _ptr(x), int(x.stride(0)), _ptr(valid), N, C, _ptr(stats[0]),
                          _ptr(stats[2]), _ptr(sums[0]), _ptr(sums[1]), _ptr(ws), ws.numel(), st)
            dx = None
            if ctx.needs_input_grad[0]:
                dx = torch.empty(N, C, dtype=torch.float32, device=dev)
                with _Timed('bn_bwd'):
                    _lib.call('gml_bn_masked_bwd_apply', _ptr(dy), int(dy.stride(0)), _ptr(x), int(x.stride(0)), _ptr(valid), N, C,
                              _ptr(stats[0]), _ptr(stats[2]), _ptr(weight), _ptr(sums[0]), _ptr(sums[1]), _ptr(count), _ptr(dx), C, st)
        return dx, None, (sums[1] if weight is not None else None), (sums[0] if ctx.has_bias else None), None


def bn_masked_running_update(count, stats, momentum, running_mean, running_var):
    """running_mean / running_var <- (1 - momentum) r + momentum stat over a padded batch's valid rows (unbiased variance, n read on
    the device; n < 2: unchanged) -- gml_bn_masked_running_update, no host read."""
    dev = running_mean.device
    with torch.cuda.device(dev):
        _lib.call('gml_bn_masked_running_update', _ptr(count), _ptr(stats[0]), _ptr(stats[1]), int(stats.size(1)), float(momentum),
                  _ptr(running_mean), _ptr(running_var), _stream(dev))


class TallLinearFunction(torch.autograd.Function):
    """F.linear for a small layer applied to many rows; only the weight gradient g^T x differs from autograd's
    (a K = rows contraction that a library GEMM runs on a single workgroup)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_b = b is not None
        return torch.nn.functional.linear(x, w, b)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = g.contiguous()
        gx = g.mm(w) if ctx.needs_input_grad[0] else None
        gw = None
        if ctx.needs_input_grad[1]:
            with torch.cuda.device(x.device):
                # (a few rows -- the reference's batch 64: 65 pooled rows -- are one short library GEMM: 5 us against the 17 us the
                #  tall-matrix kernel's two stages take on nothing)
                gw = xty(g, x.contiguous()) if (x.is_cuda and x.dtype == torch.float32 and x.size(0) >= 2048) else None
            if gw is None:
                gw = g.t().mm(x)
        gb = g.sum(0) if (ctx.has_b and ctx.needs_input_grad[2]) else None
        return gx, gw, gb


# The road of the readout head and its loss (models._step_loss; DESIGN s4.4c), decided ONCE, from plain values, BEFORE the model's
# features run.  kind: 'l1_small' (csrc/gml_head.hip, one workgroup), 'l1_big' (gml_head_big.hip), 'bce' (gml_head_bce.hip), 'node'
# (gml_node_head.hip) or 'torch'; pad_grad_zero: what model.features is told about a static batch's padding row; label: the PATHS text.
HeadRoad = _collections.namedtuple('HeadRoad', 'kind pad_grad_zero label')
HEAD_MLP32 = (False, 32, 'relu', True, None)       # models._MLP32, relu(fc1: nin -> 32) then fc2: the head row the L1 kernels serve
_BCE_LABEL = 'fused BCE head (%d -> %d -> 1, %s)'


def head_road(loss, head, listed, nin, nh, nout, R, nl, num_graphs, f32=True, aligned=True, override=None, env=_os.environ):
    """HeadRoad from plain values only (no tensor, no launch).  loss: 'l1' / 'bce' / 'node_sq'.  head: the model's _Head row (its
    `between` is the BCE kernel's activation); listed: the model's class names that head for this loss (L1: the 'mlp32' row, BCE: its
    _BCE_HEADS, node_sq: any).  fc1: nin -> nh, fc2: nh -> nout (node_sq: fc2: nin -> nout).  R: the rows model.features returns, nl:
    the labels, num_graphs: the batch's own count.  f32, aligned: head_flags.  override: a kind -- only that road where it serves the
    input, else 'torch' (tests, tools, the *_supported predicates).  GML_NO_HEAD_BIG / GML_NO_HEAD_BCE are read here and nowhere else."""
    if not listed or nout != 1:
        return HeadRoad('torch', False, "torch ops (%s on the model's own head)" % {'l1': 'L1', 'bce': 'BCE', 'node_sq': 'node loss'}[loss])
    may = lambda kind: override in (None, kind)
    ok = bool(f32 and aligned)
    if loss == 'l1':
        ok = ok and nl <= R
        if (ok and may('l1_small') and R <= 256 and nin <= 64 and nh <= 64 and nin % 4 == 0 and nh % 4 == 0
                and 4 * (R * nin + 2 * R * nh + 2 * R + nh * nin + 256) <= 160 * 1024):
            # (the one workgroup gives the rows beyond nl a zero gradient: the pool need not mask the padding graph's)
            return HeadRoad('l1_small', num_graphs <= 256 and nl <= num_graphs, 'fused L1 head, one workgroup (%d -> %d -> 1)' % (nin, nh))
        if ok and may('l1_big') and nin == 32 and nh == 32 and R >= 1 and not env.get('GML_NO_HEAD_BIG'):
            return HeadRoad('l1_big', False, 'fused L1 head, one pass + fold (32 -> 32 -> 1)')
        return HeadRoad('torch', False, 'torch ops (L1 head outside the fused kernels)')
    if loss == 'bce':                                      # (both roads give the padding graph's row a zero gradient)
        if ok and may('bce') and 1 <= nin <= 64 and 1 <= nh <= 64 and R >= 1 and nl <= R and not env.get('GML_NO_HEAD_BCE'):
            return HeadRoad('bce', True, _BCE_LABEL % (nin, nh, 'relu' if head[2] == 'relu' else 'identity'))
        return HeadRoad('torch', True, 'torch ops (BCE head outside the fused kernel)')
    if f32 and may('node') and 1 <= nin <= 64:
        return HeadRoad('node', False, 'fused node head (%d -> 1)' % nin)
    return HeadRoad('torch', False, 'torch ops (node head outside the fused kernel)')


def head_flags(loss, x, valid, w1, b1, w2, b2):
    """(f32, aligned) of head_road.  f32: x, the head's parameters and (L1) the validity are float32 on x's CUDA device.  aligned: what
    the launchers ask beyond shapes -- BCE: contiguous weights; L1: contiguous parameters, fc1.weight and fc2.weight on 16-byte
    boundaries (gml_head.hip:141, gml_head_big.hip:236); node_sq: nothing."""
    dev, f32 = x.device, x.is_cuda
    for t in (x, w1, b1, w2, b2, valid if loss == 'l1' else None):
        if t is not None and not (t.dtype == torch.float32 and t.device == dev):
            f32 = False
    if loss == 'node_sq' or not f32:
        return f32, True
    return f32, w1.is_contiguous() and w2.is_contiguous() and (loss == 'bce' or (
        (b1 is None or b1.is_contiguous()) and (b2 is None or b2.is_contiguous()) and w1.data_ptr() % 16 == 0 and w2.data_ptr() % 16 == 0))


def _head_bce_args(p, y, valid, w1, b1, w2, b2, stats):
    """the tensors as gml_head_bce_* take them; raises on what head_bce_supported would have refused"""
    p = _f32rows(p, 'pooled')
    for t, name in ((y, 'y'), (valid, 'valid'), (w1, 'fc1.weight'), (b1, 'fc1.bias'), (w2, 'fc2.weight'), (b2, 'fc2.bias')):
        if t is not None or name in ('y', 'fc1.weight', 'fc2.weight'):
            _require_cuda(t, name)
    if not head_bce_supported(p, w1, w2):
        raise ValueError('head_bce: pooled %s %s, fc1 weight %s, fc2 weight %s (float32, 1 <= nin, nh <= 64, one output)' %
                         (tuple(p.shape), p.dtype, tuple(w1.shape), tuple(w2.shape)))
    nl = int(y.numel())
    if nl > p.size(0) or (valid is not None and valid.numel() != nl):
        raise ValueError('head_bce: %d labels, %s validity entries for %d pooled rows' %
                         (nl, 'no' if valid is None else valid.numel(), p.size(0)))
    if stats is not None and not (stats.is_cuda and stats.dtype == torch.float32 and stats.numel() >= 3 and stats.is_contiguous()):
        raise ValueError('stats: a contiguous float32 CUDA tensor of 3 elements')
    y = y.to(torch.float32).contiguous()
    valid = valid.to(torch.float32).contiguous() if valid is not None else None
    c = lambda t: t.contiguous() if t is not None else None
    return p, y, valid, w1.contiguous(), c(b1), w2.contiguous(), c(b2)


# kind -> (forward entry, backward entry, workspace query or None): what the three pooled heads below differ in besides their
# trailing arguments; 'l1_big' alone lets its weight-gradient partials join an open deferred_folds scope
_HEAD_ENTRIES = dict(l1_small=('gml_head_l1_fwd_acc', 'gml_head_l1_bwd', None),
                     l1_big=('gml_head_l1_big_fwd', 'gml_head_l1_big_bwd', 'gml_head_l1_big_workspace_floats'),
                     bce=('gml_head_bce_fwd', 'gml_head_bce_bwd', 'gml_head_bce_workspace_floats'))


def _head_call(entry, t, *tail):
    """one launch of a pooled-head entry on t = (p, y, valid, w1, b1, w2, b2): the twelve common arguments, the entry's own, the stream"""
    p, y, valid, w1, b1, w2, b2 = t
    with torch.cuda.device(p.device):
        with _Timed('head'):
            _lib.call(entry, _ptr(p), int(p.stride(0)), _ptr(y), _ptr(valid), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), int(p.size(0)),
                      int(y.numel()), int(p.size(1)), int(w1.size(0)), *tail, _stream(p.device))


def _head_ws(kind, p, w1, nws=None):
    """(workspace or None, its floats) of one launch; nws: what the forward's query answered"""
    q = _HEAD_ENTRIES[kind][2]
    if nws is None:
        nws = int(getattr(_lib.lib(), q)(int(p.size(0)), int(p.size(1)), int(w1.size(0)))) if q else 0
    return (torch.empty(nws, dtype=torch.float32, device=p.device) if nws else None), nws


def _pooled_head_fwd(ctx, kind, t, act, acc):
    """loss = sum_{r < len(y)} valid[r] rowloss(fc2(act(fc1 p[r])), y[r]) in ONE pass.  Saves nothing but its inputs -- the backward
    recomputes the forward --, no host read: capturable."""
    p, w1 = t[0], t[3]
    ws, nws = _head_ws(kind, p, w1)
    loss = torch.empty((), dtype=torch.float32, device=p.device)
    if kind == 'bce':                                       # (as ever: direct callers of HeadBCEFunction show in PATHS too)
        _path('head', _BCE_LABEL % (int(p.size(1)), int(w1.size(0)), 'relu' if act else 'identity'))
    L, A, Z = _ptr(loss), _ptr(acc), _ptr(None)                # (Z: the logits, which no training step asks for)
    tail = (L, A, Z) if kind == 'l1_small' else (L, A, _ptr(ws), nws) if kind == 'l1_big' else (act, L, Z, A, _ptr(ws), nws)
    _head_call(_HEAD_ENTRIES[kind][0], t, *tail)
    ctx.save_for_backward(*t)
    ctx.kind, ctx.act, ctx.nws = kind, act, nws
    return loss


def _pooled_head_bwd(ctx, g):
    """(gp, None, None, dw1, db1, dw2, db2): the gradients of the seven tensor arguments, in ONE pass"""
    t, kind = ctx.saved_tensors, ctx.kind
    p, w1, b1, w2, b2 = t[0], t[3], t[4], t[5], t[6]
    R, nin, nh, dev = int(p.size(0)), int(p.size(1)), int(w1.size(0)), p.device
    gp = torch.empty(R, nin, dtype=torch.float32, device=dev)
    ws, nws = _head_ws(kind, p, w1, ctx.nws)
    g = g.contiguous().float()
    fq = _fold_queue() if kind == 'l1_big' else None
    if fq is not None:                                   # the partials stay in ws; the gradients are views of the flat buffer the fold fills
        npart = nh * nin + 2 * nh + 1
        flat = torch.empty(npart, dtype=torch.float32, device=dev)
        fq.append((ws, nws // npart, npart, [(flat, npart)]))
        dw1, db1 = flat[:nh * nin].view_as(w1), (flat[nh * nin:nh * nin + nh] if b1 is not None else None)
        dw2 = flat[nh * nin + nh:nh * nin + 2 * nh].view_as(w2)
        db2 = flat[nh * nin + 2 * nh:] if b2 is not None else None
        kd = (None,) * 4
    else:
        dw1, db1, dw2, db2 = kd = tuple(torch.empty_like(v) if v is not None else None for v in (w1, b1, w2, b2))
    tail = (_ptr(g), _ptr(gp), nin, _ptr(kd[0]), _ptr(kd[1]), _ptr(kd[2]), _ptr(kd[3])) + ((_ptr(ws), nws) if kind != 'l1_small' else ())
    _head_call(_HEAD_ENTRIES[kind][1], t, *(((ctx.act,) if kind == 'bce' else ()) + tail))
    return gp, None, None, dw1, db1, dw2, db2


class HeadL1Function(torch.autograd.Function):
    """loss = sum_{r < len(y)} valid[r] |fc2(relu(fc1 p[r])) - y[r]| (Zinc12k.py:343-345, :365) as ONE launch forward and ONE launch
    backward (csrc/gml_head.hip) for small batches -- the reference's batch 64.  p [R, nin] pooled rows (R >= len(y): further rows,
    e.g. the padding graph of a static batch, are ignored and get zero gradient).  loss_sum (optional, a float32 scalar on the
    device): += loss inside the same launch -- an epoch's running loss."""

    @staticmethod
    def forward(ctx, p, y, valid, w1, b1, w2, b2, loss_sum=None):
        return _pooled_head_fwd(ctx, 'l1_small', (_f32c(p, 'pooled'), y, valid, w1, b1, w2, b2), 1, loss_sum)

    @staticmethod
    def backward(ctx, g):
        return _pooled_head_bwd(ctx, g) + (None,)


class HeadL1BigFunction(torch.autograd.Function):
    """HeadL1Function for any number of rows (nin = nh = 32; csrc/gml_head_big.hip): one pass + a fold each way instead of the ~16
    launches of the general road (two library GEMMs, relu, the loss's elementwise chain and their backward) at the bench's batch size."""

    @staticmethod
    def forward(ctx, p, y, valid, w1, b1, w2, b2, loss_sum=None):
        return _pooled_head_fwd(ctx, 'l1_big', (_f32c(p, 'pooled'), y, valid, w1, b1, w2, b2), 1, loss_sum)

    @staticmethod
    def backward(ctx, g):
        return _pooled_head_bwd(ctx, g) + (None,)


class HeadBCEFunction(torch.autograd.Function):
    """loss = sum_{r < len(y)} valid[r] BCE(fc2(act(fc1 p[r])), y[r]) on logits (exp_classify.py:293-295 / :260-262, :328-329) as
    ONE pass forward and ONE backward for any number of rows (csrc/gml_head_bce.hip; act: 1 = relu, 0 = identity).  p as above.  stats
    (optional, float32 [3] on the device) accumulates {loss, correct predictions, rows with valid != 0} in the same launch
    (models.accuracy_from_stats)."""

    @staticmethod
    def forward(ctx, p, y, valid, w1, b1, w2, b2, act, stats=None):
        return _pooled_head_fwd(ctx, 'bce', _head_bce_args(p, y, valid, w1, b1, w2, b2, stats), int(bool(act)), stats)

    @staticmethod
    def backward(ctx, g):
        return _pooled_head_bwd(ctx, g) + (None, None)


POOLED_HEADS = dict(l1_small=HeadL1Function, l1_big=HeadL1BigFunction, bce=HeadBCEFunction)     # HeadRoad.kind -> its function


def head_bce_logits(p, y, valid, w1, b1, w2, b2, act):
    """(loss, logits [R]) of the fused BCE head, forward only (inspection and tests; no gradient)"""
    with torch.no_grad():
        t = _head_bce_args(p, y, valid, w1, b1, w2, b2, None)
        ws, nws = _head_ws('bce', t[0], t[3])
        loss = torch.empty((), dtype=torch.float32, device=t[0].device)
        pre = torch.empty(int(t[0].size(0)), dtype=torch.float32, device=t[0].device)
        _head_call('gml_head_bce_fwd', t, int(bool(act)), _ptr(loss), _ptr(pre), _ptr(None), _ptr(ws), nws)
    return loss, pre


def head_bce_supported(p, w1, w2):
    """True when HeadBCEFunction serves these tensors: float32 CUDA tensors on one device, p [R >= 1, nin] with unit column stride
    (any row stride >= nin), fc1 weight [nh, nin] and fc2 weight [1, nh] with 1 <= nin, nh <= 64.  The kernel asks no more than float
    alignment, which every float32 tensor has.  False sends the caller to the torch-op road."""
    if not (all(isinstance(t, torch.Tensor) for t in (p, w1, w2)) and p.dim() == w1.dim() == w2.dim() == 2):
        return False
    return (w1.size(1) == p.size(1) and w2.size(1) == w1.size(0) and p.stride(1) == 1 and p.stride(0) >= p.size(1) and
            head_road('bce', HEAD_MLP32, True, int(p.size(1)), int(w1.size(0)), int(w2.size(0)), int(p.size(0)), 0, 0,
                      *head_flags('bce', p, None, w1, None, w2, None), 'bce').kind == 'bce')


class NodeHeadLossFunction(torch.autograd.Function):
    """(loss, pre) of the node-level readout of filtering.py:268, :320: pre = fc2 x [N, 1] (fc2: nin <= 64 -> 1) and
    loss = sum (mask (pre - y[:, task]))^2 as ONE launch forward and ONE backward (csrc/gml_node_head.hip).  stats (optional, float32
    [4] on the device) receives {loss, ss_res, ss_tot, count} of the rows with mask == 1 in the same launch (models.r2_from_stats).
    No host read either way: capturable.  pre is returned for inspection and carries no gradient."""

    @staticmethod
    def forward(ctx, x, w, b, y, mask, task=0, stats=None):
        x = _f32c(x, 'x')
        N, F = int(x.size(0)), int(x.size(1))
        if w.numel() != F or y.dim() != 2 or y.size(0) != N or mask.numel() != N or not 0 <= task < y.size(1):
            raise ValueError('node head: x %s, fc2 weight %s, y %s, mask %s, task %d' %
                             (tuple(x.shape), tuple(w.shape), tuple(y.shape), tuple(mask.shape), task))
        y, mask = _f32c(y, 'y'), _f32c(mask, 'mask')
        if stats is not None and not (stats.is_cuda and stats.dtype == torch.float32 and stats.numel() >= 4 and stats.is_contiguous()):
            raise ValueError('stats: a contiguous float32 CUDA tensor of 4 elements')
        yt = y[:, task]
        pre = torch.empty(N, 1, dtype=torch.float32, device=x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        w = w.contiguous()
        with torch.cuda.device(x.device):
            with _Timed('node_head'):
                _lib.call('gml_node_head_fwd', _ptr(x), int(x.stride(0)), _ptr(w), _ptr(b), _ptr(yt), int(y.stride(0)), _ptr(mask), 1,
                          N, F, _ptr(pre), _ptr(loss), _ptr(stats), _stream(x.device))
        ctx.save_for_backward(x, w, pre, y, mask)
        ctx.task, ctx.has_b = int(task), b is not None
        ctx.mark_non_differentiable(pre)
        return loss, pre

    @staticmethod
    def backward(ctx, g, _gpre):
        x, w, pre, y, mask = ctx.saved_tensors
        N, F = int(x.size(0)), int(x.size(1))
        dev = x.device
        dx = torch.empty(N, F, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        db = torch.empty(1, dtype=torch.float32, device=dev) if ctx.has_b and ctx.needs_input_grad[2] else None
        g = g.contiguous().float()
        yt = y[:, ctx.task]
        with torch.cuda.device(dev):
            with _Timed('node_head'):
                _lib.call('gml_node_head_bwd', _ptr(g), _ptr(x), int(x.stride(0)), _ptr(w), _ptr(pre), _ptr(yt), int(y.stride(0)),
                          _ptr(mask), 1, N, F, _ptr(dx), F, _ptr(dw), _ptr(db), _stream(dev))
        return dx, dw, db, None, None, None, None


def node_head_supported(x, fc2):
    return head_road('node_sq', None, True, int(x.size(-1)), 0, int(fc2.weight.size(0)), 0, 0, 0,
                     x.dim() == 2 and head_flags('node_sq', x, None, fc2.weight, None, None, None)[0], True, 'node').kind == 'node'


def head_l1_big_supported(p, w1, w2):
    return (p.dim() == 2 and tuple(w1.shape) == (32, 32) and tuple(w2.shape) == (1, 32) and
            head_road('l1', HEAD_MLP32, True, int(p.size(1)), 32, 1, int(p.size(0)), 0, 0, p.is_cuda and p.dtype == torch.float32, True, 'l1_big').kind == 'l1_big')


def head_l1_supported(p, w1, w2):
    return head_road('l1', HEAD_MLP32, True, int(p.size(1)), int(w1.size(0)), int(w2.size(0)), int(p.size(0)), 0, 0,
                     p.is_cuda and p.dtype == torch.float32).kind == 'l1_small'


def tall_linear(x, lin):
    return TallLinearFunction.apply(x, lin.weight, lin.bias)


def _ptr32(ptr):
    """segment pointers as the kernels read them: int32, contiguous (a PyG-style int64 ``ptr`` is converted)."""
    if ptr.dtype != torch.int32:
        if ptr.dtype not in (torch.int64, torch.int16, torch.uint8):
            raise TypeError('ptr must be an integer tensor, got %s' % ptr.dtype)
        ptr = ptr.to(torch.int32)
    return ptr.contiguous()


def segment_bcast(g, ptr, nrows, mean=False):
    """gradient of segment_sum: row r of segment s receives g[s] (divided by the segment length for the mean)."""
    ptr = _ptr32(ptr)
    B, F = int(ptr.numel() - 1), int(g.size(1))
    out = torch.empty(nrows, F, dtype=torch.float32, device=g.device)
    with _Timed('pool'):
        _lib.call('gml_segment_bcast', _ptr(g), int(g.stride(0)), _ptr(ptr), _ptr(out), F, B, F, 1 if mean else 0,
                  _stream(g.device))
    return out


_SKIP_LAST_MASK = {}


def skip_last_mask(g):
    """[B, 1] ones with a zero in the last row (cached per (B, device)): the pooled gradient of a batch whose last segment is
    the padding graph of a static-shape batch (GML_POOL_SKIP_LAST) -- the forward writes that row as zeros WITHOUT reading the
    padding nodes, so nothing may flow back to them whatever the head or the loss does with the row."""
    key = (int(g.size(0)), g.device)
    m = _SKIP_LAST_MASK.get(key)
    if m is None:
        m = torch.ones(g.size(0), 1, dtype=g.dtype, device=g.device)
        m[-1] = 0
        _SKIP_LAST_MASK[key] = m
    return m


def segment_sum(x, ptr, mean=False):
    """global_add_pool / global_mean_pool over a batch whose nodes are grouped per graph (ptr [B+1] int32).  mean: bool, or the
    flag word of gml_segment_sum (bit 0 mean, bit 1 = _lib.GML_POOL_SKIP_LAST: the last segment is the padding graph of a
    static-shape batch, its row is written as zeros)."""
    ptr = _ptr32(ptr)
    B, F = int(ptr.numel() - 1), int(x.size(1))
    out = torch.empty(B, F, dtype=torch.float32, device=x.device)
    with _Timed('pool'):
        _lib.call('gml_segment_sum', _ptr(x), int(x.stride(0)), _ptr(ptr), _ptr(out), F, B, F, int(mean),
                  _stream(x.device))
    return out


def segment_sum_mask(x, ptr, mean=False):
    """segment_sum for 32-column rows + the relu pattern of every row (uint32 per row as int32 [N]: bit c = x[row][c] > 0)."""
    ptr = _ptr32(ptr)
    B, F = int(ptr.numel() - 1), int(x.size(1))
    out = torch.empty(B, F, dtype=torch.float32, device=x.device)
    mask = torch.empty(int(x.size(0)), dtype=torch.int32, device=x.device)
    with _Timed('pool'):
        _lib.call('gml_segment_sum_mask', _ptr(x), int(x.stride(0)), _ptr(ptr), _ptr(out), F, _ptr(mask), B, F, int(mean), _stream(x.device))
    return out, mask


def segment_bcast_mask(g, seg, mask, nrelu):
    """the pool's gradient per row with the relu pattern applied: out[row, c] = g[seg[row], c] * (c >= nrelu or bit c of mask[row])."""
    N = int(seg.numel())
    out = torch.empty(N, 32, dtype=torch.float32, device=g.device)
    with _Timed('pool'):
        _lib.call('gml_segment_bcast_mask', _ptr(g), int(g.stride(0)), _ptr(seg), _ptr(mask), _ptr(out), 32, N, 32, int(nrelu), _stream(g.device))
    return out


def segment_max(x, ptr):
    """global_max_pool over a batch whose nodes are grouped per graph: (max [B, F], argmax rows [B, F] int32)."""
    ptr = _ptr32(ptr)
    B, F = int(ptr.numel() - 1), int(x.size(1))
    out = torch.empty(B, F, dtype=torch.float32, device=x.device)
    arg = torch.empty(B, F, dtype=torch.int32, device=x.device)
    with _Timed('pool'):
        _lib.call('gml_segment_max', _ptr(x), int(x.stride(0)), _ptr(ptr), _ptr(out), F, _ptr(arg), B, F, _stream(x.device))
    return out, arg


def segment_max_bwd(g, ptr, arg, nrows):
    ptr = _ptr32(ptr)
    B, F = int(ptr.numel() - 1), int(g.size(1))
    out = torch.empty(nrows, F, dtype=torch.float32, device=g.device)
    with _Timed('pool'):
        _lib.call('gml_segment_max_bwd', _ptr(g), int(g.stride(0)), _ptr(ptr), _ptr(arg), _ptr(out), F, B, F, _stream(g.device))
    return out


# ---------------------------------------------------------------------------- dropout (csrc/gml_dropout.hip)
# The mask is a pure function of (seed, counter, site, element index): Philox4x32-10 keyed by the seed (include/gml.h).  The RNG
# state is an int64 [2] = {seed, counter} CUDA tensor the kernel reads on the device; advancing the counter is a plain
# `state[1:].add_(1)`, so a captured step draws fresh masks on every replay, the same ones the step would draw eagerly.

def dropout_threshold(p):
    """(t, scale) of the keep rule u >= t for a drop probability p: t = floor(p 2^32) in float64 (2^32 for p = 1: nothing is
    kept), scale = 1 / (1 - p) (0 for p = 1), rounded to float32 once where the kernel takes it.  ValueError outside [0, 1]."""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError('dropout probability has to be between 0 and 1, but got %s' % p)
    if p == 1.0:
        return 1 << 32, 0.0
    import math
    return int(math.floor(p * 4294967296.0)), 1.0 / (1.0 - p)


def dropout_state(seed, device):
    """int64 [2] = {seed, counter 0} on `device`: the RNG state dropout() reads.  seed: any integer, taken modulo 2^64."""
    seed = int(seed) & 0xffffffffffffffff
    if seed >= 1 << 63:
        seed -= 1 << 64
    return torch.tensor([seed, 0], dtype=torch.int64, device=device)


def _dropout_rows(x, name):
    _require_cuda(x, name)
    if x.dtype != torch.float32 or x.dim() != 2:
        raise TypeError('%s must be a float32 [N, C] tensor, got %s %s' % (name, x.dtype, tuple(x.shape)))
    return x if (x.stride(1) == 1 and x.stride(0) >= x.size(1)) else x.contiguous()


def dropout_fwd(x, p, state, site=0):
    """(y, mask) of one dropout launch: y [N, C] float32 (rows padded to a multiple of 4 floats: what the layers read without a
    copy), mask uint32 packed keep bits as int32 [ceil(N C / 32)] (bit e & 31 of word e >> 5)."""
    x = _dropout_rows(x, 'x')
    t, scale = dropout_threshold(p)
    if not (isinstance(state, torch.Tensor) and state.is_cuda and state.dtype == torch.int64 and state.numel() == 2
            and state.is_contiguous() and state.device == x.device):
        raise TypeError('state must be a contiguous int64 [2] CUDA tensor on the device of x (functional.dropout_state)')
    N, C = int(x.size(0)), int(x.size(1))
    dev = x.device
    with torch.cuda.device(dev):
        buf = torch.empty(N, (C + 3) // 4 * 4, dtype=torch.float32, device=dev)
        mask = torch.empty((N * C + 31) // 32, dtype=torch.int32, device=dev)
        with _Timed('dropout_fwd', 8 * N * C + (N * C) // 8 if PROFILE is not None else 0):
            _lib.call('gml_dropout_fwd', _ptr(x), int(x.stride(0)), _ptr(buf), int(buf.stride(0)), _ptr(mask), N, C,
                      ctypes.c_uint64(t), ctypes.c_float(scale), _ptr(state), ctypes.c_uint32(int(site) & 0xffffffff), _stream(dev))
    return buf[:, :C], mask


def dropout_bwd(g, mask, p):
    """dx = keep ? g * scale : +0.0 from a mask of dropout_fwd (same p)."""
    g = _dropout_rows(g, 'grad_output')
    _, scale = dropout_threshold(p)
    N, C = int(g.size(0)), int(g.size(1))
    dev = g.device
    with torch.cuda.device(dev):
        buf = torch.empty(N, (C + 3) // 4 * 4, dtype=torch.float32, device=dev)
        with _Timed('dropout_bwd', 8 * N * C + (N * C) // 8 if PROFILE is not None else 0):
            _lib.call('gml_dropout_bwd', _ptr(g), int(g.stride(0)), _ptr(mask), _ptr(buf), int(buf.stride(0)), N, C,
                      ctypes.c_float(scale), _stream(dev))
    return buf[:, :C]


class DropoutFunction(torch.autograd.Function):
    """F.dropout(x, p, training=True) on csrc/gml_dropout.hip: the backward applies the mask the forward saved, so a later
    change of the RNG state does not affect it."""

    @staticmethod
    def forward(ctx, x, p, state, site=0):
        y, mask = dropout_fwd(x, p, state, site)
        ctx.save_for_backward(mask)
        ctx.p = p
        return y

    @staticmethod
    def backward(ctx, g):
        mask, = ctx.saved_tensors
        return dropout_bwd(g, mask, ctx.p), None, None, None


def dropout(x, p, training, state, site=0):
    """F.dropout(x, p, training) with the device RNG state `state` (dropout_state) and `site` (which dropout of the model: part
    of the Philox counter).  Not training, or p == 0: x itself, nothing launched.  Otherwise a new tensor (never in place)."""
    dropout_threshold(p)                                   # ValueError outside [0, 1], in eval mode too (as torch)
    if not training or p == 0:
        return x
    return DropoutFunction.apply(x, float(p), state, int(site))


# one fused conv-backward launch as the library plans it: kernel flags, group records and their maxima, dW workspace, rows per group
ConvBwdPlan = _collections.namedtuple('ConvBwdPlan', 'flags ginfo max_edges max_window ws_bytes rows')
# which road a conv backward takes: kind 'one128' / 'one64' (one launch of the 128- / 64-row kernel), 'split48' (two launches over the
# feature slices [0, 32) and [32, Fin)) or 'unfused'; plan: the whole shape's plan or None; halves: the two slices' plans (split48)
ConvBwdRoad = _collections.namedtuple('ConvBwdRoad', 'kind plan halves')


def _bwd_plan(csr, S, Fin, Fout, exact=None):
    """ConvBwdPlan of the fused backward for this shape (exact: on exact f32 products; None = as this thread runs), or None."""
    L = _lib.lib()
    for flags in ((_lib.GML_F32_MFMA,) if (exact_mode() if exact is None else exact) else (0, _lib.GML_F32_MFMA)):
        rows = int(L.gml_spectconv_bwd_group_rows(int(S), int(Fin), int(Fout), flags))
        if rows == 0:
            continue
        if rows == 128:
            ginfo, gmax = csr.ginfo_t128, csr.gmax_t128
        else:
            ginfo, gmax = csr.ginfo_t, csr.gmax_t
        nbytes = int(L.gml_spectconv_bwd_workspace_bytes(csr.N, int(S), int(Fin), int(Fout), gmax[0], gmax[1], flags))
        if nbytes > 0:
            return ConvBwdPlan(flags, ginfo, gmax[0], gmax[1], nbytes, rows)
    return None


# 48-wide layers (sr25.py:252-262, mutag.py:272-288: hidden width 32 + 16 / 24 + 24) run as ONE launch of the 8-wave bf16x3 kernel where
# the library has that shape (round 5: S = 4, 6; GML_BWD_WIDE48=0 turns it off), else as two launches over the feature slices: dX and dW
# split by input feature; dval is linear in x, so the second launch adds its share (GML_DVAL_ACCUM).  The edge loop runs twice -- still
# ~2 x faster than the 64-row f32-MFMA kernel these layers ran on (tools/bench_configs.py).
def _conv_bwd_road(csr, S, Fin, Fout, exact, x_rows4=True, wants_handover=False):
    """ConvBwdRoad of this shape; the slices need float4-readable x rows (x_rows4) and carry no hand-over (mix / relu_cols / had)."""
    bf16x3 = lambda p: p is not None and p.rows == 128 and not p.flags & _lib.GML_F32_MFMA
    plan = _bwd_plan(csr, S, Fin, Fout, exact)
    if (32 < Fin <= 48 and not exact and not bf16x3(plan) and not wants_handover and x_rows4 and (Fin - 32) % 4 == 0
            and not (S == 8 and Fout > 16)):                  # (S = 8, 32 columns: no dval += in that kernel)
        halves = _bwd_plan(csr, S, 32, Fout, exact), _bwd_plan(csr, S, Fin - 32, Fout, exact)
        if bf16x3(halves[0]) and bf16x3(halves[1]):
            return ConvBwdRoad('split48', plan, halves)
    return ConvBwdRoad('unfused' if plan is None else 'one%d' % plan.rows, plan, None)


def fused_bwd_available(csr, S, Fin, Fout):
    return _bwd_plan(csr, S, Fin, Fout) is not None


def _plan_takes_dz(plan, S, Fin, Fout, nmix):
    return plan is not None and 1 <= nmix <= 4 and bool(_lib.lib().gml_spectconv_bwd_mix_supported(int(S), int(Fin), int(Fout), int(nmix), plan.flags))


def conv_bwd_takes_dz(csr, S, Fin, Fout, nmix):
    """True when the fused backward of this shape can form  dx = conv part + dz wmix  itself (gml_spectconv_bwd_mix)."""
    return _plan_takes_dz(_bwd_plan(csr, S, Fin, Fout), S, Fin, Fout, nmix)


BWD_DMA = _os.environ.get('GML_BWD_DMA') == '1'     # fused backward on the LDS-DMA ring kernel (bwd4) where it applies; A/B switch
BWD_HAD = _os.environ.get('GML_BWD_HAD', '1') != '0'  # ML3Layer output stage inside the conv backward (gml_spectconv_bwd_had); A/B switch


# rows a kernel may read as float4: leading dimension a multiple of 4 floats that holds `cols`, base aligned to 16 bytes; _rows_of:
# (row stride, pointer % 16) of a [n, c] tensor -- a column stride other than 1 never passes
def _rows4_ok(stride, ptr16, cols):
    return stride % 4 == 0 and stride >= (cols + 3) // 4 * 4 and ptr16 == 0


def _rows_of(t):
    return (int(t.stride(0)), t.data_ptr() % 16) if t.stride(1) == 1 else (0, 1)


def _g_rows4(G, N, Fout):
    """G as the 8-wave kernel reads its window (float4): itself, or a copy with rows padded (with zeros) to a multiple of 4 floats"""
    if _rows4_ok(*_rows_of(G), Fout):
        return G
    Gp = torch.zeros(N, (Fout + 3) // 4 * 4, dtype=torch.float32, device=G.device)
    Gp[:, :Fout] = G
    return Gp[:, :Fout]


def _conv_bwd_call(entry, csr, plan, flags, val_t, x, G, weight, dx, dval_t, dw, ws, own=(), f2=(), own_ws=(), col0=0, lddx=None):
    """one gml_spectconv_bwd* launch: the arguments every entry point shares, around the entry's `own` ones (f2 / own_ws: the had
    form's F2 and partial rows).  col0: first of the weight's input features inside the rows of x and dx (leading dimension lddx)."""
    S, Fin, Fout = weight.shape
    _lib.call(entry, _ptr(csr.rowptr_t), _ptr(csr.col_t), _ptr(plan.ginfo), _ptr(val_t), _off(x, col0), int(x.stride(0)), _ptr(G),
              int(G.stride(0)), _ptr(weight), _off(dx, col0) if dx is not None else _ptr(None), lddx or Fin, _ptr(dval_t), _ptr(dw), *own,
              csr.N, S, Fin, Fout, *f2, plan.max_edges, plan.max_window, flags, _ptr(ws), ws.numel() if ws is not None else 0, *own_ws,
              _stream(x.device))


def fused_conv_bwd(csr, plan, val_t, x, G, weight, need_x, need_val, need_w, dx_accum_into=None, mix=None, relu_cols=0, had=None):
    """one launch: dX, dval (source order), dW.  val_t: supports in source order.  mix = (dz [N, 4], wmix [nmix, Fin]):
    dX = conv part + dz wmix (instead of accumulating into a dx another kernel wrote).  relu_cols (with mix): dX[:, f] for
    f < relu_cols is written multiplied by (x[:, f] > 0) (gml_spectconv_bwd_mix_relu: the relu of the ML3Layer below).
    had = {'w': (w11, b11, w12, b12), 'parts': rows}: the ML3Layer output stage inside the launch (gml_spectconv_bwd_had; G is then a
    view of the pre-masked [N, >= Fout + 2] gradient whose columns Fout, Fout + 1 are the Hadamard units'); had['out'] receives
    (dcb, dw11, db11, dw12, db12)."""
    S, Fin, Fout = weight.shape
    dev = x.device
    assert plan.rows == 128 or (mix is None and relu_cols == 0 and had is None), 'the hand-overs ride on the one-launch 128-row backward'
    flags, nbytes = plan.flags | (_lib.GML_DMA_RING if BWD_DMA else 0), plan.ws_bytes
    G = _g_rows4(G, csr.N, Fout)
    ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev) if need_w else None
    if need_x and dx_accum_into is not None:                 # dx already holds another branch's contribution
        dx, flags = dx_accum_into, flags | _lib.GML_ACCUM
    else:
        dx = torch.empty(csr.N, Fin, dtype=torch.float32, device=dev) if need_x else None
    dval_t = torch.empty(csr.E, S, dtype=torch.float32, device=dev) if need_val else None
    dw = torch.empty(S, Fin, Fout, dtype=torch.float32, device=dev) if need_w else None
    q, f = conv_cost_bwd(csr.N, csr.E, S, Fin, Fout, need_x, need_val) if PROFILE is not None else (0, 0)
    fq = _fold_queue() if need_w else None
    if fq is not None:                                       # the dW partials stay in ws; one launch folds every layer's at scope exit
        flags |= _lib.GML_NO_FOLD
        flat = torch.empty(S * Fin * Fout, dtype=torch.float32, device=dev)       # (a view of it goes to autograd: see edge_mlp_bwd)
        fq.append((ws, nbytes // (4 * S * Fin * Fout), S * Fin * Fout, [(flat, flat.numel())]))
    if had is not None:
        w11, b11, w12, b12 = had['w']
        npart, parts = 4 * Fin + 4 + Fout, int(had['parts'])
        hws = torch.empty(parts * npart, dtype=torch.float32, device=dev)
        hfq = _fold_queue()
        if hfq is not None:                                  # (same layout as gml_ml3_split_bwd's partial rows: same fold job)
            hflat = torch.empty(npart, dtype=torch.float32, device=dev)
            hfq.append((hws, parts, npart, [(hflat, npart)]))
            dw11, dw12 = hflat[:2 * Fin].view_as(w11), hflat[2 * Fin:4 * Fin].view_as(w12)
            db11 = hflat[4 * Fin:4 * Fin + 2] if b11 is not None else None
            db12 = hflat[4 * Fin + 2:4 * Fin + 4] if b12 is not None else None
            dcb = hflat[4 * Fin + 4:]
            kd = (None,) * 5
        else:
            dw11, dw12 = torch.empty_like(w11), torch.empty_like(w12)
            db11 = torch.empty_like(b11) if b11 is not None else None
            db12 = torch.empty_like(b12) if b12 is not None else None
            dcb = torch.empty(Fout, dtype=torch.float32, device=dev)
            kd = (dcb, dw11, db11, dw12, db12)
        had['out'] = (dcb, dw11, db11, dw12, db12)
        with _Timed('spectconv_bwd', q + 8 * csr.N, f):        # (+ the own rows' two Hadamard columns; the rest it reads anyway)
            _conv_bwd_call('gml_spectconv_bwd_had', csr, plan, flags, val_t, x, G, weight, dx, dval_t, dw, ws,
                           (_ptr(w11), _ptr(b11), _ptr(w12), _ptr(b12), int(relu_cols)) + tuple(_ptr(t) for t in kd), (2,),
                           (_ptr(hws), hws.numel() * 4))
    elif mix is not None:
        dz, wmix = mix
        with _Timed('spectconv_bwd', q, f):
            if isinstance(wmix, tuple):                      # (fc11.weight, fc12.weight) as they are stored: no concatenation launch
                wa, wb = wmix
                _conv_bwd_call('gml_spectconv_bwd_mix_relu2', csr, plan, flags, val_t, x, G, weight, dx, dval_t, dw, ws,
                               (_ptr(dz), _ptr(wa), int(wa.size(0)), _ptr(wb), int(wb.size(0)), int(relu_cols)))
            else:
                _conv_bwd_call('gml_spectconv_bwd_mix_relu', csr, plan, flags, val_t, x, G, weight, dx, dval_t, dw, ws,
                               (_ptr(dz), _ptr(wmix), int(wmix.size(0)), int(relu_cols)))
    else:
        assert relu_cols == 0, 'the relu hand-over rides on the dz form of the backward'
        with _Timed('spectconv_bwd', q, f):
            _conv_bwd_call('gml_spectconv_bwd', csr, plan, flags, val_t, x, G, weight, dx, dval_t, dw, ws)
    if fq is not None:
        dw = flat.view(S, Fin, Fout)
    return dx, dval_t, dw


def fused_conv_bwd_split48(csr, plans, val_t, x, G, weight, need_x, need_val, need_w, dx_accum_into=None):
    """two launches of the 8-wave kernel over the feature slices [0, 32) and [32, Fin) (_conv_bwd_road); plans: one per slice"""
    S, Fin, Fout = weight.shape
    dev = x.device
    G = _g_rows4(G, csr.N, Fout)
    dx = dx_accum_into if (need_x and dx_accum_into is not None) else (torch.empty(csr.N, Fin, dtype=torch.float32, device=dev) if need_x else None)
    dval_t = torch.empty(csr.E, S, dtype=torch.float32, device=dev) if need_val else None
    dws = []
    q, f = conv_cost_bwd(csr.N, csr.E, S, Fin, Fout, need_x, need_val) if PROFILE is not None else (0, 0)
    with _Timed('spectconv_bwd', q, f):
        for part, (f0, f1) in enumerate(((0, 32), (32, Fin))):
            flags = plans[part].flags
            if need_x and dx_accum_into is not None:
                flags |= _lib.GML_ACCUM
            if part == 1 and need_val:
                flags |= _lib.GML_DVAL_ACCUM
            w_p = weight[:, f0:f1, :].contiguous()
            dw_p = torch.empty(S, f1 - f0, Fout, dtype=torch.float32, device=dev) if need_w else None
            ws = torch.empty(max(plans[part].ws_bytes, 4), dtype=torch.uint8, device=dev) if need_w else None
            _conv_bwd_call('gml_spectconv_bwd', csr, plans[part], flags, val_t, x, G, w_p, dx, dval_t, dw_p, ws, col0=f0, lddx=Fin)
            dws.append(dw_p)
    dw = torch.cat(dws, 1) if need_w else None
    return dx, dval_t, dw


# ---------------------------------------------------------------------------- shared backward pieces
def _conv_backward(csr, x, val, weight, G, need_x, need_val, need_w, val_t=None, want_source_order=False,
                   dx_accum_into=None, mix=None, relu_cols=0, had=None, road=None):
    """G [N,Fout] contiguous = gradient at the (pre-activation) conv output.
    Returns dx, dval, dw; dval is in source order when want_source_order (and the fused kernel ran).
    dx_accum_into: [N,Fin] buffer that already holds a partial dx; the conv contribution is added to it.
    road: the caller's _conv_bwd_road of this shape (decided here otherwise); mix / relu_cols / had: see fused_conv_bwd."""
    S, Fin, Fout = weight.shape
    N = csr.N
    dx = dval = dw = None
    if G.stride(1) != 1:
        G = G.contiguous()
    handover = mix is not None or relu_cols != 0 or had is not None
    if road is None:
        road = _conv_bwd_road(csr, S, Fin, Fout, exact_mode(), _rows4_ok(*_rows_of(x), Fin), handover)
    assert road.kind == 'one128' or not handover, 'the dz, relu and output-stage hand-overs ride on the one-launch 128-row backward'
    if road.kind != 'unfused':
        if val_t is None:
            with _Timed('val_to_source_order'):
                val_t = csr.to_source_order(val)
        if road.kind == 'split48':
            _path('conv_bwd', 'fused (group kind 128), two launches over the feature slices [0, 32) and [32, %d)' % Fin, S, Fin, Fout)
            dx, dval_t, dw = fused_conv_bwd_split48(csr, road.halves, val_t, x, G, weight, need_x, need_val, need_w, dx_accum_into)
        else:
            _path('conv_bwd', 'fused (group kind %d)' % road.plan.rows, S, Fin, Fout)
            dx, dval_t, dw = fused_conv_bwd(csr, road.plan, val_t, x, G, weight, need_x, need_val, need_w, dx_accum_into, mix, relu_cols, had)
        if need_val and not want_source_order:
            with _Timed('dval_from_source_order'):
                dval_t = csr.from_source_order(dval_t)
        return dx, dval_t, dw, (want_source_order and need_val)
    _path('conv_bwd', 'UNFUSED composition (transposed forward + SpMM + SDDMM + GEMMs)', S, Fin, Fout)
    if not G.is_contiguous():
        G = G.contiguous()
    if need_x:
        dx = dx_accum_into if dx_accum_into is not None else torch.empty(N, Fin, dtype=torch.float32, device=x.device)
        # dX = sum_s A_s (G W_s^T): rows keyed by SOURCE, features = G, weight element (s, o, f) = W[s, f, o]
        if val_t is None:
            with _Timed('val_to_source_order'):
                val_t = csr.to_source_order(val)
        fused_conv(csr.rowptr_t, csr.col_t, csr.ginfo_t, None, val_t, G, Fout, weight, (Fin * Fout, 1, Fout), None,
                   dx, Fin, N, S, Fout, Fin, _lib.GML_ACCUM if dx_accum_into is not None else 0, tag='spectconv_dx')
    if need_w:
        with _Timed('dw_spmm'):
            h = spmm(csr, val, x, S, Fin)                                # [N, S*Fin]
        with _Timed('dw_gemm'):
            dw = torch.mm(h.t(), G).view(S, Fin, Fout)
    if need_val:
        with _Timed('dval_gemm'):
            gw = torch.mm(G, weight.view(S * Fin, Fout).t())             # [N, S*Fin]
        with _Timed('dval_sddmm'):
            dval = sddmm(csr, x, gw, S, Fin)
    return dx, dval, dw, False


class SpectConvFunction(torch.autograd.Function):
    """out = act( sum_s (A_s^T x) W_s + bias ),  val = supports in target-sorted order."""

    @staticmethod
    def forward(ctx, x, val, weight, bias, csr, relu):
        x, val, weight = _f32rows(x, 'x'), _f32c(val, 'edge_attr'), _f32c(weight, 'weight')
        S, Fin, Fout = weight.shape
        if x.size(1) != Fin or val.size(1) < S or val.size(0) != csr.E or x.size(0) != csr.N:
            raise ValueError('shape mismatch: x %s, edge_attr %s, weight %s, graph N=%d E=%d'
                             % (tuple(x.shape), tuple(val.shape), tuple(weight.shape), csr.N, csr.E))
        if val.size(1) != S:
            val = val[:, :S].contiguous()
        if bias is not None:
            bias = _f32c(bias, 'bias')
        with torch.cuda.device(x.device):
            out = torch.empty(csr.N, Fout, dtype=torch.float32, device=x.device)
            x = rows4(x)
            gi, gflag = fwd_groups(csr, x, S, Fin, Fout)
            fused_conv(csr.rowptr, csr.col, gi, None, val, x, int(x.stride(0)), weight, (Fin * Fout, Fout, 1), bias, out,
                       Fout, csr.N, S, Fin, Fout, (_lib.GML_RELU if relu else 0) | gflag)
        ctx.csr, ctx.relu, ctx.has_bias = csr, relu, bias is not None
        ctx.exact = bool(exact_mode())
        ctx.save_for_backward(x, val, weight, out if relu else None)
        return out

    @staticmethod
    def backward(ctx, gout):
        with exact_products(_bwd_exact(ctx)):
            return SpectConvFunction._backward(ctx, gout)

    @staticmethod
    def _backward(ctx, gout):
        x, val, weight, out = ctx.saved_tensors
        csr = ctx.csr
        gout = _f32c(gout, 'grad_out')
        with torch.cuda.device(x.device):
            Fout = weight.size(2)
            need = ctx.needs_input_grad
            want_db = ctx.has_bias and need[3]
            db = None
            r = ml3_split_bwd(gout, out, Fout, need_dcb=want_db) if ctx.relu else None
            if r is not None:
                G, db = r[0], r[2]
            else:
                G = relu_bwd(gout, 0, Fout, out, Fout, csr.N, Fout) if ctx.relu else gout
            dx, dval, dw, _ = _conv_backward(csr, x, val, weight, G, need[0], need[1], need[2])
            if want_db and db is None:
                db = G.sum(0)
        return dx, dval, dw, db, None, None


class ChainToken(object):
    """Hand-over between two stacked ML3Layers (Zinc12k.py:338-341: x = conv2(conv1(x, ...), ...)): the upper layer's conv
    backward holds the rows of x = [relu(conv) | Hadamard columns] of the lower layer anyway, so it writes dx already
    multiplied by that relu's mask (`premasked`), and the lower layer's output-stage backward then neither reads its saved
    output nor writes a second [N, C] array.  Valid only when the upper layer is the ONLY consumer of that tensor --
    ML3Layer.chain_after() is how a model says so.  cols: relu columns of the lower layer's output (nout1)."""
    __slots__ = ('cols', 'premasked')

    def __init__(self, cols):
        self.cols, self.premasked = int(cols), False


CHAIN = not _os.environ.get('GML_NO_CHAIN')      # A/B switch for the relu hand-over between stacked ML3Layers


# ZINC's 30 + 2 top layer: the pool also leaves the relu pattern of every row (4 bytes) and the backward expands the pool's gradient with
# it -- the layer then runs pre-masked like the ones below it, output stage inside the conv backward, instead of reading its saved output.
def _pool_relu_pattern(bwd_had, mixk, nout1, nout2, exact, wanted, gy_rows4=True, conv_takes=True):
    """ONE predicate for both sides: the forward asks with what it knows (wanted: any gradient at all; inference pools plainly), the
    backward adds the gradients the had form writes, the pooled gradient's rows and what the conv plan takes."""
    return bool(bwd_had and mixk and nout1 == 30 and nout2 == 2 and not exact and wanted and gy_rows4 and conv_takes)


# How one ML3Layer backward runs (decided once, by _ml3_bwd_road; DESIGN s4.4 has the table):
#   pool_grad   None (no pool) / 'expanded' (segment_bcast) / 'per_segment' (gy_seg: never expanded) / 'masked' (segment_bcast_mask)
#   stage       'had' (inside the conv backward: parts, want_dx) / 'one_pass' (ml3_split_bwd: premasked, dz_out, mixk = it carries the
#               Hadamard branch) / 'separate' (relu_bwd + gml_node_mix_bwd)
#   lib_hadamard  the wide Hadamard branch runs as library GEMMs;  use_dz / relu_cols: the dz and relu hand-overs of the conv backward;
#   conv_accum  the conv backward adds to the dx the output stage wrote;  conv: its ConvBwdRoad
ML3BwdRoad = _collections.namedtuple('ML3BwdRoad', 'pool_grad stage parts want_dx premasked dz_out mixk lib_hadamard use_dz relu_cols '
                                                   'conv_accum need_val want_cw want_cb learnedge conv')


def _ml3_bwd_road(S, Fin, nout1, nout2, N, need, learnedge, has_cb, conv, exact, bwd_had, bwd_dma, chain, pool, pool_mask,
                  chain_out_premasked, chain_in_cols, gy_rows, x_rows4):
    """ML3BwdRoad from plain values only (no tensor, no launch).  Every hand-over (dz, relu_cols, had) rides on the one-launch 128-row
    conv backward: without that plan none is chosen."""
    # need: needs_input_grad of ML3LayerFunction; conv: _conv_bwd_road of (S, Fin, nout1); pool / pool_mask: the layer is pooled / its
    # forward left the relu pattern; chain_out_premasked: the consumer applied this layer's relu to gy; chain_in_cols: relu columns of x's
    # producer (None: no hand-over); gy_rows: (row stride, pointer % 16) of the incoming gradient; x_rows4: x has float4-readable rows
    L = _lib.lib()
    C = nout1 + nout2
    mixk = nout2 > 0 and node_mix_native(Fin, nout2)
    plan = conv.plan if conv.kind == 'one128' else None
    want_dx, want_w3 = bool(need[0]), bool(need[6] and need[8] and need[10])
    stage_ws = int(L.gml_ml3_split_bwd_workspace_bytes(int(N), Fin if mixk else 0, int(nout1), int(nout2) if mixk else 0))
    # 2 nout2 <= 4 (Zinc12k.py's 30+2 layers): the Hadamard branch hands its share of dx to the conv backward as 4 numbers per row (dz)
    # instead of writing a [N, Fin] array the conv kernel reads back
    use_dz = bool(mixk and want_dx and not _os.environ.get('GML_NO_DZ') and _plan_takes_dz(plan, S, Fin, nout1, 2 * nout2))
    # partial rows of gml_spectconv_bwd_had (0: the shape / the build has no fused output stage)
    parts = 0 if (not bwd_had or bwd_dma or exact or plan is None) else int(L.gml_spectconv_bwd_had_parts(
        int(N), int(S), int(Fin), int(nout1), int(nout2), int(want_dx), plan.max_edges, plan.max_window, plan.flags))
    pool_grad, pre = None, bool(chain and chain_out_premasked)
    if pool:
        fuse = stage_ws > 0 and (mixk or nout2 == 0) and not _os.environ.get('GML_NO_POOL_FUSE')
        pre = bool(fuse and pool_mask and _pool_relu_pattern(bwd_had, mixk, nout1, nout2, exact, want_dx and want_w3,
                                                             _rows4_ok(*gy_rows, 0), use_dz and parts > 0))
        pool_grad = 'masked' if pre else 'per_segment' if fuse else 'expanded'
        if pool_grad != 'per_segment':
            gy_rows = (C, 0)          # (the expanded gradient is a fresh [N, C] array)
    # ZINC's 30 + 2 layers with a pre-masked gradient: the output stage runs INSIDE the conv backward (one launch, no dz array, no second
    # pass over gy and x)
    had = bool(parts > 0 and (use_dz or (mixk and not want_dx and x_rows4)) and pre and nout2 == 2 and want_w3 and _rows4_ok(*gy_rows, C))
    stage = 'had' if had else 'one_pass' if (stage_ws > 0 or N == 0) else 'separate'
    use_dz = use_dz and stage == 'one_pass'
    # x is the lower ML3Layer's output and only this layer consumes it: its relu mask goes back inside dx
    relu_cols = chain_in_cols if (((had and want_dx) or use_dz) and chain and chain_in_cols is not None and not bwd_dma) else 0
    return ML3BwdRoad(pool_grad, stage, parts if had else 0, want_dx, stage == 'one_pass' and pre and _rows4_ok(*gy_rows, nout1), use_dz,
                      mixk, nout2 > 0 and not mixk, use_dz, relu_cols, bool(stage == 'one_pass' and mixk and want_dx and not use_dz),
                      bool(need[1] or (learnedge and any(need[2:6]))), bool(need[6]), bool(has_cb and need[7]), bool(learnedge), conv)


# The three output-stage forms of the ML3Layer backward: each fills g[7 .. 11] (conv1.bias, fc11 / fc12 weight and bias gradients) and
# returns what its _conv_backward call returns.  fc = (w11, b11, w12, b12).
def _ml3_stage_had(road, csr, g, gy, gy_seg, out, x, ea, ea_t, cw, fc):
    had = {'w': fc, 'parts': road.parts}
    r = _conv_backward(csr, x, ea, cw, gy[:, :cw.size(2)], road.want_dx, road.need_val, True, val_t=ea_t,
                       want_source_order=road.learnedge, relu_cols=road.relu_cols, had=had, road=road.conv)
    dcb, g[8], g[9], g[10], g[11] = had['out']
    g[7] = dcb if road.want_cb else None
    return r


def _ml3_stage_one_pass(road, csr, g, gy, gy_seg, out, x, ea, ea_t, cw, fc):
    # one pass: relu mask, conv1.bias gradient, Hadamard branch (its dx or dz written; the conv adds to the dx / takes the dz)
    G, dx0, g[7], g[8], g[9], g[10], g[11] = ml3_split_bwd(gy, out, cw.size(2), *((x,) + fc if road.mixk else ()), need_dx=road.want_dx,
                                                           need_dcb=road.want_cb, dz_out=road.dz_out, gy_seg=gy_seg, premasked=road.premasked)
    mix = (dx0, (fc[0].detach().contiguous(), fc[2].detach().contiguous())) if road.use_dz else None    # (rows of wmix from both arrays)
    return _conv_backward(csr, x, ea, cw, G, road.want_dx, road.need_val, road.want_cw, val_t=ea_t, want_source_order=road.learnedge,
                          dx_accum_into=dx0 if road.conv_accum else None, mix=mix, relu_cols=road.relu_cols, road=road.conv)


def _ml3_stage_separate(road, csr, g, gy, gy_seg, out, x, ea, ea_t, cw, fc):
    assert gy_seg is None, 'pooled gradient without the one-pass output-stage kernel'
    N, (S, Fin, nout1), C = csr.N, cw.shape, int(gy.size(1))
    G = relu_bwd(gy, 0, C, out, C, N, nout1)
    r = _conv_backward(csr, x, ea, cw, G, road.want_dx, road.need_val, road.want_cw, val_t=ea_t, want_source_order=road.learnedge, road=road.conv)
    if road.want_cb:
        g[7] = G.sum(0)
    if road.mixk:
        w11, b11, w12, b12 = fc
        ws = torch.empty(int(_lib.lib().gml_node_mix_bwd_workspace_bytes(N, Fin, C - nout1)), dtype=torch.uint8, device=x.device)
        g[8], g[9], g[10], g[11] = torch.empty_like(w11), torch.empty_like(b11), torch.empty_like(w12), torch.empty_like(b12)
        with _Timed('node_mix_bwd'):
            _lib.call('gml_node_mix_bwd', _ptr(x), int(x.stride(0)), _ptr(w11), _ptr(b11), _ptr(w12), _ptr(b12), _off(gy, nout1), C,
                      _ptr(r[0]) if road.want_dx else _ptr(None), Fin, _ptr(g[8]), _ptr(g[9]), _ptr(g[10]), _ptr(g[11]), N, Fin,
                      C - nout1, _ptr(ws), ws.numel(), _stream(x.device))
    return r


# How one ML3Layer forward runs (decided once, by _ml3_fwd_road; DESIGN s4.3c has the table):
#   edge      None (the supports as they are) / 'branch' (the kernels of the edge plan, inside ML3LayerFunction) / 'wide' (EdgeBranchWide,
#             17 .. 48 supports) / 'library' (GEMMs under autograd)
#   order     of the branch: 'source_raw' (source order, the supports as given: no value sort) / 'source' (after a gather) / 'dual' (target
#             order, the second copy scattered into source order by the edge kernel) / 'target'
#   layers    edge branches in the pass: 0 = none (the head of the stack left this layer's output in the stash), 2 .. 4 = the layers
#             stacked on this one ride along
#   pairs     the view ('source' / 'target') in which csr.sym_index is asked for the batch's unique rows, or None: not asked
#   hadamard  None / 'fused' (inside gml_ml3_fwd) / 'library';  pool  None / 'plain' / 'pattern' (the pool leaves the relu pattern)
#   chain_in / chain_out  the hand-over tokens the backward keeps;  conv  the ConvFwdRoad
ML3FwdRoad = _collections.namedtuple('ML3FwdRoad', 'edge order layers pairs hadamard pool chain_in chain_out conv')


def _ml3_fwd_road(Se, S, Fin, nout1, nout2, E, learnedge, grad_on, wanted, sup, stash, succ, pooled, exact, arith, bwd, conv,
                  chain_in_cols=None, edge_stack=True, edge_sym=True, chain=True, bwd_had=True, wide_lib=False):
    """ML3FwdRoad from plain values only (no tensor, no launch).  Whether the batch HAS pairs is data: the road says where to ask."""
    # Se / S: supports into the edge branch / into the conv; grad_on, wanted: autograd records, any input wants a gradient; sup: the
    # supports as the caller holds them -- (2-D float32 contiguous [E, .], Se wide, carry a gradient, csr.src_sorted); stash: a stash hit;
    # succ: stackable layers on top; arith: _edge_arith(); bwd: the conv backward of (S, Fin, nout1) has a fused plan; conv: ConvFwdRoad
    plain, width, sup_grad, src_sorted = sup
    mixk = nout2 > 0 and node_mix_native(Fin, nout2)
    edge, order, layers, pairs = None, None, 0, None
    if learnedge and max(Se, S) > 16:
        # more than 16 supports (no script goes beyond counting.py's 12; the sr25 sweep of SURVEY s8d raises nfreq to 47)
        edge = 'wide' if (max(Se, S) <= 48 and width and not wide_lib) else 'library'
    elif learnedge:
        # When the fused backward will run, the edge branch lives in SOURCE order (the order that kernel walks): the raw supports in that
        # order are per-batch data (SpectralDesign emits source-sorted edges: the input itself, no value sort at all), the branch writes
        # its output once, and the forward conv gathers the rows through tpos.  (r02: emitting both orders from the edge kernel cost it
        # 37 % -- it is HBM-bound and the second copy was a scattered 32-byte-row write: 'dual' is left to the forward kernels without
        # the gather.)  Inference / unfused training: target order.
        edge, layers = 'branch', 1
        if src_sorted and grad_on and plain and width and not sup_grad and S == Se and bwd and conv.gathers:
            order = 'source_raw'
            stacks = succ > 0 and edge_stack and _edge_fwd_family(Se, Se, 1 + succ, arith, E > 0, False, False).entry is not None
            layers = 0 if stash else 1 + succ if stacks else 1
        else:
            order = 'target' if not (wanted and bwd) else 'source' if conv.gathers else 'dual' if E * Se * 4 < 0xffffff00 else 'target'
        # unique support rows only where the batch pairs up: per-batch data (no gradient), one copy, a square branch (a padded one has no such form)
        if edge_sym and layers and not (sup_grad and grad_on) and order != 'dual' and S == Se:
            pairs = 'target' if order == 'target' else 'source'
    keep = chain and edge != 'wide' and edge != 'library'
    pool = None if not pooled else 'pattern' if _pool_relu_pattern(bwd_had, mixk, nout1, nout2, exact, wanted) else 'plain'
    return ML3FwdRoad(edge, order, layers, pairs, None if nout2 == 0 else 'fused' if mixk else 'library', pool,
                      bool(keep and chain_in_cols is not None and chain_in_cols <= Fin), bool(keep and not pooled), conv)


# row stride of rows4(_f32rows(x)): x's own where the kernels read its rows as they are, else the zero-padded copy's
def _rows4_stride(x):
    asis = x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= x.size(1) and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0
    return int(x.stride(0)) if asis else (int(x.size(-1)) + 3) // 4 * 4


def _road_text(road):
    return ' '.join('%s=%s' % (k, getattr(v, 'kind', None) or v.label if k == 'conv' else int(v) if isinstance(v, bool) else v)
                    for k, v in zip(road._fields, road))


def ml3_fwd_road(csr, x, Se, S, Fin, nout1, nout2, learnedge, grad_on, wanted, sup, stash=False, succ=0, pooled=False, chain_in_cols=None):
    """ML3FwdRoad of one layer call: the switches, the arithmetic and the plain properties of csr and x are read here, once"""
    exact = bool(exact_mode())
    conv = _conv_fwd_road(S, Fin, nout1, exact, getattr(csr, 'gmax128', None), csr.N, _rows4_stride(x), 0, FWD_CHUNKS)
    bwd = bool(learnedge and grad_on and max(Se, S) <= 16 and fused_bwd_available(csr, S, Fin, nout1))
    road = _ml3_fwd_road(int(Se), int(S), int(Fin), int(nout1), int(nout2), csr.E, learnedge, grad_on, wanted, sup, stash, succ, pooled,
                         exact, _edge_arith(), bwd, conv, chain_in_cols, EDGE_STACK, EDGE_SYM, CHAIN, BWD_HAD,
                         bool(_os.environ.get('GML_EDGE_WIDE_LIB')))
    if VERBOSE:
        _path('ml3_fwd', _road_text(road), S, Fin, nout1)
    return road


def _ml3_edge_fwd(road, csr, val, weights, tpos):
    """the edge branches of road.layers layers on val in ONE launch; returns (outputs, the first one's scattered copy or None)"""
    # weights = [(w1, w2, w3, w4)] per layer; the family is resolved once, with the batch's answer about pairs
    (E, Se), L = val.shape, road.layers
    with _Timed('edge_mlp_fwd', 4 * val.numel() * (L + (2 if tpos is not None else 1)), 20 * E * Se ** 2 * L):
        split = csr.presplit(val) if L > 1 else None
        sym = csr.sym_index(val, road.pairs) if road.pairs else None
        fam = _edge_fwd_family(Se, weights[0][3].size(0), L, _edge_arith(), Se <= 16 and E > 0, tpos is not None, sym is not None)
        if 'stack' in (fam.entry or ''):                   # (GML_VERBOSE: the edge functions record the family the plan named)
            return edge_mlp_fwd_stack(val, split, weights, sym, fam), None
        out, out_t = edge_mlp_fwd(val, *weights[0], tpos, csr.presplit(val), fam)
        return [out], out_t


class ML3LayerFunction(torch.autograd.Function):
    """Whole ML3Layer.forward (libs/spect_conv.py:204-212) with the concat written in place:
         ea' = edge-MLP(val)                      (learnedge)
         out[:, :nout1] = relu(SpectConv(x, ea')) (fused kernel, leading dimension nout1+nout2)
         out[:, nout1:] = tanh(fc11 x) * tanh(fc12 x)
    """

    @staticmethod
    def forward(ctx, x, val, w1, w2, w3, w4, cw, cb, w11, b11, w12, b12, csr, learnedge, nout2, road,
                pool_ptr=None, pool_seg=None, pool_mean=False, chain_in=None, chain_out=None, ea_pre=None, stack=((), [])):
        # road: the ML3FwdRoad the caller decided (ml3_fwd_road) -- this forward runs it
        # ea_pre: this layer's edge-branch output in source order, already computed by the first layer of its stack; stack =
        # (weights of the layers stacked on this one [(w1, w2, w3, w4)], list that receives their edge-branch outputs): the
        # layers all read the same raw supports, one pass serves them (edge_mlp_fwd_stack)
        # chain_in / chain_out (ChainToken): x is the output of the ML3Layer that owns chain_in and has no other consumer /
        # this layer's own token, which the consumer of its output sets (see ChainToken)
        # pool_ptr / pool_seg (int32 [B+1] / [N]): the layer is directly followed by global_add_pool / global_mean_pool
        # (Zinc12k.py:343): the pooled [B, C] tensor is returned and the pool's gradient is never expanded to [N, C]
        # val: the raw supports in SOURCE order when road.order is 'source_raw'; otherwise target-sorted order
        x, val, cw = _f32rows(x, 'x'), _f32c(val, 'edge_attr'), _f32c(cw, 'conv1.weight')
        S, Fin, nout1 = cw.shape
        N, C = csr.N, nout1 + nout2
        if x.size(0) != N or x.size(1) != Fin or val.size(0) != csr.E:
            raise ValueError('shape mismatch: x %s, edge_attr %s, conv1.weight %s, graph N=%d E=%d'
                             % (tuple(x.shape), tuple(val.shape), tuple(cw.shape), N, csr.E))
        with torch.cuda.device(x.device):
            x = rows4(x)
            ea, ea_t, epos = val, None, None
            if learnedge:
                assert road.edge == 'branch', 'more than 16 supports: ML3Layer runs that edge branch outside this function'
                ws_ = [tuple(_f32c(t, 'edge branch weight') for t in w) for w in [(w1, w2, w3, w4)] + list(stack[0])]
                w1, w2, w3, w4 = ws_[0]
                if road.layers == 0:
                    ea = ea_pre
                else:
                    val_s = csr.to_source_order(val, cache=not val.requires_grad) if road.order == 'source' else val
                    (ea, *rest), ea_t = _ml3_edge_fwd(road, csr, val_s, ws_, csr.tpos if road.order == 'dual' else None)
                    stack[1].extend(rest)                         # (the stacked layers' outputs: the caller stashes them)
                if road.order in ('source_raw', 'source'):        # the conv gathers the rows through tpos (target position -> source position)
                    ea_t, epos = ea, csr.tpos
            if ea.size(1) != S:
                raise ValueError('conv1 expects %d supports, edge branch produced %d' % (S, ea.size(1)))
            out = torch.empty(N, C, dtype=torch.float32, device=x.device)
            cb_ = _f32c(cb, 'conv1.bias') if cb is not None else None
            gi, gflag = _conv_fwd_records(csr, road.conv, S, Fin, nout1)
            mixk = road.hadamard == 'fused'
            q, f = conv_cost(N, int(ea.size(0)), S, Fin, nout1) if PROFILE is not None else (0, 0)
            if nout2 > 0:
                w11, b11, w12, b12 = (_f32c(t, n) for t, n in zip((w11, b11, w12, b12), ('fc11.weight', 'fc11.bias', 'fc12.weight', 'fc12.bias')))
                _path('hadamard', 'fused kernels' if mixk else 'library GEMMs (ninp > 64 or nout2 > 24)', '-', Fin, nout2)
            with _Timed('spectconv_fwd', q, f):                    # conv (+ Hadamard branch of the same rows)
                _lib.call('gml_ml3_fwd', _ptr(csr.rowptr), _ptr(csr.col), _ptr(gi), _ptr(epos), _ptr(ea), _ptr(x), int(x.stride(0)), _ptr(cw),
                          Fin * nout1, nout1, 1, _ptr(cb_), *[_ptr(t if mixk else None) for t in (w11, b11, w12, b12)], _ptr(out), C, N, S, Fin,
                          nout1, int(nout2) if mixk else 0, _lib.GML_RELU | gflag | _fwd_arith_flags(), _stream(x.device))
            if nout2 > 0 and not mixk:
                # ninp > 64 or nout2 > 24 (ptc.py:331-338 has ninp = 80): two plain library GEMMs + elementwise
                out[:, nout1:] = torch.tanh(_linear(x, w11, b11)) * torch.tanh(_linear(x, w12, b12))
        ctx.csr, ctx.learnedge, ctx.nout2, ctx.has_cb = csr, learnedge, nout2, cb is not None
        ctx.exact, ctx.src_order, ctx.val_is_source = bool(exact_mode()), epos is not None, road.order == 'source_raw'
        ctx.pool = (pool_ptr, pool_seg, int(pool_mean)) if pool_ptr is not None else None     # bit 0 mean, bit 1 GML_POOL_SKIP_LAST
        ctx.chain_in, ctx.chain_out = chain_in if road.chain_in else None, chain_out if road.chain_out else None
        ctx.save_for_backward(x, val, (ea if learnedge and epos is None else None), w1, w2, w3, w4, cw, w11, b11, w12, b12, out, ea_t)
        ctx.pool_mask = None
        if ctx.pool is not None:
            pooled = (segment_sum_mask if road.pool == 'pattern' else segment_sum)(out, pool_ptr, int(pool_mean) & 3)
            if road.pool == 'pattern':                         # (the pool also leaves the relu pattern of every row)
                pooled, ctx.pool_mask = pooled
            if int(pool_mean) & 2:
                skip_last_mask(pooled)                         # (created outside any later graph capture of the backward)
            return pooled
        return out

    @staticmethod
    def backward(ctx, gy):
        with exact_products(_bwd_exact(ctx)):
            return ML3LayerFunction._backward(ctx, gy)

    @staticmethod
    def _backward(ctx, gy):
        x, val, ea, w1, w2, w3, w4, cw, w11, b11, w12, b12, out, ea_t = ctx.saved_tensors
        csr, learnedge, nout2 = ctx.csr, ctx.learnedge, ctx.nout2
        S, Fin, nout1 = cw.shape
        N = csr.N
        need = ctx.needs_input_grad
        gy = _f32c(gy, 'grad_out')
        if not learnedge:
            ea = val
        if ctx.pool is not None and (ctx.pool[2] & 2) and not (ctx.pool[2] & 4):
            # GML_POOL_SKIP_LAST: the padding graph's pooled row was written, not computed -- its gradient must not reach the nodes.
            # Bit 2 (4): the caller vouches that the loss gives that row a ZERO gradient already (models.zinc_step_loss: the fused
            # head + loss ignore rows beyond the labelled ones) -- the masking launch is skipped
            gy = gy * skip_last_mask(gy)
        exact, x4 = exact_mode(), _rows4_ok(*_rows_of(x), Fin)
        road = _ml3_bwd_road(S, Fin, nout1, nout2, N, need, learnedge, ctx.has_cb, _conv_bwd_road(csr, S, Fin, nout1, exact, x4), exact,
                             BWD_HAD, BWD_DMA, CHAIN, ctx.pool is not None, ctx.pool_mask is not None,
                             ctx.chain_out is not None and ctx.chain_out.premasked,
                             ctx.chain_in.cols if ctx.chain_in is not None else None, _rows_of(gy), x4)
        if VERBOSE:
            _path('ml3_bwd', _road_text(road), S, Fin, nout1)
        # the hand-over tokens are read once: this layer's is cleared, the lower layer's set when dx leaves with its relu applied
        if ctx.chain_out is not None:
            ctx.chain_out.premasked = False
        if road.relu_cols:
            ctx.chain_in.premasked = True
        gy_seg = ctx.pool[1] if road.pool_grad == 'per_segment' else None      # (the stage then reads gy[gy_seg[row]]: never expanded)
        if road.pool_grad is not None:                         # gy is the POOLED gradient [B, C]
            pptr, pseg, pmean = ctx.pool[0], ctx.pool[1], ctx.pool[2] & 1
            if road.pool_grad == 'expanded':
                gy = segment_bcast(gy, pptr, N, pmean)
            elif pmean:
                gy = gy / (pptr[1:] - pptr[:-1]).clamp(min=1).to(gy.dtype).unsqueeze(1)
            if road.pool_grad == 'masked':
                # the pool's gradient per row with the relu pattern applied (4 + 4 bytes read, 128 written per row)
                gy = segment_bcast_mask(gy, pseg, ctx.pool_mask, nout1)
        g = [None] * 23
        with torch.cuda.device(x.device):
            if not learnedge and road.conv.plan is not None:
                ea_t = csr.to_source_order(val, cache=not val.requires_grad)   # raw supports: per-batch data (trained ones change)
            stage = {'had': _ml3_stage_had, 'one_pass': _ml3_stage_one_pass, 'separate': _ml3_stage_separate}[road.stage]
            dx, dea, g[6], dea_src = stage(road, csr, g, gy, gy_seg, out, x, ea, ea_t, cw, (w11, b11, w12, b12))
            if road.lib_hadamard:                                   # wide Hadamard branch: library GEMMs (see forward)
                ta, tb = torch.tanh(_linear(x, w11, b11)), torch.tanh(_linear(x, w12, b12))
                g2 = gy[:, nout1:]
                ga, gb = g2 * tb * (1 - ta * ta), g2 * ta * (1 - tb * tb)
                g[8], g[10] = ga.t().mm(x), gb.t().mm(x)
                g[9] = ga.sum(0) if b11 is not None else None
                g[11] = gb.sum(0) if b12 is not None else None
                if need[0]:
                    dx = dx.addmm_(ga, w11).addmm_(gb, w12)
            g[0] = dx
            if learnedge:
                if road.need_val:
                    # the edge MLP is per-edge, so it can run in whichever order dea arrived in
                    val_in = val if ctx.val_is_source else (csr.to_source_order(val, cache=not val.requires_grad) if dea_src else val)
                    with _Timed('edge_mlp_bwd', 4 * val.numel() * 2, 60 * val.size(0) * val.size(1) ** 2):
                        gin, g[2], g[3], g[4], g[5] = edge_mlp_bwd(val_in, w1, w2, w3, w4, dea, need[1], csr.presplit(val_in),
                                                                   csr.sym_index(val_in) if (EDGE_SYM and dea_src and not need[1]) else None)
                    if gin is not None and dea_src:
                        gin = csr.from_source_order(gin)
                    g[1] = gin
            else:
                g[1] = dea if need[1] else None
        return tuple(g)


# ---------------------------------------------------------------------------- PPGN block (csrc/gml_ppgn.hip)
PPGN_READOUTS = {'sum': 0, 'mean': 1, 'diag': 2}


def ppgn_block_supported(x, nmax, Cin, C):
    """the fused block (PPGNBlockFunction) serves this input: float32 [B, Cin, nmax, nmax] on the device with nmax <= 64, Cin <= 64
    and C <= 64 (gml_ppgn_supported); any mix of node counts 1 <= n_g <= nmax.  A non-contiguous view is served through a contiguous
    copy.  No shape class inside the range is gated onto the composition: one block forward + backward, fused 90th percentile against
    the composition's 10th, ms (tools/bench_ppgn.py, profiles/ppgn.json, DESIGN s4.19): inner blocks (with dx) sr25 (15 graphs, n = 25) 0.37 against 0.90,
    graph8c (11,117 graphs, n = 8) 2.02 against 12.53, EXP (1,200 graphs, nmax = 64) 6.56 against 10.10 (its first block, 3 -> 20
    without dx: 5.05 against 7.57, the closest class), a ZINC-like batch of 64 at nmax = 37 0.37 against 0.82."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4) or _os.environ.get('GML_NO_PPGN_FUSED'):
        return False
    if int(x.size(1)) != int(Cin) or int(x.size(2)) != int(nmax) or int(x.size(3)) != int(nmax) or x.size(0) < 1:
        return False
    return bool(_lib.lib().gml_ppgn_supported(int(nmax), int(Cin), int(C)))


def ppgn_block_torch(x, n, w1, b1, w2, b2, w3, b3, readout='sum'):
    """The block composed from torch ops (the road of every shape outside ppgn_block_supported; about ten launches forward):
    returns (y, r) like PPGNBlockFunction.  w*: [C, Cin] or Conv2d's [C, Cin, 1, 1]."""
    nmax = x.size(-1)
    ar = torch.arange(nmax, device=x.device)
    inside = ar.view(1, -1) < n.view(-1, 1)                                        # [B, nmax]
    m = (inside.unsqueeze(2) & inside.unsqueeze(1)).to(x.dtype).unsqueeze(1)       # [B, 1, nmax, nmax]
    conv = lambda t, w, b: torch.nn.functional.conv2d(t, w.reshape(w.size(0), w.size(1), 1, 1), b)
    a1 = torch.relu(conv(x, w1, b1) * m)
    a2 = torch.relu(conv(x, w2, b2) * m)
    p = torch.matmul(a1, a2) * m
    y = torch.relu(conv(torch.cat([p, x], 1), w3, b3) * m)
    eye = torch.eye(nmax, dtype=x.dtype, device=x.device)
    m0, m1 = m * eye, m * (1 - eye)
    r0, r1 = (y * m0).sum((2, 3)), (y * m1).sum((2, 3))
    if readout == 'diag':
        return y, r0
    if readout == 'mean':
        return y, torch.cat([r0 / m0.sum((2, 3)), r1 / m1.sum((2, 3))], 1)
    if readout != 'sum':
        raise ValueError("readout: 'sum', 'mean' or 'diag'")
    return y, torch.cat([r0, r1], 1)


class PPGNBlockFunction(torch.autograd.Function):
    """One PPGN block (sr25.py:48-52) on x [B, Cin, nmax, nmax] with node counts n [B] (int32), mask m = [i < n_g and j < n_g]:
        a1 = relu(m (W1 x + b1)),  a2 = relu(m (W2 x + b2)),  p_c = a1_c @ a2_c,  y = relu(m (W3 [p ; x] + b3))
    returns (y, r): y [B, C, nmax, nmax], exactly 0 in the padding whatever x holds there, and the layer readout r out of the kernel
    that writes y, r0_c = sum_i y_c[i, i], r1_c = sum_{i != j} y_c[i, j]:
        'sum' : [r0 | r1] [B, 2C]  (sr25.py:52 sums rows, then columns: the same quantity)
        'mean': [r0 / n | r1 / (n^2 - n)]  (exp_classify.py:60; at n = 1 the off-diagonal half is 0 / 0 = nan: the reference's
                arithmetic, kept)
        'diag': r0 [B, C]  (mutag.py:52)
    Forward: three launches; backward: four, plus one for dx when x needs a gradient (the first block's input is data).  w1, w2
    [C, Cin], w3 [C, C + Cin] (or Conv2d's 4-d weights), biases optional.  fp32 products and fp32 accumulation only, no bf16 pieces:
    exact_products() changes nothing here.  Weight and bias gradients: per-workgroup partials, one ordered fold, no atomics --
    bit-reproducible.  No host synchronisation: n is read on the device, forward + backward capture in a graph."""

    @staticmethod
    def forward(ctx, x, n, w1, b1, w2, b2, w3, b3, readout='sum'):
        x = _f32c(x, 'x')
        if x.dim() != 4 or x.size(2) != x.size(3):
            raise ValueError('PPGN block: x must be [B, Cin, nmax, nmax], got %s' % (list(x.shape),))
        B, Cin, nmax = int(x.size(0)), int(x.size(1)), int(x.size(2))
        C = int(w1.size(0))
        mode = PPGN_READOUTS[readout]
        _require_cuda(n, 'n')
        if n.dtype != torch.int32 or n.numel() != B:
            raise TypeError('PPGN block: n must be int32 [B]')
        n = n.contiguous()
        ctx.wshapes = (w1.shape, w2.shape, w3.shape)
        w1, w2, w3 = _f32c(w1.reshape(C, -1), 'w1'), _f32c(w2.reshape(C, -1), 'w2'), _f32c(w3.reshape(C, -1), 'w3')
        if w1.size(1) != Cin or tuple(w2.shape) != (C, Cin) or tuple(w3.shape) != (C, C + Cin):
            raise ValueError('PPGN block: weights [C, Cin], [C, Cin], [C, C + Cin] expected')
        b1, b2, b3 = (None if b is None else _f32c(b, 'bias') for b in (b1, b2, b3))
        dev = x.device
        with torch.cuda.device(dev):
            a12 = torch.empty(B, 2 * C, nmax, nmax, dtype=torch.float32, device=dev)
            p = torch.empty(B, C, nmax, nmax, dtype=torch.float32, device=dev)
            y = torch.empty(B, C, nmax, nmax, dtype=torch.float32, device=dev)
            r = torch.empty(B, C if mode == 2 else 2 * C, dtype=torch.float32, device=dev)
            with _Timed('ppgn_fwd'):
                _lib.call('gml_ppgn_fwd', _ptr(x), _ptr(n), B, nmax, Cin, C, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(w3), _ptr(b3),
                          mode, _ptr(a12), _ptr(p), _ptr(y), _ptr(r), _stream(dev))
        ctx.dims, ctx.mode = (B, Cin, nmax, C), mode
        ctx.has_b = (b1 is not None, b2 is not None, b3 is not None)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, n, w1, w2, w3, a12, p, y)
        return y, r

    @staticmethod
    def backward(ctx, dy, dr):
        x, n, w1, w2, w3, a12, p, y = ctx.saved_tensors
        B, Cin, nmax, C = ctx.dims
        dev = x.device
        if dy is None and dr is None:
            return (None,) * 9
        dy = None if dy is None else _f32c(dy, 'grad of y')
        dr = None if dr is None else _f32c(dr, 'grad of the readout')
        L = _lib.lib()
        with torch.cuda.device(dev):
            dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
            flat = torch.empty(int(L.gml_ppgn_dw_floats(Cin, C)), dtype=torch.float32, device=dev)
            nws = int(L.gml_ppgn_bwd_workspace_bytes(B, nmax, Cin, C))
            ws = torch.empty(max(nws // 4, 1), dtype=torch.float32, device=dev)
            with _Timed('ppgn_bwd'):
                _lib.call('gml_ppgn_bwd', _ptr(x), _ptr(n), B, nmax, Cin, C, _ptr(w1), _ptr(w2), _ptr(w3), _ptr(a12), _ptr(p), _ptr(y),
                          _ptr(dy), _ptr(dr), ctx.mode, _ptr(dx), _ptr(flat), _ptr(ws), ws.numel() * 4, _stream(dev))
        n3, n12 = C + Cin + 1, Cin + 1
        d3 = flat[:C * n3].view(C, n3)
        d12 = flat[C * n3:].view(2 * C, n12)
        hb1, hb2, hb3 = ctx.has_b
        s1, s2, s3 = ctx.wshapes                                     # (Conv2d's [C, Cin, 1, 1] get their gradient in that shape)
        dw1, dw2, dw3 = d12[:C, :Cin].reshape(s1), d12[C:, :Cin].reshape(s2), d3[:, :C + Cin].reshape(s3)
        return (dx, None, dw1, d12[:C, Cin] if hb1 else None, dw2, d12[C:, Cin] if hb2 else None, dw3, d3[:, C + Cin] if hb3 else None,
                None)


# ---------------------------------------------------------------------------- what the message-passing layers (GAT, GIN, ChebNet) share
RELU_TANH = {None: 0, 'none': 0, 'relu': 1, 'tanh': 2}


def _relu_tanh_id(act):
    if act not in RELU_TANH:
        raise ValueError("act: None, 'relu' or 'tanh', got %r" % (act,))
    return RELU_TANH[act]


def _fused_input_ok(x):
    """what every fused layer asks of its input: float32 [N >= 1, F] on the device"""
    return isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.size(0) >= 1


def csr_edge_index(csr):
    """int64 [2, E] = (source, target) of a GraphCSR in its target-sorted order (for the *_conv_torch compositions)"""
    deg = (csr.rowptr[1:] - csr.rowptr[:-1]).to(torch.int64)
    dst = torch.repeat_interleave(torch.arange(csr.N, device=csr.device), deg, output_size=csr.E)
    return torch.stack([csr.col.to(torch.int64), dst])


def _flat_and_ws(layer, N, dims, dev):
    """(dflat, workspace) of a layer's backward, float32, sized by the library's gml_<layer>_dflat_floats(*dims) and
    gml_<layer>_bwd_workspace_bytes(N, *dims)"""
    L = _lib.lib()
    flat = torch.empty(int(getattr(L, 'gml_%s_dflat_floats' % layer)(*dims)), dtype=torch.float32, device=dev)
    nws = int(getattr(L, 'gml_%s_bwd_workspace_bytes' % layer)(N, *dims))
    return flat, torch.empty(max(nws // 4, 4), dtype=torch.float32, device=dev)


# ---------------------------------------------------------------------------- GAT attention layer (csrc/gml_gat.hip)
GAT_ACTS = {None: 0, 'none': 0, 'relu': 1, 'tanh': 2, 'elu': 3}
GAT_SLOPE = 0.2


def _gat_act_id(act):
    if act not in GAT_ACTS:
        raise ValueError("act: None, 'relu', 'tanh' or 'elu', got %r" % (act,))
    return GAT_ACTS[act]


def gat_conv_supported(x, heads, channels):
    """the fused attention layer (GATConvFunction) serves this input: float32 [N >= 1, Fin] on the device, heads = 8 and channels in
    {4, 8, 12, 16, 32} (gml_gat_supported) -- every GatNet of the experiment scripts (8 heads of 8, 12 or 16 channels).  Any number of
    edges, any degree.  Everything else takes the composition gat_conv_torch.  No shape inside the range is gated onto the composition:
    one layer forward + backward, fused 90th percentile against the composition's 10th, ms (tools/bench_gat.py, profiles/gat.json,
    DESIGN s4.20): ZINC-like batch of 64 0.37 against 1.01 (25 -> 8 x 8) and 0.36 against 0.98 (96 -> 8 x 12), mutag batch 16 0.36 against
    0.79, sr25 0.21 against 0.82, the 900-node grid 0.21 against 0.81, 500 k rows 2.11 against 7.05 and 2.66 against 8.38."""
    if not _fused_input_ok(x):
        return False
    if _os.environ.get('GML_NO_GAT_FUSED'):
        return False
    return bool(_lib.lib().gml_gat_supported(int(heads), int(channels)))


def gat_conv_torch(x, edge_index, weight, att_l, att_r, bias=None, act=None, negative_slope=GAT_SLOPE):
    """GATConv (torch_geometric 1.6.1, concat=True, no attention dropout) composed from torch ops, on any device and dtype: the road
    of every shape outside gat_conv_supported and the opponent of tools/bench_gat.py.  x [N, Fin], edge_index [2, E] = (source j,
    target i), weight [H C, Fin], att_l / att_r [1, H, C] (or [H, C]), bias [H C] or None.  Edges with j == i are dropped (masked: no
    host read), one self edge per node is added (evaluated per node, not as E + N gathered rows), repeated edges count once each.
    Softmax per target and head with the row maximum subtracted and 1e-16 added to the denominator."""
    N = x.size(0)
    H, C = att_l.shape[-2], att_l.shape[-1]
    src, dst = edge_index[0], edge_index[1]
    xl = (x @ weight.t()).view(N, H, C)
    al = (xl * att_l.reshape(1, H, C)).sum(-1)
    ar = (xl * att_r.reshape(1, H, C)).sum(-1)
    lrelu = lambda s: torch.where(s > 0, s, s * negative_slope)
    keep = (src != dst).unsqueeze(1)
    eself = lrelu(al + ar)                                                        # [N, H]
    e = lrelu(al[src] + ar[dst])                                                  # [E, H]
    e = torch.where(keep, e, torch.full_like(e, float('-inf')))
    idx = dst.unsqueeze(1).expand(-1, H)
    m = eself.detach().clone().scatter_reduce_(0, idx, e.detach(), 'amax', include_self=True)
    pself = torch.exp(eself - m)
    p = torch.exp(e - m[dst])                                                     # exactly 0 on the dropped edges
    z = pself.clone().index_add_(0, dst, p) + 1e-16
    out = (pself.unsqueeze(-1) * xl).index_add_(0, dst, p.unsqueeze(-1) * xl[src]) / z.unsqueeze(-1)
    out = out.reshape(N, H * C)
    if bias is not None:
        out = out + bias
    a = _gat_act_id(act)
    if a == 1:
        return torch.relu(out)
    if a == 2:
        return torch.tanh(out)
    if a == 3:
        return torch.nn.functional.elu(out)
    return out


gat_edge_index = csr_edge_index


class GATConvFunction(torch.autograd.Function):
    """y = act(GATConv(x) + bias) over a GraphCSR of the (source, target) edges: the projection xl = x W^T (torch.matmul, fp32), the head
    logits (gml_gat_logits) and the edge softmax + weighted gather + bias + activation of every target row (gml_gat_fwd): three launches.
    Backward: gml_gat_bwd (four launches: target view, source view, partial sums, fold) -> dxl, datt_l, datt_r, dbias, then dW =
    dxl^T x and, when x needs one, dx = dxl W (torch.matmul): six.  The attention weights are recomputed in the backward from the
    logits and the row maximum / sum the forward leaves ([N, H] each); no [E, H] alpha is stored.  No atomics, no host read:
    bit-reproducible, capturable.  Plain fp32 (exact_products() changes nothing)."""

    @staticmethod
    def forward(ctx, x, csr, weight, att_l, att_r, bias, act=None):
        x = _f32c(x, 'x')
        weight = _f32c(weight, 'weight')
        H, C = int(att_l.shape[-2]), int(att_l.shape[-1])
        HC, N = H * C, int(x.size(0))
        if x.dim() != 2 or weight.dim() != 2 or weight.size(1) != x.size(1) or weight.size(0) != HC or tuple(att_r.shape[-2:]) != (H, C):
            raise ValueError('GAT layer: x [N, Fin], weight [H C, Fin], att_l / att_r [1, H, C] expected')
        if csr.N != N:
            raise ValueError('GraphCSR was built for %d nodes, x has %d rows' % (csr.N, N))
        al_w, ar_w = _f32c(att_l.reshape(HC), 'att_l'), _f32c(att_r.reshape(HC), 'att_r')
        b = None if bias is None else _f32c(bias, 'bias')
        a = _gat_act_id(act)
        dev = x.device
        with torch.cuda.device(dev):
            xl = torch.matmul(x, weight.t())
            al = torch.empty(N, H, dtype=torch.float32, device=dev)
            ar, m, z = torch.empty_like(al), torch.empty_like(al), torch.empty_like(al)
            y = torch.empty(N, HC, dtype=torch.float32, device=dev)
            st = _stream(dev)
            with _Timed('gat_fwd', q=4 * ((csr.E + N) * HC + N * HC)):
                _lib.call('gml_gat_logits', _ptr(xl), HC, _ptr(al_w), _ptr(ar_w), N, H, C, _ptr(al), _ptr(ar), st)
                _lib.call('gml_gat_fwd', _ptr(csr.rowptr), _ptr(csr.col), _ptr(xl), HC, _ptr(al), _ptr(ar), _ptr(b), N, csr.E, H, C, a,
                          _ptr(y), HC, _ptr(m), _ptr(z), st)
        ctx.csr, ctx.act, ctx.dims = csr, a, (N, H, C)
        ctx.att_shapes = (att_l.shape, att_r.shape)
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, weight, al_w, ar_w, xl, al, ar, m, z, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, al_w, ar_w, xl, al, ar, m, z, y = ctx.saved_tensors
        csr, (N, H, C) = ctx.csr, ctx.dims
        HC, dev = H * C, x.device
        dy = _f32c(dy, 'grad of y')
        with torch.cuda.device(dev):
            dxl = torch.empty(N, HC, dtype=torch.float32, device=dev)
            datt = torch.empty(3, HC, dtype=torch.float32, device=dev)
            nws = int(_lib.lib().gml_gat_bwd_workspace_bytes(N, csr.E, H, C))
            ws = torch.empty(max(nws // 4, 4), dtype=torch.float32, device=dev)
            with _Timed('gat_bwd'):
                _lib.call('gml_gat_bwd', _ptr(csr.rowptr), _ptr(csr.col), _ptr(csr.rowptr_t), _ptr(csr.col_t), _ptr(csr.pos_t), _ptr(xl), HC,
                          _ptr(al), _ptr(ar), _ptr(m), _ptr(z), _ptr(y), HC, _ptr(dy), HC, _ptr(al_w), _ptr(ar_w), N, csr.E, H, C, ctx.act,
                          _ptr(dxl), HC, _ptr(datt[0]), _ptr(datt[1]), _ptr(datt[2]) if ctx.has_bias else None, _ptr(ws), ws.numel() * 4,
                          _stream(dev))
            dw = torch.matmul(dxl.t(), x) if ctx.needs_input_grad[2] else None
            dx = torch.matmul(dxl, weight) if ctx.needs_input_grad[0] else None
        sl, sr = ctx.att_shapes
        return dx, None, dw, datt[0].reshape(sl), datt[1].reshape(sr), datt[2] if ctx.has_bias else None, None


# ---------------------------------------------------------------------------- GIN layer (csrc/gml_gin.hip)
GIN_ACTS, _gin_act_id = RELU_TANH, _relu_tanh_id


def gin_nn_linears(nn):
    """the Linears of a GINConv's nn when it is torch.nn.Sequential(Linear) or Sequential(Linear, ReLU, Linear) -- the two forms of the
    experiment scripts, which the fused layer serves --, else None"""
    if not isinstance(nn, torch.nn.Sequential) or len(nn) not in (1, 3):
        return None
    mods = list(nn)
    if type(mods[0]) is not torch.nn.Linear:
        return None
    if len(mods) == 1:
        return [mods[0]]
    if type(mods[1]) is not torch.nn.ReLU or type(mods[2]) is not torch.nn.Linear or mods[2].in_features != mods[0].out_features:
        return None
    return [mods[0], mods[2]]


def gin_conv_supported(x, Fh, Fout=None):
    """the fused GIN layer (GINConvFunction) serves this input: float32 [N >= 1, Fin] on the device, nn = Linear(Fin, Fh) (Fout None)
    or Linear(Fin, Fh) - ReLU - Linear(Fh, Fout), every width in 1 .. 64 (gml_gin_supported) -- every 64-wide GinNet of the experiment
    scripts.  Any number of edges, any degree.  Everything else (the 200-wide GinNets of ptc / proteins / enzymes_contfeat among it)
    takes the composition gin_conv_torch.  GML_NO_GIN_FUSED=1 sends every shape there.  No shape inside the range is gated onto the
    composition: one layer forward + backward, fused 90th percentile against the composition's 10th, ms (tools/bench_gin.py,
    profiles/gin.json, DESIGN s4.21): ZINC-like batch of 64 0.30 against 0.50 (25 -> 64 -> 64) and 0.30 against 0.50 (64 -> 64 -> 64),
    mutag batch 16 0.30 against 0.49 and 0.29 against 0.49, sr25 at depth 1 0.28 against 0.39 and 0.27 against 0.38, the 900-node grid
    0.28 against 0.38 (1 -> 64 -> 64) and 0.15 against 0.38, 500 k rows 1.65 against 3.44 and 2.01 against 4.27."""
    if not _fused_input_ok(x):
        return False
    if _os.environ.get('GML_NO_GIN_FUSED'):
        return False
    depth = 1 if Fout is None else 2
    return bool(_lib.lib().gml_gin_supported(int(x.size(1)), int(Fh), int(Fout or 0), depth))


def gin_conv_torch(x, edge_index, eps, linears, act=None):
    """GINConv (torch_geometric 1.6.1) composed from torch ops, on any device and dtype: the road of every shape outside
    gin_conv_supported and the opponent of tools/bench_gin.py.  x [N, Fin], edge_index [2, E] = (source j, target i), eps a tensor of
    one element, linears = [(weight, bias or None)] or [(w1, b1), (w2, b2)] with a relu between the two.
        h = index_add over the targets of x[source], then + (1 + eps) x;  out = act(nn(h))
    Every edge occurrence counts, self loops included."""
    src, dst = edge_index[0], edge_index[1]
    h = torch.zeros_like(x).index_add_(0, dst, x[src]) + (1 + eps) * x
    if len(linears) not in (1, 2):
        raise ValueError('linears: one or two (weight, bias) pairs')
    out = _linear(h, linears[0][0], linears[0][1])
    if len(linears) == 2:
        out = _linear(torch.relu(out), linears[1][0], linears[1][1])
    a = _relu_tanh_id(act)
    return torch.relu(out) if a == 1 else (torch.tanh(out) if a == 2 else out)


class GINConvFunction(torch.autograd.Function):
    """y = act(nn((1 + eps) x + sum of the neighbours)) over a GraphCSR of the (source, target) edges, nn = Linear (w2 None) or
    Linear - ReLU - Linear: ONE launch (gml_gin_fwd); the aggregate h [N, Fin] and the hidden t [N, Fh] are kept for the backward.
    Backward: gml_gin_bwd, three launches (row pass, source-view aggregation, fold), two when x needs no gradient (dx = NULL: the
    first layer of most models) -> dx, deps, dW1, db1, dW2, db2.  eps is read from device memory inside the kernels.  No atomics, no
    host read: bit-reproducible, capturable.  Plain fp32 (exact_products() changes nothing)."""

    @staticmethod
    def forward(ctx, x, csr, eps, w1, b1, w2, b2, act=None):
        x, w1 = _f32c(x, 'x'), _f32c(w1, 'w1')
        eps = _f32c(eps, 'eps')
        depth = 1 if w2 is None else 2
        if depth == 1 and b2 is not None:
            raise ValueError('GIN layer: b2 without w2')
        if x.dim() != 2 or w1.dim() != 2 or w1.size(1) != x.size(1) or eps.numel() != 1:
            raise ValueError('GIN layer: x [N, Fin], eps [1], w1 [Fh, Fin] expected')
        N, Fin, Fh = int(x.size(0)), int(x.size(1)), int(w1.size(0))
        Fout = 0
        if depth == 2:
            w2 = _f32c(w2, 'w2')
            if w2.dim() != 2 or w2.size(1) != Fh:
                raise ValueError('GIN layer: w2 [Fout, Fh] expected')
            Fout = int(w2.size(0))
        if csr.N != N:
            raise ValueError('GraphCSR was built for %d nodes, x has %d rows' % (csr.N, N))
        b1 = None if b1 is None else _f32c(b1, 'b1')
        b2 = None if b2 is None else _f32c(b2, 'b2')
        a = _relu_tanh_id(act)
        dev = x.device
        Fo = Fout if depth == 2 else Fh
        with torch.cuda.device(dev):
            h = torch.empty(N, Fin, dtype=torch.float32, device=dev)
            t = torch.empty(N, Fh, dtype=torch.float32, device=dev) if depth == 2 else None
            y = torch.empty(N, Fo, dtype=torch.float32, device=dev)
            flops = 2 * N * (Fin * Fh + Fh * Fout)
            with _Timed('gin_fwd', q=4 * ((csr.E + N) * Fin + N * (Fin + (Fh if depth == 2 else 0) + Fo)), f=flops):
                _lib.call('gml_gin_fwd', _ptr(csr.rowptr), _ptr(csr.col), _ptr(x), Fin, N, csr.E, Fin, _ptr(eps), _ptr(w1), _ptr(b1), Fh,
                          _ptr(w2), _ptr(b2), Fout, depth, a, _ptr(h), Fin, _ptr(t), Fh, _ptr(y), Fo, _stream(dev))
        ctx.csr, ctx.act, ctx.dims = csr, a, (N, Fin, Fh, Fout, depth)
        ctx.has_b = (b1 is not None, b2 is not None)
        ctx.eps_shape = eps.shape
        ctx.save_for_backward(x, eps, w1, w2, h, t, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, eps, w1, w2, h, t, y = ctx.saved_tensors
        csr, (N, Fin, Fh, Fout, depth) = ctx.csr, ctx.dims
        dev = x.device
        dy = _f32c(dy, 'grad of y')
        Fo = Fout if depth == 2 else Fh
        with torch.cuda.device(dev):
            dx = torch.empty(N, Fin, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
            flat, ws = _flat_and_ws('gin', N, (Fin, Fh, Fout, depth), dev)
            with _Timed('gin_bwd'):
                _lib.call('gml_gin_bwd', _ptr(csr.rowptr_t), _ptr(csr.col_t), _ptr(x), Fin, _ptr(h), Fin, _ptr(t), Fh, _ptr(y), Fo, _ptr(dy),
                          Fo, N, csr.E, Fin, _ptr(eps), _ptr(w1), Fh, _ptr(w2), Fout, depth, ctx.act, _ptr(dx), Fin, _ptr(flat), _ptr(ws),
                          ws.numel() * 4, _stream(dev))
        o1 = Fh * Fin
        o2 = o1 + Fh
        dw1, db1 = flat[:o1].view(Fh, Fin), flat[o1:o2]
        dw2 = db2 = None
        if depth == 2:
            o3 = o2 + Fout * Fh
            dw2, db2 = flat[o2:o3].view(Fout, Fh), flat[o3:o3 + Fout]
        hb1, hb2 = ctx.has_b
        return dx, None, flat[-1:].reshape(ctx.eps_shape), dw1, db1 if hb1 else None, dw2, db2 if hb2 else None, None


# ---------------------------------------------------------------------------- ChebNet layer (csrc/gml_cheb.hip)
def cheb_conv_supported(x, Fout, K, Fin=None):
    """the fused ChebConv layer (ChebConvFunction) serves this input: float32 [N >= 1, Fin] on the device (Fin: another width than
    x's, for a later layer of the same rows), 1 <= K <= 8 and both widths in 1 .. 64 (gml_cheb_supported) -- every ChebNet of the experiment scripts up to 64 wide.  Any number of edges, any degree.
    Everything else (the 128- and 200-wide ChebNets of enzymes / ptc / proteins / enzymes_contfeat among it) takes the composition
    cheb_conv_torch.  GML_NO_CHEB_FUSED=1 sends every shape there.  No shape inside the range is gated onto the composition: one layer
    forward + backward, fused 90th percentile (norm launch included) against the composition's 10th, ms (tools/bench_cheb.py,
    profiles/cheb.json, DESIGN s4.22): ZINC-like batch of 64 at K = 2 0.14 against 0.53 (25 -> 64) and 0.15 against 0.53 (64 -> 64),
    mutag batch 16 at K = 3 0.18 against 0.79 and 0.17 against 0.81, sr25 at K = 4 0.19 against 1.04 and 0.21 against 0.98, the 900-node
    grid at K = 7 0.16 against 1.61 and 0.30 against 1.63, 500 k rows 2.06 against 4.39 (K = 2) and 6.63 against 14.24 (K = 5)."""
    if not _fused_input_ok(x):
        return False
    if _os.environ.get('GML_NO_CHEB_FUSED'):
        return False
    return bool(_lib.lib().gml_cheb_supported(int(x.size(1)) if Fin is None else int(Fin), int(Fout), int(K)))


def _cheb_lambda(lambda_max, batch):
    """(lmax tensor or None, batch or None, scalar) of ChebConv's lambda_max argument: None = 2.0, a number for every graph, a tensor
    of one element for every graph, a tensor [B] indexed by batch"""
    if lambda_max is None:
        return None, None, 2.0
    if not isinstance(lambda_max, torch.Tensor):
        return None, None, float(lambda_max)
    lam = lambda_max.reshape(-1)
    if lam.numel() > 1 and batch is None:
        raise ValueError('lambda_max holds %d values: batch (the graph of every node) is needed to index it' % lam.numel())
    return lam, (batch if lam.numel() > 1 else None), 2.0


def cheb_norm(csr, batch=None, lambda_max=None):
    """norm [N, 2] = (deg^-1/2 over the non-self edges of the source view, 2 / lambda_max of the node's graph): what every ChebConv of
    a model reads (gml_cheb_norm, one launch, no host read: inside a captured step it follows batch and lambda_max on replay).
    lambda_max: None (2.0), a number, or a float32 tensor [B] indexed by batch [N]; values <= 0 or not finite are outside the contract."""
    dev = csr.device
    lam, bt, scalar = _cheb_lambda(lambda_max, batch)
    if lam is not None:
        _require_cuda(lam, 'lambda_max')
        lam = lam.to(torch.float32).contiguous()
    if bt is not None:
        _require_cuda(bt, 'batch')
        if bt.numel() != csr.N:
            raise ValueError('batch holds %d entries, the graph has %d nodes' % (bt.numel(), csr.N))
        bt = bt.to(torch.int32).contiguous()
    with torch.cuda.device(dev):
        norm = torch.empty(csr.N, 2, dtype=torch.float32, device=dev)
        _lib.call('gml_cheb_norm', _ptr(csr.rowptr_t), _ptr(csr.col_t), _ptr(bt), _ptr(lam), 0 if lam is None else int(lam.numel()),
                  scalar, csr.N, csr.E, _ptr(norm), _stream(dev))
    return norm


def cheb_conv_torch(x, edge_index, weight, bias=None, batch=None, lambda_max=None, act=None):
    """ChebConv (torch_geometric 1.6.1, normalization 'sym') composed from torch ops of static shape, on any device and dtype: the road
    of every shape outside cheb_conv_supported and the opponent of tools/bench_cheb.py.  x [N, Fin], edge_index [2, E] = (source j,
    target i), weight [K, Fin, Fout], bias [Fout] or None.  Self loops are dropped (masked, not removed: no host read), every other
    edge occurrence counts;  deg over the sources, L^[i, j] = -s[i] dis[i] dis[j], L^[i, i] = s[i] - 1, s = 2 / lambda_max;
    Tx_0 = x, Tx_1 = L^ x, Tx_k = 2 L^ Tx_{k-1} - Tx_{k-2};  out = act(bias + sum_k Tx_k W_k)."""
    src, dst = edge_index[0], edge_index[1]
    N = int(x.size(0))
    keep = (src != dst).to(x.dtype)
    deg = torch.zeros(N, dtype=x.dtype, device=x.device).index_add_(0, src, keep)
    dis = torch.where(deg > 0, deg.clamp(min=1).pow(-0.5), torch.zeros_like(deg))
    lam, bt, scalar = _cheb_lambda(lambda_max, batch)
    if lam is None:
        s = torch.full((N,), 2.0 / scalar, dtype=x.dtype, device=x.device)
    else:
        lam = lam.to(dtype=x.dtype, device=x.device)
        s = 2.0 / (lam[bt.to(torch.int64)] if bt is not None else lam.expand(N))
    w = (-(s[dst] * dis[dst]) * dis[src] * keep).unsqueeze(1)
    diag = (s - 1).unsqueeze(1)

    def lap(t):
        return torch.zeros_like(t).index_add_(0, dst, w * t[src]) + diag * t
    t0 = x
    out = t0 @ weight[0]
    if weight.size(0) > 1:
        t1 = lap(t0)
        out = out + t1 @ weight[1]
        for k in range(2, int(weight.size(0))):
            t0, t1 = t1, 2 * lap(t1) - t0
            out = out + t1 @ weight[k]
    if bias is not None:
        out = out + bias
    a = _relu_tanh_id(act)
    return torch.relu(out) if a == 1 else (torch.tanh(out) if a == 2 else out)


class ChebConvFunction(torch.autograd.Function):
    """y = act(bias + sum_k Tx_k W_k) over a GraphCSR of the (source, target) edges and the norm of cheb_norm: K - 1 launches (one at
    K = 1; gml_cheb_fwd); Tx_1 .. Tx_{K-1} [N, (K - 1) Fin] are kept for the backward.  Backward: gml_cheb_bwd -- the row pass, K - 1
    adjoint steps over the source view, the fold; two launches when x needs no gradient (dx = NULL: the first layer of most models).
    No atomics, no host read: bit-reproducible, capturable.  Plain fp32 (exact_products() changes nothing)."""

    @staticmethod
    def forward(ctx, x, csr, norm, weight, bias, act=None):
        x, weight = _f32c(x, 'x'), _f32c(weight, 'weight')
        if x.dim() != 2 or weight.dim() != 3 or weight.size(1) != x.size(1):
            raise ValueError('ChebConv layer: x [N, Fin], weight [K, Fin, Fout] expected')
        N, Fin = int(x.size(0)), int(x.size(1))
        K, Fout = int(weight.size(0)), int(weight.size(2))
        if csr.N != N:
            raise ValueError('GraphCSR was built for %d nodes, x has %d rows' % (csr.N, N))
        norm = _f32c(norm, 'norm')
        if tuple(norm.shape) != (N, 2):
            raise ValueError('ChebConv layer: norm [N, 2] (functional.cheb_norm) expected')
        bias = None if bias is None else _f32c(bias, 'bias')
        a = _relu_tanh_id(act)
        dev = x.device
        with torch.cuda.device(dev):
            T = torch.empty(N, (K - 1) * Fin, dtype=torch.float32, device=dev) if K > 1 else None
            y = torch.empty(N, Fout, dtype=torch.float32, device=dev)
            with _Timed('cheb_fwd', q=4 * ((K - 1) * (csr.E + 3 * N) * Fin + N * Fin + (2 * K - 1) * N * Fout), f=2 * N * K * Fin * Fout):
                _lib.call('gml_cheb_fwd', _ptr(csr.rowptr), _ptr(csr.col), _ptr(norm), _ptr(x), Fin, N, csr.E, Fin, _ptr(weight),
                          _ptr(bias), Fout, K, a, _ptr(T), (K - 1) * Fin, _ptr(y), Fout, _stream(dev))
        ctx.csr, ctx.act, ctx.dims, ctx.has_bias = csr, a, (N, Fin, Fout, K), bias is not None
        ctx.save_for_backward(x, norm, weight, T, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, norm, weight, T, y = ctx.saved_tensors
        csr, (N, Fin, Fout, K) = ctx.csr, ctx.dims
        dev = x.device
        dy = _f32c(dy, 'grad of y')
        with torch.cuda.device(dev):
            dx = torch.empty(N, Fin, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
            flat, ws = _flat_and_ws('cheb', N, (Fin, Fout, K), dev)
            with _Timed('cheb_bwd'):
                _lib.call('gml_cheb_bwd', _ptr(csr.rowptr_t), _ptr(csr.col_t), _ptr(norm), _ptr(x), Fin, _ptr(T), (K - 1) * Fin, _ptr(y), Fout,
                          _ptr(dy), Fout, N, csr.E, Fin, _ptr(weight), Fout, K, ctx.act, _ptr(dx), Fin, _ptr(flat), _ptr(ws),
                          ws.numel() * 4, _stream(dev))
        nw = K * Fin * Fout
        return dx, None, None, flat[:nw].view(K, Fin, Fout), flat[nw:] if ctx.has_bias else None, None
