"""Dense-block evaluation of SpectConv for batches of equal-size graphs with near-dense masks (SURVEY s8f rank 3:
MNIST-75, recfield >= 3 -- the 4-hop mask of a 75-node superpixel graph is ~80 % full, so block-CSR degenerates to dense
blocks; the TF reference formulates the layer exactly this way, libs/layers_tf.py:231-236).

    Hcat[b n + j, s Fin + f] = sum_i D[b, s][j, i] X[b n + i, f]        gml_dense_support_mm  (csrc/gml_dense.hip)
    out                      = Hcat Wcat + bias                         one tall GEMM  [B n, S Fin] x [S Fin, Fout]

The batched support product is the hand-written part (one workgroup per graph, the supports streamed once from bf16
(hi, lo) images, bf16x3 on the matrix cores); its adjoint d X = sum_s D_s^T d Hcat_s is the same kernel on the transposed
images.  The tall GEMM and its two gradient GEMMs contract over S Fin = 384 .. 768 or over all nodes of the batch -- plain
library GEMM shapes, left to rocBLAS through torch.  ``GML_DENSE_LIB=1`` (or the exact-product mode GML_F32_MFMA=1, which
this kernel does not have) evaluates the support product with torch.bmm instead: the round-1 path, kept as the A/B
baseline of tools/bench_mnist.py.  Same parameters and values as ``SpectConv`` on the sparse path
(tests/test_gpu_parity.py compares both with the oracle and with the TF-graph fixture).

One LARGE graph (96 < n <= 1024, F <= 64: the 2-D grid of filtering.py, 900 nodes, a 40 % full mask) takes the same form on
csrc/gml_dense_big.hip: the work is cut across (support, row block, K slice) instead of across graphs, the projection stays the
tall GEMM (the chained one-launch kernels are n <= 96 only).

Batches of equal-size graphs of 96 < n <= 256 nodes (freqclass.py: bandclass graphs of 200 nodes, 2-hop masks 6-8 % full, S = 6,
layers 66 -> 64 + 2) take csrc/gml_dense_mid.hip: one workgroup per (graph, 64-row block, support), F <= 128 in one pass.  The
supports of the whole data set are packed once into an ``EqualSupports`` bank; a batch names its graphs by bank slot (gid), so a
batch is x, y and gid only -- a static shape without edge tensors (``DeviceDataset.batch_dense``).

Which of these serves a shape is decided in ONE place: ``dense_road`` (host integers in, a ``DenseRoad`` record out).
"""
import collections
import ctypes
import os

import torch

from . import _lib
from . import functional as Fn
from .graph import _ptr, _stream

USE_LIBRARY = os.environ.get('GML_DENSE_LIB', '0') not in ('0', '')


class DenseSupports(object):
    """Per-batch (in practice per-data-set: the supports are constants) dense support blocks of B graphs of n nodes.

    blocks [B, S, n, n] fp32 (row = target node j, column = source node i; only kept for the library path);
    fwd / bwd: bf16 (hi, lo) images [B, S, 2, n, KP] of the blocks / of their transposes (gml_dense_pack)."""

    def __init__(self, blocks, keep_blocks):
        B, S, n, _ = blocks.shape
        self.B, self.S, self.n = int(B), int(S), int(n)
        self.KP = (self.n + 31) // 32 * 32
        self.blocks = blocks if keep_blocks else None
        self.fwd, self.bwd = (None, None) if keep_blocks else (self._pack(blocks, 0), self._pack(blocks, 1))

    def _pack(self, blocks, transpose):
        img = torch.empty(self.B, self.S, 2, self.n, self.KP, dtype=torch.int16, device=blocks.device)
        _lib.call('gml_dense_big_pack' if self.n > SMALL_N else 'gml_dense_pack', _ptr(blocks), _ptr(img), self.B * self.S, self.n, self.KP, transpose, _stream(blocks.device))
        return img


def _library():
    return USE_LIBRARY or Fn.exact_mode()


SMALL_N, SMALL_F = 96, 128   # gml_dense.hip: one workgroup per graph of n <= SMALL_N nodes, F <= SMALL_F features
CHAIN_FOUT = 128             # and its one-launch layer (gml_dense_conv_fwd / _bwd_x): projections of up to CHAIN_FOUT columns
BIG_N, BIG_F = 1024, 64      # gml_dense_big.hip: ONE graph of SMALL_N < n <= BIG_N nodes, F <= BIG_F features
MID_N, MID_F = 256, 128      # gml_dense_mid.hip: B graphs (or a bank) of SMALL_N < n <= MID_N nodes each, F <= MID_F features

# product: what evaluates the support product -- 'library' (torch.bmm fp32), 'small' (gml_dense.hip), 'mid' (gml_dense_mid.hip),
#          'big' (gml_dense_big.hip), or None: no dense kernel covers the shape
# chained: _DenseConv serves the whole layer in one launch
# fmax:    the feature limit of the kernel of this size class (None: the library has none; 0: there is no such kernel)
# label:   the suffix of the Fn._path labels of _SupportProduct
DenseRoad = collections.namedtuple('DenseRoad', 'product chained fmax label')


def dense_road(num_graphs, n, Fin, Fout=None, bank=False, library=False):
    """DenseRoad of num_graphs graphs of n nodes with Fin features, from host integers and booleans only (no tensor, no launch).
    Fout: the width of the projection behind the product, None for a bare product.  bank: the supports are an EqualSupports bank.
    library: the library mode (_library()) is on -- it serves the size classes the kernels serve, at any Fin."""
    if 1 <= n <= SMALL_N:                                    # (any number of graphs)
        product, fmax, label = 'small', SMALL_F, ''
    elif SMALL_N < n <= BIG_N and num_graphs == 1 and not bank:
        product, fmax, label = 'big', BIG_F, ', large graph'
    elif SMALL_N < n <= MID_N and (num_graphs >= 2 or (bool(bank) and num_graphs >= 1)):
        product, fmax, label = 'mid', MID_F, ', batched blocks'
    else:
        return DenseRoad(None, False, 0, '')
    if library:
        return DenseRoad('library', False, None, '')
    covered = 1 <= Fin <= fmax
    return DenseRoad(product if covered else None, covered and product == 'small' and Fout is not None and Fout <= CHAIN_FOUT, fmax, label)


def big_applies(num_graphs, n, F):
    """True when the large-graph dense support product covers this batch (host integers only)."""
    return dense_road(num_graphs, n, F).product == 'big'


def mid_applies(num_graphs, n, F, bank=False):
    """True when the batched-blocks support product (csrc/gml_dense_mid.hip) covers this batch (host integers only): two or more
    graphs -- or any number of graphs that name their slots in a bank (EqualSupports) -- of SMALL_N < n <= MID_N nodes each."""
    return dense_road(num_graphs, n, F, bank=bank).product == 'mid'


def _coo_blocks(src, dst, val, g0, g1, S, n):
    """fp32 blocks [g1 - g0, S, n, n] of the graphs g0 .. g1 - 1 from COO supports with global node ids (graph = id // n):
    block[g, s][j, i] = value of edge i -> j"""
    b = torch.div(src, n, rounding_mode='floor')
    sel = (b >= g0) & (b < g1)
    src, dst, val, b = src[sel], dst[sel], val[sel], b[sel]
    blocks = torch.zeros(g1 - g0, S, n, n, dtype=torch.float32, device=val.device)
    blocks[b - g0, :, dst - b * n, src - b * n] = val
    return blocks


class EqualSupports(object):
    """Support bank of a data set of G graphs of EQUAL size n, SMALL_N < n <= MID_N (collated COO supports: edge_index2 [2, E] with
    global node ids, edge_attr2 [E, S], ptr [G + 1]; the mask lists every (i, j) once).  fwd / bwd: int16 [G, S, 2, n, KP] bf16
    (hi, lo) images of the blocks (row = target node) / of their transposes (gml_dense_big_pack), packed in slabs of graphs whose
    transient fp32 blocks stay below SLAB_BYTES; blocks: fp32 [G, S, n, n], built on first use -- the library road only
    (functional.exact_mode() / GML_DENSE_LIB=1).  A batch names its graphs by bank slot (attach_bank: gid)."""

    SLAB_BYTES = 256 << 20

    def __init__(self, edge_index2, edge_attr2, ptr):
        sizes = (ptr[1:] - ptr[:-1]).cpu().tolist()                # (one host read per data set)
        if not sizes or min(sizes) != max(sizes) or not SMALL_N < int(sizes[0]) <= MID_N:
            raise ValueError('the equal-size bank takes graphs of one size n, %d < n <= %d: got sizes %s .. %s over %d graphs'
                             % (SMALL_N, MID_N, min(sizes) if sizes else '-', max(sizes) if sizes else '-', len(sizes)))
        self.G = self.B = len(sizes)
        self.S, self.n = int(edge_attr2.size(1)), int(sizes[0])
        self.KP = (self.n + 31) // 32 * 32
        self._ei = edge_index2.to(torch.int64).contiguous()
        self._ea = edge_attr2.to(torch.float32).contiguous()
        self._blocks = None
        dev = self._ea.device
        G, S, n, KP = self.G, self.S, self.n, self.KP
        self.fwd = torch.empty(G, S, 2, n, KP, dtype=torch.int16, device=dev)
        self.bwd = torch.empty_like(self.fwd)
        slab = max(1, self.SLAB_BYTES // (4 * S * n * n))
        for g0 in range(0, G, slab):
            g1 = min(G, g0 + slab)
            blk = _coo_blocks(self._ei[0], self._ei[1], self._ea, g0, g1, S, n)
            for img, tr in ((self.fwd, 0), (self.bwd, 1)):
                _lib.call('gml_dense_big_pack', _ptr(blk), _ptr(img[g0:g1]), (g1 - g0) * S, n, KP, tr, _stream(dev))
            del blk

    @property
    def blocks(self):
        if self._blocks is None:
            self._blocks = _coo_blocks(self._ei[0], self._ei[1], self._ea, 0, self.G, self.S, self.n)
        return self._blocks


def dense_supports(edge_index2, edge_attr2, ptr, n):
    """DenseSupports of a batch whose graphs all have exactly n nodes (ptr [B+1]): block[b, s][j, i] = value of edge
    i -> j of support s (the mask lists every (i, j) once).  n <= SMALL_N: any number of graphs; ONE graph of up to BIG_N nodes;
    two or more graphs of up to MID_N nodes (the bank of the batch itself, slots in batch order)."""
    B = int(ptr.numel() - 1)
    S = int(edge_attr2.size(1))
    if B * n != int(ptr[-1]):
        raise ValueError('dense blocks need equal-size graphs: %d graphs, %d nodes, n=%d' % (B, int(ptr[-1]), n))
    if dense_road(B, n, 1).product is None:
        raise ValueError('dense blocks are built for n <= %d nodes per graph, graphs of up to %d nodes, or one graph of up to %d nodes: '
                         'got %d graphs of %d' % (SMALL_N, MID_N, BIG_N, B, n))
    src, dst = edge_index2[0], edge_index2[1]
    b = torch.div(src, n, rounding_mode='floor')
    i, j = src - b * n, dst - b * n
    blocks = torch.zeros(B, S, n, n, dtype=torch.float32, device=edge_attr2.device)
    blocks[b, :, j, i] = edge_attr2.float()
    return DenseSupports(blocks, keep_blocks=_library())


def batch_supports(data, n):
    """The DenseSupports of a batch of graphs of n nodes each, cached on the batch like its CSR (data._spT): built when missing, when
    they hold another n, or when they hold the side (fp32 blocks against packed images) the current mode does not read."""
    sp = getattr(data, '_spT', None)
    if sp is None or sp.n != n or (sp.blocks is None) == bool(_library()):
        sp = data._spT = dense_supports(data.edge_index2, data.edge_attr2, data.ptr, n)
    return sp


def _road(sup, rows, F, Fout=None, library=False):
    """dense_road of `rows` activation rows on these supports (a bank: of the graphs the rows name); ValueError where no kernel covers them"""
    bank = isinstance(sup, EqualSupports)
    B = rows // max(sup.n, 1) if bank else sup.B
    road = dense_road(B, sup.n, F, Fout, bank, library)
    if road.product is None:
        raise ValueError('no dense-block kernel covers %d graphs of n = %d nodes with Fin = %d (Fin <= %d at this size)' % (B, sup.n, F, road.fmax))
    return road


def support_mm(img, act, sup, F, sa, so, sum_s, gid=None):
    """gml_dense_support_mm on packed images: act [B n, >= F (+ s sa)] -> [B n, F] (sum_s) or [B n, S so].
    One graph of more than SMALL_N nodes: gml_dense_big_support_mm (csrc/gml_dense_big.hip); several, or a bank (EqualSupports) whose
    slots gid (int32 [B]; None = the first B slots in order) names: gml_dense_mid_support_mm (csrc/gml_dense_mid.hip)."""
    act = act.contiguous()
    product = _road(sup, int(act.size(0)), int(F)).product
    if product == 'mid':
        B = int(act.size(0)) // sup.n
        if B * sup.n != int(act.size(0)) or (gid is not None and int(gid.numel()) != B) or (gid is None and B > sup.B):
            raise ValueError('%d rows do not match %s graphs of %d nodes' % (int(act.size(0)), 'the bank slots of %d' % int(gid.numel())
                                                                             if gid is not None else 'at most %d' % sup.B, sup.n))
        out = torch.empty(B * sup.n, F if sum_s else sup.S * so, dtype=torch.float32, device=act.device)
        _lib.call('gml_dense_mid_support_mm', _ptr(img), _ptr(gid), _ptr(act), int(act.stride(0)), int(sa), _ptr(out), int(out.stride(0)),
                  int(so), int(bool(sum_s)), B, sup.B, sup.S, sup.n, sup.KP, int(F), _stream(act.device))
        return out
    if gid is not None:
        raise ValueError('bank slots (gid) go with an EqualSupports bank')
    out = torch.empty(sup.B * sup.n, F if sum_s else sup.S * so, dtype=torch.float32, device=act.device)
    if product == 'big':
        nws = int(_lib.lib().gml_dense_big_workspace_bytes(sup.S, sup.n, int(F), int(bool(sum_s))))
        ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=act.device)
        _lib.call('gml_dense_big_support_mm', _ptr(img), _ptr(act), int(act.stride(0)), int(sa), _ptr(out), int(out.stride(0)), int(so),
                  int(bool(sum_s)), sup.S, sup.n, sup.KP, int(F), _ptr(ws), nws, _stream(act.device))
        return out
    _lib.call('gml_dense_support_mm', _ptr(img), _ptr(act), int(act.stride(0)), int(sa), _ptr(out), int(out.stride(0)), int(so),
              int(bool(sum_s)), sup.B, sup.S, sup.n, sup.KP, int(F), _stream(act.device))
    return out


class _SupportProduct(torch.autograd.Function):
    """Hcat = [D_0 X | ... | D_{S-1} X] per graph; gradient d X = sum_s D_s^T d Hcat_s (the supports are constants)."""

    @staticmethod
    def forward(ctx, x, sup, gid=None):
        ctx.sup, ctx.Fin, ctx.gid = sup, int(x.size(1)), gid
        ctx.label = _road(sup, int(x.size(0)), ctx.Fin).label
        Fn._path('dense', 'support product fwd (bf16x3 HIP%s)' % ctx.label, sup.S, ctx.Fin, ctx.Fin)
        return support_mm(sup.fwd, x, sup, ctx.Fin, 0, ctx.Fin, False, gid)

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        Fn._path('dense', 'support product bwd (bf16x3 HIP%s)' % ctx.label, ctx.sup.S, ctx.Fin, ctx.Fin)
        return support_mm(ctx.sup.bwd, g, ctx.sup, ctx.Fin, ctx.Fin, 0, True, ctx.gid), None, None


def _splits(rows, lo=1024):
    """number of row slabs of the weight-gradient GEMM: the largest divisor of rows <= 64 that leaves slabs of >= lo rows"""
    for p in range(64, 1, -1):
        if rows % p == 0 and rows // p >= lo:
            return p
    return 1


class _TallGemm(torch.autograd.Function):
    """out = h w + bias for h [B n, S Fin] (hundreds of thousands of rows), w [S Fin, Fout].  Forward and d h are library
    GEMMs as they are; d w = h^T g contracts over ALL rows into a 768 x 128 result, which rocBLAS tiles into ~24
    workgroups (352 us at 76,800 rows, profiles/r02_mnist75_*): it is evaluated as a batched GEMM over row slabs
    (every CU busy) followed by a fixed-order sum of the slab results."""

    @staticmethod
    def forward(ctx, h, w, bias):
        ctx.save_for_backward(h, w)
        ctx.has_bias = bias is not None
        return h.mm(w) if bias is None else torch.addmm(bias, h, w)

    @staticmethod
    def backward(ctx, g):
        h, w = ctx.saved_tensors
        g = g.contiguous()
        dh = g.mm(w.t()) if ctx.needs_input_grad[0] else None
        dw = None
        if ctx.needs_input_grad[1]:
            rows = int(h.size(0))
            P = _splits(rows)
            dw = torch.bmm(h.view(P, rows // P, h.size(1)).transpose(1, 2), g.view(P, rows // P, g.size(1))).sum(0) if P > 1 else h.t().mm(g)
        db = g.sum(0) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return dh, dw, db


# Weight gradient: by default Hcat is written in the forward and dW = Hcat^T g runs as a row-slab batched library GEMM (rounds 2-4).
# GML_DENSE_DW_HIP=1: gml_dense_conv_bwd_w (round 5) -- no Hcat, the support product recomputed per graph and contracted with g on the
# matrix cores, hand-written.  Parity-tested, but SLOWER (MNIST-75 step at 4,096 graphs: 5.5 ms against 3.6 ms; 1,024 graphs: 1.55 against
# 1.19): a workgroup per (support, 64-column block, graph slice) recomputes the product per column block and pays the full load
# latency per graph (208 VGPRs at Fin = 128: one workgroup per CU).  What it needs is in DESIGN s8.
DW_LIBRARY = os.environ.get('GML_DENSE_DW_HIP', '0') in ('0', '')


class _DenseConv(torch.autograd.Function):
    """out = sum_s (D_s X) W_s + bias in ONE launch: the support product's accumulators are the projection's operand
    (csrc/gml_dense.hip: gml_k_dense_conv_fwd), as libs/layers_tf.py:231-236 forms the layer.  Hcat is written only as the
    saved tensor of the weight gradient dW = Hcat^T g (gml_xty_wide, or the row-slab batched GEMM of _TallGemm where it does not
    apply); dX = sum_s D_s^T (g W_s^T) is one launch on the transposed images (gml_k_dense_conv_bwdx)."""

    @staticmethod
    def forward(ctx, x, weight, bias, sup, relu=False):
        S, Fin, Fout = weight.shape
        x = x.contiguous()
        dev = x.device
        rows = sup.B * sup.n
        wimg = torch.empty(int(_lib.lib().gml_dense_wimg_elems(S, Fin, Fout)), dtype=torch.int16, device=dev)
        _lib.call('gml_dense_pack_w', _ptr(weight.contiguous()), _ptr(wimg), S, Fin, Fout, _stream(dev))
        need_h = ctx.needs_input_grad[1] and DW_LIBRARY           # (round 5: the weight gradient recomputes the support product -- no Hcat)
        hcat = torch.empty(rows, S * Fin, dtype=torch.float32, device=dev) if need_h else None
        out = torch.empty(rows, Fout, dtype=torch.float32, device=dev)
        Fn._path('dense', 'support product + projection chained (bf16x3 HIP)', S, Fin, Fout)
        # algorithmic bytes: the packed support images (bf16 hi + lo), x, out, and Hcat when the weight gradient wants it
        q_img = sup.B * S * 2 * sup.n * sup.KP * 2
        with Fn._Timed('dense_conv_fwd', q_img + 4 * rows * (Fin + Fout + (S * Fin if need_h else 0)), 2 * sup.B * S * sup.n * sup.n * Fin + 2 * rows * S * Fin * Fout,
                       q2=q_img + 4 * rows * (Fin + Fout)):                 # compulsory: without the Hcat this design writes for its own dW
            _lib.call('gml_dense_conv_fwd', _ptr(sup.fwd), _ptr(x), int(x.stride(0)), _ptr(wimg), _ptr(bias), _ptr(out), Fout,
                      _ptr(hcat), sup.B, S, sup.n, sup.KP, Fin, Fout, 1 if relu else 0, _stream(dev))
        # relu (round 5): applied in the kernel's epilogue (libs/layers_tf.py:238: act(output)); the backward's mask and the bias
        # gradient come out of ONE pass over g and the saved output (functional.ml3_split_bwd) -- before: a relu launch forward, a
        # threshold launch and a column sum backward, 1.6 GB of elementwise traffic per MNIST-75 step at 4,096 graphs
        ctx.save_for_backward(hcat if hcat is not None else x, weight, out if relu else None)
        ctx.sup, ctx.has_bias, ctx.has_h, ctx.relu = sup, bias is not None, hcat is not None, bool(relu)
        return out

    @staticmethod
    def backward(ctx, g):
        hcat, weight, yout = ctx.saved_tensors
        sup = ctx.sup
        S, Fin, Fout = weight.shape
        g = g.contiguous()
        dx = dw = db = None
        if ctx.relu:
            r = Fn.ml3_split_bwd(g, yout, Fout, need_dcb=ctx.has_bias and ctx.needs_input_grad[2])
            if r is not None:
                g = r[0]
                db = r[2]
                if not g.is_contiguous():
                    g = g.contiguous()
            else:
                g = g * (yout > 0)
        if ctx.needs_input_grad[0]:
            # dX = sum_s D_s^T (g W_s^T) in one launch: d Hcat stays on the CU (gml_k_dense_conv_bwdx)
            dev = g.device
            wimgT = torch.empty(int(_lib.lib().gml_dense_wimgt_elems(S, Fin, Fout)), dtype=torch.int16, device=dev)
            _lib.call('gml_dense_pack_wt', _ptr(weight.contiguous()), _ptr(wimgT), S, Fin, Fout, _stream(dev))
            dx = torch.empty(sup.B * sup.n, Fin, dtype=torch.float32, device=dev)
            Fn._path('dense', 'projection + support product chained, backward (bf16x3 HIP)', S, Fin, Fout)
            with Fn._Timed('dense_conv_bwd_x', sup.B * S * 2 * sup.n * sup.KP * 2 + 4 * sup.B * sup.n * (Fin + Fout),
                           2 * sup.B * S * sup.n * sup.n * Fin + 2 * sup.B * sup.n * S * Fin * Fout):
                _lib.call('gml_dense_conv_bwd_x', _ptr(sup.bwd), _ptr(g), int(g.stride(0)), _ptr(wimgT), _ptr(dx), Fin,
                          sup.B, S, sup.n, sup.KP, Fin, Fout, _stream(dev))
        if ctx.needs_input_grad[1] and not ctx.has_h:
            # dW = sum over the graphs of (D_s X)^T g: the support product recomputed on the matrix cores, contracted with g over the graph's
            # rows, no Hcat in HBM and no library GEMM (gml_dense_conv_bwd_w, csrc/gml_dense.hip)
            x, dev = hcat, g.device
            Fn._path('dense', 'weight gradient: support product recomputed + row contraction (bf16x3 HIP)', S, Fin, Fout)
            ws = torch.empty(max(int(_lib.lib().gml_dense_dw_workspace_bytes(sup.B, S, Fin, Fout)), 4), dtype=torch.uint8, device=dev)
            dw = torch.empty(S, Fin, Fout, dtype=torch.float32, device=dev)
            _lib.call('gml_dense_conv_bwd_w', _ptr(sup.fwd), _ptr(x), int(x.stride(0)), _ptr(g), int(g.stride(0)), _ptr(dw), sup.B, S, sup.n,
                      sup.KP, Fin, Fout, _ptr(ws), ws.numel(), _stream(dev))
        elif ctx.needs_input_grad[1]:
            rows = int(hcat.size(0))
            P = _splits(rows)
            # round 5: Hcat^T g on the bf16 matrix cores (gml_xty_wide); a shape it does not take (None): the library GEMM
            with Fn._Timed('dense_dw_xty_wide', 4 * rows * (S * Fin + Fout), 2 * rows * S * Fin * Fout, q2=4 * rows * (Fin + Fout)):
                dw = Fn.xty_wide(hcat, g)
            dw = dw.view(S, Fin, Fout) if dw is not None else None
            if dw is None:
                with Fn._Timed('dense_dw_library_gemm', 4 * rows * (S * Fin + Fout), 2 * rows * S * Fin * Fout):
                    dw = (torch.bmm(hcat.view(P, rows // P, S * Fin).transpose(1, 2), g.view(P, rows // P, Fout)).sum(0) if P > 1
                          else hcat.t().mm(g)).view(S, Fin, Fout)
        if ctx.has_bias and ctx.needs_input_grad[2] and db is None:
            db = g.sum(0)
        return dx, dw, db, None, None


def spectconv_dense(x, sup, weight, bias, n, relu=False, gid=None):
    """x [B*n, Fin], sup from dense_supports, weight [S, Fin, Fout] -> [B*n, Fout] = act(sum_s (D_s x) W_s + bias), act = relu or none.
    sup an EqualSupports bank: gid int32 [B] names the bank slot of every graph of x (None: the bank's first B graphs in order).
    The road is dense_road's under the library mode of this call; supports built in the other mode raise ValueError."""
    S, Fin, Fout = weight.shape
    bank = isinstance(sup, EqualSupports)
    B = int(x.size(0)) // max(n, 1) if bank else sup.B
    if sup.n != n or sup.S != S or x.size(0) != B * n or (gid is not None and (not bank or int(gid.numel()) != B)) or (gid is None and B > sup.B):
        raise ValueError('supports [%d graphs, S=%d, n=%d] do not match x %s / weight %s%s' %
                         (sup.B, sup.S, sup.n, tuple(x.shape), tuple(weight.shape), '' if gid is None else ' / %d bank slots' % int(gid.numel())))
    road = _road(sup, int(x.size(0)), Fin, Fout, _library())   # the mode of THIS call decides (GML_DENSE_LIB=1 / GML_F32_MFMA=1), not sup's
    library = road.product == 'library'
    if (sup.blocks if library else sup.fwd) is None:
        raise ValueError('these supports were built %s the library mode (GML_DENSE_LIB=1 / exact products) and this call runs %s it: '
                         'rebuild them in the mode they are used in (dense_supports / batch_supports)' % (('outside', 'inside') if library else ('inside', 'outside')))
    if library:
        Fn._path('dense', 'support product (torch.bmm fp32)', S, Fin, Fout)
        D = sup.blocks if not bank else (sup.blocks[:B] if gid is None else sup.blocks[gid.long()])
        h = torch.bmm(D.reshape(B, S * n, n), x.view(B, n, Fin))
        h = h.view(B, S, n, Fin).permute(0, 2, 1, 3).reshape(B * n, S * Fin)
    elif road.chained:
        return _DenseConv.apply(x, weight, bias, sup, relu)
    else:
        h = _SupportProduct.apply(x, sup, gid)
    out = _TallGemm.apply(h, weight.reshape(S * Fin, Fout), bias)
    return torch.relu(out) if relu else out


# ---------------------------------------------------------------------------- graphs of different sizes (csrc/gml_dense_rag.hip)
# The TF GNNML3 of enzymes_contfeats_gnnml3_tf.py (libs/models_tf.py:275-343, libs/layers_tf.py:276-298): dense per-graph blocks
# matmul(dropout(support[:, i]), x) over ENZYMES graphs of 2 .. 126 nodes whose recfield-5 masks are 97 % full.  The supports of the
# whole data set are packed ONCE into a bank of bf16 (hi, lo) images [G, S, 2, 128, 128]; a batch names its graphs by bank slot
# (gid), its node rows stay compact, and the kernel walks only the row tiles and K steps each graph has.
RAG_NP = 128                 # gml_dense_rag.hip: at most 128 nodes per graph
RAG_F = 256                  # and at most 256 features per product


class RaggedSupports(object):
    """Support bank of a data set of G graphs (collated COO supports: edge_index2 [2, E] with global node ids, edge_attr2 [E, S],
    batch [N], ptr [G + 1]).  fwd / bwd: int16 [G, S, 2, 128, 128] bf16 (hi, lo) images of the blocks (row = target node) / of their
    transposes (gml_dense_rag_pack); sizes: the node counts as host integers; blocks: fp32 [G, S, 128, 128], built on first use --
    the library road only (functional.exact_mode())."""

    def __init__(self, edge_index2, edge_attr2, batch, ptr):
        sizes = (ptr[1:] - ptr[:-1]).cpu().tolist()
        for g, n in enumerate(sizes):
            if n > RAG_NP:
                raise ValueError('graph %d has %d nodes: the ragged dense blocks take at most %d per graph' % (g, n, RAG_NP))
        self.G, self.S, self.sizes = len(sizes), int(edge_attr2.size(1)), [int(n) for n in sizes]
        dev = edge_attr2.device
        self._ei = edge_index2.to(torch.int64).contiguous()
        self._ea = edge_attr2.to(torch.float32).contiguous()
        self._batch = batch.to(torch.int64).contiguous()
        self.ptr = Fn._ptr32(ptr)
        self._blocks = None
        self.fwd = torch.empty(self.G, self.S, 2, RAG_NP, RAG_NP, dtype=torch.int16, device=dev)
        self.bwd = torch.empty_like(self.fwd)
        _lib.call('gml_dense_rag_pack', _ptr(self._ei), _ptr(self._ea), _ptr(self._batch), _ptr(self.ptr), _ptr(self.fwd), _ptr(self.bwd),
                  int(self._ei.size(1)), int(self._batch.numel()), self.G, self.S, _stream(dev))

    @property
    def blocks(self):
        if self._blocks is None:
            src, dst = self._ei[0], self._ei[1]
            g = self._batch[src]
            off = self.ptr.to(torch.int64)[g]
            blk = torch.zeros(self.G, self.S, RAG_NP, RAG_NP, dtype=torch.float32, device=self._ea.device)
            blk[g, :, dst - off, src - off] = self._ea
            self._blocks = blk
        return self._blocks


def attach_bank(batch, bank, gid=None):
    """batch with the fields a bank-reading dense model reads: bank (RaggedSupports or EqualSupports) and gid (int32 [B] on the bank's device: the bank slot
    of every graph of the batch; None = the batch is the bank's first B graphs in order)."""
    batch.bank, batch.gid = bank, (None if gid is None else gid.to(torch.int32).contiguous())
    return batch


def ragged_keep_bits(ptr, B, S, p, state, site, need_bwd=True):
    """(mask_fwd, mask_bwd or None, scale): the keep bits of one dropout site over the support entries of a batch of B graphs,
    int32 [B, S, 128, 4] each way (gml_dense_rag_mask; include/gml.h has the element index)."""
    t, scale = Fn.dropout_threshold(p)
    dev = ptr.device
    mf = torch.empty(B, S, RAG_NP, 4, dtype=torch.int32, device=dev)
    mb = torch.empty_like(mf) if need_bwd else None
    _lib.call('gml_dense_rag_mask', _ptr(ptr), _ptr(mf), _ptr(mb), B, S, ctypes.c_uint64(t), _ptr(state),
              ctypes.c_uint32(int(site) & 0xffffffff), _stream(dev))
    return mf, mb, scale


def ragged_support_mm(img, mask, scale, gid, ptr, act, G, S, F, sa, so, sum_s):
    """gml_dense_rag_support_mm: act [N, >= F (+ s sa)] -> [N, F] (sum_s) or [N, S so] on the compact node rows of the batch."""
    act = act.contiguous()
    out = torch.empty(int(act.size(0)), F if sum_s else S * so, dtype=torch.float32, device=act.device)
    _lib.call('gml_dense_rag_support_mm', _ptr(img), _ptr(mask), ctypes.c_float(scale), _ptr(gid), _ptr(ptr), _ptr(act), int(act.stride(0)),
              int(sa), _ptr(out), int(out.stride(0)), int(so), int(bool(sum_s)), int(ptr.numel() - 1), int(S), int(G), int(F),
              _stream(act.device))
    return out


class _RaggedProduct(torch.autograd.Function):
    """Hcat = [(D_0 o M_0) X | ... ] per graph (M: the keep bits times scale, or all ones); d X = sum_s (D_s o M_s)^T d Hcat_s on the
    transposed images with the transposed bits the forward saved."""

    @staticmethod
    def forward(ctx, x, bank, gid, ptr, mf, mb, scale):
        ctx.bank, ctx.gid, ctx.ptr, ctx.mb, ctx.scale, ctx.Fin, ctx.masked = bank, gid, ptr, mb, scale, int(x.size(1)), mf is not None
        Fn._path('dense', 'ragged support product fwd (bf16x3 HIP)', bank.S, ctx.Fin, ctx.Fin)
        return ragged_support_mm(bank.fwd, mf, scale, gid, ptr, x, bank.G, bank.S, ctx.Fin, 0, ctx.Fin, False)

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return (None,) * 7
        if ctx.masked and ctx.mb is None:
            raise RuntimeError('the transposed keep bits were not produced: x did not require a gradient in the forward')
        bank = ctx.bank
        Fn._path('dense', 'ragged support product bwd (bf16x3 HIP)', bank.S, ctx.Fin, ctx.Fin)
        return (ragged_support_mm(bank.bwd, ctx.mb, ctx.scale, ctx.gid, ctx.ptr, g, bank.G, bank.S, ctx.Fin, ctx.Fin, 0, True),) + (None,) * 6


def _ragged_library(x, bank, gid, ptr, mf, scale):
    """The library road: the same product by torch in fp32 on blocks padded to 128 (torch.bmm + the elementwise mask from the SAME
    keep bits); autograd differentiates it.  No host read: the pad positions come from ptr on the device."""
    B, S, N, Fin = int(ptr.numel() - 1), bank.S, int(x.size(0)), int(x.size(1))
    dev = x.device
    D = bank.blocks[:B] if gid is None else bank.blocks[gid.long()]
    if mf is not None:
        sh = torch.arange(32, device=dev, dtype=torch.int32)
        keep = ((mf.view(B, S, RAG_NP, 4, 1) >> sh) & 1).view(B, S, RAG_NP, RAG_NP)
        D = D * keep.to(torch.float32) * scale
    p64 = ptr.to(torch.int64)
    r = torch.arange(RAG_NP, device=dev)
    valid = r.unsqueeze(0) < (p64[1:] - p64[:-1]).unsqueeze(1)                       # [B, 128]
    rows = (p64[:-1].unsqueeze(1) + r.unsqueeze(0)).clamp_(max=max(N - 1, 0))
    xpad = x[rows.reshape(-1)].view(B, RAG_NP, Fin) * valid.unsqueeze(2).to(x.dtype)
    h = torch.bmm(D.reshape(B, S * RAG_NP, RAG_NP), xpad).view(B, S, RAG_NP, Fin).permute(0, 2, 1, 3)   # [B, 128, S, Fin]
    node = torch.arange(N, device=dev)
    b = torch.searchsorted(p64[1:].contiguous(), node, right=True)
    return h.reshape(B * RAG_NP, S * Fin)[b * RAG_NP + (node - p64[b])]


def spectconv_ragged(x, bank, gid, ptr, weight, bias=None, relu=False, p=0.0, state=None, site=0, training=False):
    """act(sum_s ((D_s o M_s) x) W_s + bias) on the compact node rows x [N, Fin] of a batch of graphs of different sizes: bank
    (RaggedSupports), gid int32 [B] (bank slot per graph, None = identity), ptr int32 [B + 1], weight [S, Fin, Fout].  M_s: dropout
    of the support entries with probability p (training and p > 0: one gml_dense_rag_mask launch with the RNG state `state` and
    `site`; otherwise no mask launch).  The projection is _TallGemm (its dW = Hcat^T g is a library GEMM: gml_xty_wide stops at 128
    output columns and these layers are 200 wide).  functional.exact_mode(): the library road (_ragged_library)."""
    S, Fin, Fout = weight.shape
    if S != bank.S or Fin != x.size(1):
        raise ValueError('bank with S=%d does not match x %s / weight %s' % (bank.S, tuple(x.shape), tuple(weight.shape)))
    ptr = Fn._ptr32(ptr)
    B = int(ptr.numel() - 1)
    x = x.contiguous()
    mf = mb = None
    scale = 1.0
    lib = _library()
    if training and p > 0:
        mf, mb, scale = ragged_keep_bits(ptr, B, S, p, state, site, need_bwd=x.requires_grad and not lib)
    if lib:
        Fn._path('dense', 'ragged support product (torch.bmm fp32)', S, Fin, Fout)
        h = _ragged_library(x, bank, gid, ptr, mf, scale)
    else:
        if Fin > RAG_F:
            raise ValueError('the ragged dense-block kernel covers Fin <= %d, got %d' % (RAG_F, Fin))
        h = _RaggedProduct.apply(x, bank, gid, ptr, mf, mb, scale)
    out = _TallGemm.apply(h, weight.reshape(S * Fin, Fout), bias)
    return torch.relu(out) if relu else out
