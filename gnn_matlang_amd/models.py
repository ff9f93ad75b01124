"""GNNML1 / GNNML3 model assemblies of the BASELINE configs on top of the MI355X layers.

The reference defines these classes inside its experiment scripts with hard-coded sizes
(Zinc12k.py:310-345, counting.py:335-372, sr25.py:248-278, mutag.py:214-309); here they are one
configurable class each with the same attribute names, so ``state_dict`` keys match the reference's.
``forward`` takes a ``gnn_matlang_amd.Batch`` (PyG-compatible field names: x, edge_index,
edge_index2, edge_attr2, batch, ptr, y).
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

from . import functional as Fn
from .functional import segment_bcast, segment_max, segment_max_bwd, segment_sum, skip_last_mask, tall_linear, _ptr32
from .spect_conv import ML3Layer, SpectConv
from .dist import SyncBatchNorm1d


class BatchNorm1d(torch.nn.BatchNorm1d):
    """torch.nn.BatchNorm1d (same parameters, buffers, state_dict keys: mutag.py:272-288) whose TRAINING pass over a float32 CUDA
    [N, C] input runs on csrc/gml_bn.hip (C <= 64, C % 4 == 0, float4-addressable rows); eval mode, other shapes and dtypes: the
    base class.  GML_TORCH_BN=1 in the environment: always the base class (A/B)."""

    def forward(self, x, valid=None):
        """valid: None (a plain batch: every row counts) or the row validity of a padded static batch (float [N], nonzero = a real row):
        training statistics, running statistics and gradients then cover the valid rows only (gml_bn_masked_*), y is zero elsewhere."""
        if valid is not None:
            return self._forward_masked(x, valid)
        import os
        if not (self.training or self.running_mean is None) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 \
                or x.size(1) > 64 or x.size(1) % 4 or x.stride(1) != 1 or x.stride(0) % 4 or x.stride(0) < x.size(1) or x.data_ptr() % 16 \
                or x.size(0) < 2 \
                or os.environ.get('GML_TORCH_BN'):
            return super().forward(x)
        from .functional import BatchNormFunction
        y, stats = BatchNormFunction.apply(x, self.weight, self.bias, self.eps)
        if self.training and self.running_mean is not None:
            with torch.no_grad():
                self.num_batches_tracked += 1
                m = self.momentum if self.momentum is not None else 1.0 / float(self.num_batches_tracked)
                n = x.size(0)
                self.running_mean.mul_(1 - m).add_(stats[0], alpha=m)
                self.running_var.mul_(1 - m).add_(stats[1], alpha=m * n / (n - 1))
        return y

    def _forward_masked(self, x, valid):
        valid = valid.to(torch.float32).contiguous()
        if not self.training and self.running_mean is not None:
            return super().forward(x) * (valid != 0).to(x.dtype).unsqueeze(1)      # running statistics: row by row
        if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or valid.numel() != x.size(0) or x.size(1) > 64 or x.size(1) % 4 \
                or x.stride(1) != 1 or x.stride(0) % 4 or x.stride(0) < x.size(1) or x.data_ptr() % 16:
            raise NotImplementedError('BatchNorm over a padded batch runs on csrc/gml_bn.hip only: float32 CUDA [N, C <= 64], C % 4 == 0, '
                                      'float4-addressable rows, one validity entry per row')
        if self.momentum is None and self.running_mean is not None:
            raise NotImplementedError('BatchNorm over a padded batch: momentum=None (a cumulative average) needs a host read')
        from .functional import MaskedBatchNormFunction, bn_masked_running_update
        y, stats, count = MaskedBatchNormFunction.apply(x, valid, self.weight, self.bias, self.eps)
        if self.running_mean is not None:
            with torch.no_grad():
                self.num_batches_tracked += 1
                bn_masked_running_update(count, stats, self.momentum, self.running_mean, self.running_var)
        return y


def _node_valid(data):
    """float [N]: 1 for the real nodes of a padded static batch, 0 for its padding nodes (graph B = the last one); cached on the batch."""
    v = getattr(data, '_node_valid', None)
    if v is None:
        v = data._node_valid = (data.batch != int(data.ptr.numel()) - 2).to(torch.float32)
    return v


def _adjacency(data):
    """data.csr('edge_index'): a padded static batch has it only when built with adjacency=True -- fail loudly otherwise (the support
    edges are not the raw adjacency)."""
    if getattr(data, 'pad_graph', False) and 'edge_index' not in data._csr and getattr(data, 'edge_index', None) is None:
        raise ValueError('this model reads the raw adjacency (edge_index): build the padded batch with adjacency=True '
                         '(DeviceDataset.batch_padded / batch_assembled / epoch_static)')
    return data.csr('edge_index')


class _SegmentPool(torch.autograd.Function):
    """global_add_pool / global_mean_pool (torch_geometric.nn, used at Zinc12k.py:343, mutag.py:307)."""

    @staticmethod
    def forward(ctx, x, ptr, batch, mean):
        ctx.save_for_backward(ptr, batch)
        ctx.mean = mean
        out = segment_sum(x.contiguous(), ptr, mean)
        if int(mean) & 2:
            skip_last_mask(out)
        return out

    @staticmethod
    def backward(ctx, g):
        ptr, batch = ctx.saved_tensors
        g = g.contiguous()
        if int(ctx.mean) & 2:          # GML_POOL_SKIP_LAST: the padding graph's row does not depend on x -- no gradient to its nodes
            g = g * skip_last_mask(g)
        return segment_bcast(g, ptr, batch.numel(), bool(int(ctx.mean) & 1)), None, None, None


class _SegmentMax(torch.autograd.Function):
    """global_max_pool (torch_geometric.nn, used at /root/reference/enzymes.py:384): the gradient goes to the arg-max row."""

    @staticmethod
    def forward(ctx, x, ptr):
        out, arg = segment_max(x.contiguous(), ptr)
        ctx.save_for_backward(ptr, arg)
        ctx.nrows = x.size(0)
        return out

    @staticmethod
    def backward(ctx, g):
        ptr, arg = ctx.saved_tensors
        return segment_max_bwd(g.contiguous(), ptr, arg, ctx.nrows), None


def global_max_pool(x, data):
    return _SegmentMax.apply(x, data.ptr)


def _pad_flag(data):
    return 2 if getattr(data, 'pad_graph', False) else 0       # GML_POOL_SKIP_LAST: the padding graph of a static-shape batch


def global_add_pool(x, data):
    return _SegmentPool.apply(x, data.ptr, data.batch, _pad_flag(data))


def global_mean_pool(x, data):
    return _SegmentPool.apply(x, data.ptr, data.batch, 1 | _pad_flag(data))


_POOLS = dict(add=global_add_pool, mean=global_mean_pool, max=global_max_pool)


def _pool(pool, x, data):
    """pool: a name of _POOLS, or a tuple of names -- torch.cat of those pools in that column order (ptc.py:361: mean | max,
    enzymes.py:384: add | max).  On a padded static batch the padding graph's max row is whatever its nodes hold: the loss masks it."""
    if isinstance(pool, tuple):
        return torch.cat([_POOLS[p](x, data) for p in pool], 1)
    return _POOLS[pool](x, data)


def _init_dropout(model, p):
    """model.dropout = p; p > 0: the RNG state as a NON-persistent buffer `dropout_state` (int64 {seed, counter}: the reference's
    state_dict loads with strict=True, .to() moves it), its seed drawn from torch's default generator (torch.manual_seed decides it).
    Reset it with model.dropout_state.copy_(...) or functional.dropout_state(seed, device)."""
    Fn.dropout_threshold(p)                                      # ValueError outside [0, 1]
    model.dropout = float(p)
    if model.dropout > 0:
        seed = int(torch.randint(-2 ** 63, 2 ** 63 - 1, (), dtype=torch.int64))
        model.register_buffer('dropout_state', torch.tensor([seed, 0], dtype=torch.int64), persistent=False)


def _dropout_pass(model):
    """True for a training forward of a model with dropout: the counter advances once (a device-side add: captured with the step,
    so every forward, eager or replayed, draws fresh masks)."""
    if not (model.training and model.dropout > 0):
        return False
    model.dropout_state[1:].add_(1)
    return True


# The heads of GNNML3, GNNML1Blocks and GAT, each described once: out(fc2(between(fc1(bn1 x)))) without the pieces it leaves out.
#   bn1      a plain torch.nn.BatchNorm1d of the pooled rows in front (the name is the head's: no block / layer BatchNorms beside it)
#   fc1      its width: a number, 'nclass', 'hidden' (the constructor's, required > 0), 'hidden?' (declared when hidden > 0) or None
#   between  'relu' or None, on fc1's output
#   fc2      whether there is one (its width: nclass)
#   out      None, 'tanh' or 'log_softmax'
# Each class maps the names it accepts to these rows (its _HEADS).
_Head = namedtuple('_Head', 'bn1 fc1 between fc2 out')
_MLP32 = _Head(False, 32, 'relu', True, None)                   # Zinc12k.py:306-307, freqclass.py:298-300, mutag.py:264-266
_MLP = _Head(False, 'hidden', 'relu', True, None)               # exp_classify.py:280-281, Zinc12k.py:244-245, counting.py:264-266
_LIN2 = _Head(False, 'hidden', None, True, None)                # counting.py:332-333, exp_classify.py:240-241: NO activation
_TANH10 = _Head(False, 10, None, False, 'tanh')                 # sr25.py:248-278 (nclass is not read)
_TANH = _Head(False, 'nclass', None, False, 'tanh')             # sr25.py:189
_LIN10 = _Head(False, 'nclass', None, False, None)              # sr25.py, graph8c.py: fc1 x and nothing else
_LOG_SOFTMAX = _Head(False, 'hidden?', 'relu', True, 'log_softmax')   # ptc.py:270-271, :323-363, enzymes.py:276, proteins.py:259-289
_BN_MLP32 = _Head(True, 32, 'relu', True, 'log_softmax')        # mnist75.py:262-326
_BN_MLP = _Head(True, 'hidden', 'relu', True, 'log_softmax')    # mnist75.py:144-148
_NODE = _Head(False, None, None, True, None)                    # filtering.py:198, :231, :250: fc2 on every NODE row, with pool=None


def _declare_head(model, nin, hidden, nclass):
    """bn1, fc1, fc2 of model._HEADS[model.head] on the model, in that order and under those names (the reference's state_dict keys)"""
    h = model._HEADS[model.head]
    if h.fc1 == 'hidden' and not hidden > 0:
        raise ValueError("head='%s' needs hidden > 0 (fc1: nin -> hidden, fc2: hidden -> nclass)" % model.head)
    width = {'hidden': hidden, 'hidden?': hidden, 'nclass': nclass}.get(h.fc1, h.fc1)
    if h.bn1:
        model.bn1 = torch.nn.BatchNorm1d(nin)
    if width:
        model.fc1 = torch.nn.Linear(nin, width)
    if h.fc2:
        model.fc2 = torch.nn.Linear(width or nin, nclass)


def _apply_head(model, x, _capture=None):
    """model._HEADS[model.head] on the rows x; _capture: a dict that receives fc1's pre-activation as 'head_pre'"""
    h = model._HEADS[model.head]
    if h.bn1:
        x = model.bn1(x)
    if hasattr(model, 'fc1'):
        x = tall_linear(x, model.fc1)
        if _capture is not None:
            _capture['head_pre'] = x.detach()                  # (the parity checker takes the head's relu mask from here)
        if h.between == 'relu':
            x = F.relu(x)
    if h.fc2:
        x = tall_linear(x, model.fc2)
    if h.out == 'tanh':
        return torch.tanh(x)
    return F.log_softmax(x, dim=1) if h.out == 'log_softmax' else x


def _bn_valid(model, data, has_bn):
    """what the bnI of a training forward get as valid=: the row validity of a padded static batch (real nodes only), None otherwise"""
    return _node_valid(data) if getattr(data, 'pad_graph', False) and model.training and has_bn else None


def _layer_bn(model, i, x, nvalid):
    bn = getattr(model, 'bn%d' % i)
    return bn(x) if nvalid is None else bn(x, valid=nvalid)


# Road choice of a node-level GNNML3 on ONE large graph (gnnml3_road): the dense road (dense_block.py on
# csrc/gml_dense_big.hip) is taken from this mask fill E / N^2 upwards.  Measured (tools/bench_filtering.py,
# profiles/filtering_twodgrid.json: one ML3 layer 48 -> 32 + 16 forward + backward on the 30 x 30 grid, S = 11, ms sparse / dense,
# both roads alternating in one process):
#     recfield 2, fill 0.0137: 0.405 / 0.633      recfield 3, fill 0.0412: 0.794 / 0.741
#     recfield 4, fill 0.1319: 2.010 / 0.673      recfield 5, fill 0.3990: 6.609 / 0.797
# The sparse road is faster at fill 0.0137, the dense road from 0.0412 upwards (1.07 x there, 3.0 x at 0.13, 8.3 x at the filtering
# graph's own 0.40): the constant sits between the two.
DENSE_BIG_MIN_FILL = 0.025

# The road of ONE GNNML3 forward.  kind: 'sparse' (CSR kernels), 'dense_n' (the model's own equal-size blocks), 'big' (ONE large
# graph, csrc/gml_dense_big.hip) or 'mid' (the slots of an EqualSupports bank, csrc/gml_dense_mid.hip); chain: whether the relu
# hand-over between stacked sparse layers is declared for this call.
GNNML3Road = namedtuple('GNNML3Road', 'kind chain')


def gnnml3_road(head, dense_n, bn, learnedge, fmax, chain, num_graphs, N, E, pad_graph, bank, road=None, drop=False, min_fill=DENSE_BIG_MIN_FILL):
    """GNNML3Road from plain values only (no tensor, no launch).  The model: head, dense_n, bn, any learnedge, its widest conv input
    fmax, GNNML3._chain.  The batch: graphs, N nodes, E support edges (None: no edge tensors), pad_graph, whether it carries an
    EqualSupports bank.  road: forward's _road override; drop: a dropout pass."""
    from .dense_block import big_applies
    plain = not (dense_n or bn or pad_graph or learnedge)
    if bank and plain and road != 'sparse':                    # opt-in through the bank: no fill threshold picks it
        kind = 'mid'
    elif bank and E is None:
        raise ValueError("the sparse road cannot serve this batch: it has no edge tensors (DeviceDataset.batch_dense: x, y and bank slots only); "
                         "the sparse road needs a batch collated with edge_index2 / edge_attr2")
    # by itself: a node-level model (every pooled model keeps the sparse road) on ONE graph of 96 < N <= 1024 nodes whose mask fill
    # E / N^2 reaches min_fill, supports used as they are, layer inputs within the kernel's features; the override is not checked
    elif road == 'dense' if road else (head == 'node' and plain and E is not None and big_applies(num_graphs, N, fmax) and E >= min_fill * N * N):
        kind = 'big'
    else:
        kind = 'dense_n' if dense_n else 'sparse'
    return GNNML3Road(kind, bool(chain) and not drop and kind == 'sparse')


class GNNML3(torch.nn.Module):
    """head: a name of _HEADS (the table at _Head); 'node' goes with pool=None: no pooling, one output row per NODE."""

    _HEADS = dict(mlp32=_MLP32, tanh10=_TANH10, mlp=_MLP, log_softmax=_LOG_SOFTMAX, node=_NODE)
    _BCE_HEADS = ('mlp',)                  # the heads exp_classify_step_loss fuses (_exp_head)

    def __init__(self, ninp, ne, nout1, nout2, nlayers, learnedge=True, bn=False, pool='add', head='mlp32',
                 nclass=1, readout_bn=False, dense_n=0, chain=True, dropout=0.0, hidden=0, pool_bn=None):
        super().__init__()
        # head 'log_softmax' (the TU scripts: ptc.py:323-363, enzymes.py:345-386, proteins.py:259-289): [relu(fc1 x) when hidden > 0]
        # -> fc2 -> log_softmax, after an optional BatchNorm of the pooled vector named pool_bn ('bn4': enzymes.py:362).
        # pool: 'add' | 'mean' | 'max', or a tuple such as ('mean', 'max'): cat of those pools, in that column order.
        # dropout > 0: F.dropout(x, p) in front of every layer in training (site = the layer index), masks from the device RNG state
        # `dropout_state` (functional.dropout)
        Fn.dropout_threshold(dropout)
        if head not in self._HEADS:
            raise ValueError('head: %s' % ' / '.join(self._HEADS))
        if pool_bn is not None and (bn or readout_bn or head != 'log_softmax'):
            raise ValueError("pool_bn goes with head='log_softmax' and neither bn nor readout_bn")
        # chain=False: do not declare the relu hand-over between stacked layers (ML3Layer.chain_after).  The hand-over is
        # valid only while convN+1 is the SOLE consumer of convN's output tensor: a forward hook, an auxiliary loss or a
        # feature tap on an intermediate output adds a second gradient the lower layer would then leave unmasked -- pass
        # chain=False for such models (GML_NO_CHAIN=1 switches it off process-wide).
        # dense_n > 0: equal-size graphs of dense_n nodes with near-dense masks (MNIST-75) are evaluated as dense
        # blocks (dense_block.py: HIP batched support product + one tall GEMM per layer); same parameters, same values
        if (head == 'node') != (pool is None):
            raise ValueError("head='node' goes with pool=None (one output row per node) and no other head does")
        if head == 'node' and (readout_bn or pool_bn is not None):
            raise ValueError("head='node' has no pooled vector to normalise (readout_bn / pool_bn)")
        if dense_n and (learnedge or nout2):
            raise ValueError('the dense-block path covers plain SpectConv stacks (learnedge=False, nout2=0)')
        self.dense_n = int(dense_n)
        widths = list(nout1) if isinstance(nout1, (list, tuple)) else [nout1] * nlayers    # per-layer nout1
        self.nlayers, self.bn, self.pool, self.head, self.readout_bn = nlayers, bn, pool, head, readout_bn
        fin = ninp
        self._learnedge, self._fin_max = bool(learnedge), max([ninp] + [w + nout2 for w in widths[:nlayers - 1]])   # (what gnnml3_road reads of the layers)
        for i in range(nlayers):
            setattr(self, 'conv%d' % (i + 1),
                    ML3Layer(learnedge=learnedge, nedgeinput=ne, nedgeoutput=ne,
                             ninp=fin, nout1=widths[i], nout2=nout2))
            fin = widths[i] + nout2
            if bn:
                setattr(self, 'bn%d' % (i + 1), BatchNorm1d(fin))
        self._chain = chain and not bn and not self.dense_n
        self._chain_on = bool(self._chain)                      # what is declared now: forward() re-declares on a change only
        if self._chain:
            # x = conv2(conv1(x, ...), ...) with nothing else reading the intermediate outputs (Zinc12k.py:338-341,
            # counting.py:361-366, sr25.py:266-270): the relu hand-over between stacked layers applies on the sparse road, outside
            # dropout passes (a dropout sits between the layers there): gnnml3_road says so per call
            self._declare_chain(True)
        nin = fin * (len(pool) if isinstance(pool, tuple) else 1)
        if readout_bn:                       # TF ReadoutLayer: batch_normalization of the pooled vector
            # tf.layers.batch_normalization defaults (libs/layers_tf.py:349): epsilon 1e-3, momentum 0.99 (= 0.01 in torch's convention)
            self.bnr = SyncBatchNorm1d(nin, eps=1e-3, momentum=0.01)   # global-batch statistics under data parallelism (dist.py)
        self.pool_bn = pool_bn
        if pool_bn is not None:
            setattr(self, pool_bn, torch.nn.BatchNorm1d(nin))   # torch defaults (enzymes.py:362)
        _declare_head(self, nin, hidden, nclass)
        _init_dropout(self, dropout)          # (after the parameters: the seed draw does not shift their initialisation)

    def _declare_chain(self, on):
        for i in range(1, self.nlayers):
            getattr(self, 'conv%d' % (i + 1)).chain_after(getattr(self, 'conv%d' % i) if on else None)

    def _road_of(self, data, _road=None, drop=False):
        """gnnml3_road of this model on this batch: host integers and flags only"""
        from .dense_block import EqualSupports
        ei2 = getattr(data, 'edge_index2', None)
        return gnnml3_road(self.head, self.dense_n, self.bn, self._learnedge, self._fin_max, self._chain, int(data.ptr.numel()) - 1,
                           int(data.x.size(0)), None if ei2 is None else int(ei2.size(1)), bool(getattr(data, 'pad_graph', False)),
                           isinstance(getattr(data, 'bank', None), EqualSupports), _road, drop)

    def forward(self, data, _features=False, _capture=None, _pad_grad_zero=False, _road=None):
        """_road (tests and tools/bench_filtering.py): 'dense' / 'sparse' overrides the road choice of gnnml3_road for a batch both
        roads cover; None: the choice.  A batch with an EqualSupports bank takes the batched dense road unless _road='sparse',
        which needs the batch's edge tensors (ValueError without them)."""
        if getattr(data, 'pad_graph', False) and self.training and (self.readout_bn or self.pool_bn is not None):
            # the padding graph's pooled row would enter the batch statistics of the readout BatchNorm
            raise NotImplementedError('readout BatchNorm takes plain batches: a padded static batch (pad_graph) would count its padding '
                                      'row in the statistics')
        drop = _dropout_pass(self)
        road = self._road_of(data, _road, drop)
        if road.chain != self._chain_on:
            # the relu hand-over is withdrawn for dropout passes and on the dense roads, and back for the next sparse call
            self._declare_chain(road.chain)
            self._chain_on = road.chain
        nvalid = _bn_valid(self, data, self.bn)
        if road.kind == 'sparse':
            x, pooled = self._forward_sparse(data, drop, nvalid, _pad_grad_zero)
            return self._readout(x, data, pooled, _features, _capture)
        from .dense_block import batch_supports
        n = data.bank.n if road.kind == 'mid' else self.dense_n if road.kind == 'dense_n' else int(data.x.size(0))
        sp, gid = (data.bank, getattr(data, 'gid', None)) if road.kind == 'mid' else (batch_supports(data, n), None)
        return self._readout(self._forward_dense(data.x, drop, nvalid, sp, n, gid), data, False, _features, _capture)

    def _forward_dense(self, x, drop, nvalid, sp, n, gid):
        """cat[relu(dense conv), tanh(fc11 x) * tanh(fc12 x)] per layer (and its BatchNorm: dense_n models only) on the dense blocks
        sp of graphs of n nodes: the batch's own (dense_block.batch_supports) or the slots gid of an EqualSupports bank.  Which
        kernel serves the support product is dense_block.dense_road's answer; under exact_products() the fp32 library product."""
        from .dense_block import spectconv_dense
        for i in range(self.nlayers):
            layer = getattr(self, 'conv%d' % (i + 1))
            if drop:
                x = Fn.dropout(x, self.dropout, True, self.dropout_state, site=i)
            a = spectconv_dense(x, sp, layer.conv1.weight, layer.conv1.bias, n, relu=True, gid=gid)
            if layer.nout2 > 0:
                Fn._path('dense', 'Hadamard half (library GEMMs + tanh)', '-', int(x.size(1)), layer.nout2)
                a = torch.cat([a, torch.tanh(tall_linear(x, layer.fc11)) * torch.tanh(tall_linear(x, layer.fc12))], 1)
            x = _layer_bn(self, i + 1, a, nvalid) if self.bn else a
        return x

    def _forward_sparse(self, data, drop, nvalid, _pad_grad_zero):
        """the layers on the CSR kernels: (x, whether the last layer pooled already)"""
        x, csr, pooled = data.x, data.csr('edge_index2'), False
        for i in range(self.nlayers):
            layer = getattr(self, 'conv%d' % (i + 1))
            if drop:
                x = Fn.dropout(x, self.dropout, True, self.dropout_state, site=i)
            if i == self.nlayers - 1 and not self.bn and self.pool in ('add', 'mean') and torch.is_grad_enabled():
                # the pool directly follows the last layer: one autograd node, the pool's gradient is not expanded to [N, C]
                if getattr(data, '_batch_i32', None) is None:
                    data._batch_i32 = data.batch.to(torch.int32).contiguous()
                x = layer.forward_pooled(x, csr, data.edge_attr2, _ptr32(data.ptr), data._batch_i32,
                                         int(self.pool == 'mean') | (2 if getattr(data, 'pad_graph', False) else 0) | (4 if _pad_grad_zero else 0))   # 2: GML_POOL_SKIP_LAST; 4: its gradient is zero already
                pooled = True
            elif self.bn and i == 0:
                # BatchNorm layers behind the first layer amplify the ~1e-5 relative error of the split bf16 products in ITS weight /
                # bias gradients past 1e-4 of their scale (mutag.py:272-288: 1.6e-4 measured): that one layer runs on the exact
                # f32-product kernels, forward and backward (the narrowest layer of the stack: 8 -> 48 features)
                with Fn.exact_products():
                    x = layer(x, csr, data.edge_attr2)
            else:
                x = layer(x, csr, data.edge_attr2)
            if self.bn:
                x = _layer_bn(self, i + 1, x, nvalid)
        return x, pooled

    def _readout(self, x, data, pooled, _features, _capture):
        """pool (unless the last layer pooled already, or the model is node-level), the readout normalisations and the head"""
        if not pooled and self.pool is not None:
            x = _pool(self.pool, x, data)
        if self.readout_bn:
            x = self.bnr(x)
        if self.pool_bn is not None:
            x = getattr(self, self.pool_bn)(x)
        return x if _features else _apply_head(self, x, _capture)

    def features(self, data, pad_grad_zero=False):
        """the pooled (and, with readout_bn, normalised) graph features the head is applied to: [num_graphs, nin].
        pad_grad_zero: the caller's loss gives the padding graph's row (static batches) a zero gradient -- no masking launch."""
        return self.forward(data, _features=True, _pad_grad_zero=pad_grad_zero)


class DSSGCN(torch.nn.Module):
    """DSSGCN_GC_BATCH (libs/models_tf.py:275-343) as enzymes_contfeats_gnnml3_tf.py:25-32 configures it: two bias-free graph
    convolutions relu(sum_s (dropout(C_s) dropout(x)) W_s) (GraphConvolutionwithDephSepBatch, libs/layers_tf.py:247-298: dropout on the
    layer input AND on the support entries, independently per support and layer), the 'meanmax' aggregation, relu(fc1), fc2 (both with
    bias, dropout on their inputs).  conv1 / conv2 are SpectConv modules used as the parameter holders (convN.weight [S, Fin, Fout],
    every support slice initialised as libs/inits_tf.py's glorot([Fin, Fout])); the layers run as ragged dense blocks
    (dense_block.spectconv_ragged on csrc/gml_dense_rag.hip).  forward takes a Batch with `bank` and `gid` attached
    (dense_block.attach_bank).  Dropout sites: the input dropout of layer i (conv1, conv2, fc1, fc2 = 0 .. 3) is site 2 i, its
    support dropout site 2 i + 1; one counter step per training forward."""

    def __init__(self, ninp, ne, widths=(200, 200), pool=('mean', 'max'), dense=(100,), nclass=6, dropout=0.1, kernel_dropout=True):
        super().__init__()
        Fn.dropout_threshold(dropout)
        self.nconv, self.pool, self.kernel_dropout = len(widths), pool, bool(kernel_dropout)
        fin = ninp
        for i, w in enumerate(widths):
            setattr(self, 'conv%d' % (i + 1), SpectConv(fin, w, K=ne, selfconn=False, bias=False))
            fin = w
        fin *= len(pool) if isinstance(pool, tuple) else 1
        dims = list(dense) + [nclass]
        self.nfc = len(dims)
        for i, w in enumerate(dims):
            setattr(self, 'fc%d' % (i + 1), torch.nn.Linear(fin, w))
            fin = w
        _init_dropout(self, dropout)

    def forward(self, data):
        from .dense_block import spectconv_ragged
        drop = _dropout_pass(self)
        state = self.dropout_state if drop else None
        x = data.x
        for i in range(self.nconv):
            conv = getattr(self, 'conv%d' % (i + 1))
            x = Fn.dropout(x, self.dropout, drop, state, site=2 * i)
            x = spectconv_ragged(x, data.bank, data.gid, data.ptr, conv.weight, None, relu=True,
                                 p=self.dropout if self.kernel_dropout else 0.0, state=state, site=2 * i + 1, training=drop)
        # pools on the compact rows.  The script's reduce_max (libs/layers_tf.py:320) runs over rows zero-padded to the largest graph:
        # the conv layers have no bias and end in relu, so every real row is >= 0 and a padding row is exactly 0 -- the same maximum.
        x = _pool(self.pool, x, data)
        for i in range(self.nfc):
            x = Fn.dropout(x, self.dropout, drop, state, site=2 * (self.nconv + i))
            x = getattr(self, 'fc%d' % (i + 1))(x)
            if i + 1 < self.nfc:
                x = torch.relu(x)
        return x


def _gnnml1_block(x, csr, fc1, conv, fc2, fc3, mode, act):
    """the block as one fused launch (functional.GNNML1BlockFunction) or None when the widths are outside the kernel (modes 0..3,
    csrc/gml_gnnml1.hip: input > 144, a part > 64; mode 4, csrc/gml_gnnml1_sum.hip: input > 192, n1 = n2 > 128, n3 > 64; mode 5,
    csrc/gml_gnnml1_act.hip: input > 144, n > 64, or tanh) or the conv is not the plain K = 1 form the scripts use.  Unit edge values
    (sr25.py:231, mutag.py:253: torch.ones).  No row-count gate in mode 4: the fused road's 90th percentile is below the
    composition's 10th for both blocks at 1.7 k and at 500 k rows (tools/bench_gnnml1_sum.py, profiles/gnnml1_sum.json, DESIGN s4.15);
    none in mode 5 for the same reason, at 900 and at 500 k rows (tools/bench_filtering_gnnml1.py, profiles/filtering_gnnml1.json:
    0.33 against 0.79 - 0.85 ms, 0.46 - 0.62 against 4.92 - 5.06 ms; DESIGN s4.18)."""
    if conv.weight.size(0) != 1 or conv.selfconn or conv.depthwise:
        return None
    Fin, n1, n2, n3 = int(x.size(1)), int(fc1.weight.size(0)), int(conv.weight.size(2)), int(fc2.weight.size(0))
    if not Fn.gnnml1_block_supported(x, Fin, n1, n2, n3, mode, act):
        return None
    return Fn.GNNML1BlockFunction.apply(x, csr, None, fc1.weight, fc1.bias, conv.weight, conv.bias, fc2.weight, fc2.bias,
                                        fc3.weight, fc3.bias, mode, act)


class _Stack(torch.nn.Module):
    """What GNNML1Blocks and GAT share: nlayers layers over the raw adjacency, F.dropout in front of every layer in training
    (dropout > 0), bnI after the layers named in bn_after (1-based; nbn: how many of bn1 .. bn<nbn> are DECLARED -- the scripts declare
    some they never call, and their checkpoints load with strict=True), the pools of _pool (or pool=None together with head='node':
    a node-level model) and a head of the class's _HEADS.  A padded static batch hands _node_valid to the bnI in training: padding
    nodes only reach padding nodes (their own self loops), the BatchNorm layers count real nodes only.  A subclass declares its
    layers and supplies _layers(x, graph, _road) (or _batch_layers(data, x, graph, _road)): the function (i, x) -> the output of layer i."""

    def _init_stack(self, nlayers, bn_after, nbn, bn_width, pool, head):
        """the checks and attributes of the shared arguments, and bn1 .. bn<nbn>"""
        if (pool is None) != (head == 'node'):
            raise ValueError("pool=None and head='node' go together: a node-level model has no pooling and reads out every row")
        if any(not 1 <= int(b) <= min(nlayers, nbn) for b in bn_after):
            raise ValueError('bn_after names layers 1 .. nlayers whose BatchNorm is declared (nbn)')
        if self._HEADS[head].bn1 and nbn:
            raise ValueError("head='%s' names its BatchNorm bn1: no layer BatchNorms (nbn == 0)" % head)
        self.nlayers, self.pool, self.head, self.bn_after = int(nlayers), pool, head, frozenset(int(b) for b in bn_after)
        for i in range(1, nbn + 1):
            setattr(self, 'bn%d' % i, BatchNorm1d(bn_width))

    def _init_head(self, nin, hidden, nclass, dropout):
        """the head on nin features per pool, then the dropout state"""
        _declare_head(self, nin * (len(self.pool) if isinstance(self.pool, tuple) else 1), hidden, nclass)
        _init_dropout(self, dropout)           # (after the parameters: the seed draw does not shift their initialisation)

    def forward(self, data, _features=False, _road=None):
        x = data.x
        if self._HEADS[self.head].bn1 and self.training and getattr(data, 'pad_graph', False):
            # bn1 normalises the pooled rows: the padding graph's row and absent slots would enter its statistics
            raise NotImplementedError("head '%s' takes plain batches in training: a padded static batch would count its padding "
                                      'graph and absent slots in the statistics of bn1' % self.head)
        graph = _adjacency(data)
        nvalid = _bn_valid(self, data, self.bn_after)
        layer = self._batch_layers(data, x, graph, _road)
        drop = _dropout_pass(self)
        for i in range(1, self.nlayers + 1):
            if drop:
                x = Fn.dropout(x, self.dropout, True, self.dropout_state, site=i - 1)
            x = layer(i, x)
            if i in self.bn_after:
                x = _layer_bn(self, i, x, nvalid)
        if self.pool is not None:
            x = _pool(self.pool, x, data)
        return x if _features else _apply_head(self, x)

    def _batch_layers(self, data, x, graph, _road):
        """_layers for this batch; a subclass whose layers read more of the batch than its adjacency (Cheb: lmax) overrides this one"""
        return self._layers(x, graph, _road)

    def features(self, data, pad_grad_zero=False):
        """the features the head is applied to: the pooled graph rows [num_graphs, nin], with head='node' the node rows [N, nin]
        (pad_grad_zero: accepted for symmetry with GNNML3.features; the pool here masks the padding graph's gradient itself)."""
        return self.forward(data, _features=True)


class GNNML1Blocks(_Stack):
    """The GNNML1 of every experiment script (mutag.py:214-266, sr25.py:192-246, graph8c.py:205-246, mnist75.py:262-326,
    exp_classify.py:209-262, Zinc12k.py:248-307, counting.py:268-333, freqclass.py:235-300, ptc.py:273-321, enzymes.py:278-343,
    proteins.py:208-257, enzymes_contfeat.py:284-346, filtering.py:200-250, exp_iso.py:195-247) as one class: `nblocks` blocks
         form 'sum'         :  x <- act( fc_i1 x + conv_i1 x + fc_i2 x * fc_i3 x )                          (kernel mode 0, sr25.py:231-240;
                               n1 == n2 == n3, block output n1 wide)
         form 'product'     :  x <- cat[ act(fc_i1 x), act(conv_i1 x), act(fc_i2 x * fc_i3 x) ]              (mode 1)
         form 'factors'     :  x <- cat[ act(fc_i1 x), act(conv_i1 x), act(fc_i2 x) * act(fc_i3 x) ]        (mode 2, mutag.py:253-262)
         form 'tanh_factors':  x <- cat[ act(fc_i1 x), act(conv_i1 x), tanh(fc_i2 x) * tanh(fc_i3 x) ]      (mode 3, ptc.py:311)
         form 'sum_factors' :  x <- cat[ act(fc_i1 x) + act(conv_i1 x), act(fc_i2 x) * act(fc_i3 x) ]       (mode 4, enzymes_contfeat.py:336;
                               n1 == n2, block output n1 + n3 wide)
         form 'act_sum'     :  x <- act(fc_i1 x) + act(conv_i1 x) + act(fc_i2 x * fc_i3 x)                  (mode 5, filtering.py:246-248;
                               n1 == n2 == n3, block output n1 wide; fused for relu, tanh runs on the composition)
    of widths = (n1, n2, n3) (fc_i1 -> n1, conv_i1 = SpectConv(K = 1, selfconn=False) over the raw adjacency with unit edge values
    -> n2, fc_i2 / fc_i3 -> n3), each through _gnnml1_block (one fused launch) with the composition as the road of any other shape.
    bn_after, nbn, dropout, pool: as _Stack has them (the layers are the blocks); head: a name of _HEADS (the table at _Head).
    Same attribute names as the reference, so its state_dict loads."""

    _MODES = dict(sum=0, product=1, factors=2, tanh_factors=3, sum_factors=4)      # the kernel modes of the first five forms
    _FORMS = dict(_MODES, act_sum=5)                                               # every form -> its kernel mode
    _HEADS = dict(mlp32=_MLP32, lin2=_LIN2, lin10=_LIN10, bn_mlp=_BN_MLP32, log_softmax=_LOG_SOFTMAX, node=_NODE)
    _BCE_HEADS = ('mlp32', 'lin2')                                                 # the heads exp_classify_step_loss fuses (_exp_head)

    def __init__(self, ninp, widths, nblocks, form='product', act='relu', bn_after=(), nbn=0, pool='add', head='mlp32', hidden=0,
                 nclass=1, dropout=0.0):
        super().__init__()
        n1, n2, n3 = (int(w) for w in widths)
        if form not in self._FORMS or act not in ('tanh', 'relu') or head not in self._HEADS:
            raise ValueError('form: %s; act: tanh / relu; head: %s' % (' / '.join(self._FORMS), ' / '.join(self._HEADS)))
        if form == 'sum' and not n1 == n2 == n3:
            raise ValueError("form='sum' adds fc_i1 x, conv_i1 x and fc_i2 x * fc_i3 x: three equal widths")
        if form == 'act_sum' and not n1 == n2 == n3:
            raise ValueError("form='act_sum' adds act(fc_i1 x), act(conv_i1 x) and act(fc_i2 x * fc_i3 x): three equal widths")
        if form == 'sum_factors' and n1 != n2:
            raise ValueError("form='sum_factors' adds act(fc_i1 x) and act(conv_i1 x): widths[0] == widths[1]")
        self.nblocks, self.form, self.act = int(nblocks), form, act
        nin = {'sum': n1, 'act_sum': n1, 'sum_factors': n1 + n3}.get(form, n1 + n2 + n3)
        self._init_stack(nblocks, bn_after, nbn, nin, pool, head)
        for i, fin in enumerate([ninp] + [nin] * (nblocks - 1), start=1):
            setattr(self, 'conv%d1' % i, SpectConv(fin, n2, 1, selfconn=False))
            setattr(self, 'fc%d1' % i, torch.nn.Linear(fin, n1))
            setattr(self, 'fc%d2' % i, torch.nn.Linear(fin, n3))
            setattr(self, 'fc%d3' % i, torch.nn.Linear(fin, n3))
        self._init_head(nin, hidden, nclass, dropout)

    def _layers(self, x, csr, _road):
        """_road: accepted for models.filtering_step_loss, which hands it to every node-level model; there is one road here"""
        ones = torch.ones(csr.E, 1, dtype=x.dtype, device=x.device)
        return lambda i, x: self._block(i, x, csr, ones)

    def _block(self, i, x, csr, ones):
        g = lambda n: getattr(self, n % i)
        mode, actid = self._FORMS[self.form], 0 if self.act == 'tanh' else 1
        y = _gnnml1_block(x, csr, g('fc%d1'), g('conv%d1'), g('fc%d2'), g('fc%d3'), mode, actid)
        if y is not None:
            return y
        A = torch.tanh if actid == 0 else F.relu
        a, c, f2, f3 = g('fc%d1')(x), g('conv%d1')(x, csr, ones), g('fc%d2')(x), g('fc%d3')(x)
        if mode == 0:
            return A(a + c + f2 * f3)
        if mode == 4:
            return torch.cat([A(a) + A(c), A(f2) * A(f3)], 1)
        if mode == 5:
            return A(a) + A(c) + A(f2 * f3)
        h = A(f2 * f3) if mode == 1 else (A(f2) * A(f3) if mode == 2 else torch.tanh(f2) * torch.tanh(f3))
        return torch.cat([A(a), A(c), h], 1)


def mutag_gnnml1(ninp=8):                  # mutag.py:214-266 (three blocks 16 | 32 | 16, factor form, relu, a BatchNorm after each, mean-pool, relu(fc1: 64 -> 32), fc2: 32 -> 1)
    return GNNML1Blocks(ninp, (16, 32, 16), 3, form='factors', act='relu', bn_after=(1, 2, 3), nbn=3, pool='mean', head='mlp32')


def zinc_gnnml1(ninp=25):                  # Zinc12k.py:248-307 (four blocks 16 | 16 | 16, product form, relu, add-pool, relu(fc1: 48 -> 32), fc2: 32 -> 1)
    return GNNML1Blocks(ninp, (16, 16, 16), 4, form='product', act='relu', pool='add', head='mlp32')


def counting_gnnml1(ninp=2):               # counting.py:268-333 (five blocks 32 | 32 | 32, product form, relu, add-pool, fc2(fc1 x): 96 -> 32 -> 1, no activation)
    return GNNML1Blocks(ninp, (32, 32, 32), 5, form='product', act='relu', pool='add', head='lin2', hidden=32)


def freqclass_gnnml1(ninp=1, dropout=0.2):  # freqclass.py:235-300 (three blocks 32 | 32 | 32, product form, relu, dropout 0.2, mean-pool, relu(fc1: 96 -> 32), fc2: 32 -> 1)
    return GNNML1Blocks(ninp, (32, 32, 32), 3, form='product', act='relu', pool='mean', head='mlp32', dropout=dropout)


def freqclass_gnnml3(ninp=1, ne=6, dropout=0.2):
    """freqclass.py:300-338, the script's default model (:344): three ML3Layer(learnedge=False, nout1=64, nout2=2) over the ne = 6
    supports of SpectralDesign(recfield=2, dv=4, nfreq=5), dropout 0.2 in front of every layer, mean-pool, relu(fc1: 66 -> 32),
    fc2: 32 -> 1.  The bandclass graphs all have 200 nodes: batches of DeviceDataset.batch_dense (an EqualSupports bank, no edge
    tensors) take the batched dense road (csrc/gml_dense_mid.hip); batches collated with edges the sparse road.  Loss and accuracy:
    freqclass_step_loss / accuracy_from_stats."""
    return GNNML3(ninp, ne, 64, 2, 3, learnedge=False, pool='mean', head='mlp', hidden=32, dropout=dropout)


def ptc_gnnml1(ninp=20, dropout=0.1):
    """ptc.py:273-321: two blocks 32 | 64 | 2 of [relu | relu | tanh . tanh], bn1 after block 1 only (bn2 .. bn4 declared, never
    called), (add, max) pools, relu(fc1: 196 -> 100), log_softmax(fc2: 100 -> 2).  bn1 is 98 wide: beyond the masked BatchNorm
    kernel (C <= 64), so a padded static batch in TRAINING raises BatchNorm1d's NotImplementedError; plain batches and evaluation
    run."""
    return GNNML1Blocks(ninp, (32, 64, 2), 2, form='tanh_factors', act='relu', bn_after=(1,), nbn=4, pool=('add', 'max'),
                        head='log_softmax', hidden=100, nclass=2, dropout=dropout)


def enzymes_gnnml1(ninp=4, dropout=0.1):   # enzymes.py:278-343 (four blocks 16 | 16 | 16, factor form, relu, a BatchNorm after each, (mean, max) pools, log_softmax(fc2: 96 -> 6))
    return GNNML1Blocks(ninp, (16, 16, 16), 4, form='factors', act='relu', bn_after=(1, 2, 3, 4), nbn=4, pool=('mean', 'max'),
                        head='log_softmax', nclass=6, dropout=dropout)


def proteins_gnnml1(ninp=4, dropout=0.1):  # proteins.py:208-257 (two blocks 64 | 64 | 16, factor form, relu; bn1, bn2 declared, never called; (mean, max) pools, log_softmax(fc2: 288 -> 2))
    return GNNML1Blocks(ninp, (64, 64, 16), 2, form='factors', act='relu', nbn=2, pool=('mean', 'max'), head='log_softmax',
                        nclass=2, dropout=dropout)


def enzymes_contfeat_gnnml1(ninp=22, dropout=0.2):
    """enzymes_contfeat.py:284-346: two blocks 128 | 128 | 64 of [relu + relu | relu . relu] (192 wide), a BatchNorm after each,
    (mean, max) pools, log_softmax(fc2: 384 -> 6); the input: the 21 continuous ENZYMES features and the degree column
    (readers.load_tu(contfeat=True), standardize_tu).  bn1 / bn2 are 192 wide: beyond the masked BatchNorm kernel (C <= 64), so a padded
    static batch in TRAINING raises BatchNorm1d's NotImplementedError, as ptc_gnnml1 does; plain batches and evaluation run."""
    return GNNML1Blocks(ninp, (128, 128, 64), 2, form='sum_factors', act='relu', bn_after=(1, 2), nbn=2, pool=('mean', 'max'),
                        head='log_softmax', nclass=6, dropout=dropout)


def sr25_gnnml1(ninp=2):                   # sr25.py:192-246 (nout = 64, sum form, tanh, add-pool, fc1 -> 10)
    return GNNML1Blocks(ninp, (64, 64, 64), 3, form='sum', act='tanh', pool='add', head='lin10', nclass=10)


def graph8c_gnnml1(ninp=2):                # graph8c.py:195-246 (nout = 64, sum form, tanh, add-pool, fc1 -> 10)
    return GNNML1Blocks(ninp, (64, 64, 64), 3, form='sum', act='tanh', pool='add', head='lin10', nclass=10)


def mnist75_gnnml1(ninp=3, dropout=0.0):   # mnist75.py:262-326 (relu, mean-pool, bn1, 32 -> 10; the script's dropout: p = 0.1)
    return GNNML1Blocks(ninp, (64, 64, 64), 3, form='sum', act='relu', pool='mean', head='bn_mlp', nclass=10, dropout=dropout)


def filtering_gnnml1(ninp=1, concat=False):
    """filtering.py:200-250, the GNNML1 its model line offers beside GNNML3 (:287): three blocks 32 | 32 | 32 with relu, node-level
    (no pooling, no fc1, fc2: nin -> 1 on every node).  concat=False, the script's setting: the sum of the three activated parts
    (form 'act_sum', nin = 32); concat=True: their concatenation (form 'product', nin = 96; :241-243).  Loss and R^2:
    filtering_step_loss / r2_from_stats, as for filtering_gnnml3."""
    return GNNML1Blocks(ninp, (32, 32, 32), 3, form='product' if concat else 'act_sum', act='relu', pool=None, head='node', nclass=1)


def filtering_gnnml3(ninp=1, ne=11):      # filtering.py:252-280 (node-level: three layers 32 + 16, fc2: 48 -> 1, no pooling, no fc1)
    return GNNML3(ninp, ne, 32, 16, 3, learnedge=False, pool=None, head='node', nclass=1)


def zinc_gnnml3(ninp=25, ne=8):            # Zinc12k.py:316-329
    return GNNML3(ninp, ne, 30, 2, 4)


def counting_gnnml3(ninp=2, ne=12):        # counting.py:343-358
    return GNNML3(ninp, ne, 16, 16, 5)


def sr25_gnnml3(ninp=2, ne=6):             # sr25.py:252-262
    return GNNML3(ninp, ne, 32, 16, 3, head='tanh10')


def graph8c_gnnml3(ninp=2, ne=6):          # graph8c.py:252-278 (the sr25 shapes: 32 + 16 outputs, 3 layers, add-pool, tanh(fc1) -> 10)
    return GNNML3(ninp, ne, 32, 16, 3, head='tanh10')


def exp_gnnml1(ninp=2):                    # exp_iso.py:195-247 (sr25's shapes: nout = 64, sum form, tanh, add-pool, fc1 -> 10)
    return GNNML1Blocks(ninp, (64, 64, 64), 3, form='sum', act='tanh', pool='add', head='lin10', nclass=10)


def exp_gnnml3(ninp=2, ne=6):              # exp_iso.py:249-278 (the same shapes; ne = 6 supports of SpectralDesign(nfreq=5))
    return GNNML3(ninp, ne, 32, 16, 3, head='tanh10')


def exp_classify_gnnml3(ninp=2, ne=6):     # exp_classify.py:264-295 (three layers 32 + 16, learned supports, mean-pool, relu(fc1: 48 -> 10), fc2: 10 -> 1)
    return GNNML3(ninp, ne, 32, 16, 3, learnedge=True, pool='mean', head='mlp', hidden=10, nclass=1)


def exp_classify_gnnml1(ninp=2):           # exp_classify.py:209-262 (nout = 64, sum form, relu, mean-pool, fc1: 64 -> 10, fc2: 10 -> 1, no activation between)
    return GNNML1Blocks(ninp, (64, 64, 64), 3, form='sum', act='relu', pool='mean', head='lin2', hidden=10, nclass=1)


def mnist_gnnml3(ninp=2, ne=6, dense_n=0):  # mnist75_gnnml3_tf.py:62, libs/models_tf.py:223-268 (DSGCNN)
    return GNNML3(ninp, ne, [64, 128, 128], 0, 3, learnedge=False, pool='mean', head='mlp32', nclass=10,
                  readout_bn=True, dense_n=dense_n)


def mutag_gnnml3(ninp=8, ne=4):            # mutag.py:272-288
    return GNNML3(ninp, ne, 24, 24, 3, learnedge=False, bn=True, pool='mean')


def ptc_gnnml3(ninp=20, ne=11, dropout=0.2):    # ptc.py:323-363
    return GNNML3(ninp, ne, 64, 16, 4, learnedge=True, pool=('mean', 'max'), head='log_softmax', hidden=100, nclass=2,
                  dropout=dropout)


def enzymes_gnnml3(ninp=4, ne=5, dropout=0.1):  # enzymes.py:345-386
    return GNNML3(ninp, ne, 64, 0, 4, learnedge=False, pool=('add', 'max'), head='log_softmax', nclass=6, pool_bn='bn4',
                  dropout=dropout)


def proteins_gnnml3(ninp=4, ne=4, dropout=0.1):  # proteins.py:259-289
    return GNNML3(ninp, ne, 64, 0, 2, learnedge=False, pool=('mean', 'max'), head='log_softmax', nclass=2, dropout=dropout)


def enzymes_contfeat_gnnml3(ninp=22, ne=4, dropout=0.1):  # enzymes_contfeats_gnnml3_tf.py:25-32, libs/models_tf.py:275-343 (two bias-free convs 22 -> 200 -> 200 over ne = 4 supports with input + support dropout, (mean, max) pools, relu(fc1: 400 -> 100), fc2: 100 -> 6)
    # support order: the script's is [identity, band 0, band 1, band 2], SpectralDesign's [band 0, band 1, band 2, identity]:
    # weights_i <-> weight[(3, 0, 1, 2)[i]]
    return DSSGCN(ninp, ne, widths=(200, 200), pool=('mean', 'max'), dense=(100,), nclass=6, dropout=dropout)


class PPGN(torch.nn.Module):
    """The PPGN baseline of the experiment scripts (Maron et al.; sr25.py:20-72, exp_iso.py:22-74, exp_classify.py:24-83,
    Zinc12k.py:25-95, counting.py:35-122, mutag.py:18-72) as one class: `nblocks` blocks on the dense tensors of ppgn.ppgn_inputs,
        x1 = relu(m mlp{b}_1 x),  x2 = relu(m mlp{b}_2 x),  x <- relu(m mlp{b}_3 [x1 @ x2 ; x])     (1 x 1 convolutions, m: the n x n mask)
    each through functional.PPGNBlockFunction (three launches forward, readout included) where functional.ppgn_block_supported says so
    (nmax <= 64, widths <= 64), else through the torch-op composition functional.ppgn_block_torch.  The readouts of all blocks
    ('sum': [diagonal sums | off-diagonal sums], 'mean': the two divided by n and n^2 - n -- at n = 1 the reference divides 0 by 0
    and so does this, 'diag': the diagonal sums only) are concatenated and go through h1 (hidden wide; head_act 'tanh', 'relu' or
    None) and, with nout, h2.  Parameters are torch.nn.Conv2d(., ., 1) modules mlp{b}_1, mlp{b}_2, mlp{b}_3 and Linear h1 (h2), created
    in the reference's order: its state_dict loads with strict=True and torch.manual_seed(s) gives its weights.  forward(data) reads
    data.X2 [B, ninp, nmax, nmax] and data.ppgn_n [B] (ppgn.attach); nmax is informative (the tensors carry it).  Device only."""

    def __init__(self, ninp, nneuron=32, nblocks=3, bias=True, readout='sum', hidden=10, head_act='tanh', nout=None, nmax=0):
        super().__init__()
        if readout not in Fn.PPGN_READOUTS or head_act not in ('tanh', 'relu', None):
            raise ValueError("readout: 'sum' / 'mean' / 'diag'; head_act: 'tanh' / 'relu' / None")
        self.nmax, self.nneuron, self.nblocks, self.readout, self.head_act = int(nmax), int(nneuron), int(nblocks), readout, head_act
        cin = int(ninp)
        for b in range(1, self.nblocks + 1):
            setattr(self, 'mlp%d_1' % b, torch.nn.Conv2d(cin, nneuron, 1, bias=bias))
            setattr(self, 'mlp%d_2' % b, torch.nn.Conv2d(cin, nneuron, 1, bias=bias))
            setattr(self, 'mlp%d_3' % b, torch.nn.Conv2d(nneuron + cin, nneuron, 1, bias=bias))
            cin = int(nneuron)
        self.h1 = torch.nn.Linear((1 if readout == 'diag' else 2) * self.nblocks * nneuron, hidden)
        if nout:
            self.h2 = torch.nn.Linear(hidden, nout)

    def forward(self, data, _features=False, _road=None):
        """_features: the concatenated block readouts (what h1 is applied to); _road: 'torch' forces the composition"""
        x, n = data.X2, data.ppgn_n
        Fn._require_cuda(x, 'data.X2')
        Fn._require_cuda(n, 'data.ppgn_n')
        outs = []
        for b in range(1, self.nblocks + 1):
            m1, m2, m3 = (getattr(self, 'mlp%d_%d' % (b, k)) for k in (1, 2, 3))
            C = int(m1.weight.size(0))
            if _road != 'torch' and Fn.ppgn_block_supported(x, x.size(-1), x.size(1), C):
                x, r = Fn.PPGNBlockFunction.apply(x, n, m1.weight, m1.bias, m2.weight, m2.bias, m3.weight, m3.bias, self.readout)
            else:
                x, r = Fn.ppgn_block_torch(x, n, m1.weight, m1.bias, m2.weight, m2.bias, m3.weight, m3.bias, self.readout)
            outs.append(r)
        x = torch.cat(outs, 1)
        if _features:
            return x
        x = tall_linear(x, self.h1)
        if self.head_act is not None:
            x = torch.tanh(x) if self.head_act == 'tanh' else F.relu(x)
        return tall_linear(x, self.h2) if hasattr(self, 'h2') else x

    def features(self, data):
        return self.forward(data, _features=True)


def sr25_ppgn(ninp=3):                     # sr25.py:20-72 (nmax 25; three blocks of 32 with biases, sum readout, tanh(h1: 192 -> 10))
    return PPGN(ninp, 32, 3, bias=True, readout='sum', hidden=10, head_act='tanh', nmax=25)


def graph8c_ppgn(ninp=3):                  # graph8c.py (the sr25 shapes at nmax 8)
    return PPGN(ninp, 32, 3, bias=True, readout='sum', hidden=10, head_act='tanh', nmax=8)


def exp_ppgn(ninp=3):                      # exp_iso.py:22-74 (nmax 64; three bias-free blocks of 20, sum readout, tanh(h1: 120 -> 10))
    return PPGN(ninp, 20, 3, bias=False, readout='sum', hidden=10, head_act='tanh', nmax=64)


def exp_classify_ppgn(ninp=3):             # exp_classify.py:24-83 (nmax 64; three bias-free blocks of 20, mean readout, relu(h1: 120 -> 10), h2: 10 -> 1)
    return PPGN(ninp, 20, 3, bias=False, readout='mean', hidden=10, head_act='relu', nout=1, nmax=64)


def zinc_ppgn(ninp=23):                    # Zinc12k.py:25-95 (nmax 37; four bias-free blocks of 32, sum readout, relu(h1: 256 -> 64), h2: 64 -> 1)
    return PPGN(ninp, 32, 4, bias=False, readout='sum', hidden=64, head_act='relu', nout=1, nmax=37)


def counting_ppgn(ninp=3):                 # counting.py:35-122 (nmax 30; five bias-free blocks of 40, sum readout, relu(h1: 400 -> 64), h2: 64 -> 1)
    return PPGN(ninp, 40, 5, bias=False, readout='sum', hidden=64, head_act='relu', nout=1, nmax=30)


def mutag_ppgn(ninp=9):                    # mutag.py:18-72 (nmax 28; three blocks of 32 with biases, diagonal readout, relu(h1: 96 -> 32), h2: 32 -> 1)
    return PPGN(ninp, 32, 3, bias=True, readout='diag', hidden=32, head_act='relu', nout=1, nmax=28)


class GAT(_Stack):
    """The GatNet of every PyG experiment script (Zinc12k.py:221-245, sr25.py:169-191, ...) as one class: conv1 .. convK =
    gat.GATConv(., widths[i], heads=8, concat=True) over the raw adjacency, x <- act(conv_i x) with act 'elu', 'tanh' or 'relu' applied
    inside the layer's launch; bn_after, nbn, dropout, pool: as _Stack has them; head: a name of _HEADS (the table at _Head).
    Same attribute names as the scripts, so their state_dicts load.  A padded static batch (batch_padded(..., adjacency=True)) works:
    a padding node carries only its self loop, which is dropped and re-added like any other, so it sees itself alone; the pools skip
    the padding graph and the bnI get the row validity.  Each layer takes the fused road where functional.gat_conv_supported allows,
    else functional.gat_conv_torch; _road='torch' forces the composition."""

    _HEADS = dict(mlp=_MLP, tanh=_TANH, log_softmax=_LOG_SOFTMAX, bn_mlp=_BN_MLP, node=_NODE)

    def __init__(self, ninp, widths, act='elu', pool='add', head='mlp', hidden=0, nclass=1, dropout=0.0, bn_after=(), nbn=0, heads=8):
        super().__init__()
        from .gat import GATConv
        widths = [int(w) for w in widths]
        if act not in ('elu', 'tanh', 'relu') or head not in self._HEADS:
            raise ValueError('act: elu / tanh / relu; head: %s' % ' / '.join(self._HEADS))
        self.act = act
        fin = int(ninp)
        for i, w in enumerate(widths, start=1):
            setattr(self, 'conv%d' % i, GATConv(fin, w, heads=heads, concat=True, dropout=0.0))
            fin = heads * w
        self._init_stack(len(widths), bn_after, nbn, fin, pool, head)
        self._init_head(fin, hidden, nclass, dropout)

    def _layers(self, x, graph, _road):
        road = 'torch' if _road == 'torch' else None
        return lambda i, x: getattr(self, 'conv%d' % i)(x, graph, act=self.act, _road=road)


def zinc_gat(ninp=25):                     # Zinc12k.py:221-245 (8 | 12 | 12 | 12 channels, elu, add-pool, relu(fc1: 96 -> 64), fc2: 64 -> 1)
    return GAT(ninp, (8, 12, 12, 12), act='elu', pool='add', head='mlp', hidden=64)


def mutag_gat(ninp=8):                     # mutag.py:186-212 (8 | 16 | 16, elu, mean-pool, relu(fc1: 128 -> 10), fc2: 10 -> 1)
    return GAT(ninp, (8, 16, 16), act='elu', pool='mean', head='mlp', hidden=10)


def enzymes_gat(ninp=4):                   # enzymes.py:245-276 (8 | 16 | 16 | 16, elu, (mean, max) pools, log_softmax(fc2: 256 -> 6), no fc1)
    return GAT(ninp, (8, 16, 16, 16), act='elu', pool=('mean', 'max'), head='log_softmax', nclass=6)


def freqclass_gat(ninp=1, dropout=0.2):    # freqclass.py:208-233 (8 | 16 | 16, elu, dropout 0.2, mean-pool, relu(fc1: 128 -> 32), fc2: 32 -> 1)
    return GAT(ninp, (8, 16, 16), act='elu', pool='mean', head='mlp', hidden=32, dropout=dropout)


def ptc_gat(ninp=20, dropout=0.1):         # ptc.py:233-271 (16 x 4, elu, dropout 0.1; bn1, bn2 declared, never called; (mean, max) pools, relu(fc1: 256 -> 100), log_softmax(fc2: 100 -> 2))
    return GAT(ninp, (16, 16, 16, 16), act='elu', pool=('mean', 'max'), head='log_softmax', hidden=100, nclass=2, dropout=dropout, nbn=2)


def proteins_gat(ninp=4, dropout=0.1):     # proteins.py:168-206 (16 | 16, elu, dropout 0.1; bn1, bn2 declared, never called; (mean, max) pools, relu(fc1: 256 -> 100), log_softmax(fc2: 100 -> 2))
    return GAT(ninp, (16, 16), act='elu', pool=('mean', 'max'), head='log_softmax', hidden=100, nclass=2, dropout=dropout, nbn=2)


def enzymes_contfeat_gat(ninp=22, dropout=0.1):
    """enzymes_contfeat.py:244-282: 16 | 16, elu, dropout 0.1, bn1 / bn2 after the layers, (mean, max) pools, relu(fc1: 256 -> 100),
    log_softmax(fc2: 100 -> 6).  bn1 / bn2 are 128 wide: beyond the masked BatchNorm kernel (C <= 64), so a padded static batch in
    TRAINING raises BatchNorm1d's NotImplementedError, as enzymes_contfeat_gnnml1 does; plain batches and evaluation run."""
    return GAT(ninp, (16, 16), act='elu', pool=('mean', 'max'), head='log_softmax', hidden=100, nclass=6, dropout=dropout,
               bn_after=(1, 2), nbn=2)


def sr25_gat(ninp=2):                      # sr25.py:169-191 (16 | 16 | 16, tanh, add-pool, tanh(fc1: 128 -> 10))
    return GAT(ninp, (16, 16, 16), act='tanh', pool='add', head='tanh', nclass=10)


def graph8c_gat(ninp=2):                   # graph8c.py:171-193 (the sr25 shapes)
    return GAT(ninp, (16, 16, 16), act='tanh', pool='add', head='tanh', nclass=10)


def exp_gat(ninp=2):                       # exp_iso.py:171-193 (the sr25 shapes)
    return GAT(ninp, (16, 16, 16), act='tanh', pool='add', head='tanh', nclass=10)


def exp_classify_gat(ninp=2):              # exp_classify.py:184-207 (16 | 16 | 16, relu, mean-pool, relu(fc1: 128 -> 10), fc2: 10 -> 1)
    return GAT(ninp, (16, 16, 16), act='relu', pool='mean', head='mlp', hidden=10)


def counting_gat(ninp=2):                  # counting.py:239-266 (16 x 5, relu, add-pool, relu(fc1: 128 -> 32), fc2: 32 -> 1)
    return GAT(ninp, (16, 16, 16, 16, 16), act='relu', pool='add', head='mlp', hidden=32)


def filtering_gat(ninp=1):                 # filtering.py:176-198 (16 | 16 | 16, elu, node-level: fc2: 128 -> 1 on every node, no pooling)
    return GAT(ninp, (16, 16, 16), act='elu', pool=None, head='node', nclass=1)


def mnist75_gat(ninp=3, dropout=0.1):      # mnist75.py:119-148 (8 | 16 | 16, elu, dropout 0.1, mean-pool, bn1 on the pooled rows, relu(fc1: 128 -> 32), log_softmax(fc2: 32 -> 10))
    return GAT(ninp, (8, 16, 16), act='elu', pool='mean', head='bn_mlp', hidden=32, nclass=10, dropout=dropout)


class GIN(_Stack):
    """The GinNet of the PyG experiment scripts (Zinc12k.py:97-143, sr25.py:74-105, ...) as one class: conv1 .. convK =
    gin.GINConv(nn_i, eps, train_eps=True) over the raw adjacency with nn_i = Sequential(Linear(., width)) (depth 1) or
    Sequential(Linear(., width), ReLU(), Linear(width, width)) (depth 2), x <- act(conv_i x) with act 'relu' or 'tanh' applied inside
    the layer's launch; bn_after, nbn, dropout, pool: as _Stack has them; head: a name of _HEADS (the table at _Head).
    eps: a number (every layer starts from it), or 'uniform': one np.random.uniform() per layer, all drawn BEFORE the first Linear is
    built, as the expressivity scripts do (sr25.py:78-80).  share_nn = {4: 3}: conv4 is built on conv3's nn (enzymes.py:116-117 hands
    nn3 to conv4; nn4 is never attached), so a state_dict carries conv3.nn.* and conv4.nn.* for the same tensors.
    Same attribute names as the scripts, so their state_dicts load.  A padded static batch (batch_padded(..., adjacency=True)) works:
    a padding node carries only self loops, which count like any edge, so it reaches itself alone; the pools skip the padding graph and
    the bnI get the row validity.  Each layer takes the fused road where functional.gin_conv_supported allows (widths up to 64), else
    functional.gin_conv_torch; _road='torch' forces the composition."""

    _HEADS = dict(mlp=_MLP, tanh=_TANH, log_softmax=_LOG_SOFTMAX, node=_NODE)

    def __init__(self, ninp, width, nlayers, depth=2, act='relu', eps=0.0, share_nn=None, bn_after=(), nbn=0, dropout=0.0, pool='add',
                 head='mlp', hidden=0, nclass=1):
        super().__init__()
        from .gin import GINConv
        width, nlayers, share_nn = int(width), int(nlayers), dict(share_nn or {})
        if act not in ('tanh', 'relu') or head not in self._HEADS or depth not in (1, 2):
            raise ValueError('act: tanh / relu; depth: 1 / 2; head: %s' % ' / '.join(self._HEADS))
        if any(not 1 <= int(src) < int(i) <= nlayers for i, src in share_nn.items()):
            raise ValueError('share_nn = {layer: an earlier layer whose nn it is built on}')
        if eps == 'uniform':
            import numpy as np
            eps0 = [float(np.random.uniform()) for _ in range(nlayers)]       # (r1, r2, r3 first: sr25.py:78-80)
        else:
            eps0 = [float(eps)] * nlayers
        self.act, self.width, self.depth, self.share_nn = act, width, int(depth), {int(i): int(s) for i, s in share_nn.items()}
        self._init_stack(nlayers, bn_after, nbn, width, pool, head)
        fin = int(ninp)
        for i in range(1, nlayers + 1):
            if i in share_nn:
                nn = getattr(self, 'conv%d' % share_nn[i]).nn
            elif depth == 1:
                nn = torch.nn.Sequential(torch.nn.Linear(fin, width))
            else:
                nn = torch.nn.Sequential(torch.nn.Linear(fin, width), torch.nn.ReLU(), torch.nn.Linear(width, width))
            setattr(self, 'conv%d' % i, GINConv(nn, eps=eps0[i - 1], train_eps=True))
            if i <= nbn:                                   # (the scripts declare convI, then bnI: the same state_dict key order)
                self._modules['bn%d' % i] = self._modules.pop('bn%d' % i)
            fin = width
        self._init_head(width, hidden, nclass, dropout)

    def _layers(self, x, graph, _road):
        road = 'torch' if _road == 'torch' else None
        return lambda i, x: getattr(self, 'conv%d' % i)(x, graph, act=self.act, _road=road)


def sr25_gin(ninp=2):                      # sr25.py:74-105 (3 x Linear 64, eps from np.random.uniform(), tanh, add-pool, tanh(fc1: 64 -> 10))
    return GIN(ninp, 64, 3, depth=1, act='tanh', eps='uniform', pool='add', head='tanh', nclass=10)


def graph8c_gin(ninp=2):                   # graph8c.py:74-105 (the sr25 shapes)
    return GIN(ninp, 64, 3, depth=1, act='tanh', eps='uniform', pool='add', head='tanh', nclass=10)


def exp_gin(ninp=2):                       # exp_iso.py:76-107 (the sr25 shapes)
    return GIN(ninp, 64, 3, depth=1, act='tanh', eps='uniform', pool='add', head='tanh', nclass=10)


def exp_classify_gin(ninp=2):              # exp_classify.py:85-117 (3 x Linear 64, eps from np.random.uniform(), relu, mean-pool, relu(fc1: 64 -> 10), fc2: 10 -> 1)
    return GIN(ninp, 64, 3, depth=1, act='relu', eps='uniform', pool='mean', head='mlp', hidden=10)


def zinc_gin(ninp=25):                     # Zinc12k.py:97-143 (4 x L-ReLU-L 64, relu, bn1-4 after the layers, add-pool, relu(fc1: 64 -> 32), fc2: 32 -> 1)
    return GIN(ninp, 64, 4, bn_after=(1, 2, 3, 4), nbn=4, pool='add', head='mlp', hidden=32)


def counting_gin(ninp=2):                  # counting.py:124-159 (5 x L-ReLU-L 64, relu, add-pool, relu(fc1: 64 -> 32), fc2: 32 -> 1)
    return GIN(ninp, 64, 5, pool='add', head='mlp', hidden=32)


def mutag_gin(ninp=8):                     # mutag.py:74-111 (3 x L-ReLU-L 64, relu, bn1-3, mean-pool, relu(fc1: 64 -> 10), fc2: 10 -> 1)
    return GIN(ninp, 64, 3, bn_after=(1, 2, 3), nbn=3, pool='mean', head='mlp', hidden=10)


def freqclass_gin(ninp=1, dropout=0.2):    # freqclass.py:90-129 (3 x L-ReLU-L 64, relu, dropout 0.2, bn1-3, mean-pool, relu(fc1: 64 -> 32), fc2: 32 -> 1)
    return GIN(ninp, 64, 3, bn_after=(1, 2, 3), nbn=3, dropout=dropout, pool='mean', head='mlp', hidden=32)


def filtering_gin(ninp=1):                 # filtering.py:86-111 (3 x L-ReLU-L 64, relu, node-level: fc2: 64 -> 1 on every node, no pooling)
    return GIN(ninp, 64, 3, pool=None, head='node', nclass=1)


def enzymes_gin(ninp=4, dropout=0.1):
    """enzymes.py:100-148: 4 x L-ReLU-L 64 with conv4 built on nn3 (:116-117; nn4 is never attached), relu, dropout 0.1, bn1-4,
    (mean, max) pools, log_softmax(fc2: 128 -> 6), no fc1"""
    return GIN(ninp, 64, 4, share_nn={4: 3}, bn_after=(1, 2, 3, 4), nbn=4, dropout=dropout, pool=('mean', 'max'), head='log_softmax', nclass=6)


def ptc_gin(ninp=20, dropout=0.2):
    """ptc.py:95-126: 2 x L-ReLU-L 200, relu, dropout 0.2, bn1-2, (add, max) pools, log_softmax(fc2: 400 -> 2).  200 wide: beyond the
    fused layer (widths up to 64), so both layers run on functional.gin_conv_torch; bn1 / bn2 are beyond the masked BatchNorm kernel, so
    a padded static batch in TRAINING raises BatchNorm1d's NotImplementedError; plain batches and evaluation run."""
    return GIN(ninp, 200, 2, bn_after=(1, 2), nbn=2, dropout=dropout, pool=('add', 'max'), head='log_softmax', nclass=2)


def proteins_gin(ninp=4, dropout=0.2):     # proteins.py:31-63 (the ptc shapes and roads)
    return GIN(ninp, 200, 2, bn_after=(1, 2), nbn=2, dropout=dropout, pool=('add', 'max'), head='log_softmax', nclass=2)


def enzymes_contfeat_gin(ninp=22, dropout=0.2):    # enzymes_contfeat.py:104-137 (the ptc shapes and roads with (mean, max) pools, fc2: 400 -> 6)
    return GIN(ninp, 200, 2, bn_after=(1, 2), nbn=2, dropout=dropout, pool=('mean', 'max'), head='log_softmax', nclass=6)


class Cheb(_Stack):
    """The ChebNet of the PyG experiment scripts (Zinc12k.py:193-219, sr25.py:149-167, ...) as one class: conv1 .. convL =
    cheb.ChebConv(., widths[i], K) over the raw adjacency, x <- act(conv_i x) with act 'relu' or 'tanh' applied inside the layer's
    last launch; bn_after, nbn, dropout, pool: as _Stack has them (the scripts declare their bnI AFTER the convs: the same key order
    here); head: a name of _HEADS (the table at _Head).  Same attribute names as the scripts, so their state_dicts load.
    lmax=True: the layers get lambda_max = data.lmax [num_graphs] indexed by data.batch, as the scripts that pass
    lambda_max=data.lmax do -- carry it with graph_fields=('lmax',); lmax=False: lambda_max = None (2.0), as mutag.py:178,
    freqclass.py:198 and enzymes.py:233 call their layers.  The norm (functional.cheb_norm) is computed ONCE per forward call and
    handed to every layer; it is not cached on the batch, so a captured step that replays over rewritten batch tensors recomputes it
    inside the graph.  A padded static batch (batch_padded(..., adjacency=True)) works: a padding node carries only self loops, which
    are dropped, so it is isolated and with x = 0 its output is act(bias); the pools skip the padding graph and the bnI get the row
    validity.  Each layer takes the fused road where functional.cheb_conv_supported allows (K <= 8, widths up to 64), else
    functional.cheb_conv_torch; _road='torch' forces the composition."""

    _HEADS = dict(mlp=_MLP, tanh=_TANH, log_softmax=_LOG_SOFTMAX, bn_mlp=_BN_MLP, node=_NODE)

    def __init__(self, ninp, widths, K, act='relu', bn_after=(), nbn=0, dropout=0.0, pool='add', head='mlp', hidden=0, nclass=1, lmax=True):
        super().__init__()
        from .cheb import ChebConv
        widths = [int(w) for w in widths]
        if act not in ('tanh', 'relu') or head not in self._HEADS or not widths:
            raise ValueError('act: tanh / relu; at least one width; head: %s' % ' / '.join(self._HEADS))
        self.act, self.K, self.lmax = act, int(K), bool(lmax)
        fin = int(ninp)
        for i, w in enumerate(widths, start=1):
            setattr(self, 'conv%d' % i, ChebConv(fin, w, self.K))
            fin = w
        self._init_stack(len(widths), bn_after, nbn, fin, pool, head)
        self._init_head(fin, hidden, nclass, dropout)

    def _batch_layers(self, data, x, graph, _road):
        lam = None
        if self.lmax:
            lam = getattr(data, 'lmax', None)
            if lam is None:
                raise ValueError("this ChebNet reads data.lmax (one lambda_max per graph): carry it with graph_fields=('lmax',) "
                                 '(graph.collate / DeviceDataset.from_graphs)')
        road = 'torch' if _road == 'torch' else None
        convs = [getattr(self, 'conv%d' % i) for i in range(1, self.nlayers + 1)]
        fused = road is None and any(Fn.cheb_conv_supported(x, c.out_channels, self.K, Fin=c.in_channels) for c in convs)
        norm = Fn.cheb_norm(graph, data.batch, lam) if fused else None          # once per forward call, never cached on the batch
        return lambda i, x: convs[i - 1](x, graph, batch=data.batch, lambda_max=lam, act=self.act, norm=norm, _road=road)


def zinc_cheb(ninp=25):                    # Zinc12k.py:193-219 (S = 2: line 197 overrides the S = 5 default; 64 x 4, relu, add-pool, relu(fc1: 64 -> 32), fc2: 32 -> 1)
    return Cheb(ninp, (64, 64, 64, 64), 2, act='relu', pool='add', head='mlp', hidden=32)


def sr25_cheb(ninp=2):                     # sr25.py:149-167 (S = 4; 32 | 64 | 64, tanh, add-pool, tanh(fc1: 64 -> 10))
    return Cheb(ninp, (32, 64, 64), 4, act='tanh', pool='add', head='tanh', nclass=10)


def graph8c_cheb(ninp=2):                  # graph8c.py:151-169 (the sr25 shapes)
    return Cheb(ninp, (32, 64, 64), 4, act='tanh', pool='add', head='tanh', nclass=10)


def exp_cheb(ninp=2):                      # exp_iso.py:151-169 (the sr25 shapes)
    return Cheb(ninp, (32, 64, 64), 4, act='tanh', pool='add', head='tanh', nclass=10)


def exp_classify_cheb(ninp=2):             # exp_classify.py:163-182 (S = 5; 32 | 64 | 64, relu, mean-pool, relu(fc1: 64 -> 10), fc2: 10 -> 1)
    return Cheb(ninp, (32, 64, 64), 5, act='relu', pool='mean', head='mlp', hidden=10)


def counting_cheb(ninp=2):                 # counting.py:213-237 (S = 5; 48 x 5, relu, add-pool, relu(fc1: 48 -> 32), fc2: 32 -> 1)
    return Cheb(ninp, (48, 48, 48, 48, 48), 5, act='relu', pool='add', head='mlp', hidden=32)


def mutag_cheb(ninp=8):                    # mutag.py:161-184 (S = 3; 32 x 3, relu, NO lambda_max: 2.0; mean-pool, relu(fc1: 32 -> 32), fc2: 32 -> 1)
    return Cheb(ninp, (32, 32, 32), 3, act='relu', pool='mean', head='mlp', hidden=32, lmax=False)


def freqclass_cheb(ninp=1, dropout=0.2):   # freqclass.py:182-206 (S = 5; 32 | 64 | 64, relu, dropout 0.2, NO lambda_max: 2.0; mean-pool, relu(fc1: 64 -> 32), fc2: 32 -> 1)
    return Cheb(ninp, (32, 64, 64), 5, act='relu', dropout=dropout, pool='mean', head='mlp', hidden=32, lmax=False)


def filtering_cheb(ninp=1):                # filtering.py:155-174 (S = 7; 64 x 3, relu, node-level: fc2: 64 -> 1 on every node, no pooling)
    return Cheb(ninp, (64, 64, 64), 7, act='relu', pool=None, head='node', nclass=1)


def mnist75_cheb(ninp=3, dropout=0.1):     # mnist75.py:150-185 (S = 5; 64 x 3, relu, dropout 0.1, mean-pool, bn1 on the pooled rows, relu(fc1: 64 -> 32), log_softmax(fc2: 32 -> 10))
    return Cheb(ninp, (64, 64, 64), 5, act='relu', dropout=dropout, pool='mean', head='bn_mlp', hidden=32, nclass=10)


def enzymes_cheb(ninp=4, dropout=0.1):
    """enzymes.py:215-243: S = 3, 128 x 4, relu, dropout 0.1, NO lambda_max (2.0), (mean, max) pools, log_softmax(fc2: 256 -> 6), no
    fc1.  128 wide: conv1 (ninp -> 128) and the rest are beyond the fused layer (widths up to 64) and run on functional.cheb_conv_torch."""
    return Cheb(ninp, (128, 128, 128, 128), 3, act='relu', dropout=dropout, pool=('mean', 'max'), head='log_softmax', nclass=6, lmax=False)


def ptc_cheb(ninp=20, dropout=0.2):
    """ptc.py:193-231: S = 3, 200 x 4, relu, dropout 0.2; bn1, bn2 declared, never called; (mean, max) pools, log_softmax(fc2: 400 ->
    2).  200 wide: every layer runs on functional.cheb_conv_torch."""
    return Cheb(ninp, (200, 200, 200, 200), 3, act='relu', nbn=2, dropout=dropout, pool=('mean', 'max'), head='log_softmax', nclass=2)


def proteins_cheb(ninp=4, dropout=0.2):
    """proteins.py:128-166: S = 3, 200 x 2, relu, dropout 0.2, bn1 / bn2 after the layers, (mean, max) pools, log_softmax(fc2: 400 -> 2).
    200 wide: both layers run on functional.cheb_conv_torch; bn1 / bn2 are beyond the masked BatchNorm kernel, so a padded static batch
    in TRAINING raises BatchNorm1d's NotImplementedError; plain batches and evaluation run."""
    return Cheb(ninp, (200, 200), 3, act='relu', bn_after=(1, 2), nbn=2, dropout=dropout, pool=('mean', 'max'), head='log_softmax', nclass=2)


def enzymes_contfeat_cheb(ninp=22, dropout=0.2):   # enzymes_contfeat.py:203-242 (the proteins shapes and roads, fc2: 400 -> 6)
    return Cheb(ninp, (200, 200), 3, act='relu', bn_after=(1, 2), nbn=2, dropout=dropout, pool=('mean', 'max'), head='log_softmax', nclass=6)


def _graph_valid(valid, data):
    """valid, or the graph_valid [B] of a padded static batch, or None (a plain batch)"""
    return valid if valid is not None else getattr(data, 'graph_valid', None)


def _valid_sum(rowloss, pre, y, valid):
    """the loss sum of a padded static batch: rowloss(pre[:B], y[:B]) [B] over its first B = valid.numel() rows, weighted by valid
    (the padding graph's row and absent slots count zero)"""
    nl = int(valid.numel())
    return (rowloss(pre[:nl], y[:nl]) * valid).sum()


def _bce_rows(pre, y):
    return F.binary_cross_entropy(torch.sigmoid(pre[:, 0]), y.to(pre.dtype), reduction='none')


def zinc_loss(pre, y):                     # Zinc12k.py:365
    return F.l1_loss(pre, y.unsqueeze(-1), reduction='sum')


def _exp_head(model, loss='bce'):
    """(fc1, fc2, act) of a model whose head the fused kernels of `loss` may serve, act = 1 (relu) / 0 (identity), else None.  'l1':
    the row 'mlp32'; 'bce': a head that is fc2(act(fc1 x)) and nothing else AND that its class lists in _BCE_HEADS -- the description
    alone would also admit GNNML3 'mlp32' and GAT 'mlp', which have never taken the fused BCE road: widening it is a change of
    behaviour, not of this function."""
    h = getattr(model, '_HEADS', {}).get(getattr(model, 'head', None))            # (PPGN, DSSGCN: no head name at all)
    if h is None or not (h == _MLP32 if loss == 'l1' else model.head in getattr(model, '_BCE_HEADS', ())):
        return None
    assert h.fc1 and h.fc2 and not h.bn1 and h.out is None, h
    return model.fc1, model.fc2, int(h.between == 'relu')


def _l1_torch(pre, data, nl, valid, loss_sum, ntask):
    l = _valid_sum(lambda p, y: (p[:, 0] - y).abs(), pre, data.y, valid) if valid is not None else zinc_loss(pre, data.y)
    if loss_sum is not None:
        loss_sum.add_(l.detach())
    return l


def _bce_torch(pre, data, nl, valid, stats, ntask):
    loss = exp_classify_loss(pre, data.y, valid)
    if stats is not None:
        with torch.no_grad():
            v = valid if valid is not None else torch.ones(nl, dtype=pre.dtype, device=pre.device)
            ok = ((pre[:nl, 0] > 0) == (data.y[:nl] == 1)).to(pre.dtype)
            stats[:3].add_(torch.stack([loss.detach(), (ok * v).sum(), (v != 0).to(pre.dtype).sum()]))
    return loss


def _node_sq_torch(pre, data, nl, valid, stats, ntask):
    loss = filtering_loss(pre, data.y, data.mask, ntask)
    if stats is not None:
        with torch.no_grad():
            m = (data.mask == 1).to(pre.dtype)
            yt = data.y[:, ntask:ntask + 1]
            cnt = m.sum()
            ybar = (m * yt).sum() / cnt.clamp(min=1)
            stats[:4].copy_(torch.stack([loss.detach(), (m * (yt - pre) ** 2).sum(), (m * (yt - ybar) ** 2).sum(), cnt]))
    return loss


_TORCH_ROADS = dict(l1=_l1_torch, bce=_bce_torch, node_sq=_node_sq_torch)


def _step_loss(loss, model, data, valid=None, acc=None, ntask=0, _road=None, _head_road=None):
    """What zinc_step_loss, exp_classify_step_loss and filtering_step_loss share.  The road of the head is ONE record
    (functional.head_road) built from host values before any layer runs; the model's features run ONCE, with the record's
    pad_grad_zero; then the fused head of the record's kind, or the torch-op road of the same loss with its acc arithmetic.  A model
    whose head no fused kernel of this loss may serve runs its own forward.  _head_road: the record's override ('torch': tests, tools)."""
    node = loss == 'node_sq'
    head = (None, model.fc2, 0) if node else _exp_head(model, loss)
    nl = 0 if node else int(data.y.numel()) if valid is None else int(valid.numel())
    if head is None or not (node or int(head[1].weight.size(0)) == 1):
        Fn._path('head', Fn.head_road(loss, None, False, 0, 0, 0, 0, nl, 0).label)
        return _TORCH_ROADS[loss](model(data), data, nl, valid, acc, ntask)
    fc1, fc2, act = head
    w2, b2 = fc2.weight, fc2.bias
    w1, b1 = (None, None) if node else (fc1.weight, fc1.bias)
    R, nin = int(data.x.size(0)) if node else int(data.ptr.numel()) - 1, int((w2 if node else w1).size(1))
    road = Fn.head_road(loss, None if node else model._HEADS[model.head], True, nin, int(w2.size(1)), int(w2.size(0)), R, nl,
                        int(data.num_graphs) if hasattr(data, 'num_graphs') else nl,
                        *Fn.head_flags(loss, data.x, valid, w2 if node else w1, b1, w2, b2), _head_road)
    if road.kind != 'bce':                                  # (HeadBCEFunction writes its own entry, for direct callers too)
        Fn._path('head', road.label)
    x = model.forward(data, _features=True, _road=_road) if node else model.features(data, pad_grad_zero=road.pad_grad_zero)
    if road.kind == 'torch':
        return _TORCH_ROADS[loss](tall_linear(x, fc2) if node else _apply_head(model, x), data, nl, valid, acc, ntask)
    # the postcondition of features that the record was built on
    assert x.dim() == 2 and (node or x.size(0) == R) and x.size(1) == nin and x.dtype == torch.float32 and x.stride(1) == 1, (road, x.shape, x.dtype)
    if node:
        return Fn.NodeHeadLossFunction.apply(x, w2, b2, data.y, data.mask, int(ntask), acc)[0]
    y = data.y[:nl] if road.kind == 'bce' else data.y[:nl].float().contiguous()
    return Fn.POOLED_HEADS[road.kind].apply(x, y, valid, w1, b1, w2, b2, *((act, acc) if road.kind == 'bce' else (acc,)))


def zinc_step_loss(model, data, valid=None, loss_sum=None, _head_road=None):
    """zinc_loss(model(data), data.y) -- with the head and the loss as ONE launch each way where a kernel serves the batch
    (functional.head_road: 'l1_small', the reference's batch 64, or 'l1_big', any size; a static batch's padding graph and absent slots
    are masked through `valid` / data.graph_valid).  Same value and gradients up to summation order; other heads take the torch ops."""
    return _step_loss('l1', model, data, _graph_valid(valid, data), loss_sum, _head_road=_head_road)


def filtering_loss(pre, y, mask, ntask=0):   # filtering.py:320
    return torch.square(mask * (pre - y[:, ntask:ntask + 1])).sum()


def filtering_step_loss(model, data, ntask=0, stats=None, _road=None, _head_road=None):
    """filtering_loss(model(data), data.y, data.mask, ntask) -- the ``loss_fn(model, data)`` of dist.TrainStep -- with the readout
    fc2, the masked loss and the sums of R^2 as ONE launch each way (functional.NodeHeadLossFunction).  stats: optional float32 [4]
    on the device, receives {loss, ss_res, ss_tot, count} over the rows with mask == 1 (r2_from_stats); no host read.  _road: the
    model's (GNNML3.forward)."""
    return _step_loss('node_sq', model, data, None, stats, ntask, _road, _head_road)


def r2_from_stats(stats):
    """sklearn's r2_score of filtering.py:324-327 from the four sums of filtering_step_loss: 1 - ss_res / ss_tot.  A tensor op on
    whatever device stats lives on (no host read); numpy arrays and sequences work too."""
    return 1 - stats[1] / stats[2]


def exp_classify_loss(pre, y, valid=None):   # exp_classify.py:328-329
    """F.binary_cross_entropy(sigmoid(pre), y.float().unsqueeze(-1), reduction='sum') -- the general road and the CPU.  valid: a
    padded static batch's graph_valid [B] -- the sum over the real graphs of its first B rows, as mutag_loss masks them."""
    if valid is None:
        return F.binary_cross_entropy(torch.sigmoid(pre), y.to(pre.dtype).unsqueeze(-1), reduction='sum')
    return _valid_sum(_bce_rows, pre, y, valid)


def exp_classify_step_loss(model, data, valid=None, stats=None, _head_road=None):
    """exp_classify_loss(model(data), data.y) -- the ``loss_fn(model, data)`` of dist.TrainStep -- with the head, the loss, the
    number of correct predictions and their backward as ONE launch each way (functional.head_road: 'bce') where the head is
    fc2(act(fc1 x)) with one output and at most 64 units a side; otherwise the torch-op road.  Plain and padded static batches
    (valid = data.graph_valid), training and evaluation under torch.no_grad() alike.  stats: optional float32 [3] on the device,
    ACCUMULATES {loss, correct predictions, graphs counted} (accuracy_from_stats); no host read."""
    return _step_loss('bce', model, data, _graph_valid(valid, data), stats, _head_road=_head_road)


# freqclass.py:368-375 / :385-390: the same sum BCE on sigmoid(pre[:, 0]) and the same count of round(sigmoid) == y.  The head of
# freqclass_gnnml3 has 66 inputs, outside gml_head_bce.hip's 64: it takes the torch-op road of the function above (the GNNML1 model's
# 96 inputs do too); accuracy_from_stats reads the sums.
freqclass_step_loss = exp_classify_step_loss


def accuracy_from_stats(stats):
    """correct predictions / graphs counted from the sums of exp_classify_step_loss (exp_classify.py:334, :337).  A tensor op on
    whatever device stats lives on (no host read); numpy arrays and sequences work too."""
    return stats[1] / stats[2]


def counting_loss(pre, y):                 # counting.py:411
    return torch.square(pre - y.view(-1, 1)).sum()


def mnist_loss(pre, y):                    # libs/metrics_tf.py softmax cross entropy, batch mean
    return F.cross_entropy(pre, y.long())


def mutag_loss(pre, y, valid=None):        # mutag.py:345-348
    """valid: a padded static batch's graph_valid [B] -- the BCE sum over the real graphs of its first B rows (mutag.py:349-351)."""
    if valid is None:
        return F.binary_cross_entropy(torch.sigmoid(pre)[:, 0], y, reduction='sum')
    return _valid_sum(_bce_rows, pre, y, valid)


def mutag_step_loss(model, data, valid=None):
    """mutag_loss(model(data), data.y) for plain and padded batches alike (a padded batch: valid = data.graph_valid) -- the
    ``loss_fn(model, data)`` of dist.TrainStep."""
    return mutag_loss(model(data), data.y, _graph_valid(valid, data))


def tu_loss(pre, y, valid=None):             # ptc.py:416, enzymes.py / proteins.py: F.nll_loss(pred, data.y, reduction='sum')
    """valid: a padded static batch's graph_valid [B] -- the NLL sum over the real graphs of its first B rows (the padding graph's
    row and absent slots count zero)."""
    if valid is None:
        return F.nll_loss(pre, y.long(), reduction='sum')
    return _valid_sum(lambda p, t: F.nll_loss(p, t.long().clamp(0, int(p.size(1)) - 1), reduction='none'), pre, y, valid)


def tu_step_loss(model, data, valid=None):
    """tu_loss(model(data), data.y) for plain and padded batches alike -- the ``loss_fn(model, data)`` of dist.TrainStep."""
    return tu_loss(model(data), data.y, _graph_valid(valid, data))


def dssgcn_loss(model, logits, y, weight_decay=1e-4):   # libs/models_tf.py:286-301
    """mean softmax cross entropy over the batch + weight_decay . sum of tf.nn.l2_loss(W) = |W|^2 / 2 over every non-bias parameter."""
    l2 = sum(w.square().sum() for n, w in model.named_parameters() if not n.endswith('bias'))
    return F.cross_entropy(logits, y.long()) + (0.5 * weight_decay) * l2
