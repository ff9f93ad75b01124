"""GINConv: the 1-WL baseline of the experiment scripts (GinNet, e.g. Zinc12k.py:97-143, sr25.py:74-105) with the parameters and
names of torch_geometric 1.6.1's GINConv -- the version the reference's README pins:

    h[i] = sum over the edges (j -> i) of x[j] + (1 + eps) x[i];   out = nn(h)

Every edge occurrence counts, a self loop included; nothing is dropped or added.  eps [1] is a Parameter with train_eps=True (every
script), else a buffer under the same key.  nn = Sequential(Linear) or Sequential(Linear, ReLU, Linear) inside the range of
functional.gin_conv_supported runs as one launch of csrc/gml_gin.hip (functional.GINConvFunction); any other nn aggregates with
torch ops and then calls nn.
"""
import torch

from . import functional as Fn
from .graph import GraphCSR, csr_for


class GINConv(torch.nn.Module):
    """state_dict: eps, then nn's own keys (nn.0.weight, nn.0.bias[, nn.2.weight, nn.2.bias]).  forward(x, csr_or_edge_index,
    act=None): act in (None, 'relu', 'tanh') is the activation the scripts apply AFTER the layer; on the fused road it is applied in
    the launch that writes the output."""

    def __init__(self, nn, eps=0., train_eps=False):
        super().__init__()
        self.nn = nn
        self.initial_eps = eps
        if train_eps:
            self.eps = torch.nn.Parameter(torch.Tensor([eps]))
        else:
            self.register_buffer('eps', torch.Tensor([eps]))
        self.reset_parameters()

    def reset_parameters(self):
        mods = list(self.nn.children()) if hasattr(self.nn, 'children') else []
        for m in mods or [self.nn]:                      # (1.6.1's reset(): the children, or nn itself when it has none)
            if hasattr(m, 'reset_parameters'):
                m.reset_parameters()
        self.eps.data.fill_(self.initial_eps)

    def forward(self, x, edge_index, act=None, _road=None):
        """edge_index: int64 [2, E] = (source, target) or its GraphCSR.  _road='torch' forces the composition."""
        if isinstance(x, (tuple, list)):
            raise NotImplementedError('GINConv: x as a tuple (bipartite inputs) is not implemented')
        lins = Fn.gin_nn_linears(self.nn)
        if lins is not None and _road != 'torch' and Fn.gin_conv_supported(x, lins[0].out_features, lins[1].out_features if len(lins) == 2 else None):
            csr = csr_for(edge_index, int(x.size(0)))
            l2 = lins[1] if len(lins) == 2 else None
            return Fn.GINConvFunction.apply(x, csr, self.eps, lins[0].weight, lins[0].bias, None if l2 is None else l2.weight,
                                            None if l2 is None else l2.bias, act)
        if isinstance(edge_index, GraphCSR):
            edge_index = Fn.csr_edge_index(edge_index)
        if lins is not None:
            Fn._path('gin', 'torch ops (outside the fused layer)', '-', int(x.size(1)), lins[-1].out_features)
            return Fn.gin_conv_torch(x, edge_index, self.eps, [(l.weight, l.bias) for l in lins], act)
        Fn._path('gin', 'torch ops (an nn other than Linear / Linear-ReLU-Linear)', '-', int(x.size(1)), '-')
        h = torch.zeros_like(x).index_add_(0, edge_index[1], x[edge_index[0]]) + (1 + self.eps) * x
        return _act(self.nn(h), act)

    def __repr__(self):
        return '%s(nn=%s)' % (self.__class__.__name__, self.nn)


def _act(v, act):
    a = Fn._relu_tanh_id(act)
    return torch.relu(v) if a == 1 else (torch.tanh(v) if a == 2 else v)
