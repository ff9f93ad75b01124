"""GATConv: the attention baseline of the experiment scripts (GatNet, e.g. Zinc12k.py:221-245, sr25.py:169-191) with the parameters,
names and initialisation of torch_geometric 1.6.1's GATConv -- the version the reference's README pins; the scripts' docstring
"number of param (in+3)*head*out" agrees with it: weight H C x in, att_l and att_r H C each, bias H C.

    xl = lin_l(x) [N, H, C];   e(j -> i) = leaky_relu(<xl[j], att_l> + <xl[i], att_r>, 0.2);   alpha = softmax over the edges into i
    out[i] = sum_j alpha xl[j]  (heads concatenated) + bias

after dropping every edge with j == i and adding one self edge per node.  The attention path runs on csrc/gml_gat.hip
(functional.GATConvFunction) where functional.gat_conv_supported says so, else as the composition functional.gat_conv_torch.
"""
import torch
from torch.nn import Parameter

from . import functional as Fn
from .graph import GraphCSR, csr_for
from .spect_conv import glorot, zeros


class GATConv(torch.nn.Module):
    """lin_l.weight [H C, in] (lin_r is the same module: a state_dict carries both keys for one tensor), att_l, att_r [1, H, C],
    bias [H C].  forward(x, csr_or_edge_index, act=None): act in (None, 'relu', 'tanh', 'elu') is applied in the launch that writes
    the output.  The variants no script uses raise NotImplementedError."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, add_self_loops=True, bias=True):
        super().__init__()
        if isinstance(in_channels, (tuple, list)):
            raise NotImplementedError('GATConv: in_channels as a tuple (bipartite inputs) is not implemented')
        if not concat:
            raise NotImplementedError('GATConv: concat=False (the mean of the heads) is not implemented')
        if dropout != 0.0:
            raise NotImplementedError('GATConv: dropout > 0 (attention dropout) is not implemented')
        if not add_self_loops:
            raise NotImplementedError('GATConv: add_self_loops=False is not implemented')
        if negative_slope != Fn.GAT_SLOPE:
            raise NotImplementedError('GATConv: negative_slope other than 0.2 is not implemented')
        self.in_channels, self.out_channels, self.heads = int(in_channels), int(out_channels), int(heads)
        self.concat, self.negative_slope, self.dropout, self.add_self_loops = True, float(negative_slope), 0.0, True
        self.lin_l = torch.nn.Linear(self.in_channels, self.heads * self.out_channels, bias=False)
        self.lin_r = self.lin_l
        self.att_l = Parameter(torch.empty(1, self.heads, self.out_channels))
        self.att_r = Parameter(torch.empty(1, self.heads, self.out_channels))
        if bias:
            self.bias = Parameter(torch.empty(self.heads * self.out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        glorot(self.lin_l.weight)
        glorot(self.att_l)
        glorot(self.att_r)
        zeros(self.bias)

    def forward(self, x, edge_index, act=None, _road=None):
        """edge_index: int64 [2, E] = (source, target) or its GraphCSR.  _road='torch' forces the composition."""
        if isinstance(x, (tuple, list)):
            raise NotImplementedError('GATConv: x as a tuple (bipartite inputs) is not implemented')
        if _road != 'torch' and Fn.gat_conv_supported(x, self.heads, self.out_channels):
            csr = csr_for(edge_index, int(x.size(0)))
            return Fn.GATConvFunction.apply(x, csr, self.lin_l.weight, self.att_l, self.att_r, self.bias, act)
        Fn._path('gat', 'torch ops (outside the fused attention kernel)', '-', self.in_channels, self.heads * self.out_channels)
        if isinstance(edge_index, GraphCSR):
            edge_index = Fn.csr_edge_index(edge_index)
        return Fn.gat_conv_torch(x, edge_index, self.lin_l.weight, self.att_l, self.att_r, self.bias, act)

    def __repr__(self):
        return '%s(%d, %d, heads=%d)' % (self.__class__.__name__, self.in_channels, self.out_channels, self.heads)
