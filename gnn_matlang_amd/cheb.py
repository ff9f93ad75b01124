"""ChebConv: the spectral baseline of the experiment scripts (ChebNet, e.g. Zinc12k.py:193-219, sr25.py:149-167) with the parameters
and names of torch_geometric 1.6.1's ChebConv -- the version the reference's README pins -- at normalization='sym':

    Tx_0 = x,  Tx_1 = L^ x,  Tx_k = 2 L^ Tx_{k-1} - Tx_{k-2};   out = bias + sum_k Tx_k weight[k]
    L^ = (2 / lambda_max) (I - D^-1/2 A D^-1/2) - I

Self loops of edge_index are dropped, every other edge occurrence counts (duplicates included); D counts a node's edges as a SOURCE.
lambda_max is None (2.0, as 1.6.1 takes for 'sym'), a number, or a tensor [B] indexed by batch.  Inside the range of
functional.cheb_conv_supported (K <= 8, widths <= 64) the layer runs on csrc/gml_cheb.hip (functional.ChebConvFunction); every other
shape takes the composition functional.cheb_conv_torch.
"""
import math

import torch

from . import functional as Fn
from .graph import GraphCSR, csr_for


class ChebConv(torch.nn.Module):
    """state_dict: weight [K, in_channels, out_channels], then bias [out_channels]; glorot(weight), zeros(bias) as 1.6.1.
    forward(x, csr_or_edge_index, batch=None, lambda_max=None, act=None, norm=None): act in (None, 'relu', 'tanh') is the activation
    the scripts apply AFTER the layer; on the fused road it is applied in the launch that writes the output.  norm: the result of
    functional.cheb_norm for this graph, batch and lambda_max, which every layer of a model shares (batch and lambda_max are then
    not read on the fused road).  lambda_max <= 0 or not finite is outside the contract: the module reads nothing on the host, so it
    cannot check, and the output is then inf / nan or meaningless."""

    def __init__(self, in_channels, out_channels, K, normalization='sym', bias=True):
        super().__init__()
        if int(K) < 1:
            raise ValueError('ChebConv: K >= 1, got %r' % (K,))
        if normalization != 'sym':
            raise NotImplementedError("ChebConv: normalization=%r is not implemented (only 'sym', which every experiment script uses)"
                                      % (normalization,))
        self.in_channels, self.out_channels, self.normalization = int(in_channels), int(out_channels), normalization
        self.weight = torch.nn.Parameter(torch.empty(int(K), self.in_channels, self.out_channels))
        if bias:
            self.bias = torch.nn.Parameter(torch.empty(self.out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        a = math.sqrt(6.0 / (self.weight.size(-2) + self.weight.size(-1)))      # (1.6.1's glorot: the last two dimensions)
        self.weight.data.uniform_(-a, a)
        if self.bias is not None:
            self.bias.data.fill_(0)

    def forward(self, x, edge_index, batch=None, lambda_max=None, act=None, norm=None, _road=None):
        """edge_index: int64 [2, E] = (source, target) or its GraphCSR.  _road='torch' forces the composition."""
        K = int(self.weight.size(0))
        if _road != 'torch' and Fn.cheb_conv_supported(x, self.out_channels, K):
            csr = csr_for(edge_index, int(x.size(0)))
            if norm is None:
                norm = Fn.cheb_norm(csr, batch, lambda_max)
            return Fn.ChebConvFunction.apply(x, csr, norm, self.weight, self.bias, act)
        if isinstance(edge_index, GraphCSR):
            edge_index = Fn.csr_edge_index(edge_index)
        Fn._path('cheb', 'torch ops (outside the fused layer)', K, int(x.size(1)), self.out_channels)
        return Fn.cheb_conv_torch(x, edge_index, self.weight, self.bias, batch, lambda_max, act)

    def __repr__(self):
        return '%s(%d, %d, K=%d, normalization=%s)' % (self.__class__.__name__, self.in_channels, self.out_channels,
                                                        self.weight.size(0), self.normalization)
