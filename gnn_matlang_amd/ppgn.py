"""The dense input tensors of PPGN (Maron et al., the 3-WL baseline of every experiment script), built on the device.

libs/utils.py:613-624 stores, per graph, X2 [1, nfeat + 2, nmax, nmax] and M [1, 2, nmax, nmax]:
    X2 channel 0     the adjacency (1 at every (source, target) of edge_index)
    X2 channel 1     the identity on the first n diagonal entries
    X2 channel 2 + j diag(x[:, j]) for the first nfeat feature columns -- nfeat is counted BEFORE SpectralDesign appends the degree,
                     so the degree column is never placed (the reference's quirk, kept)
    M channel 0      the diagonal mask, channel 1 the off-diagonal mask inside n x n
and everything is zero in the padding.  ppgn_inputs builds them for a whole device Batch in one fill and one launch
(csrc/gml_ppgn.hip: gml_ppgn_inputs) with no host read; ppgn_inputs_host restates one graph in numpy (the tests' reference)."""
import numpy as np
import torch

from . import _lib
from .graph import _ptr, _stream, _require_cuda


def ppgn_inputs_host(x, edge_index, nmax, nfeat):
    """numpy restatement for ONE graph: x [n, F >= nfeat], edge_index [2, e] (local node ids) -> X2 [nfeat + 2, nmax, nmax],
    M [2, nmax, nmax] float32 and n."""
    x = np.asarray(x, dtype=np.float32)
    x = x.reshape(x.shape[0], -1)
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    n, nmax, nfeat = int(x.shape[0]), int(nmax), int(nfeat)
    if n > nmax:
        raise ValueError('ppgn_inputs_host: a graph of %d nodes does not fit nmax = %d' % (n, nmax))
    if nfeat > x.shape[1]:
        raise ValueError('ppgn_inputs_host: nfeat = %d, x has %d columns' % (nfeat, x.shape[1]))
    X2 = np.zeros((nfeat + 2, nmax, nmax), dtype=np.float32)
    M = np.zeros((2, nmax, nmax), dtype=np.float32)
    X2[0, ei[0], ei[1]] = 1
    d = np.arange(n)
    X2[1, d, d] = 1
    for j in range(nfeat):
        X2[2 + j, d, d] = x[:, j]
    M[0, d, d] = 1
    M[1, :n, :n] = 1 - M[0, :n, :n]
    return X2, M, n


def ppgn_inputs(batch, nmax, nfeat):
    """X2 [B, nfeat + 2, nmax, nmax], M [B, 2, nmax, nmax] (float32) and n [B] (int32) of a device Batch (x, edge_index, ptr, batch).
    One zero fill (X2 and M share one allocation) and one launch; no host read while a graph is being captured.  Raises for a graph
    larger than nmax -- a host check of n, skipped under capture (there such a graph gets no pixel at all)."""
    x = batch.x
    _require_cuda(x, 'batch.x')
    if x.dtype != torch.float32 or x.dim() != 2:
        raise TypeError('ppgn_inputs: batch.x must be float32 [N, F]')
    nmax, nfeat = int(nmax), int(nfeat)
    if nmax < 1 or not 0 <= nfeat <= x.size(1):
        raise ValueError('ppgn_inputs: nmax >= 1 and 0 <= nfeat <= %d expected, got nmax = %d, nfeat = %d' % (x.size(1), nmax, nfeat))
    dev = x.device
    from .functional import _ptr32
    ptr = _ptr32(batch.ptr)
    B, N = int(ptr.numel() - 1), int(x.size(0))
    ei = batch.edge_index
    if ei.dtype != torch.int64:
        ei = ei.to(torch.int64)
    ei = ei.contiguous()
    E = int(ei.size(1))
    gid = batch.batch
    if gid.dtype != torch.int64:
        gid = gid.to(torch.int64)
    gid = gid.contiguous()
    if x.stride(1) != 1:
        x = x.contiguous()
    P = nmax * nmax
    with torch.cuda.device(dev):
        buf = torch.zeros(B * (nfeat + 4) * P, dtype=torch.float32, device=dev)
        X2 = buf[:B * (nfeat + 2) * P].view(B, nfeat + 2, nmax, nmax)
        M = buf[B * (nfeat + 2) * P:].view(B, 2, nmax, nmax)
        n = torch.empty(B, dtype=torch.int32, device=dev)
        _lib.call('gml_ppgn_inputs', _ptr(x), int(x.stride(0)), nfeat, _ptr(ei[0]), _ptr(ei[1]), E, _ptr(ptr), _ptr(gid), N, B, nmax,
                  _ptr(X2), _ptr(M), _ptr(n), _stream(dev))
        if B and not torch.cuda.is_current_stream_capturing():
            big = int(n.max())
            if big > nmax:
                raise ValueError('ppgn_inputs: a graph of %d nodes does not fit nmax = %d' % (big, nmax))
    return X2, M, n


def attach(batch, nmax, nfeat):
    """store X2, M and ppgn_n on the batch (models.PPGN reads data.X2 and data.ppgn_n; expressivity.count_similar works as it is)"""
    batch.X2, batch.M, batch.ppgn_n = ppgn_inputs(batch, nmax, nfeat)
    return batch
