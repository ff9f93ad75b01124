"""Expressive-power evaluation: which pairs of non-isomorphic graphs an untrained model maps to the same embedding over many
random seeds -- the isomorphism tests of sr25.py:281-300, graph8c.py:282-302 and exp_iso.py:284-304:

    for s in seeds:  torch.manual_seed(s); E = model()(all graphs)
        M += |E_i - E_j|_1 > 0.001      all pairs i < j (sr25, graph8c) or the pairs (2k, 2k+1) (EXP)
        similar = number of pairs with M == 0

Here M is a bitmap on the device (csrc/gml_pairs.hip, include/gml.h): one bit per pair, set once a seed separates the pair.  The
distance is summed in numpy's float32 order and compared with float32(tol), so the counts equal the reference's numpy ones.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .graph import _ptr, _stream


class PairTracker(object):
    """Never-separated pairs of `num_graphs` graph embeddings, accumulated over updates.

    pairs=None: every pair i < j; else an int [P, 2] list of pairs (EXP: (2k, 2k + 1)).  tol: the reference's 0.001, compared
    in float32.  update() has no host read, so it can be captured in a graph; similar() and similar_pairs() read the count."""

    def __init__(self, num_graphs, tol=1e-3, pairs=None, device=None):
        G = int(num_graphs)
        if G < 0 or _lib.lib().gml_pair_bitmap_words(G, -1) < 0:
            raise ValueError('PairTracker: num_graphs must be in [0, 65536], got %d' % G)
        self.G, self.tol = G, float(np.float32(tol))
        dev = torch.device('cuda' if device is None else device)
        if dev.type != 'cuda':
            raise ValueError('PairTracker: the bitmap lives on a GPU, got device %s' % dev)
        self.device = dev if dev.index is not None else torch.device('cuda', torch.cuda.current_device())
        if pairs is None:
            self.pairs, self.P = None, -1
        else:
            p = torch.as_tensor(pairs)
            if p.dim() != 2 or p.size(1) != 2 or p.dtype.is_floating_point or p.dtype == torch.bool:
                raise ValueError('PairTracker: pairs must be an integer [P, 2] array')
            if p.numel() and (int(p.min()) < 0 or int(p.max()) >= G):
                raise ValueError('PairTracker: pair indices must lie in [0, %d)' % G)
            self.pairs = p.to(device=self.device, dtype=torch.int32).contiguous()
            self.P = int(self.pairs.size(0))
        nw = int(_lib.lib().gml_pair_bitmap_words(G, self.P))
        self.bits = torch.zeros(max(nw, 1), dtype=torch.int64, device=self.device)
        self.count = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._ws = None

    @property
    def num_pairs(self):
        return self.G * (self.G - 1) // 2 if self.pairs is None else self.P

    def reset(self):
        """forget every update: no pair separated"""
        self.bits.zero_()

    def _check(self, emb):
        if not isinstance(emb, torch.Tensor) or emb.dtype != torch.float32:
            raise TypeError('PairTracker.update: float32 tensor expected, got %s' % getattr(emb, 'dtype', type(emb)))
        if emb.device != self.device:
            raise ValueError('PairTracker.update: embeddings on %s, tracker on %s' % (emb.device, self.device))
        if emb.dim() != 2 or emb.size(0) != self.G or not 1 <= emb.size(1) <= 128:
            raise ValueError('PairTracker.update: [%d, D] embeddings with 1 <= D <= 128 expected, got %s' % (self.G, list(emb.shape)))
        if emb.stride(1) != 1 or emb.stride(0) < emb.size(1):
            emb = emb.contiguous()
        return emb

    def update(self, emb):
        """mark the pairs these embeddings [G, D] separate (sum_k |E_i - E_j| > tol)"""
        emb = self._check(emb)
        L, D, ld = _lib.lib(), int(emb.size(1)), int(emb.stride(0))
        with torch.cuda.device(self.device):
            st = _stream(self.device)
            if self.pairs is None:
                _lib.check(L.gml_pair_distinct_all(_ptr(emb), ld, self.G, D, ctypes.c_float(self.tol), _ptr(self.bits), st))
            else:
                _lib.check(L.gml_pair_distinct_list(_ptr(emb), ld, self.G, _ptr(self.pairs), self.P, D, ctypes.c_float(self.tol),
                                                    _ptr(self.bits), st))

    def count_device(self):
        """the never-separated count as an int64 [1] device tensor (no host read: capturable).  The tensor is the tracker's own
        buffer, overwritten by the next count."""
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().gml_pair_count_similar(_ptr(self.bits), self.G, _ptr(self.pairs), max(self.P, 0), _ptr(self.count),
                                                         _stream(self.device)))
        return self.count

    def similar(self):
        """the reference's `sm`: pairs never separated by any update (one host read)"""
        return int(self.count_device().item())

    def similar_pairs(self, cap=None):
        """int64 [K, 2] never-separated pairs (i, j): ascending (i, j) for all pairs, list order for a pair list.  cap: return at
        most that many (the first ones); None: all of them (one extra host read for the size)."""
        L = _lib.lib()
        if self._ws is None:
            nb = int(L.gml_pair_list_workspace_bytes(self.G, self.P))
            self._ws = torch.empty(max(nb // 8, 1), dtype=torch.int64, device=self.device)
        if cap is None:
            cap = self.similar()
        cap = int(cap)
        out = torch.empty(max(cap, 1), 2, dtype=torch.int64, device=self.device)
        cnt = torch.empty(1, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(L.gml_pair_list_similar(_ptr(self.bits), self.G, _ptr(self.pairs), max(self.P, 0), _ptr(out), cap, _ptr(cnt),
                                               _ptr(self._ws), self._ws.numel() * 8, _stream(self.device)))
        k = min(int(cnt.item()), cap)
        return out[:k]


def exp_pairs(num_graphs):
    """the pairs (2k, 2k + 1) of EXP (exp_iso.py:301: E[0::2] against E[1::2])"""
    k = np.arange(num_graphs // 2, dtype=np.int64)
    return np.stack([2 * k, 2 * k + 1], 1)


def count_similar(factory, batch, seeds, tol=1e-3, pairs=None, tracker=None):
    """The reference loop: for each seed, torch.manual_seed(seed), build the model on the CPU with factory(), move it to the
    batch's device in eval mode, embed the whole data set in one no_grad forward and update the pair bitmap.  batch: the whole
    data set as one device Batch (graph.collate(...).to(dev)).  Returns the cumulative never-separated count after each seed (the
    lines the scripts print); pass a PairTracker as `tracker` to keep the bitmap (similar_pairs())."""
    dev = batch.x.device
    if dev.type != 'cuda':
        raise ValueError('count_similar: the batch must be on a GPU')
    if tracker is None:
        tracker = PairTracker(batch.num_graphs, tol=tol, pairs=pairs, device=dev)
    counts = []
    for s in seeds:
        torch.manual_seed(int(s))
        model = factory().to(dev).eval()
        with torch.no_grad():
            emb = model(batch)
        tracker.update(emb.float())
        counts.append(tracker.similar())
    return counts
