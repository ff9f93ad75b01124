"""Device-resident data set and batch assembly (the role ``InMemoryDataset`` + ``DataLoader`` play in the reference
scripts, e.g. /root/reference/Zinc12k.py:13-22, where every batch is collated on the host and copied with
``data.to(device)``, Zinc12k.py:360).

Here the whole data set -- node features, raw edges, the structural edges of the mask and their ``m x S`` supports
(``SpectralDesign``'s output) -- is concatenated once and kept in HBM (ZINC-12k with its supports is ~110 MB); a batch is
assembled ON the device from a tensor of graph ids with a handful of gathers, so an epoch of shuffled mini-batches never
touches the host arrays again.  The result is a ``Batch`` with PyG-compatible field names.
"""
import numpy as np
import torch

from .graph import Batch


def pair_support_edges(edge_index2, edge_ptr2, node_ptr, edge_attr2):
    """Mirror pairing of every graph's support edges (torch only; CPU or GPU tensors), with the semantics of include/gml.h
    gml_edge_sym_flags: per edge (graph-LOCAL ids, each graph's edges in its own order) flag 2 = evaluate, and its mirror (dst, src)
    takes the same row (src < dst, the two rows bitwise equal); 0 = covered by its mirror; 1 = evaluate alone (self loops, repeated
    edges, edges without a mirror or whose mirror differs in any bit).  The mirror is found by a sort of the (src, dst) keys, so the
    order of the targets inside a source row does not matter.  Returns (flag [E] int32, mirror [E] int64: the mirror's position for
    flag 2, else -1; sym_ptr [G + 1] int64, uid [U] int32, mir [U] int32): per graph g its entries sym_ptr[g] .. sym_ptr[g + 1] -- the
    edges with flag > 0 in edge order, as graph-local positions, and their mirror's local position (-1: none)."""
    dev = edge_index2.device
    E, G = int(edge_index2.size(1)), int(node_ptr.numel()) - 1
    e = edge_ptr2[1:] - edge_ptr2[:-1]
    gid = torch.repeat_interleave(torch.arange(G, device=dev), e, output_size=E)
    nbase, ebase = node_ptr[gid], edge_ptr2[gid]
    src, dst = edge_index2[0] + nbase, edge_index2[1] + nbase
    n = int(node_ptr[-1]) + 1
    key, mkey = src * n + dst, dst * n + src
    skey, order = torch.sort(key)
    dup = torch.searchsorted(skey, key, right=True) - torch.searchsorted(skey, key) > 1
    mlo = torch.searchsorted(skey, mkey)
    one_mirror = torch.searchsorted(skey, mkey, right=True) - mlo == 1
    mpos = order[mlo.clamp(max=max(E - 1, 0))]
    rows = edge_attr2.contiguous().view(torch.int32)
    pair = (src != dst) & ~dup & one_mirror
    same = pair & (rows == rows[mpos]).all(1)
    flag = torch.ones(E, dtype=torch.int32, device=dev)
    flag[same & (src > dst)] = 0
    flag[same & (src < dst)] = 2
    mirror = torch.where(flag == 2, mpos, torch.full_like(mpos, -1))
    sel = torch.nonzero(flag > 0, as_tuple=False).view(-1)
    uid = (sel - ebase[sel]).int()
    ms = mirror[sel]
    mir = torch.where(ms >= 0, ms - ebase[sel], ms).int()
    sym_ptr = torch.zeros(G + 1, dtype=torch.int64, device=dev)
    sym_ptr[1:] = torch.cumsum(torch.bincount(gid[sel], minlength=G), 0)
    return flag, mirror, sym_ptr, uid, mir


class DeviceDataset(object):
    """x [N,F], node_ptr [G+1], edge_index / edge_index2 (graph-LOCAL node ids) with edge_ptr / edge_ptr2 [G+1],
    edge_attr2 [E2,S], y [G]; all on one device."""

    def __init__(self, x, node_ptr, edge_index, edge_ptr, edge_index2, edge_ptr2, edge_attr2, y):
        self.x, self.node_ptr, self.edge_index, self.edge_ptr = x, node_ptr, edge_index, edge_ptr
        self.edge_index2, self.edge_ptr2, self.edge_attr2, self.y = edge_index2, edge_ptr2, edge_attr2, y
        self.graph_fields = {}                                 # name -> float32 [G]: one value per graph (from_graphs(graph_fields=))

    def __len__(self):
        return int(self.node_ptr.numel() - 1)

    def tiled(self, reps):
        """The data set repeated `reps` times (graph g + k G is graph g): a large data set of known graphs."""
        dev = self.node_ptr.device
        k = torch.arange(reps, device=dev).view(-1, 1)

        def ptr(p):
            return torch.cat([(p[:-1].view(1, -1) + k * p[-1]).reshape(-1), (p[-1:] * reps)])
        two = lambda t: t.repeat(1, reps) if t is not None else None
        out = DeviceDataset(self.x.repeat(reps, 1), ptr(self.node_ptr), two(self.edge_index), ptr(self.edge_ptr), two(self.edge_index2),
                            ptr(self.edge_ptr2) if self.edge_ptr2 is not None else None,
                            self.edge_attr2.repeat(reps, 1) if self.edge_attr2 is not None else None, self.y.repeat(reps))
        out.graph_fields = dict((k, v.repeat(reps)) for k, v in self.graph_fields.items())
        return out

    def _graph_fields(self, ids, padded=False):
        """the graph fields of the graphs ``ids`` (torch indexing of static shape, no host read).  padded: B + 1 entries like y; absent
        slots (ids == len(self)) and the padding graph hold the field's neutral value: 2.0 for lmax (torch_geometric's lambda_max of
        the 'sym' Laplacian when none is given), 0 for any other field."""
        out = {}
        for k, v in self.graph_fields.items():
            if not padded:
                out[k] = v[ids]
                continue
            G = len(self)
            fill = torch.full((1,), 2.0 if k == 'lmax' else 0.0, dtype=v.dtype, device=v.device)
            out[k] = torch.cat([torch.where(ids < G, v[ids.clamp(max=G - 1)], fill.expand(ids.numel())), fill])
        return out

    @staticmethod
    def from_graphs(graphs, device, graph_fields=()):
        """graphs: dicts with x, edge_index, y and (optionally) edge_index2 / edge_attr2, as ``SpectralDesign`` returns.
        graph_fields: keys that hold ONE float per graph (('lmax',), which the ChebNets read), kept as float32 [G] in the dict
        ``graph_fields`` and carried into every batch as Batch.<key>.  Nothing is carried unless it is named here."""
        graphs = list(graphs)
        xs = [np.asarray(g['x'], dtype=np.float32) for g in graphs]
        nptr = np.zeros(len(graphs) + 1, dtype=np.int64)
        nptr[1:] = np.cumsum([x.shape[0] for x in xs])

        def edges(key):
            es = [np.asarray(g[key], dtype=np.int64) for g in graphs]
            ptr = np.zeros(len(graphs) + 1, dtype=np.int64)
            ptr[1:] = np.cumsum([e.shape[1] for e in es])
            return torch.from_numpy(np.concatenate(es, 1)).to(device), torch.from_numpy(ptr).to(device)
        ei, ep = edges('edge_index')
        if 'edge_index2' in graphs[0]:
            ei2, ep2 = edges('edge_index2')
            ea2 = torch.from_numpy(np.concatenate([np.asarray(g['edge_attr2'], dtype=np.float32) for g in graphs])).to(device)
        else:
            ei2 = ep2 = ea2 = None
        y = torch.tensor(np.asarray([g.get('y', 0) for g in graphs])).to(device)
        ds = DeviceDataset(torch.from_numpy(np.concatenate(xs)).to(device), torch.from_numpy(nptr).to(device),
                           ei, ep, ei2, ep2, ea2, y)
        for k in tuple(graph_fields):
            ds.graph_fields[k] = torch.tensor([float(np.asarray(g[k]).reshape(-1)[0]) for g in graphs], dtype=torch.float32).to(device)
        return ds

    @staticmethod
    def _ranges(ptr, ids):
        """(flat source positions of the segments ids select, new segment pointer [B+1]); one host read (the total)."""
        lo, n = ptr[ids], ptr[ids + 1] - ptr[ids]
        newptr = torch.zeros(ids.numel() + 1, dtype=torch.int64, device=ids.device)
        newptr[1:] = torch.cumsum(n, 0)
        total = int(newptr[-1])
        seg = torch.repeat_interleave(torch.arange(ids.numel(), device=ids.device), n, output_size=total)
        pos = torch.arange(total, device=ids.device) - newptr[seg] + lo[seg]
        return pos, newptr, seg

    def batch(self, ids):
        """Block-diagonal batch of the graphs ``ids`` (int64 tensor on the data set's device), in that order."""
        npos, nptr, nseg = self._ranges(self.node_ptr, ids)
        out = dict(x=self.x[npos], batch=nseg, ptr=nptr.int(), y=self.y[ids])
        base = nptr[:-1]

        def take(ei, ep):
            epos, _, eseg = self._ranges(ep, ids)
            return ei[:, epos] + base[eseg].unsqueeze(0), epos
        out['edge_index'], _ = take(self.edge_index, self.edge_ptr)
        if self.edge_index2 is not None:
            out['edge_index2'], epos2 = take(self.edge_index2, self.edge_ptr2)
            out['edge_attr2'] = self.edge_attr2[epos2]
        out.update(self._graph_fields(ids))
        return Batch(**out)

    # ------------------------------------------------------------------ equal-size graphs of 97 .. 256 nodes: dense blocks from a bank
    def equal_bank(self):
        """dense_block.EqualSupports of the whole data set (cached): its graphs must all have the same n, 96 < n <= 256 (freqclass.py:
        bandclass graphs of 200 nodes) -- ValueError otherwise.  One host read (the graph sizes)."""
        bank = getattr(self, '_equal_bank', None)
        if bank is None:
            from .dense_block import EqualSupports
            if self.edge_index2 is None:
                raise ValueError('equal_bank: the data set has no supports (edge_index2 / edge_attr2)')
            sizes = (self.node_ptr[1:] - self.node_ptr[:-1])
            lo, hi = (int(v) for v in torch.stack([sizes.min(), sizes.max()]).cpu()) if sizes.numel() else (0, 0)
            if lo != hi:
                raise ValueError('equal_bank: the graphs have %d .. %d nodes; the equal-size bank takes ONE size' % (lo, hi))
            E = int(self.edge_index2.size(1))
            eg = torch.searchsorted(self.edge_ptr2[1:].contiguous(), torch.arange(E, device=self.edge_ptr2.device), right=True)
            bank = self._equal_bank = EqualSupports(self.edge_index2 + (eg * lo).unsqueeze(0), self.edge_attr2, self.node_ptr)
        return bank

    def batch_dense(self, ids, out=None):
        """Batch of the graphs ``ids`` (int64 tensor on the data set's device, or a sequence) for the batched dense road
        (models.GNNML3 with the EqualSupports bank of equal_bank()): x [B n, F], y [B], batch, ptr, bank and gid = the bank slots --
        and NO edge tensors: the layers read the supports from the bank.  The shape depends on B alone, so ONE captured step serves
        an epoch: out = a batch of an earlier call with as many ids -- its x, y and gid are overwritten in place and it is returned.
        No host read when ids is a device tensor."""
        bank = self.equal_bank()
        dev = self.x.device
        if not isinstance(ids, torch.Tensor):
            ids = torch.as_tensor(ids, dtype=torch.int64)
        ids = ids.to(device=dev, dtype=torch.int64)
        B, n, F = int(ids.numel()), bank.n, int(self.x.size(1))
        xs = self.x.view(bank.G, n, F)
        if out is not None:
            if getattr(out, 'bank', None) is not bank or int(out.gid.numel()) != B:
                raise ValueError('batch_dense: out= must be a batch_dense batch of this data set with %d graphs' % B)
            torch.index_select(xs, 0, ids, out=out.x.view(B, n, F))
            torch.index_select(self.y, 0, ids, out=out.y)
            out.gid.copy_(ids)
            return out
        return Batch(x=xs[ids].reshape(B * n, F), y=self.y[ids], gid=ids.to(torch.int32),
                     batch=torch.arange(B, device=dev).repeat_interleave(n, output_size=B * n),
                     ptr=torch.arange(B + 1, device=dev, dtype=torch.int32) * n, bank=bank)

    # ------------------------------------------------------------------ static shapes: one captured step for every batch
    def bounds(self, batch_size):
        """dict(n_pad, e2_pad, dmax, deal, caps) that hold for EVERY batch of batch_size graphs of this data set -- what a
        HIP-graph-captured step is sized with (one host read per data set, not per batch).  caps = (edges, column window)
        per 128 source rows; n_pad leaves room for e2_pad / deal padding nodes, so that the padding edges can be dealt `deal`
        (<= dmax) per node and the caps also hold on the padding."""
        n = (self.node_ptr[1:] - self.node_ptr[:-1])
        e = (self.edge_ptr2[1:] - self.edge_ptr2[:-1])
        gid = torch.repeat_interleave(torch.arange(len(self), device=n.device), e)
        deg = torch.bincount(self.edge_index2[0] + self.node_ptr[gid], minlength=int(self.x.size(0)))
        # the raw adjacency (edge_index): its padded edge count and deal ride on the same host read (additive keys, below)
        ea_ = (self.edge_ptr[1:] - self.edge_ptr[:-1])
        gida = torch.repeat_interleave(torch.arange(len(self), device=n.device), ea_)
        dega = torch.cat([torch.bincount(self.edge_index[r] + self.node_ptr[gida], minlength=int(self.x.size(0))) for r in (0, 1)])
        nmax, n_top, e_top, dmax, ea_top, dmaxa = [int(v) for v in torch.stack([
            n.max(), torch.topk(n, min(batch_size, n.numel()))[0].sum(), torch.topk(e, min(batch_size, e.numel()))[0].sum(),
            deg.max(), torch.topk(ea_, min(batch_size, ea_.numel()))[0].sum(), dega.max()]).tolist()]
        dmax = max(dmax, 1)
        e2_pad = (e_top + 63) // 64 * 64
        # padding edges are dealt `deal` per padding node = the data set's mean degree, rounded up: a 128-row group of padding then
        # carries the edge count of a group of real rows (dealt dmax per node -- rounds 2-3 -- the padding groups held 2.2 x the edges
        # of a real group and a one-group-per-workgroup launch waited for them: ZINC batch 64, conv forward 52 -> 23 us)
        deal = max(1, min(dmax, -(-int(self.edge_index2.size(1)) // max(int(self.x.size(0)), 1))))
        n_pad = (n_top + (e2_pad + deal - 1) // deal + 127) // 128 * 128
        # raw adjacency (batch_padded / batch_assembled with adjacency=True): e_pad edges; the padding edges are unit self loops on
        # the n_pad - n_top (>= 1: e2_pad >= 1 padding-room nodes above) padding nodes every batch has at least, e_deal per node;
        # e_caps bound its 128-row groups like caps.  caps64: caps for 64-row groups (the 4-wave kernel families' records)
        e_pad = (ea_top + 63) // 64 * 64
        e_deal = max(1, -(-e_pad // max(n_pad - n_top, 1)))
        return dict(n_pad=n_pad, e2_pad=e2_pad, dmax=dmax, deal=deal, caps=(128 * dmax, 128 + 2 * nmax),
                    e_pad=e_pad, e_deal=e_deal, e_caps=(128 * max(dmaxa, e_deal, 1), 128 + 2 * nmax), caps64=(64 * dmax, 64 + 2 * nmax))

    def batch_padded(self, ids, bounds, adjacency=False):
        """The batch of graphs ``ids`` (entries equal to len(self) = no graph) padded to bounds['n_pad'] nodes and
        bounds['e2_pad'] support edges with torch ops of STATIC shapes only (no host read): padding nodes carry zero
        features and form one extra graph (index B) at the end; padding edges are zero-valued self loops dealt bounds['deal'] per
        padding node (sorted by source like the rest; a zero support stays zero through the bias-free edge MLP and moves
        no gradient).  Returns a Batch with ptr [B + 2], y [B + 1] and ``graph_valid`` [B] (0 for absent graphs).
        adjacency=True: also the raw adjacency ``edge_index`` padded to bounds['e_pad'] edges -- each real graph's edges in its own
        order, offset to its node range, then self loops on padding nodes only, dealt bounds['e_deal'] per padding node (the GNNML1
        models give them unit values; a padding node never reaches a real one)."""
        n_pad, e2_pad, dmax = bounds['n_pad'], bounds['e2_pad'], bounds.get('deal', bounds['dmax'])
        dev = ids.device
        B = int(ids.numel())
        G = len(self)
        has = ids < G
        idc = ids.clamp(max=G - 1)

        def layout(ptr, total_pad):
            lo = ptr[idc]
            cnt = torch.where(has, ptr[idc + 1] - lo, torch.zeros_like(lo))
            new = torch.zeros(B + 1, dtype=torch.int64, device=dev)
            new[1:] = torch.cumsum(cnt, 0)
            j = torch.arange(total_pad, device=dev)
            seg = torch.searchsorted(new[1:].contiguous(), j, right=True)      # = B at and beyond the real total
            ok = seg < B
            sc = seg.clamp(max=B - 1)
            return torch.where(ok, j - new[sc] + lo[sc], torch.zeros_like(j)), new, seg, ok, sc, j
        npos, nptr, nseg, nok, _, _ = layout(self.node_ptr, n_pad)
        epos, eptr, _, eok, esc, k = layout(self.edge_ptr2, e2_pad)
        x = self.x[npos] * nok.unsqueeze(1).to(self.x.dtype)
        pad_node = (nptr[-1] + (k - eptr[-1]).clamp(min=0) // dmax).clamp(max=n_pad - 1)
        ei2 = torch.where(eok.unsqueeze(0), self.edge_index2[:, epos] + nptr[esc].unsqueeze(0), pad_node.unsqueeze(0))
        ea2 = self.edge_attr2[epos] * eok.unsqueeze(1).to(self.edge_attr2.dtype)
        ptr = torch.cat([nptr, torch.full((1,), n_pad, dtype=torch.int64, device=dev)]).int()
        y = torch.cat([torch.where(has, self.y[idc], torch.zeros_like(self.y[idc])), torch.zeros(1, dtype=self.y.dtype, device=dev)])
        # (no `edge_index` unless asked for: a consumer of data.csr('edge_index'), e.g. a GNNML1 model or a K = 1 raw-adjacency conv,
        #  must fail loudly on a padded batch without it instead of computing on the support edges)
        b = Batch(x=x, edge_index2=ei2, edge_attr2=ea2, batch=nseg, ptr=ptr, y=y, graph_valid=has.to(self.x.dtype),
                  **self._graph_fields(ids, padded=True))
        if adjacency:
            e_pad, e_deal = bounds['e_pad'], bounds['e_deal']
            apos, aptr, _, aok, asc, ka = layout(self.edge_ptr, e_pad)
            pad_a = (nptr[-1] + (ka - aptr[-1]).clamp(min=0) // e_deal).clamp(max=n_pad - 1)
            b.edge_index = torch.where(aok.unsqueeze(0), self.edge_index[:, apos] + nptr[asc].unsqueeze(0), pad_a.unsqueeze(0))
        b.static_caps = bounds['caps']
        b.pad_graph = True                                 # the last graph is padding: pooling skips it (its pooled row is zero)
        return b

    # ------------------------------------------------------------------ precomputed per-graph structure: a batch in ONE launch
    def prepare(self):
        """Once per data set: every graph's own index structure -- the stable target sort of its (source-sorted) support edges,
        its inverse, both local row-pointer prefixes -- and the bf16 pre-split of all supports.  A batch is the block-diagonal
        union of graphs whose structure never changes, so ``batch_assembled`` only adds offsets (csrc/gml_csr.hip
        gml_batch_assemble).  Returns self."""
        if getattr(self, '_prep', None) is not None:
            return self
        from . import functional as Fn
        dev = self.x.device
        E2, Nall, G = int(self.edge_index2.size(1)), int(self.x.size(0)), len(self)
        if self.y.dtype != torch.float32 or self.x.dtype != torch.float32:
            raise TypeError('prepare(): float32 features and targets')
        e = self.edge_ptr2[1:] - self.edge_ptr2[:-1]
        gid = torch.repeat_interleave(torch.arange(G, device=dev), e, output_size=E2)
        nbase, ebase = self.node_ptr[gid], self.edge_ptr2[gid]
        src, dst = self.edge_index2[0] + nbase, self.edge_index2[1] + nbase
        if E2 > 1 and not bool((src[1:] >= src[:-1]).all()):
            raise ValueError('prepare(): the support edges of every graph must be sorted by source (SpectralDesign emits them so)')
        # targets ascending inside every source row too (SpectralDesign's row-major order; any order is accepted): the source view of an
        # exact batch keeps each graph's edge order, and the pairing pass of GraphCSR.sym_index needs its rows sorted
        rows_sorted = E2 <= 1 or bool(((src[1:] > src[:-1]) | (dst[1:] >= dst[:-1])).all())
        order = torch.sort(dst, stable=True)[1]                           # global stable target sort = per-graph stable target sort
        k = torch.arange(E2, device=dev)
        tperm = (order - ebase[order]).int()                              # [position in target order] -> local source-order position
        tinv = torch.empty(E2, dtype=torch.int32, device=dev)
        tinv[order] = (k - ebase[order]).int()                            # [source-order position] -> local position in target order
        first = self.edge_ptr2[torch.repeat_interleave(torch.arange(G, device=dev), self.node_ptr[1:] - self.node_ptr[:-1], output_size=Nall)]

        def local_rows(keys):
            cnt = torch.bincount(keys, minlength=Nall)
            return (torch.cumsum(cnt, 0) - cnt - first).int()
        S = int(self.edge_attr2.size(1))
        es = Fn.edge_presplit(self.edge_attr2.contiguous()) if S <= 8 else None
        self._prep = dict(tperm=tperm.contiguous(), tinv=tinv, rp_src=local_rows(src), rp_dst=local_rows(dst), es=es, rows_sorted=rows_sorted,
                          x=self.x.contiguous(), ea=self.edge_attr2.contiguous(), ei2=self.edge_index2.contiguous(), y=self.y.contiguous())
        self._prep.update(self.adjacency_structure())
        return self

    def pairing(self):
        """The data set's mirror pairing for the edge branch (``pair_support_edges``), computed once per data set (like ``prepare()``'s
        per-graph structure, which batch_assembled offsets the same way): dict(sym_ptr, uid, mir), or None when it does not pay -- supports of S outside 2 .. 16 (the unique-row kernels) or
        more than 0.9 E unique rows (the rule GraphCSR.sym_index applies per batch, decided here once per data set)."""
        if not hasattr(self, '_sym'):
            S, E = int(self.edge_attr2.size(1)), int(self.edge_index2.size(1))
            self._sym = None
            if 2 <= S <= 16 and E > 0:
                _, _, sym_ptr, uid, mir = pair_support_edges(self.edge_index2, self.edge_ptr2, self.node_ptr, self.edge_attr2)
                if uid.numel() <= 0.9 * E:
                    self._sym = dict(sym_ptr=sym_ptr.contiguous(), uid=uid.contiguous(), mir=mir.contiguous())
        return self._sym

    def adjacency_structure(self):
        """Per graph, the structure of its raw adjacency (edge_index, any order inside a graph): the stable target AND source sorts
        of its edges (a_tperm / a_sperm: k-th sorted edge -> input position), the positions that link the two views (a_pos: target-
        sorted position of the k-th source-sorted edge, a_tpos: the converse), both local row-pointer prefixes -- what
        csrc/gml_csr.hip gml_batch_assemble_edges offsets per graph.  Torch ops only (prepare() keeps the result)."""
        dev, Nall, G = self.x.device, int(self.x.size(0)), len(self)
        EA = int(self.edge_index.size(1))
        ga = torch.repeat_interleave(torch.arange(G, device=dev), self.edge_ptr[1:] - self.edge_ptr[:-1], output_size=EA)
        abase, eabase = self.node_ptr[ga], self.edge_ptr[ga]
        asrc, adst = self.edge_index[0] + abase, self.edge_index[1] + abase
        ka = torch.arange(EA, device=dev)
        ot, os_ = torch.sort(adst, stable=True)[1], torch.sort(asrc, stable=True)[1]     # global stable sorts = per-graph stable sorts
        tinv_a, sinv_a = torch.empty(EA, dtype=torch.int64, device=dev), torch.empty(EA, dtype=torch.int64, device=dev)
        tinv_a[ot] = ka - eabase[ot]                                       # [input position] -> local target-sorted position
        sinv_a[os_] = ka - eabase[os_]                                     # [input position] -> local source-sorted position
        firsta = self.edge_ptr[torch.repeat_interleave(torch.arange(G, device=dev), self.node_ptr[1:] - self.node_ptr[:-1], output_size=Nall)]

        def local_rows_a(keys):
            cnt = torch.bincount(keys, minlength=Nall)
            return (torch.cumsum(cnt, 0) - cnt - firsta).int().contiguous()
        out = dict(a_tperm=(ot - eabase[ot]).int().contiguous(), a_sperm=(os_ - eabase[os_]).int().contiguous(),
                   a_pos=tinv_a[os_].int().contiguous(), a_tpos=sinv_a[ot].int().contiguous(),
                   a_rp_src=local_rows_a(asrc), a_rp_dst=local_rows_a(adst), a_ei=self.edge_index.contiguous())
        out['a_sorted'] = bool((out['a_sperm'] == (ka - eabase).int()).all()) if EA else True   # input order = source order
        return out

    def batch_assembled(self, ids, bounds, adjacency=False, groups64=False, sym=False):
        """``batch_padded(ids, bounds)`` AND its index structure (Batch.csr('edge_index2')) in one kernel launch plus the two
        group-record passes, from the per-graph structure ``prepare()`` computed once: bit-identical tensors and CSR arrays
        (tests/test_gpu_parity.py), no host read, capturable.
        adjacency=True: also Batch.csr('edge_index'), both views of ``batch_padded(ids, bounds, adjacency=True)``'s raw adjacency
        (gml_batch_assemble_edges: one launch + its 128-row group records) -- what the GNNML1 models read.
        groups64=True: also the 64-row group records of the support CSR (maxima: bounds['caps64']) -- the 4-wave kernel families of
        the exact-product layer of BatchNorm models (mutag GNNML3) read them, and a captured step cannot build them lazily.
        Any B (gml_batch_assemble_any: the per-graph prefixes in global memory; up to 4096 graphs without ``sym`` the single launch above):
        bounds=None: EXACT mode -- no padding graph, nodes or edges; bit-identical to ``batch(ids)`` + GraphCSR.from_edge_index (ptr
        [B + 1], y [B], no graph_valid; two host reads per batch: the totals, then the group maxima).  A padded batch of this launch that
        exceeds bounds (repeated ids) keeps its leading graphs that fit and flags it: csr('edge_index2').check() raises.
        sym=True: also the data set's mirror pairing (``pairing()``) offset to the batch -- the list of support rows the edge branch has
        to evaluate, its length on the device -- which GraphCSR.sym_index returns for the batch's supports (static shapes and HIP-graph
        capture included).  A data set without a pairing gives the batch without it."""
        from . import _lib
        from .graph import GraphCSR, _ptr, _stream
        self.prepare()
        P = self._prep
        if bounds is None or sym or int(ids.numel()) > 4096:
            return self._assemble_any(ids, bounds, adjacency, groups64, sym)
        n_pad, e2_pad, dmax = bounds['n_pad'], bounds['e2_pad'], bounds.get('deal', bounds['dmax'])
        dev = ids.device
        B, F, S = int(ids.numel()), int(self.x.size(1)), int(self.edge_attr2.size(1))
        if ids.dtype != torch.int64 or not ids.is_contiguous():
            raise ValueError('ids: contiguous int64')
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        ldx = (F + 3) // 4 * 4                                         # float4-addressable rows: the first layer reads them without a padding copy
        xbuf, ea = torch.empty(n_pad, ldx, **f32), torch.empty(e2_pad, S, **f32)
        x = xbuf[:, :F]
        es = torch.empty(e2_pad, 8, **i32) if P['es'] is not None else None
        y, valid = torch.empty(B + 1, **f32), torch.empty(B, **f32)
        ptr, batch = torch.empty(B + 2, **i32), torch.empty(n_pad, **i32)
        g = GraphCSR()
        g.N, g.E, g.device = n_pad, e2_pad, dev
        g.rowptr, g.col, g.perm = torch.empty(n_pad + 1, **i32), torch.empty(e2_pad, **i32), torch.empty(e2_pad, **i32)
        g.rowptr_t, g.col_t, g.pos_t = torch.empty(n_pad + 1, **i32), torch.empty(e2_pad, **i32), torch.empty(e2_pad, **i32)
        ident = P.get('ident')
        if ident is None or ident.numel() != e2_pad:
            ident = P['ident'] = torch.arange(e2_pad, **i32)
        g.perm_t, g.tpos = ident, g.perm
        d = _lib.BatchDesc()
        for name, t in (('node_ptr', self.node_ptr), ('edge_ptr2', self.edge_ptr2), ('x', P['x']), ('edge_index2', P['ei2']), ('edge_attr2', P['ea']),
                        ('es', P['es']), ('tperm', P['tperm']), ('tinv', P['tinv']), ('rp_src', P['rp_src']), ('rp_dst', P['rp_dst']), ('y', P['y']),
                        ('ids', ids), ('x_out', xbuf), ('ea_out', ea), ('es_out', es), ('y_out', y), ('valid_out', valid), ('ptr_out', ptr),
                        ('batch_out', batch), ('rowptr', g.rowptr), ('col', g.col), ('perm', g.perm), ('rowptr_t', g.rowptr_t),
                        ('col_t', g.col_t), ('pos_t', g.pos_t)):
            setattr(d, name, _ptr(t) if t is not None else None)
        d.G, d.E2all, d.F, d.S, d.B, d.n_pad, d.e2_pad, d.dmax = len(self), int(self.edge_index2.size(1)), F, S, B, n_pad, e2_pad, dmax
        d.ldx_out = ldx
        with torch.cuda.device(dev):
            st = _stream(dev)
            import ctypes
            ng2 = max((n_pad + 127) // 128, 1)
            rec128 = int(_lib.lib().gml_csr_group_record_ints(128))
            both = torch.empty(2, ng2, rec128, **i32)                      # (every int of a 128-row record is written: no fill)
            g.ginfo_t128, g.ginfo128 = both[0], both[1]
            d.ginfo128, d.ginfo_t128 = _ptr(g.ginfo128), _ptr(g.ginfo_t128)  # round 5: the group records of both views come out of the same launch
            _lib.call('gml_batch_assemble', ctypes.addressof(d), st)
            if groups64:
                ng = max((n_pad + 63) // 64, 1)
                rec64 = int(_lib.lib().gml_csr_group_record_ints(64))
                g64 = torch.empty(2, ng, rec64, **i32)
                _lib.call('gml_csr_group_info2', _ptr(g.rowptr), _ptr(g.col), _ptr(g64[0]), _ptr(g.rowptr_t), _ptr(g.col_t), _ptr(g64[1]),
                          n_pad, 64, st)
                g._ginfo, g._ginfo_t = g64[0], g64[1]
                g._gmax = g._gmax_t = (int(bounds['caps64'][0]), int(bounds['caps64'][1]))
            ga = self._assemble_edges(ids, bounds, st) if adjacency else None
        g.gmax_t128 = g.gmax128 = (int(bounds['caps'][0]), int(bounds['caps'][1]))
        g.src_sorted = True
        g.static_shape = True
        if es is not None:                                                # the pre-split supports travel with the batch (functional.presplit_of)
            g._val_cache[('p', ea.data_ptr(), ea._version, tuple(ea.shape))] = (ea, es)
        b = Batch(x=x, edge_attr2=ea, batch=batch, ptr=ptr, y=y, graph_valid=valid, **self._graph_fields(ids, padded=True))
        b.static_caps = bounds['caps']
        b.pad_graph = True
        b._csr['edge_index2'] = g
        if ga is not None:
            b._csr['edge_index'] = ga
        b._batch_i32 = batch
        return b

    def _assemble_any(self, ids, bounds, adjacency, groups64, sym):
        """batch_assembled for any B, padded (bounds) or exact (bounds=None), with or without the pairing (gml_batch_assemble_any)."""
        from . import _lib
        from .graph import GraphCSR, _ptr, _stream
        import ctypes
        P = self._prep
        exact = bounds is None
        dev = ids.device
        B, F, S = int(ids.numel()), int(self.x.size(1)), int(self.edge_attr2.size(1))
        if ids.dtype != torch.int64 or not ids.is_contiguous():
            raise ValueError('ids: contiguous int64')
        if B <= 0:
            raise ValueError('batch_assembled: at least one slot')
        if adjacency and (exact or B > 4096):
            raise ValueError('batch_assembled: adjacency=True needs a padded batch of at most 4096 graphs (gml_batch_assemble_edges)')
        pair = self.pairing() if sym else None
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        L = _lib.lib()
        a = _lib.BatchAnyDesc()
        d = a.b
        ws = torch.empty(int(L.gml_batch_any_workspace_bytes(B)), dtype=torch.uint8, device=dev)
        a.ws, a.ws_bytes, a.exact = _ptr(ws), ws.numel(), int(exact)
        for name, t in (('node_ptr', self.node_ptr), ('edge_ptr2', self.edge_ptr2), ('x', P['x']), ('edge_index2', P['ei2']), ('edge_attr2', P['ea']),
                        ('es', P['es']), ('tperm', P['tperm']), ('tinv', P['tinv']), ('rp_src', P['rp_src']), ('rp_dst', P['rp_dst']), ('y', P['y']),
                        ('ids', ids)):
            setattr(d, name, _ptr(t) if t is not None else None)
        d.G, d.E2all, d.F, d.S, d.B = len(self), int(self.edge_index2.size(1)), F, S, B
        if pair is not None:
            a.sym_ptr, a.sym_uid, a.sym_mir = _ptr(pair['sym_ptr']), _ptr(pair['uid']), _ptr(pair['mir'])
        with torch.cuda.device(dev):
            st = _stream(dev)
            if exact:
                # the first host read: the batch's totals (nnew[B], enew[B] of the workspace, include/gml.h)
                _lib.call('gml_batch_scan', ctypes.addressof(a), st)
                w = ws.view(torch.int64)
                n_pad, e2_pad = [int(v) for v in torch.stack([w[4 * B], w[5 * B + 1]]).tolist()]
                if n_pad <= 0:
                    raise ValueError('batch_assembled: the batch has no node')
                a.scanned, dmax, bad = 1, 1, None
            else:
                n_pad, e2_pad, dmax = bounds['n_pad'], bounds['e2_pad'], bounds.get('deal', bounds['dmax'])
                bad = torch.zeros(1, **i32)
                a.bad = _ptr(bad)
            d.n_pad, d.e2_pad, d.dmax = n_pad, e2_pad, dmax
            nb = B if exact else B + 1
            ldx = (F + 3) // 4 * 4
            xbuf, ea = torch.empty(n_pad, ldx, **f32), torch.empty(e2_pad, S, **f32)
            es = torch.empty(e2_pad, 8, **i32) if P['es'] is not None else None
            y, valid = torch.empty(nb, **f32), (None if exact else torch.empty(B, **f32))
            ptr, batch = torch.empty(nb + 1, **i32), torch.empty(n_pad, **i32)
            g = GraphCSR()
            g.N, g.E, g.device = n_pad, e2_pad, dev
            g.rowptr, g.col, g.perm = torch.empty(n_pad + 1, **i32), torch.empty(e2_pad, **i32), torch.empty(e2_pad, **i32)
            g.rowptr_t, g.col_t, g.pos_t = torch.empty(n_pad + 1, **i32), torch.empty(e2_pad, **i32), torch.empty(e2_pad, **i32)
            ident = P.get('ident')
            if ident is None or ident.numel() != e2_pad:
                ident = torch.arange(e2_pad, **i32)
                if not exact:
                    P['ident'] = ident
            g.perm_t, g.tpos = ident, g.perm
            ng2 = max((n_pad + 127) // 128, 1)
            both = torch.empty(2, ng2, int(L.gml_csr_group_record_ints(128)), **i32)
            g.ginfo_t128, g.ginfo128 = both[0], both[1]
            for name, t in (('x_out', xbuf), ('ea_out', ea), ('es_out', es), ('y_out', y), ('valid_out', valid), ('ptr_out', ptr), ('batch_out', batch),
                            ('rowptr', g.rowptr), ('col', g.col), ('perm', g.perm), ('rowptr_t', g.rowptr_t), ('col_t', g.col_t), ('pos_t', g.pos_t),
                            ('ginfo128', g.ginfo128), ('ginfo_t128', g.ginfo_t128)):
                setattr(d, name, _ptr(t) if t is not None else None)
            d.ldx_out = ldx
            uid = mir = count = None
            if pair is not None:
                uid, mir, count = torch.empty(max(e2_pad, 1), **i32), torch.empty(max(e2_pad, 1), **i32), torch.empty(1, **i32)
                a.uid_out, a.mir_out, a.count = _ptr(uid), _ptr(mir), _ptr(count)
            _lib.call('gml_batch_assemble_any', ctypes.addressof(a), st)
            if groups64:
                ng = max((n_pad + 63) // 64, 1)
                g64 = torch.empty(2, ng, int(L.gml_csr_group_record_ints(64)), **i32)
                _lib.call('gml_csr_group_info2', _ptr(g.rowptr), _ptr(g.col), _ptr(g64[0]), _ptr(g.rowptr_t), _ptr(g.col_t), _ptr(g64[1]),
                          n_pad, 64, st)
                g._ginfo, g._ginfo_t = g64[0], g64[1]
                if exact:
                    m64 = torch.stack([g64[0][:, 1].max(), g64[0][:, 3].max(), g64[1][:, 1].max(), g64[1][:, 3].max()]).tolist()
                    g._gmax, g._gmax_t = (int(m64[0]), int(m64[1])), (int(m64[2]), int(m64[3]))
                else:
                    g._gmax = g._gmax_t = (int(bounds['caps64'][0]), int(bounds['caps64'][1]))
            ga = self._assemble_edges(ids, bounds, st) if adjacency else None
        if exact:
            # the second host read: the batch's group maxima (what GraphCSR.from_edge_index reads for a new batch)
            mx = torch.stack([g.ginfo_t128[:, 1].max(), g.ginfo_t128[:, 3].max(), g.ginfo128[:, 1].max(), g.ginfo128[:, 3].max()]).tolist()
            g.gmax_t128, g.gmax128 = (int(mx[0]), int(mx[1])), (int(mx[2]), int(mx[3]))
            # (what from_edge_index records for the same edges: sources ascend inside every target row of the stable target sort)
            g.col_sorted, g.col_t_sorted = True, P['rows_sorted']
        else:
            g.gmax_t128 = g.gmax128 = (int(bounds['caps'][0]), int(bounds['caps'][1]))
            g.static_shape = True
            g._bad = bad
        g.src_sorted = True
        if es is not None:
            g._val_cache[('p', ea.data_ptr(), ea._version, tuple(ea.shape))] = (ea, es)
        if pair is not None:
            g._sym_dev = (ea, uid, mir, count)
        x = xbuf[:, :F]
        if exact:
            b = Batch(x=x, edge_attr2=ea, batch=batch, ptr=ptr, y=y, **self._graph_fields(ids))
        else:
            b = Batch(x=x, edge_attr2=ea, batch=batch, ptr=ptr, y=y, graph_valid=valid, **self._graph_fields(ids, padded=True))
            b.static_caps = bounds['caps']
            b.pad_graph = True
        b._csr['edge_index2'] = g
        if ga is not None:
            b._csr['edge_index'] = ga
        b._batch_i32 = batch
        return b

    def _assemble_edges(self, ids, bounds, st):
        """GraphCSR of the padded raw adjacency of the graphs ``ids`` (batch_assembled(adjacency=True))."""
        from . import _lib
        from .graph import GraphCSR, _ptr
        import ctypes
        P = self._prep
        n_pad, e_pad, dev = bounds['n_pad'], bounds['e_pad'], ids.device
        i32 = dict(dtype=torch.int32, device=dev)
        g = GraphCSR()
        g.N, g.E, g.device = n_pad, e_pad, dev
        ar = torch.empty(2, n_pad + 1, **i32)
        ae = torch.empty(6, e_pad, **i32)
        g.rowptr, g.rowptr_t = ar[0], ar[1]
        g.col, g.perm, g.col_t, g.perm_t, g.pos_t, g.tpos = ae[0], ae[1], ae[2], ae[3], ae[4], ae[5]
        ng2 = max((n_pad + 127) // 128, 1)
        both = torch.empty(2, ng2, int(_lib.lib().gml_csr_group_record_ints(128)), **i32)
        g.ginfo128, g.ginfo_t128 = both[0], both[1]
        d = _lib.BatchEdgesDesc()
        for name, t in (('node_ptr', self.node_ptr), ('edge_ptr', self.edge_ptr), ('edge_index', P['a_ei']), ('tperm', P['a_tperm']),
                        ('sperm', P['a_sperm']), ('pos', P['a_pos']), ('tpos', P['a_tpos']), ('rp_src', P['a_rp_src']),
                        ('rp_dst', P['a_rp_dst']), ('ids', ids), ('rowptr', g.rowptr), ('col', g.col), ('perm', g.perm),
                        ('rowptr_t', g.rowptr_t), ('col_t', g.col_t), ('perm_t', g.perm_t), ('pos_t', g.pos_t), ('tpos_out', g.tpos),
                        ('ginfo128', g.ginfo128), ('ginfo_t128', g.ginfo_t128)):
            setattr(d, name, _ptr(t) if t.numel() else None)
        d.G, d.Eall, d.B, d.n_pad, d.e_pad, d.deal = len(self), int(self.edge_index.size(1)), int(ids.numel()), n_pad, e_pad, bounds['e_deal']
        _lib.call('gml_batch_assemble_edges', ctypes.addressof(d), st)
        g.gmax128 = g.gmax_t128 = (int(bounds['e_caps'][0]), int(bounds['e_caps'][1]))
        g.src_sorted = bool(P['a_sorted'])
        g.static_shape = True
        return g

    def epoch_static(self, batch_size, generator=None, shuffle=True, bounds=None, adjacency=False, groups64=False):
        """One shuffled epoch as STATIC-shape batches (``batch_assembled``): no host read per batch, every batch of the same padded
        shape -- absent slots in the last one.  Use the loss form of a padded batch: ``((pre[:B, 0] - b.y[:B]).abs() * b.graph_valid).sum()``
        (Zinc12k.py:365's L1 sum over the real graphs); models.mutag_loss(..., valid=b.graph_valid) for mutag.
        adjacency / groups64: passed to ``batch_assembled`` (the GNNML1 models need adjacency=True)."""
        G = len(self)
        dev = self.node_ptr.device
        bd = bounds if bounds is not None else self.bounds(batch_size)
        perm = torch.randperm(G, generator=generator).to(dev) if shuffle else torch.arange(G, device=dev)
        perm = torch.cat([perm, torch.full(((-G) % batch_size,), G, dtype=torch.int64, device=dev)])
        for i in range(0, perm.numel(), batch_size):
            yield self.batch_assembled(perm[i:i + batch_size].contiguous(), bd, adjacency=adjacency, groups64=groups64)

    def epoch_assembled(self, batch_size, generator=None, shuffle=True, exact=True, sym=True, bounds=None):
        """One shuffled epoch of ``batch_assembled`` batches of any size.  exact=True: fresh batches without padding (two host reads
        each, none inside the step; the last batch holds the remaining graphs); exact=False: static padded shapes (bounds: as
        ``epoch_static``, absent slots in the last batch).  sym: the data set's mirror pairing travels with every batch (the edge branch
        then evaluates the unique support rows only)."""
        G = len(self)
        dev = self.node_ptr.device
        bd = None if exact else (bounds if bounds is not None else self.bounds(batch_size))
        perm = torch.randperm(G, generator=generator).to(dev) if shuffle else torch.arange(G, device=dev)
        if not exact:
            perm = torch.cat([perm, torch.full(((-G) % batch_size,), G, dtype=torch.int64, device=dev)])
        for i in range(0, perm.numel(), batch_size):
            yield self.batch_assembled(perm[i:i + batch_size].contiguous(), bd, sym=sym)

    def epoch(self, batch_size, generator=None, shuffle=True):
        """yields one shuffled epoch of batches (the DataLoader(shuffle=True) loop of Zinc12k.py:20,359)."""
        G = len(self)
        dev = self.node_ptr.device
        perm = torch.randperm(G, generator=generator).to(dev) if shuffle else torch.arange(G, device=dev)
        for i in range(0, G, batch_size):
            yield self.batch(perm[i:i + batch_size])
