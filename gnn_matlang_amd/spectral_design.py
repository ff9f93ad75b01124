"""Support precompute (Alg.1) -- drop-in for ``libs.utils.SpectralDesign``
(/root/reference/libs/utils.py:525-626), host side.

The reference processes one graph per call in a Python loop (one LAPACK eigh + nfreq dense
products each).  Here graphs are grouped by node count and every step runs on a stacked
[G, n, n] array (one batched LAPACK/BLAS call per group), which is what makes building the
10^4-10^5-graph synthetic workloads practical; the arithmetic and its dtype walk are kept
identical to the reference so results agree to the last bits LAPACK gives:
  A, SP float32;  d, 1/sqrt(d), (A D)^T D float32;  nL, eigh(nL), Gaussian filters float64;
  eigh(A) float32 when laplacien=False;  M = (A+I) squared recfield-1 times (:566-573, i.e. a
  2^(recfield-1)-hop mask);  COO emitted in row-major order (:608-610).
The PPGN baseline tensors (X2, M; :613-624) are built on the device by ``ppgn.ppgn_inputs`` for a whole batch, not here:
``nmax`` is accepted and unused.
The GPU port of this step is the first "next" row.
"""
import numpy as np
import torch


class SpectralDesign(object):
    def __init__(self, nmax=0, recfield=1, dv=5, nfreq=5, adddegree=False, laplacien=True, addadj=False, vmax=None):
        self.recfield = recfield      # 0: adj, 1: adj+I, r: (adj+I)^(2^(r-1)) > 0
        self.dv = dv                  # Gaussian bandwidth
        self.nfreq = nfreq            # number of band-pass supports
        self.adddegree = adddegree    # append degree to the node features
        self.laplacien = laplacien    # spectrum of the normalized Laplacian (else of A)
        self.addadj = addadj          # extra support = A
        self.vmax = vmax              # fixed upper end of the frequency grid
        self.nmax = nmax              # PPGN only: ignored

    @property
    def nsup(self):
        return self.nfreq + 1 + (1 if self.addadj else 0)

    # ------------------------------------------------------------------ batched core
    def _design_group(self, A):
        """A [G,n,n] float32 adjacency stack -> (M bool [G,n,n], SP float32 [G,S,n,n], lmax float32 [G])."""
        G, n, _ = A.shape
        eye = np.eye(n)
        if self.recfield == 0:
            M = A
        else:
            M = A + eye
            for _ in range(1, self.recfield):
                M = np.matmul(M, M)
        M = M > 0

        d = A.sum(axis=1)                                            # column sums, float32
        with np.errstate(divide='ignore', invalid='ignore'):
            dis = 1 / np.sqrt(d)
        dis[np.isinf(dis)] = 0
        dis[np.isnan(dis)] = 0
        t1 = A * dis[:, None, :]                                     # A.dot(D), float32
        t2 = t1.transpose(0, 2, 1) * dis[:, None, :]                 # (A D)^T.dot(D), float32
        nL = eye - t2                                                # float64
        V, U = np.linalg.eigh(nL)
        V[V < 0] = 0
        lmax = V.max(axis=1).astype(np.float32)
        if not self.laplacien:
            V, U = np.linalg.eigh(A)                                 # float32, like the reference
        top = V.max(axis=1) if self.vmax is None else np.full(G, self.vmax)
        centers = np.linspace(V.min(axis=1), top, self.nfreq, axis=0)    # [nfreq, G]
        SP = np.zeros((G, self.nsup, n, n), dtype=np.float32)
        Ut = np.ascontiguousarray(U.transpose(0, 2, 1))
        for i in range(self.nfreq):
            wgt = np.exp(-(self.dv * (V - centers[i][:, None]) ** 2))    # float64 [G,n]
            SP[:, i] = M * np.matmul(U, wgt[:, :, None] * Ut)
        SP[:, self.nfreq] = eye
        if self.addadj:
            SP[:, self.nfreq + 1] = A
        return M, SP, lmax

    def design_many(self, graphs):
        """graphs: list of (x [n,f], edge_index [2,e], y) -> list of dicts with the reference's fields
        x, edge_index, edge_index2 [2,m] int64, edge_attr2 [m,S] float32, lmax, y (numpy)."""
        out = [None] * len(graphs)
        by_n = {}
        for i, g in enumerate(graphs):
            by_n.setdefault(int(np.asarray(g[0]).shape[0]), []).append(i)
        for n, ids in by_n.items():
            A = np.zeros((len(ids), n, n), dtype=np.float32)
            for k, i in enumerate(ids):
                ei = np.asarray(graphs[i][1])
                A[k, ei[0], ei[1]] = 1
            M, SP, lmax = self._design_group(A)
            gi, r, c = np.nonzero(M)                                 # row-major inside each graph
            cut = np.searchsorted(gi, np.arange(len(ids) + 1))
            for k, i in enumerate(ids):
                x = np.asarray(graphs[i][0], dtype=np.float32)
                if self.adddegree:
                    x = np.concatenate([x, A[k].sum(0)[:, None]], 1).astype(np.float32)
                rr, cc = r[cut[k]:cut[k + 1]], c[cut[k]:cut[k + 1]]
                out[i] = dict(x=x, edge_index=np.asarray(graphs[i][1], dtype=np.int64),
                              edge_index2=np.vstack((rr, cc)).astype(np.int64),
                              edge_attr2=np.ascontiguousarray(SP[k][:, rr, cc].T),
                              lmax=lmax[k], y=graphs[i][2] if len(graphs[i]) > 2 else 0)
        return out

    # ------------------------------------------------------------------ device path (whole batch, one launch pair)
    MAX_DEVICE_NODES = 80

    def design_device(self, x, edge_index, ptr):
        """Supports of a collated batch on the GPU (libgml_hip.so: gml_spectral_count / gml_spectral_design).
        x [N,f] float32, edge_index [2,e] int64 (global ids, each graph's edges contiguous, graphs in order),
        ptr [B+1] node offsets -- all CUDA tensors.  Returns dict(x, edge_index2 [2,m] int64, edge_attr2 [m,S] float32,
        lmax [B] float32); same values as the host path to float64 roundoff of the eigen-solver, same mask and order."""
        from . import _lib
        from .functional import _ptr, _stream
        dev = x.device
        if dev.type != 'cuda':
            raise RuntimeError('design_device needs CUDA tensors (the host path is design_many / __call__)')
        with torch.cuda.device(dev):
            ptr32 = ptr.to(device=dev, dtype=torch.int32).contiguous()
            B = int(ptr32.numel() - 1)
            ei = edge_index.to(device=dev, dtype=torch.int64).contiguous()
            e = int(ei.size(1))
            sizes = (ptr32[1:] - ptr32[:-1])
            nmax = int(sizes.max().item()) if B else 0
            if nmax > self.MAX_DEVICE_NODES or self.nfreq > 16:
                # graphs beyond the LDS-resident Jacobi kernel (proteins: up to 620 nodes, filtering.py: 900): those go through
                # the device's dense libraries graph by graph, the others through the kernels; merged in graph order
                return self._design_device_mixed(x, ei, ptr32, sizes)
            # edges per graph: graph id of each edge's source, counted
            gid = torch.bucketize(ei[0], ptr32[1:].to(torch.int64), right=True) if e else ei.new_zeros(0)
            eptr = torch.zeros(B + 1, dtype=torch.int32, device=dev)
            if e:
                eptr[1:] = torch.bincount(gid, minlength=B).cumsum(0).to(torch.int32)
            nnz = torch.empty(B, dtype=torch.int32, device=dev)
            st = _stream(dev)
            _lib.call('gml_spectral_count', _ptr(ptr32), _ptr(eptr), _ptr(ei), e, B, nmax, int(self.recfield), _ptr(nnz), st)
            out_ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
            out_ptr[1:] = nnz.to(torch.int64).cumsum(0)
            m = int(out_ptr[-1].item())
            S = self.nsup
            ei2 = torch.empty(2, m, dtype=torch.int64, device=dev)
            ea2 = torch.empty(m, S, dtype=torch.float32, device=dev)
            lmax = torch.empty(B, dtype=torch.float32, device=dev)
            _lib.call('gml_spectral_design', _ptr(ptr32), _ptr(eptr), _ptr(ei), e, B, nmax, int(self.recfield),
                      int(self.nfreq), float(self.dv), 0 if self.vmax is None else 1,
                      float(0.0 if self.vmax is None else self.vmax), 1 if self.laplacien else 0,
                      1 if self.addadj else 0, _ptr(out_ptr), m, _ptr(ei2), _ptr(ea2), _ptr(lmax), st)
            xo = x
            if self.adddegree:
                deg = torch.zeros(x.size(0), dtype=torch.float32, device=dev)
                if e:                                               # column sums of the 0/1 adjacency (duplicate edges count once)
                    key = torch.unique(ei[0] * x.size(0) + ei[1])
                    deg.index_add_(0, key % x.size(0), torch.ones_like(key, dtype=torch.float32))
                xo = torch.cat([x.float(), deg[:, None]], 1)
        return dict(x=xo, edge_index2=ei2, edge_attr2=ea2, lmax=lmax)

    def _design_large(self, n, src, dst, dev):
        """one graph of n nodes on the device with library calls (float64 eigh = rocSOLVER, GEMMs): the arithmetic of
        _design_group / libs/utils.py:546-610.  src, dst: local node ids.  Returns (rows, cols) of the mask in row-major
        order, the [m, S] supports and lmax."""
        A = torch.zeros(n, n, dtype=torch.float32, device=dev)
        if src.numel():
            A[src, dst] = 1
        eye = torch.eye(n, dtype=torch.float64, device=dev)
        if self.recfield == 0:
            M = A.double()
        else:
            M = A.double() + eye
            for _ in range(1, self.recfield):
                M = (M @ M > 0).double()                               # (the count itself is never used: only > 0; keeps it finite)
        M = M > 0
        d = A.sum(0)                                                   # column sums, float32
        dis = torch.where(d > 0, 1 / torch.sqrt(d), torch.zeros_like(d))
        t1 = A * dis[None, :]
        t2 = t1.t() * dis[None, :]
        nL = eye - t2.double()
        V, U = torch.linalg.eigh(nL)
        V = V.clamp(min=0)
        lmax = V.max().float()
        if not self.laplacien:
            V, U = torch.linalg.eigh(A.double())                       # (float64 like the device kernels; the reference: float32)
        top = V.max() if self.vmax is None else torch.tensor(float(self.vmax), dtype=torch.float64, device=dev)
        lo = V.min()
        r, c = M.nonzero(as_tuple=True)                                # row-major
        SP = torch.empty(r.numel(), self.nsup, dtype=torch.float32, device=dev)
        for i in range(self.nfreq):
            ctr = lo + (top - lo) * (i / (self.nfreq - 1)) if self.nfreq > 1 else lo
            wgt = torch.exp(-(self.dv * (V - ctr) ** 2))
            SP[:, i] = ((U * wgt[None, :]) @ U.t())[r, c].float()
        SP[:, self.nfreq] = (r == c).float()
        if self.addadj:
            SP[:, self.nfreq + 1] = A[r, c]
        return r, c, SP, lmax

    def _design_device_mixed(self, x, ei, ptr32, sizes):
        dev = x.device
        B = int(sizes.numel())
        ptr = ptr32.to(torch.int64)
        N = int(ptr[-1].item())
        small = (sizes <= self.MAX_DEVICE_NODES) if self.nfreq <= 16 else torch.zeros_like(sizes, dtype=torch.bool)
        node_g = torch.repeat_interleave(torch.arange(B, device=dev), sizes.to(torch.int64))       # graph of every node
        edge_g = node_g[ei[0]] if ei.size(1) else ei.new_zeros(0)
        nnz = torch.zeros(B, dtype=torch.int64, device=dev)
        lmax = torch.zeros(B, dtype=torch.float32, device=dev)
        S = self.nsup
        parts = []                                                     # (graph ids of the entries, rank inside the graph, ei2 [2, m], ea2 [m, S])
        sm_ids = small.nonzero().flatten()
        if sm_ids.numel():
            keep = small[node_g]
            old = keep.nonzero().flatten()                             # compact node id -> original node id
            new = torch.cumsum(keep.to(torch.int64), 0) - 1            # original -> compact (valid where keep)
            ek = small[edge_g] if ei.size(1) else torch.zeros(0, dtype=torch.bool, device=dev)
            cptr = torch.zeros(sm_ids.numel() + 1, dtype=torch.int64, device=dev)
            cptr[1:] = sizes[sm_ids].to(torch.int64).cumsum(0)
            d = SpectralDesign(recfield=self.recfield, dv=self.dv, nfreq=self.nfreq, adddegree=False, laplacien=self.laplacien,
                               addadj=self.addadj, vmax=self.vmax).design_device(x[old], new[ei[:, ek]], cptr.to(torch.int32))
            cg = torch.bucketize(d['edge_index2'][0], cptr[1:], right=True)          # compact graph of every entry
            cnt = torch.bincount(cg, minlength=sm_ids.numel())
            nnz[sm_ids] = cnt
            lmax[sm_ids] = d['lmax']
            start = torch.cumsum(cnt, 0) - cnt
            parts.append((sm_ids[cg], torch.arange(cg.numel(), device=dev) - start[cg], old[d['edge_index2']], d['edge_attr2']))
        for b in (~small).nonzero().flatten().tolist():
            n, lo = int(sizes[b].item()), int(ptr[b].item())
            sel = (edge_g == b) if ei.size(1) else torch.zeros(0, dtype=torch.bool, device=dev)
            r, c, SP, lm = self._design_large(n, ei[0, sel] - lo, ei[1, sel] - lo, dev)
            nnz[b] = r.numel()
            lmax[b] = lm
            parts.append((torch.full((r.numel(),), b, dtype=torch.int64, device=dev), torch.arange(r.numel(), device=dev),
                          torch.stack([r + lo, c + lo]), SP))
        out_ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        out_ptr[1:] = nnz.cumsum(0)
        m = int(out_ptr[-1].item())
        ei2 = torch.empty(2, m, dtype=torch.int64, device=dev)
        ea2 = torch.empty(m, S, dtype=torch.float32, device=dev)
        for g, rank, e2, a2 in parts:
            pos = out_ptr[g] + rank
            ei2[:, pos] = e2
            ea2[pos] = a2
        xo = x
        if self.adddegree:
            deg = torch.zeros(N, dtype=torch.float32, device=dev)
            if ei.size(1):
                key = torch.unique(ei[0] * N + ei[1])
                deg.index_add_(0, key % N, torch.ones_like(key, dtype=torch.float32))
            xo = torch.cat([x.float(), deg[:, None]], 1)
        return dict(x=xo, edge_index2=ei2, edge_attr2=ea2, lmax=lmax)

    # ------------------------------------------------------------------ reference call convention
    def __call__(self, data):
        """``data``: any object with ``x`` [n,f] and ``edge_index`` [2,e] tensors (a PyG ``Data`` works).
        Sets x (float32, + degree), edge_index2, edge_attr2, lmax on it and returns it."""
        x = data.x.detach().cpu().numpy() if isinstance(data.x, torch.Tensor) else np.asarray(data.x)
        ei = data.edge_index.detach().cpu().numpy() if isinstance(data.edge_index, torch.Tensor) \
            else np.asarray(data.edge_index)
        d = self.design_many([(x, ei, 0)])[0]
        data.x = torch.from_numpy(d['x'])
        data.edge_index2 = torch.from_numpy(d['edge_index2'])
        data.edge_attr2 = torch.from_numpy(d['edge_attr2'])
        data.lmax = d['lmax']
        return data
