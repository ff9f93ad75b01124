"""Raw data readers of the two file formats the reference's GNNML data sets come in, numpy only.

The reference loads them through scipy (``sio.loadmat``, libs/utils.py:195) and networkx (``nx.read_graph6``,
libs/utils.py:509) inside PyG ``InMemoryDataset.process`` bodies; neither PyG nor the dataset classes exist here
(SURVEY D7), so the product carries its own readers and the two ``process`` bodies the BASELINE configs use:

  read_mat      MATLAB Level-5 .mat: numeric / char / cell / struct / sparse arrays, compressed elements (zlib)
  read_graph6   graph6 text (one graph per line, optional >>graph6<< header)
  load_mutag    libs/utils.py:192-209  (A, F, y of dataset/mutag/raw/mutag.mat -> x, edge_index, y per graph)
  load_sr       libs/utils.py:506-513  (sr251256.g6 -> x = ones, undirected edge_index, y = 0)
  load_tu       libs/utils.py:24-174   (ptc.mat / enzymes.mat / proteins.mat -> x, edge_index, integer class label)
  load_graph8c  libs/utils.py:453-487  (graph8c.g6 -> x = ones, undirected edge_index, y = 0)
  load_exp      libs/utils.py:424-451  (EXP's GRAPHSAT.pkl as converted by tools/convert_exp.py -> x, edge_index, y)
  load_twodgrid libs/utils.py:333-355  (TwoDGrid30.mat -> train / test / val records of ONE grid: x, per-node y [n, 3], mask)
  load_bandclass libs/utils.py:289-305 (bandclass.mat -> x [n, 1], edge_index, 0 / 1 label per graph; freqclass.py)

Each returns graphs as (x [n, f] float32, edge_index [2, e] int64 in row-major ``np.where`` order, y), the input format
of ``SpectralDesign.design_many`` / ``graph.collate``.
"""
import struct
import zlib

import numpy as np

_MI = {1: ('b', 1), 2: ('B', 1), 3: ('h', 2), 4: ('H', 2), 5: ('i', 4), 6: ('I', 4), 7: ('f', 4), 9: ('d', 8),
       12: ('q', 8), 13: ('Q', 8), 16: ('B', 1), 17: ('H', 2), 18: ('I', 4)}
_MI_MATRIX, _MI_COMPRESSED = 14, 15
_MX_CELL, _MX_STRUCT, _MX_OBJECT, _MX_CHAR, _MX_SPARSE = 1, 2, 3, 4, 5


class _Reader(object):
    def __init__(self, buf, order):
        self.b, self.o, self.p = buf, order, 0

    def tag(self):
        """(type, nbytes, data offset, offset of the next element); handles the small-element form"""
        t, = struct.unpack_from(self.o + 'I', self.b, self.p)
        if t >> 16:                                           # small data element: 2-byte size, 2-byte type, 4 data bytes
            return t & 0xffff, t >> 16, self.p + 4, self.p + 8
        n, = struct.unpack_from(self.o + 'I', self.b, self.p + 4)
        return t, n, self.p + 8, self.p + 8 + ((n + 7) // 8) * 8 if t != _MI_COMPRESSED else self.p + 8 + n

    def numeric(self):
        t, n, d, nxt = self.tag()
        self.p = nxt
        code, size = _MI[t]
        return np.frombuffer(self.b, dtype=np.dtype(code).newbyteorder(self.o), count=n // size, offset=d)

    def element(self):
        """next top-level or nested element -> (name, value)"""
        t, n, d, nxt = self.tag()
        if t == _MI_COMPRESSED:
            sub = _Reader(zlib.decompress(self.b[d:d + n]), self.o)
            self.p = nxt
            return sub.element()
        if t != _MI_MATRIX:
            self.p = nxt
            return None, None
        end = nxt
        if n == 0:                                            # empty matrix placeholder
            self.p = end
            return '', np.zeros((0, 0))
        self.p = d
        flags = self.numeric()
        cls, is_complex = int(flags[0]) & 0xff, bool(int(flags[0]) & 0x800)
        dims = [int(v) for v in self.numeric()]
        name = self.numeric().tobytes().decode('latin1')
        if cls == _MX_CELL:
            out = np.empty(int(np.prod(dims)), dtype=object)
            for i in range(out.size):
                out[i] = self.element()[1]
            val = out.reshape(dims, order='F')
        elif cls in (_MX_STRUCT, _MX_OBJECT):
            if cls == _MX_OBJECT:
                self.numeric()
            flen = int(self.numeric()[0])
            raw = self.numeric().tobytes()
            fields = [raw[i:i + flen].split(b'\0', 1)[0].decode('latin1') for i in range(0, len(raw), flen)]
            cnt = int(np.prod(dims))
            recs = [{f: self.element()[1] for f in fields} for _ in range(cnt)]
            val = recs[0] if cnt == 1 else np.array(recs, dtype=object).reshape(dims, order='F')
        elif cls == _MX_SPARSE:
            ir, jc = self.numeric().astype(np.int64), self.numeric().astype(np.int64)
            re = self.numeric()
            val = np.zeros(dims, dtype=np.float64 if re.dtype.kind == 'f' else re.dtype)
            for c in range(dims[1]):
                val[ir[jc[c]:jc[c + 1]], c] = re[jc[c]:jc[c + 1]]
        else:
            re = self.numeric()
            if is_complex:
                re = re + 1j * self.numeric()
            if cls == _MX_CHAR:
                chars = ''.join(chr(int(c)) for c in re)
                val = chars if len(dims) == 2 and dims[0] <= 1 else np.array(list(chars)).reshape(dims, order='F')
            else:
                val = np.array(re).reshape(dims, order='F')   # MATLAB stores column-major
        self.p = end
        return name, val


def read_mat(path):
    """dict name -> array of a MATLAB 5.0 MAT-file (the subset above; what ``scipy.io.loadmat`` returns for it, with cell
    arrays as object arrays)."""
    buf = open(path, 'rb').read()
    if len(buf) < 128 or not buf.startswith(b'MATLAB 5.0 MAT-file'):
        raise ValueError('%s is not a Level-5 MAT-file' % path)
    order = '<' if buf[126:128] == b'IM' else '>'
    r = _Reader(buf, order)
    r.p = 128
    out = {}
    while r.p + 8 <= len(buf):
        name, val = r.element()
        if name is not None:
            out[name] = val
    return out


def read_graph6(path):
    """list of symmetric 0/1 adjacency matrices (uint8) of a graph6 file (n < 258048)"""
    graphs = []
    for line in open(path, 'rb').read().split(b'\n'):
        line = line.strip()
        if line.startswith(b'>>graph6<<'):
            line = line[10:]
        if not line:
            continue
        d = np.frombuffer(line, dtype=np.uint8).astype(np.int64) - 63
        if d.min() < 0 or d.max() > 63:
            raise ValueError('%s: not graph6 text' % path)
        if d[0] <= 62:
            n, d = int(d[0]), d[1:]
        elif d[1] <= 62:
            n, d = int((d[1] << 12) | (d[2] << 6) | d[3]), d[4:]
        else:
            raise ValueError('%s: graphs of this size are not supported' % path)
        bits = ((d[:, None] >> np.arange(5, -1, -1)) & 1).reshape(-1)          # 6 bits per character, high bit first
        iu = np.triu_indices(n, 1)
        order = np.lexsort((iu[0], iu[1]))                                     # bit k = x(i, j), columns first: (0,1),(0,2),(1,2),...
        A = np.zeros((n, n), dtype=np.uint8)
        A[iu[0][order], iu[1][order]] = bits[:order.size]
        graphs.append(A | A.T)
    return graphs


def _edges(A):
    r, c = np.where(A > 0)
    return np.vstack((r, c)).astype(np.int64)


def load_mutag(path):
    """libs/utils.py:192-209: graphs of mutag.mat as (x, edge_index, y), y = (label + 1) // 2"""
    a = read_mat(path)
    A, F = a['A'].reshape(-1), a['F'].reshape(-1)
    Y = ((a['y'].astype(np.int64) + 1) // 2).astype(np.float32).reshape(-1)
    return [(np.asarray(F[i], dtype=np.float32), _edges(A[i]), np.float32(Y[i])) for i in range(A.size)]


def load_sr(path):
    """libs/utils.py:506-513: x = ones [n, 1], symmetric edges, y = 0 (sr25.py, graph8c.py)"""
    return [(np.ones((A.shape[0], 1), dtype=np.float32), _edges(A), np.float32(0)) for A in read_graph6(path)]


def load_graph8c(path):
    """libs/utils.py:453-487 (Grapg8cDataset): the 11,117 connected graphs of 8 nodes of graph8c.g6, read as load_sr reads
    sr25 -- x = ones [8, 1], both directions of every edge, y = 0 (graph8c.py:16-18)"""
    return load_sr(path)


def load_exp(path):
    """libs/utils.py:424-451 (PlanarSATPairsDataset): the 1,200 graphs of EXP in file order -- graphs 2k and 2k + 1 form a pair
    (exp_iso.py:301) -- from the npz tools/convert_exp.py writes: (x float32 [n, 1], edge_index int64 [2, e] as stored, y int64)"""
    z = np.load(path, allow_pickle=False)
    x, ei, y, npt, ept = z['x'], z['edge_index'], z['y'], z['node_ptr'], z['edge_ptr']
    return [(np.asarray(x[npt[g]:npt[g + 1]], dtype=np.float32), np.asarray(ei[:, ept[g]:ept[g + 1]], dtype=np.int64), np.int64(y[g]))
            for g in range(y.size)]


def exp_classify_splits(graphs):
    """exp_classify.py:19-21: (val, test, train) = graphs [0, 200), [200, 400), [400, 1200) of the EXP list in file order -- raw
    graphs of load_exp or the designed ones, any sequence that slices.  Pairs stay whole: every bound is even."""
    if len(graphs) != 1200:
        raise ValueError('exp_classify_splits: EXP has 1,200 graphs, got %d' % len(graphs))
    return graphs[0:200], graphs[200:400], graphs[400:1200]


# feature columns the reference's TU dataset classes keep (contfeat=False): PtcDataset all of them, EnzymesDataset and
# ProteinsDataset F[i][:, 0:3] (libs/utils.py:51, 101, 151)
_TU_COLS = dict(ptc=None, enzymes=3, proteins=3)


def load_tu(path, name, contfeat=False):
    """libs/utils.py:24-174: graphs of ptc.mat / enzymes.mat / proteins.mat (name 'ptc' | 'enzymes' | 'proteins') as
    (x, edge_index, y): edges where A > 0, x = the kept feature columns as float32, y = the int64 class label from Y ([G, 1] in
    ptc.mat and proteins.mat, [1, G] in enzymes.mat).  contfeat=True keeps EVERY column of F for 'enzymes' and 'proteins'
    (libs/utils.py:105-107, 157-160: the continuous attributes behind the three label columns; enzymes_contfeat.py)."""
    if name not in _TU_COLS:
        raise ValueError("load_tu: name must be 'ptc', 'enzymes' or 'proteins', got %r" % (name,))
    a = read_mat(path)
    A, F = a['A'].reshape(-1), a['F'].reshape(-1)
    Y = np.asarray(a['Y']).astype(np.int64).reshape(-1)
    if Y.size != A.size:
        raise ValueError('%s: %d labels for %d graphs' % (path, Y.size, A.size))
    k = None if contfeat else _TU_COLS[name]
    return [(np.asarray(F[i] if k is None else F[i][:, 0:k], dtype=np.float32), _edges(A[i]), np.int64(Y[i])) for i in range(A.size)]


def standardize_tu(graphs, train_idx, ddof=1):
    """enzymes_contfeat.py:366-370: x <- (x - mean) / std of EVERY graph, mean and std (unbiased, as torch.std) per column over
    the nodes of the training graphs `train_idx`.  ddof=0: the population std, np.std as normalize_wrt_train of
    enzymes_contfeats_gnnml3_tf.py:119-129 takes it.  graphs: the tuples of load_tu or the records of SpectralDesign.design_many
    (the script standardises after the degree column is appended).  Returns (graphs, (mean, std)): new tuples / records with
    float32 x, the statistics as float64 arrays."""
    xs = lambda g: np.asarray(g['x'] if isinstance(g, dict) else g[0])
    tr = np.concatenate([xs(graphs[int(i)]) for i in train_idx], 0).astype(np.float64)
    if tr.shape[0] < 1 + ddof:
        raise ValueError('standardize_tu: the training graphs have %d nodes; the %s std needs %d' %
                         (tr.shape[0], 'unbiased' if ddof else 'population', 1 + ddof))
    mean, std = tr.mean(0), tr.std(0, ddof=ddof)
    out = []
    for g in graphs:
        x = ((xs(g).astype(np.float64) - mean) / std).astype(np.float32)
        out.append(dict(g, x=x) if isinstance(g, dict) else (x,) + tuple(g[1:]))
    return out, (mean, std)


def load_twodgrid(path):
    """libs/utils.py:333-355 (TwoDGrid30): the three records of TwoDGrid30.mat in the order train, test, val (filtering.py:20-22), as
    dicts for ``SpectralDesign.design_many`` / ``graph.collate(node_fields=('y', 'mask'))``.  All three share ONE edge_index
    (np.where(A > 0)) and ONE mask array; x = F[:, 0:1] | F[:, 4:5] | F[:, 8:9], y = F[:, 1:4] | F[:, 5:8] | F[:, 9:12] (band-,
    low-, high-pass response per node), mask = F[:, 12:13] (1 = the node counts in the loss and in R^2).  Everything float32."""
    a = read_mat(path)
    F = np.asarray(a['F']).astype(np.float32)
    if F.ndim != 2 or F.shape[1] < 13:
        raise ValueError('%s: F must be [n, >= 13], got %s' % (path, F.shape))
    ei = _edges(np.asarray(a['A']))
    mask = np.ascontiguousarray(F[:, 12:13])
    return [dict(x=np.ascontiguousarray(F[:, c:c + 1]), edge_index=ei, y=np.ascontiguousarray(F[:, c + 1:c + 4]), mask=mask)
            for c in (0, 4, 8)]


def load_bandclass(path):
    """libs/utils.py:289-305 (BandClassDataset): the graphs of bandclass.mat -- A [G, n, n] adjacencies, F [G, n] one signal per
    node, Y [G, 1] the 0 / 1 label -- as (x float32 [n, 1], edge_index where A > 0, y float32), the records freqclass.py trains
    on (its sum BCE takes data.y as a float)."""
    a = read_mat(path)
    A, F, Y = np.asarray(a['A']), np.asarray(a['F']), np.asarray(a['Y'])
    if A.ndim != 3 or A.shape[1] != A.shape[2] or F.shape != A.shape[:2] or Y.reshape(-1).size != A.shape[0]:
        raise ValueError('%s: expected A [G, n, n], F [G, n], Y [G, 1], got %s, %s, %s' % (path, A.shape, F.shape, Y.shape))
    Y = Y.reshape(-1)
    return [(np.ascontiguousarray(F[i].astype(np.float32).reshape(-1, 1)), _edges(A[i]), np.float32(Y[i])) for i in range(A.shape[0])]


def design_twodgrid(records, design):
    """records of load_twodgrid + a SpectralDesign -> the three designed records (dicts with edge_index2 / edge_attr2 / lmax added).
    The three share one graph, so the eigen-decomposition runs once and they share the support arrays too."""
    d = design.design_many([(records[0]['x'], records[0]['edge_index'], 0)])[0]
    return [dict(d, x=np.asarray(r['x'], dtype=np.float32), y=r['y'], mask=r['mask']) for r in records]
