"""Convert the EXP data set (Abboud et al., IJCAI'21: 600 pairs of 1-WL-equivalent, non-isomorphic planar graphs) from the
reference's ``dataset/EXP/raw/GRAPHSAT.pkl`` into ``tests/golden/raw/exp.npz``, the file ``readers.load_exp`` reads.

The pickle is a list of ``torch_geometric.data.Data`` objects.  It is read with a restricted unpickler: the Data class maps to
a plain stub that keeps its attribute dict, and the only other globals allowed are the tensor rebuilds and OrderedDict.  The
tensor storages themselves are nested torch.save blobs and load with ``torch.load(weights_only=True)``.

    python tools/convert_exp.py /path/to/GRAPHSAT.pkl [tests/golden/raw/exp.npz]

The npz holds the graphs in file order (libs/utils.py:424-451 keeps it):
    x          float32 [sum n, 1]    node features as stored
    edge_index int64   [2, sum e]    per graph, local node ids, in stored order
    y          int64   [G]           the pair label
    node_ptr   int64   [G + 1]       graph g's nodes are x[node_ptr[g]:node_ptr[g + 1]]
    edge_ptr   int64   [G + 1]       graph g's edges are edge_index[:, edge_ptr[g]:edge_ptr[g + 1]]
"""
import collections
import io
import os
import pickle
import sys

import numpy as np
import torch


class _Data(object):
    """stand-in for torch_geometric.data.Data: the pickled state is its attribute dict"""

    def __setstate__(self, state):
        self.__dict__.update(state)


def _load_from_bytes(b):
    return torch.load(io.BytesIO(b), weights_only=True)


_ALLOWED = {
    ('torch_geometric.data.data', 'Data'): _Data,
    ('torch.storage', '_load_from_bytes'): _load_from_bytes,
    ('torch._utils', '_rebuild_tensor_v2'): torch._utils._rebuild_tensor_v2,
    ('collections', 'OrderedDict'): collections.OrderedDict,
}


class _Unpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if (module, name) not in _ALLOWED:
            raise pickle.UnpicklingError('global %s.%s is not allowed' % (module, name))
        return _ALLOWED[(module, name)]


def read_pkl(path):
    """[(x float32 [n, 1], edge_index int64 [2, e], y int64)] of GRAPHSAT.pkl, in file order"""
    with open(path, 'rb') as f:
        data = _Unpickler(f).load()
    out = []
    for d in data:
        a = d.__dict__
        a = a.get('_store', a)          # newer PyG keeps the attributes in a storage dict
        x = np.asarray(a['x'].numpy(), dtype=np.float32).reshape(-1, 1)
        ei = np.asarray(a['edge_index'].numpy(), dtype=np.int64)
        y = int(np.asarray(a['y'].numpy()).reshape(-1)[0])
        out.append((x, ei, y))
    return out


def main(src, dst):
    graphs = read_pkl(src)
    node_ptr = np.concatenate([[0], np.cumsum([g[0].shape[0] for g in graphs])]).astype(np.int64)
    edge_ptr = np.concatenate([[0], np.cumsum([g[1].shape[1] for g in graphs])]).astype(np.int64)
    np.savez_compressed(dst, x=np.concatenate([g[0] for g in graphs]), edge_index=np.concatenate([g[1] for g in graphs], 1),
                        y=np.array([g[2] for g in graphs], dtype=np.int64), node_ptr=node_ptr, edge_ptr=edge_ptr)
    print('%s: %d graphs, %d nodes, %d edges -> %s (%d bytes)' % (src, len(graphs), node_ptr[-1], edge_ptr[-1], dst,
                                                                  os.path.getsize(dst)))


if __name__ == '__main__':
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, 'tests', 'golden', 'raw', 'exp.npz'))
