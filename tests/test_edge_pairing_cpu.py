"""The per-data-set mirror pairing of the support edges (dataset.pair_support_edges, what DeviceDataset.pairing() keeps for
batch_assembled(sym=True)) on CPU tensors, against a numpy brute force of the gml_edge_sym_flags semantics: hand-made graphs with
targets shuffled inside a source row, self loops, one-sided and repeated edges and pairs that differ by one ulp; and on designed
graphs."""
import numpy as np
import pytest
import torch

from gnn_matlang_amd.dataset import DeviceDataset, pair_support_edges


def brute(graphs):
    """graphs: [(edge_index [2, e] local ids, rows [e, S] float32)] -> flag, mirror (global positions), uid / mir lists per graph"""
    flags, mirrors, per = [], [], []
    base = 0
    for ei, rows in graphs:
        e = ei.shape[1]
        bits = rows.view(np.int32)
        f, m = np.ones(e, np.int32), -np.ones(e, np.int64)
        for k in range(e):
            s, d = ei[0, k], ei[1, k]
            own = np.nonzero((ei[0] == s) & (ei[1] == d))[0]
            rev = np.nonzero((ei[0] == d) & (ei[1] == s))[0]
            if s == d or own.size != 1 or rev.size != 1:
                continue
            a = rev[0]
            if not np.array_equal(bits[k], bits[a]):
                continue
            if s < d:
                f[k], m[k] = 2, base + a
            else:
                f[k] = 0
        sel = np.nonzero(f > 0)[0]
        per.append((sel.astype(np.int32), np.where(m[sel] >= 0, m[sel] - base, -1).astype(np.int32)))
        flags.append(f)
        mirrors.append(m)
        base += e
    return np.concatenate(flags), np.concatenate(mirrors), per


def run(graphs, nodes):
    ei = torch.from_numpy(np.concatenate([g[0] for g in graphs], 1).astype(np.int64))
    ea = torch.from_numpy(np.concatenate([g[1] for g in graphs]).astype(np.float32))
    eptr = torch.from_numpy(np.concatenate([[0], np.cumsum([g[0].shape[1] for g in graphs])]).astype(np.int64))
    nptr = torch.from_numpy(np.concatenate([[0], np.cumsum(nodes)]).astype(np.int64))
    return pair_support_edges(ei, eptr, nptr, ea)


def check(graphs, nodes):
    flag, mirror, sym_ptr, uid, mir = run(graphs, nodes)
    bf, bm, per = brute(graphs)
    assert np.array_equal(flag.numpy(), bf)
    assert np.array_equal(mirror.numpy(), bm)
    sp = sym_ptr.numpy()
    assert sp[0] == 0 and sp[-1] == uid.numel() == mir.numel() and uid.dtype == mir.dtype == torch.int32
    for g, (u, m) in enumerate(per):
        assert np.array_equal(uid.numpy()[sp[g]:sp[g + 1]], u), g
        assert np.array_equal(mir.numpy()[sp[g]:sp[g + 1]], m), g
    return flag


def test_targets_shuffled_inside_a_source_row():
    """(0,2),(0,1),(1,0),(2,0): row 0's targets descend -- a bisection inside the row would miss (1,0)'s mirror"""
    ei = np.array([[0, 0, 1, 2], [2, 1, 0, 0]])
    rows = np.tile(np.float32([[0.5, -1.25, 3.0, 0.0]]), (4, 1))
    flag = check([(ei, rows)], [3])
    assert flag.tolist() == [2, 2, 0, 0]


def test_self_loops_one_sided_repeated_and_one_ulp_pairs():
    rng = np.random.default_rng(3)
    S = 5
    r = rng.standard_normal((1, S)).astype(np.float32)
    ulp = r.copy()
    ulp[0, 2] = np.nextafter(ulp[0, 2], np.float32(np.inf))
    # graph A: a self loop, a one-sided edge (0 -> 3), an equal pair (1, 2), a pair one ulp apart (2, 3), a repeated edge (3 -> 1 twice)
    eiA = np.array([[0, 0, 1, 2, 2, 3, 3, 3, 1],
                    [0, 3, 2, 1, 3, 2, 1, 1, 3]])
    rowsA = np.concatenate([r, r, r, r, r, ulp, r, r, r])
    # graph B: every edge paired, targets shuffled in the rows
    eiB = np.array([[0, 0, 1, 1, 2, 2], [2, 1, 2, 0, 0, 1]])
    rowsB = rng.standard_normal((6, S)).astype(np.float32)
    # make each mirror pair bitwise equal: (0,1)<->(1,0), (0,2)<->(2,0), (1,2)<->(2,1)
    for k in range(6):
        s, d = eiB[0, k], eiB[1, k]
        a = int(np.nonzero((eiB[0] == d) & (eiB[1] == s))[0][0])
        if s < d:
            rowsB[a] = rowsB[k]
    # graph C: no edges
    eiC = np.zeros((2, 0), np.int64)
    rowsC = np.zeros((0, S), np.float32)
    flag = check([(eiA, rowsA), (eiC, rowsC), (eiB, rowsB)], [4, 2, 3])
    fa = flag[:9].tolist()
    assert fa[0] == 1                                      # self loop
    assert fa[1] == 1                                      # one-sided
    assert fa[2] == 2 and fa[3] == 0                       # equal pair
    assert fa[4] == 1 and fa[5] == 1                       # one ulp apart: evaluated alone, both
    assert fa[6] == fa[7] == fa[8] == 1                    # repeated (3, 1) and its reverse
    assert sorted(flag[9:].tolist()) == [0, 0, 0, 2, 2, 2]


def test_designed_graphs_match_the_brute_force():
    from gnn_matlang_amd import SpectralDesign, synthetic
    raw = synthetic.make_graphs('zinc', 12, seed=11)
    ds = SpectralDesign(recfield=2, dv=2, nfreq=7).design_many(raw)
    graphs = [(np.asarray(g['edge_index2'], np.int64), np.asarray(g['edge_attr2'], np.float32)) for g in ds]
    flag = check(graphs, [np.asarray(g['x']).shape[0] for g in ds])
    assert (flag == 0).sum() > 0                           # the supports do pair up


def test_pairing_is_kept_once_per_data_set_and_follows_the_unique_row_rule():
    from gnn_matlang_amd import SpectralDesign, synthetic
    raw = synthetic.make_graphs('zinc', 6, seed=2)
    ds = SpectralDesign(recfield=2, dv=2, nfreq=7).design_many(raw)
    dd = DeviceDataset.from_graphs(ds, torch.device('cpu'))
    dd.y = dd.y.float()
    p = dd.pairing()
    assert p is not None and dd.pairing() is p
    assert p['uid'].numel() <= 0.9 * dd.edge_index2.size(1)
    # asymmetric supports: nothing pairs, so the data set carries no pairing (batches behave as without sym)
    dd2 = DeviceDataset.from_graphs(ds, torch.device('cpu'))
    dd2.y = dd2.y.float()
    dd2.edge_attr2 = torch.randn_like(dd2.edge_attr2)
    assert dd2.pairing() is None


def test_batch_any_descriptor_layout():
    """gml_batch_any_desc: the gml_batch_desc first, then the mode words and pointers (include/gml.h)"""
    import ctypes
    from gnn_matlang_amd import _lib
    d = _lib.BatchAnyDesc
    assert d.b.offset == 0 and d.exact.offset == ctypes.sizeof(_lib.BatchDesc)
    assert d.sym_ptr.offset % 8 == 0 and d.ws_bytes.offset == d.ws.offset + 8
    for name in ('gml_batch_any_workspace_bytes', 'gml_batch_scan', 'gml_batch_assemble_any', 'gml_edge_mlp_fwd_stack6_sym_dev',
                 'gml_edge_mlp_bwd_sym_dev'):
        assert name in _lib.SIGNATURES
