"""Static-shape batches that carry the raw adjacency (DeviceDataset.batch_padded(..., adjacency=True)) and the new bounds() keys,
on CPU tensors (torch ops only), on the real mutag graphs; the ctypes layout of gml_batch_edges_desc; the masked mutag loss and the
loud failures of models on padded batches they cannot take."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

BS = 16                                                    # mutag.py:320-351 trains at batch 16


@pytest.fixture(scope='module')
def mutag():
    from gnn_matlang_amd import SpectralDesign, readers
    from gnn_matlang_amd.dataset import DeviceDataset
    raw = readers.load_mutag(os.path.join(GOLDEN, 'raw', 'mutag.mat'))
    ds = SpectralDesign(recfield=1, dv=4, nfreq=3, adddegree=True).design_many(raw)
    dd = DeviceDataset.from_graphs(ds, torch.device('cpu'))
    dd.y = dd.y.float()
    return ds, dd


def _old_bounds(ds, batch_size):
    """bounds() as the package defined it before the raw-adjacency keys: recomputed here from the definitions, with numpy."""
    n = np.array([g['x'].shape[0] for g in ds])
    e = np.array([g['edge_index2'].shape[1] for g in ds])
    dmax = max(max(int(np.bincount(g['edge_index2'][0]).max()) for g in ds), 1)
    nmax, n_top, e_top = int(n.max()), int(np.sort(n)[::-1][:batch_size].sum()), int(np.sort(e)[::-1][:batch_size].sum())
    e2_pad = (e_top + 63) // 64 * 64
    deal = max(1, min(dmax, -(-int(e.sum()) // max(int(n.sum()), 1))))
    n_pad = (n_top + (e2_pad + deal - 1) // deal + 127) // 128 * 128
    return dict(n_pad=n_pad, e2_pad=e2_pad, dmax=dmax, deal=deal, caps=(128 * dmax, 128 + 2 * nmax))


def _group_caps(rowptr, col, rows):
    """(max edges, max column window) over groups of `rows` consecutive rows of one CSR view (gml_csr_group_info's ints 1 and 3)."""
    N = rowptr.numel() - 1
    me, mw = 0, 0
    for r0 in range(0, N, rows):
        kb, ke = int(rowptr[r0]), int(rowptr[min(r0 + rows, N)])
        me = max(me, ke - kb)
        if ke > kb:
            c = col[kb:ke]
            mw = max(mw, int(c.max() - c.min()) + 1)
    return me, mw


def _csr(key, other, N):
    order = torch.sort(key, stable=True)[1]
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.bincount(key, minlength=N), 0)]), other[order]


def test_old_bounds_keys_are_unchanged(mutag):
    ds, dd = mutag
    for bs in (1, 5, BS, 64):
        got = dd.bounds(bs)
        old = _old_bounds(ds, bs)
        assert {k: got[k] for k in old} == old, bs
        assert set(got) == set(old) | {'e_pad', 'e_deal', 'e_caps', 'caps64'}


def test_padded_batch_carries_the_raw_adjacency(mutag):
    ds, dd = mutag
    G = len(dd)
    bd = dd.bounds(BS)
    gen = torch.Generator().manual_seed(11)
    perm = torch.cat([torch.randperm(G, generator=gen), torch.full(((-G) % BS,), G, dtype=torch.int64)])
    batches = [perm[i:i + BS] for i in range(0, perm.numel(), BS)]
    batches += [torch.tensor([3, G, 3, 0, G, 187] + [G] * (BS - 6)), torch.full((BS,), G, dtype=torch.int64)]   # repeats, all absent
    for ids in batches:
        b = dd.batch_padded(ids, bd, adjacency=True)
        n_pad, e_pad = bd['n_pad'], bd['e_pad']
        ei = b.edge_index
        assert ei.dtype == torch.int64 and tuple(ei.shape) == (2, e_pad)
        ptr = b.ptr.long()
        n_real = int(ptr[BS])
        e_real = 0
        for s, gid in enumerate(ids.tolist()):
            if gid >= G:
                assert ptr[s + 1] == ptr[s]
                continue
            raw = torch.from_numpy(ds[gid]['edge_index'])
            k = raw.size(1)
            # each real graph's raw edges, in its own order, offset to its node range
            assert torch.equal(ei[:, e_real:e_real + k], raw + ptr[s]), (gid, s)
            e_real += k
        assert e_real <= e_pad
        pad = ei[:, e_real:]
        # every padding edge is a self loop on a padding node
        assert bool((pad[0] == pad[1]).all()) and bool((pad[0] >= n_real).all()) and bool((pad[0] < n_pad).all())
        # the padding edges are dealt at most e_deal per padding node
        if pad.size(1):
            assert int(torch.bincount(pad[0]).max()) <= bd['e_deal']
        # the new keys hold: no node beyond the degree the caps assume, every 128-row group of both views inside e_caps
        deg = torch.bincount(ei[0], minlength=n_pad).max().item(), torch.bincount(ei[1], minlength=n_pad).max().item()
        assert max(deg) * 128 <= bd['e_caps'][0]
        for key, other in ((ei[1], ei[0]), (ei[0], ei[1])):
            rp, col = _csr(key, other, n_pad)
            me, mw = _group_caps(rp, col, 128)
            assert me <= bd['e_caps'][0] and mw <= bd['e_caps'][1]
        # caps64 bounds the 64-row groups of the support view (the records batch_assembled(groups64=True) provides)
        e2 = b.edge_index2
        for key, other in ((e2[1], e2[0]), (e2[0], e2[1])):
            rp, col = _csr(key, other, n_pad)
            me, mw = _group_caps(rp, col, 64)
            assert me <= bd['caps64'][0] and mw <= bd['caps64'][1]
        # the rest of the batch is the batch without adjacency
        b0 = dd.batch_padded(ids, bd)
        assert not hasattr(b0, 'edge_index')
        for name in ('x', 'edge_index2', 'edge_attr2', 'batch', 'ptr', 'y', 'graph_valid'):
            assert torch.equal(getattr(b0, name), getattr(b, name)), name


def test_prepare_links_both_views_of_the_raw_adjacency():
    """DeviceDataset.adjacency_structure() (what prepare() records for the raw adjacency) on graphs whose edges are NOT sorted by
    source: tperm / sperm are the stable sorts, pos / tpos link them (what gml_batch_assemble_edges offsets per graph)."""
    from gnn_matlang_amd import SpectralDesign, synthetic
    from gnn_matlang_amd.dataset import DeviceDataset
    rng = np.random.default_rng(5)
    raw = []
    for x, ei, y in synthetic.make_graphs('zinc', 9, seed=4):
        raw.append((x, ei[:, rng.permutation(ei.shape[1])], np.float32(y)))
    dd = DeviceDataset.from_graphs(SpectralDesign(recfield=1, dv=4, nfreq=3).design_many(raw), torch.device('cpu'))
    dd.y = dd.y.float()
    P = dd.adjacency_structure()                                   # (prepare() keeps it; prepare() itself also splits on the device)
    assert not P['a_sorted']
    for g in range(len(dd)):
        e0, e1 = int(dd.edge_ptr[g]), int(dd.edge_ptr[g + 1])
        ei = dd.edge_index[:, e0:e1]
        tp, sp = P['a_tperm'][e0:e1].long(), P['a_sperm'][e0:e1].long()
        assert torch.equal(tp, torch.sort(ei[1], stable=True)[1]) and torch.equal(sp, torch.sort(ei[0], stable=True)[1])
        tinv = torch.empty_like(tp)
        tinv[tp] = torch.arange(tp.numel())
        assert torch.equal(P['a_pos'][e0:e1].long(), tinv[sp])
        assert torch.equal(P['a_tpos'][e0:e1].long()[P['a_pos'][e0:e1].long()], torch.arange(tp.numel()))
        n0, n1 = int(dd.node_ptr[g]), int(dd.node_ptr[g + 1])
        for key, rp in ((ei[0], P['a_rp_src']), (ei[1], P['a_rp_dst'])):
            cnt = torch.bincount(key, minlength=n1 - n0)
            assert torch.equal(rp[n0:n1].long(), torch.cumsum(cnt, 0) - cnt)


def test_batch_edges_descriptor_layout_matches_the_header(tmp_path):
    """gml_batch_edges_desc (include/gml.h) against _lib.BatchEdgesDesc: same size and field offsets as gcc gives the header."""
    import subprocess
    from gnn_matlang_amd import _lib
    fields = [f[0] for f in _lib.BatchEdgesDesc._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gml.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(gml_batch_edges_desc));\n' +
                   ''.join('  printf("%%zu\\n", offsetof(gml_batch_edges_desc, %s));\n' % f for f in fields) + '  return 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split()
    assert int(out[0]) == ctypes.sizeof(_lib.BatchEdgesDesc)
    for f, line in zip(fields, out[1:]):
        assert int(line) == getattr(_lib.BatchEdgesDesc, f).offset, f


def test_masked_mutag_loss_is_the_loss_of_the_real_graphs():
    from gnn_matlang_amd import models
    torch.manual_seed(0)
    pre, y = torch.randn(7, 1), (torch.rand(7) > 0.5).float()
    keep = [0, 2, 3, 5]
    valid = torch.zeros(6)
    valid[keep] = 1
    got = models.mutag_loss(pre, y, valid=valid)
    ref = models.mutag_loss(pre[keep], y[keep])
    assert torch.allclose(got, ref, rtol=1e-6, atol=0)
    assert torch.equal(models.mutag_loss(pre, y), torch.nn.functional.binary_cross_entropy(torch.sigmoid(pre)[:, 0], y, reduction='sum'))


def test_models_refuse_padded_batches_they_cannot_take(mutag):
    from gnn_matlang_amd import models
    ds, dd = mutag
    bd = dd.bounds(BS)
    b = dd.batch_padded(torch.arange(BS), bd)                      # no adjacency
    for m in (models.mutag_gnnml1(8), models.sr25_gnnml1(8)):
        with pytest.raises(ValueError, match='adjacency=True'):
            m(b)
    ba = dd.batch_padded(torch.arange(BS), bd, adjacency=True)
    with pytest.raises(NotImplementedError, match='bn_mlp'):
        models.mnist75_gnnml1(8)(ba)                                # graph-level BatchNorm over pooled rows
    with pytest.raises(NotImplementedError, match='readout'):
        models.mnist_gnnml3(8, 5)(b)                               # readout BatchNorm
