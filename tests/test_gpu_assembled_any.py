"""Batch assembly for any batch size (gml_batch_assemble_any), padded and exact, with the data set's mirror pairing offset to the batch
(batch_assembled(sym=True)), and the edge-branch kernels that read the unique-row count on the device (gml_edge_mlp_*_sym_dev)."""
import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def base(dev):
    """512 designed ZINC-like graphs (the bench's supports: recfield 2, dv 2, nfreq 7)"""
    from gnn_matlang_amd import SpectralDesign, synthetic
    from gnn_matlang_amd.dataset import DeviceDataset
    raw = synthetic.make_graphs('zinc', 512, seed=77)
    dd = DeviceDataset.from_graphs(SpectralDesign(recfield=2, dv=2, nfreq=7).design_many(raw), dev)
    dd.y = dd.y.float()
    return dd


@pytest.fixture(scope='module')
def big(base):
    """10,240 graphs: the 512 tiled 20 times"""
    dd = base.tiled(20)
    dd.prepare()
    return dd


def _ids(G, B, dev, absent=True, seed=0):
    """B distinct graph ids in shuffled order, with a few repeated ids and (absent=True) absent slots (id G)"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randperm(G, generator=g)[:B]
    if B >= 4:
        ids[1] = ids[0]
        ids[B // 2] = ids[3]
        if absent:
            ids[2] = G
            ids[-1] = G
    return ids.to(dev).contiguous()


VIEWS = ('rowptr', 'col', 'perm', 'rowptr_t', 'col_t', 'perm_t', 'pos_t', 'tpos', 'ginfo128', 'ginfo_t128')


def _same_csr(a, b, what):
    assert (a.N, a.E) == (b.N, b.E), what
    for nm in VIEWS:
        assert torch.equal(getattr(a, nm), getattr(b, nm)), '%s: %s' % (what, nm)


@pytest.mark.parametrize('B', [8, 4096, 5000])
def test_padded_any_batch_is_bit_identical_to_batch_padded(dev, big, B):
    """batch_assembled(ids, bounds) for any B (and sym=True, which always takes the any-B launch) against batch_padded + the CSR build:
    every batch tensor, both views, the group records; up to 4096 graphs also against the single-launch gml_batch_assemble."""
    G = len(big)
    bd = big.bounds(B)
    ids = _ids(G, B, dev)
    bp = big.batch_padded(ids, bd)
    cp = bp.csr('edge_index2')
    outs = [big.batch_assembled(ids, bd, sym=True)]
    if B > 4096:
        outs.append(big.batch_assembled(ids, bd))
    else:
        outs.append(big.batch_assembled(ids, bd, sym=False))            # the single-launch kernel
    for k, ba in enumerate(outs):
        for nm in ('x', 'edge_attr2', 'y', 'graph_valid', 'ptr'):
            assert torch.equal(getattr(bp, nm).float() if nm != 'ptr' else bp.ptr, getattr(ba, nm)), (k, nm)
        assert torch.equal(bp.batch.int(), ba.batch), k
        ca = ba.csr('edge_index2')
        _same_csr(ca, cp, 'assembled %d' % k)
        assert ca.static_shape and ca.gmax128 == tuple(bd['caps']) and ca.gmax128[0] >= cp.gmax128[0] and ca.gmax128[1] >= cp.gmax128[1]
        ca.check()
    assert outs[0].csr('edge_index2')._sym_dev is not None and outs[1].csr('edge_index2')._sym_dev is None


@pytest.mark.parametrize('B', [8, 5000])
def test_exact_batch_is_bit_identical_to_batch_and_from_edge_index(dev, big, B):
    """bounds=None: no padding at all -- the batch of batch(ids) and GraphCSR.from_edge_index on it, bit for bit (maxima included)"""
    from gnn_matlang_amd.graph import GraphCSR
    G = len(big)
    ids = _ids(G, B, dev, absent=False, seed=1)
    b = big.batch(ids)
    c = GraphCSR.from_edge_index(b.edge_index2, int(b.x.size(0)))
    for sym in (False, True):
        be = big.batch_assembled(ids, None, sym=sym)
        for nm in ('x', 'edge_attr2', 'y', 'ptr'):
            assert torch.equal(getattr(b, nm), getattr(be, nm)), (sym, nm)
        assert torch.equal(b.batch.int(), be.batch) and be.num_graphs == B
        ce = be.csr('edge_index2')
        _same_csr(ce, c, 'exact sym=%s' % sym)
        assert (ce.gmax128, ce.gmax_t128) == (c.gmax128, c.gmax_t128) and not ce.static_shape
    if B <= 4096:                                          # the same graphs through the single launch, padded: the real part agrees
        bd = big.bounds(B)
        bo = big.batch_assembled(ids, bd)
        n, e = int(b.x.size(0)), int(b.edge_attr2.size(0))
        assert torch.equal(bo.x[:n], be.x) and torch.equal(bo.edge_attr2[:e], be.edge_attr2)
        co = bo.csr('edge_index2')
        assert torch.equal(co.col_t[:e], ce.col_t) and torch.equal(co.pos_t[:e], ce.pos_t) and torch.equal(co.rowptr[:n], ce.rowptr[:n])


def test_overflow_is_flagged_and_keeps_the_leading_graphs(dev, big):
    """bounds of 2 graphs, 8 large graphs asked for: check() raises, nothing is written out of place -- the batch is batch_padded of
    the leading graphs that fit, the others absent"""
    G = len(big)
    n = big.node_ptr[1:] - big.node_ptr[:-1]
    ids = torch.sort(n, descending=True)[1][:8].contiguous()
    bd = big.bounds(2)
    ba = big.batch_assembled(ids, bd, sym=True)                       # (sym / B > 4096: the any-B launch, which flags)
    with pytest.raises(ValueError, match='exceeds the bounds'):
        ba.csr('edge_index2').check()
    kept = int(ba.graph_valid.sum().item())
    assert 1 <= kept < 8 and torch.equal(ba.graph_valid[:kept], torch.ones(kept, device=dev))
    ids2 = ids.clone()
    ids2[kept:] = G
    bp = big.batch_padded(ids2, bd)
    for nm in ('x', 'edge_attr2', 'y', 'graph_valid', 'ptr'):
        assert torch.equal(getattr(bp, nm).float() if nm != 'ptr' else bp.ptr, getattr(ba, nm)), nm
    _same_csr(ba.csr('edge_index2'), bp.csr('edge_index2'), 'overflow')
    big.batch_assembled(ids2, bd, sym=True).csr('edge_index2').check()  # the same batch without the excess passes


def _flags_list(b):
    """gml_edge_sym_flags on the batch's source view + compaction (no 0.9 rule): (uid, mir)"""
    from gnn_matlang_amd import _lib
    from gnn_matlang_amd.graph import _ptr, _stream
    c = b.csr('edge_index2')
    v = b.edge_attr2.contiguous()
    flag = torch.empty(c.E, dtype=torch.int32, device=v.device)
    mirror = torch.empty(c.E, dtype=torch.int32, device=v.device)
    _lib.call('gml_edge_sym_flags', _ptr(c.rowptr_t), _ptr(c.col_t), _ptr(v), c.N, c.E, int(v.size(1)), _ptr(flag), _ptr(mirror),
              _stream(v.device))
    idx = torch.nonzero(flag, as_tuple=False).view(-1)
    return idx.int(), mirror[idx]


@pytest.mark.parametrize('mode', ['padded8', 'padded5000', 'exact5000'])
def test_pairing_list_equals_sym_flags_and_compaction(dev, big, mode):
    B = int(mode[-4:]) if mode.endswith('5000') else 8
    ids = _ids(len(big), B, dev, absent=mode.startswith('padded'), seed=2)
    b = big.batch_assembled(ids, None if mode.startswith('exact') else big.bounds(B), sym=True)
    c = b.csr('edge_index2')
    uid, mir, count = c.sym_index(b.edge_attr2)
    assert uid.numel() == mir.numel() == c.E and count.numel() == 1
    U = int(count.item())
    ruid, rmir = _flags_list(b)
    assert U == ruid.numel()
    assert torch.equal(uid[:U], ruid) and torch.equal(mir[:U], rmir)
    assert int((rmir >= 0).sum()) > 0                     # the supports do pair up


@pytest.mark.parametrize('S', [8, 12])
def test_device_count_kernels_equal_the_host_count_kernels(dev, big, S):
    """gml_edge_mlp_fwd_stack6_sym_dev / gml_edge_mlp_bwd_sym_dev (count on the device, capacity E) against the host-count kernels on
    the same list: forward outputs bitwise equal, weight gradients to fp32 summation order"""
    from gnn_matlang_amd import functional as Fn
    b = big.batch_assembled(_ids(len(big), 600, dev, seed=3), big.bounds(600), sym=True)
    uid, mir, count = b.csr('edge_index2').sym_index(b.edge_attr2)
    U = int(count.item())
    E = int(uid.numel())
    torch.manual_seed(5)
    vals = torch.randn(E, S, device=dev)
    u, m = uid[:U].long(), mir[:U].long()
    has = m >= 0
    vals[m[has]] = vals[u[has]]                            # the list's pairs carry the same row (as the list promises)
    layers = 2 if S == 8 else 1
    ws = [tuple(torch.randn(*shp, device=dev) * 0.4 for shp in ((2 * S, S), (2 * S, S), (2 * S, S), (S, 4 * S))) for _ in range(layers)]
    host = Fn.edge_mlp_fwd_stack(vals, None, ws, (uid[:U].contiguous(), mir[:U].contiguous()))
    devc = Fn.edge_mlp_fwd_stack(vals, None, ws, (uid, mir, count))
    assert host is not None and devc is not None
    for l in range(layers):
        assert torch.equal(host[l], devc[l]), l
    gout = torch.randn_like(vals)
    split = Fn.edge_presplit(vals)
    w1, w2, w3, w4 = ws[0]
    ref = Fn.edge_mlp_bwd(vals, w1, w2, w3, w4, gout, False, split, (uid[:U].contiguous(), mir[:U].contiguous()))
    got = Fn.edge_mlp_bwd(vals, w1, w2, w3, w4, gout, False, split, (uid, mir, count))
    for name, a, r in zip(('dw1', 'dw2', 'dw3', 'dw4'), got[1:], ref[1:]):
        e = rel_err(a.cpu().numpy(), r.cpu().numpy())
        assert e <= 1e-5, (name, e)
    with Fn.deferred_folds(list(ws[0])):                   # the partial rows of the capacity-sized grid, folded later
        got2 = Fn.edge_mlp_bwd(vals, w1, w2, w3, w4, gout, False, split, (uid, mir, count))
    for name, a, r in zip(('dw1', 'dw2', 'dw3', 'dw4'), got2[1:], got[1:]):
        assert rel_err(a.cpu().numpy(), r.cpu().numpy()) <= 1e-6, name
    zero = torch.zeros(1, dtype=torch.int32, device=dev)   # an empty list: nothing evaluated, zero gradients
    got0 = Fn.edge_mlp_bwd(vals, w1, w2, w3, w4, gout, False, split, (uid, mir, zero))
    assert all(float(t.abs().max()) == 0.0 for t in got0[1:])


def _count_calls(monkeypatch, name):
    from gnn_matlang_amd import _lib
    L = _lib.lib()
    fn = getattr(L, name)
    n = [0]

    def wrap(*a):
        n[0] += 1
        return fn(*a)
    monkeypatch.setattr(L, name, wrap)
    return n


@pytest.mark.parametrize('exact', [False, True])
def test_model_step_on_a_sym_batch_equals_the_plain_batch(dev, big, exact, monkeypatch):
    """ZINC GNNML3 forward + backward on batch_assembled(sym=True) vs the same batch with sym=False: logits and loss bitwise equal
    (the forward is exact per row), parameter gradients within 1e-5 of their scale (the summation order of the edge branch's weight
    gradients changes); the device-count kernels are the ones that ran"""
    from gnn_matlang_amd import functional as Fn, models
    B = 3000
    ids = _ids(len(big), B, dev, absent=not exact, seed=4)
    bd = None if exact else big.bounds(B)
    torch.manual_seed(0)
    m = models.zinc_gnnml3().to(dev)
    res = {}
    nf = _count_calls(monkeypatch, 'gml_edge_mlp_fwd_stack6_sym_dev')
    nb = _count_calls(monkeypatch, 'gml_edge_mlp_bwd_sym_dev')
    for sym in (True, False):
        b = big.batch_assembled(ids, bd, sym=sym)
        m.zero_grad()
        pre = m(b)
        if exact:
            loss = models.zinc_loss(pre, b.y)
        else:
            loss = ((pre[:B, 0] - b.y[:B]).abs() * b.graph_valid).sum()
        loss.backward()
        res[sym] = (pre.detach().clone(), loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()})
        if sym:
            assert nf[0] >= 1 and nb[0] >= 1, (nf[0], nb[0])
            calls = (nf[0], nb[0])
    assert (nf[0], nb[0]) == calls                         # sym=False: the plain kernels
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
    for n in res[True][2]:
        e = rel_err(res[True][2][n].cpu().numpy(), res[False][2][n].cpu().numpy())
        assert e <= 1e-5, (n, e)


def test_captured_bs64_epoch_with_sym_is_bitwise_equal_to_the_eager_epoch(dev, base):
    """one captured ZINC GNNML3 training step at batch 64 over batch_assembled(sym=True) (assembly, forward, L1 loss, backward with
    deferred folds, OneLaunchAdam), replayed over a shuffled epoch, against the same epoch run eagerly: per-batch losses and final
    parameters bitwise equal (capture on one side stream)"""
    from gnn_matlang_amd import functional as Fn, models
    from gnn_matlang_amd.optim import OneLaunchAdam
    dd = base
    dd.prepare()
    BS = 64
    bd = dd.bounds(BS)
    G = len(dd)

    def train(captured):
        torch.manual_seed(0)
        m = models.zinc_gnnml3().to(dev)
        opt = OneLaunchAdam(m.parameters(), lr=1e-3)
        ids_buf = torch.zeros(BS, dtype=torch.int64, device=dev)
        loss_buf = torch.zeros((), device=dev)
        one = torch.ones((), device=dev)

        def step():
            b = dd.batch_assembled(ids_buf, bd, sym=True)
            opt.zero_grad(set_to_none=True)
            l = models.zinc_step_loss(m, b)
            with Fn.deferred_folds(list(m.parameters())):
                l.backward(one)
            opt.step()
            loss_buf.copy_(l.detach())
        run = step
        if captured:
            snap = {k: v.clone() for k, v in m.state_dict().items()}
            ids_buf.copy_(torch.arange(BS, device=dev))
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    step()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step()
            with torch.no_grad():
                for k, v in m.state_dict().items():
                    v.copy_(snap[k])
                for st in opt.state.values():
                    st['exp_avg'].zero_()
                    st['exp_avg_sq'].zero_()
                    st['step'].zero_()
            torch.cuda.synchronize()
            run = graph.replay
        perm = torch.randperm(G, generator=torch.Generator().manual_seed(9))
        perm = torch.cat([perm, torch.full(((-G) % BS,), G, dtype=torch.int64)]).to(dev)
        losses = []
        for i in range(0, perm.numel(), BS):
            ids_buf.copy_(perm[i:i + BS])
            run()
            losses.append(loss_buf.clone())
        torch.cuda.synchronize()
        return torch.stack(losses).cpu(), {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    le, se = train(False)
    lc, sc = train(True)
    assert torch.isfinite(le).all() and le.numel() == G // BS
    assert torch.equal(le, lc), (le - lc).abs().max()
    for k in se:
        assert torch.equal(se[k], sc[k]), k
