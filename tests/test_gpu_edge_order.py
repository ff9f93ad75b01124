"""The edge branch over unique support rows (gml_edge_sym_flags + the *_sym kernels, GraphCSR.sym_index) on edge lists in any order:
targets shuffled inside every source row, edges shuffled globally, multigraphs whose repeated edges are not neighbours in their row.
The pairing pass finds an edge's mirror by bisection inside a row and a repeated edge by its neighbours, so it needs the columns of
a view ascending inside every row; GraphCSR records that per view when the index is built (col_t_sorted: source view, col_sorted:
target view) and sym_index pairs only such views.  Every check here is against a reference that does not depend on edge order: a
numpy brute force of the pairing, float64 autograd of the edge branch, the float64 oracle model."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from test_gpu_parity import _sym_batch

pytestmark = pytest.mark.gpu

TOL = 1e-4
ORDERS = ('designed', 'rows', 'global')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from gnn_matlang_amd import _lib
    assert _lib.lib().gml_version() >= 1
    return torch.device('cuda:0')


def close(got, ref, tol=TOL, what=''):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    e = rel_err(got, ref)
    assert e <= tol, '%s: rel err %.3e > %.1e' % (what, e, tol)


# ------------------------------------------------------------------------------------------ inputs
def _order(ei, how, seed):
    """permutation of the columns of edge_index [2, E]: 'designed' -- as given; 'rows' -- sources kept ascending, the targets of every
    source row in random order; 'global' -- any order"""
    E = ei.size(1)
    if how == 'designed':
        return torch.arange(E, device=ei.device)
    r = torch.randperm(E, generator=torch.Generator().manual_seed(seed)).to(ei.device)
    if how == 'rows':
        r = r[torch.sort(ei[0][r], stable=True)[1]]
    return r


def _reordered(b, how, seed=0):
    """a copy of batch b with its support edges (edge_index2 and the rows of edge_attr2, one permutation) in the order `how`"""
    from gnn_matlang_amd.graph import Batch
    p = _order(b.edge_index2, how, seed)
    out = Batch(**{k: v for k, v in b.__dict__.items() if not k.startswith('_')})
    out.edge_index2 = b.edge_index2[:, p].contiguous()
    out.edge_attr2 = b.edge_attr2[p].contiguous()
    return out


def _counting_sym_batch(dev):
    """counting.py's twelve supports, made bitwise symmetric as in test_gpu_parity.test_edge_branch_over_unique_rows_twelve_supports
    (every edge takes the row of its src <= dst orientation: the design itself leaves mirrors one ulp apart)"""
    from gnn_matlang_amd import SpectralDesign, collate, synthetic
    raw = synthetic.make_graphs('counting', 96, seed=12)
    b = collate(SpectralDesign(recfield=1, dv=1, nfreq=10, adddegree=True, laplacien=False, addadj=True).design_many(raw))
    ei = b.edge_index2.numpy()
    N = int(b.x.size(0))
    key, rkey = ei[0].astype(np.int64) * N + ei[1], ei[1].astype(np.int64) * N + ei[0]
    order = np.argsort(key)
    rev = order[np.searchsorted(key[order], rkey)]
    ea = b.edge_attr2.numpy()
    b.edge_attr2 = torch.from_numpy(np.where((ei[0] <= ei[1])[:, None], ea, ea[rev]))
    b = b.to(dev)
    assert b.edge_attr2.size(1) == 12
    return b


def _six_batch(dev):
    """sr25.py's six supports (SpectralDesign(recfield=1, dv=2, nfreq=5, adddegree=True)) on ZINC-like graphs"""
    from gnn_matlang_amd import SpectralDesign, collate, synthetic
    raw = synthetic.make_graphs('zinc', 80, seed=8)
    b = collate(SpectralDesign(recfield=1, dv=2, nfreq=5, adddegree=True).design_many(raw)).to(dev)
    assert b.edge_attr2.size(1) == 6
    return b


def _multigraph(dev):
    """(edge_index sorted by (src, dst), rows, N): a symmetric structure plus edges repeated on one side and on both sides, one-sided
    edges and self loops; the rows are a function of the unordered pair, so mirrors are bitwise equal"""
    g = torch.Generator().manual_seed(5)
    N = 300
    a = torch.randint(0, N, (2, 1500), generator=g)
    und = torch.unique(torch.cat([a, a.flip(0)], 1), dim=1)
    extra = torch.cat([und[:, :200], und[:, :200]], 1)                       # 200 edges repeated twice more, one side only
    both = torch.cat([und[:, 400:450], und[:, 400:450].flip(0)], 1)          # 50 pairs repeated on both sides
    oneside = torch.stack([torch.randint(0, N, (120,), generator=g), torch.randint(0, N, (120,), generator=g)])
    ei = torch.cat([und, extra, both, oneside, torch.arange(N).repeat(2, 1)], 1)
    ei = ei[:, torch.argsort(ei[0] * N + ei[1], stable=True)]
    lo, hi = torch.minimum(ei[0], ei[1]), torch.maximum(ei[0], ei[1])
    base = torch.randn(N * N // 64 + 8, 8, generator=g)
    return ei.to(dev), base[(lo * 7 + hi * 13) % base.size(0)].contiguous().to(dev), N


# ------------------------------------------------------------------------------------------ the pairing against a brute force
def _brute(row, col, bits):
    """gml_edge_sym_flags' semantics over one view, by edge KEYS (no use of the order): position k with (i, j) = (row[k], col[k]) gets
    flag 2 when (i, j) occurs once, (j, i) occurs once (at position a), rows k and a are bitwise equal and i < j (mirror = a); flag 0
    under the same conditions with i > j; flag 1 otherwise (mirror -1)"""
    where = {}
    for k, key in enumerate(zip(row.tolist(), col.tolist())):
        where.setdefault(key, []).append(k)
    flag, mirror = np.ones(row.size, np.int64), -np.ones(row.size, np.int64)
    for (i, j), ks in where.items():
        rev = where.get((j, i), ())
        if i == j or len(ks) != 1 or len(rev) != 1:
            continue
        k, a = ks[0], rev[0]
        if not np.array_equal(bits[k], bits[a]):
            continue
        if i < j:
            flag[k], mirror[k] = 2, a
        else:
            flag[k] = 0
    return flag, mirror


def _view(csr, view):
    rp, col = (csr.rowptr_t, csr.col_t) if view == 'source' else (csr.rowptr, csr.col)
    rp, col = rp.cpu().numpy().astype(np.int64), col.cpu().numpy().astype(np.int64)
    return np.repeat(np.arange(rp.size - 1), np.diff(rp)), col


def _check_pairing(csr, vals, view):
    """sym_index(vals, view) is None or the brute force's list, every edge covered exactly once; a view recorded sorted really is"""
    sym = csr.sym_index(vals, view)
    row, col = _view(csr, view)
    recorded = csr.col_t_sorted if view == 'source' else csr.col_sorted
    if recorded:
        assert ((row[1:] != row[:-1]) | (col[1:] >= col[:-1])).all(), '%s view recorded sorted, but a row descends' % view
    flag, mirror = _brute(row, col, vals.cpu().numpy().view(np.int32))
    if sym is None:
        # the only reasons to stay on the plain kernels: the view's rows are not known sorted, or pairing would save < 10 %
        assert not recorded or (flag > 0).sum() > 0.9 * row.size, view
        return None
    assert recorded
    uid, mir = sym[0].cpu().numpy(), sym[1].cpu().numpy()
    np.testing.assert_array_equal(uid, np.nonzero(flag)[0])
    np.testing.assert_array_equal(mir, mirror[uid])
    covered = np.zeros(row.size, np.int64)
    np.add.at(covered, uid, 1)
    np.add.at(covered, mir[mir >= 0], 1)
    assert (covered == 1).all(), 'rows written %s times' % np.unique(covered)
    return sym


def _expect_lists(csr, how):
    """which views sym_index may pair after each reordering -- and must, where the batch's rows allow it: designed order (sources and
    targets ascending) both views; targets shuffled inside source rows: the target view (its sources still ascend in every row);
    a global shuffle: none (the source view's rows and the target view's rows are both out of order)"""
    assert csr.src_sorted == (how != 'global')
    assert csr.col_sorted == (how != 'global') and csr.col_t_sorted == (how == 'designed'), (how, csr.col_sorted, csr.col_t_sorted)
    return {'source': how == 'designed', 'target': how != 'global'}


@pytest.mark.parametrize('how', ORDERS)
@pytest.mark.parametrize('case', ['zinc', 'zinc-ulp', 'multigraph'])
def test_pairing_matches_a_brute_force_in_any_edge_order(dev, case, how):
    """(a) designed ZINC supports, (d) the same with 30 % of the rows one ulp off their mirror, (c) a multigraph (repeated edges that
    are not neighbours in their row once the rows are shuffled, self loops, one-sided edges) -- each as designed, with the targets
    shuffled inside every source row, and globally shuffled (b): both views against the brute force; the designed order keeps its
    pairing in both views (a gate too strict would otherwise pass unnoticed)"""
    from gnn_matlang_amd.graph import GraphCSR
    if case == 'multigraph':
        ei, rows, N = _multigraph(dev)
        p = _order(ei, how, seed=1)
        ei, rows = ei[:, p].contiguous(), rows[p].contiguous()
    else:
        b = _reordered(_sym_batch(dev, perturb=0.3 if case == 'zinc-ulp' else 0.0), how, seed=2)
        ei, rows, N = b.edge_index2, b.edge_attr2, int(b.x.size(0))
    csr = GraphCSR.from_edge_index(ei, N)
    want = _expect_lists(csr, how)
    vals_t = csr.sort_values(rows)
    vals_s = csr.to_source_order(vals_t)
    for view, vals in (('source', vals_s), ('target', vals_t)):
        sym = _check_pairing(csr, vals, view)
        assert (sym is not None) == want[view], (case, how, view)


# ------------------------------------------------------------------------------------------ the edge branch on shuffled inputs
def _branch64(vals, w):
    e = vals.double().cpu()
    p = [t.double().cpu().requires_grad_(True) for t in w]
    h = torch.cat([torch.relu(e @ p[0].t()), torch.tanh(e @ p[1].t()) * torch.tanh(e @ p[2].t())], 1)
    return torch.relu(h @ p[3].t()), p


@pytest.mark.parametrize('how', ['rows', 'global'])
@pytest.mark.parametrize('S,layers', [(8, 1), (8, 2), (8, 4), (6, 1), (12, 1)])
def test_edge_branch_on_shuffled_edges(dev, S, layers, how):
    """the edge branch as the layer runs it (pairing on: the list sym_index gives the view, else the plain kernels) on shuffled edge
    lists, in both views: the forward bitwise equal to the plain forward, dW1..dW4 equal to the plain backward to summation order
    (1e-5 of their scale; 3e-5 at twelve supports, the bound of the designed-order test) and to float64 autograd (1e-4)"""
    from gnn_matlang_amd import functional as Fn
    b = _sym_batch(dev) if S == 8 else _six_batch(dev) if S == 6 else _counting_sym_batch(dev)
    b = _reordered(b, how, seed=3)
    csr = b.csr('edge_index2')
    want = _expect_lists(csr, how)
    torch.manual_seed(S + layers)
    ws = [tuple(torch.randn(*shp, device=dev) * (0.3 if S == 12 else 0.4) for shp in ((2 * S, S), (2 * S, S), (2 * S, S), (S, 4 * S)))
          for _ in range(layers)]
    vals_t = csr.sort_values(b.edge_attr2)
    for view, vals in (('source', csr.to_source_order(vals_t, cache=True)), ('target', vals_t)):
        sym = _check_pairing(csr, vals, view)
        assert (sym is not None) == want[view], (how, view)
        split = csr.presplit(vals)
        plain = Fn.edge_mlp_fwd_stack(vals, split, ws, None) if layers > 1 else [Fn.edge_mlp_fwd(vals, *ws[0], None, split)[0]]
        shared = Fn.edge_mlp_fwd_stack(vals, split, ws, sym) if sym is not None else plain
        assert shared is not None and len(shared) == layers
        for l in range(layers):
            assert torch.equal(plain[l], shared[l]), '%s view, layer %d: forward over unique rows differs' % (view, l)
        gout = torch.randn_like(vals)
        w1, w2, w3, w4 = ws[0]
        ref = Fn.edge_mlp_bwd(vals, w1, w2, w3, w4, gout, False, split, None)
        got = Fn.edge_mlp_bwd(vals, w1, w2, w3, w4, gout, False, split, sym)
        assert got[0] is None
        for name, a, r in zip(('dw1', 'dw2', 'dw3', 'dw4'), got[1:], ref[1:]):
            close(a, r, tol=3e-5 if S == 12 else 1e-5, what='%s view: backward %s vs the plain backward' % (view, name))
        for l in range(layers):
            out, p64 = _branch64(vals, ws[l])
            close(shared[l], out.float(), tol=1e-5, what='%s view, layer %d: forward vs float64' % (view, l))
            if l == 0:
                out.backward(gout.double().cpu())
                for name, a, p in zip(('dw1', 'dw2', 'dw3', 'dw4'), got[1:], p64):
                    close(a, p.grad.float(), what='%s view: backward %s vs float64' % (view, name))


# ------------------------------------------------------------------------------------------ model steps in any edge order
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


def _regular_batch(dev):
    """sr25-shaped input: 2 features, six supports (random regular graphs, SpectralDesign(recfield=1, dv=2, nfreq=5, adddegree=True))"""
    from gnn_matlang_amd import SpectralDesign, collate, synthetic
    raw = synthetic.make_graphs('regular', 40, seed=8)
    b = collate(SpectralDesign(recfield=1, dv=2, nfreq=5, adddegree=True).design_many(raw))
    assert b.x.size(1) == 2 and b.edge_attr2.size(1) == 6
    return b


@pytest.mark.parametrize('model', ['zinc', 'sr25'])
def test_model_step_does_not_depend_on_edge_order(dev, model, monkeypatch):
    """ZINC GNNML3 / sr25 GNNML3, one batch in three edge orders (designed, targets shuffled inside source rows, globally shuffled),
    GML_EDGE_SYM on and off: the training step (logits, every parameter gradient of a fixed linear loss) against the float64 oracle
    at 1e-4, and the eval forward (m.eval(), no grad) likewise.  Bitwise: pairing on / off within each order; the in-row shuffle
    against the designed order -- the forward sums a target's messages in stable target order, which a shuffle inside source rows
    leaves as it is, and the edge branch computes each edge's row alone.  Every pairing the layers ask for is given exactly where the
    view's rows allow it, and the ZINC model in the designed order really takes the unique-row road in training and in eval (launch
    count)."""
    from gnn_matlang_amd import SpectralDesign, collate, synthetic, functional as Fn, models
    from gnn_matlang_amd.graph import GraphCSR
    from oracle import models_oracle as MO
    if model == 'zinc':
        host = collate(SpectralDesign(recfield=2, dv=2, nfreq=7).design_many(synthetic.make_graphs('zinc', 64, seed=21)))
        ctor, ref = models.zinc_gnnml3, MO.zinc_gnnml3()
    else:
        host = _regular_batch(dev)
        ctor, ref = models.sr25_gnnml3, MO.sr25_gnnml3()
    torch.manual_seed(0)
    m = ctor().to(dev)
    ref.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
    ref = ref.double()
    base = host.to(dev)
    G = host.num_graphs
    wout = torch.randn(G, 10 if model == 'sr25' else 1, generator=torch.Generator().manual_seed(1)).to(dev)
    # the float64 reference, once: the oracle's sums do not depend on the edge order beyond float64 rounding
    args = (host.x.double(), host.edge_index2, host.edge_attr2.double(), host.batch, G)
    ref.train()
    pre64 = ref(*args)
    (pre64 * wout.cpu().double()).sum().backward()
    grad64 = {n: p.grad.detach().clone() for n, p in ref.named_parameters()}
    with torch.no_grad():
        ev64 = ref.eval()(*args)
    nf = _count_calls(monkeypatch, 'gml_edge_mlp_fwd_stack6_sym')
    asked = []
    sym_index = GraphCSR.sym_index

    def spy(self, val, view='source'):
        out = sym_index(self, val, view)
        asked.append((view, out is not None))
        return out
    monkeypatch.setattr(GraphCSR, 'sym_index', spy)
    res = {}
    for how in ORDERS:
        b = _reordered(base, how, seed=4)
        csr = b.csr('edge_index2')
        want = _expect_lists(csr, how)
        for on in (True, False):
            old = Fn.EDGE_SYM
            Fn.EDGE_SYM = on
            try:
                n0, a0 = nf[0], len(asked)
                m.train()
                m.zero_grad()
                pre = m(b)
                (pre * wout).sum().backward()
                n1, a1 = nf[0], len(asked)
                m.eval()
                with torch.no_grad():
                    ev = m(b)
                n2 = nf[0]
            finally:
                Fn.EDGE_SYM = old
                m.train()
            res[how, on] = (pre.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()}, ev.clone())
            what = '%s, %s order, pairing %s: ' % (model, how, 'on' if on else 'off')
            for view, got in asked[a0:]:
                assert got == want[view], what + '%s view paired: %s' % (view, got)
            if not on or how == 'global':
                assert n2 == n0, what + 'unique-row launches'
            if on and how == 'designed' and model == 'zinc':        # (the bench's model: paired in training and in eval)
                assert n1 > n0 and n2 > n1 and any(g for _, g in asked[a0:a1]), what + 'the unique-row road was not taken'
            close(pre, pre64, what=what + 'logits vs float64')
            for n, g64 in grad64.items():
                close(res[how, on][1][n], g64, what=what + 'grad %s vs float64' % n)
            close(ev, ev64, what=what + 'eval logits vs float64')
        assert torch.equal(res[how, True][0], res[how, False][0]), how
        assert torch.equal(res[how, True][2], res[how, False][2]), how
    assert torch.equal(res['rows', True][0], res['designed', True][0])
    assert torch.equal(res['rows', True][2], res['designed', True][2])


# ------------------------------------------------------------------------------------------ exact assembled batches
def _shuffled_rows_dataset(dev):
    """designed ZINC graphs whose support edges have their targets shuffled inside every source row (rows of edge_attr2 with them)"""
    from gnn_matlang_amd import SpectralDesign, synthetic
    from gnn_matlang_amd.dataset import DeviceDataset
    rng = np.random.default_rng(6)
    ds = SpectralDesign(recfield=2, dv=2, nfreq=7).design_many(synthetic.make_graphs('zinc', 256, seed=31))
    out = []
    for g in ds:
        g = dict(g)
        ei = np.asarray(g['edge_index2'])
        p = np.lexsort((rng.random(ei.shape[1]), ei[0]))
        g['edge_index2'], g['edge_attr2'] = ei[:, p], np.asarray(g['edge_attr2'])[p]
        out.append(g)
    dd = DeviceDataset.from_graphs(out, dev)
    dd.y = dd.y.float()
    return dd


def _step(m, b):
    from gnn_matlang_amd import models
    m.zero_grad()
    pre = m(b)
    loss = models.zinc_loss(pre, b.y)
    loss.backward()
    return pre.detach().clone(), loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()}


def test_exact_assembled_batch_with_targets_shuffled_in_rows(dev):
    """batch_assembled(ids, None, sym=False) on a data set whose rows are out of order: the same arrays, the same per-view sortedness
    and the same training step, bit for bit, as batch(ids) + GraphCSR.from_edge_index; sym=True (the data set's key-sorted pairing,
    which does not need sorted rows) the same logits and loss bitwise and gradients within 1e-5"""
    from gnn_matlang_amd import models
    from gnn_matlang_amd.graph import GraphCSR
    dd = _shuffled_rows_dataset(dev)
    dd.prepare()
    ids = torch.randperm(len(dd), generator=torch.Generator().manual_seed(7))[:200].to(dev).contiguous()
    b = dd.batch(ids)
    b._csr['edge_index2'] = c = GraphCSR.from_edge_index(b.edge_index2, int(b.x.size(0)))
    assert c.src_sorted and c.col_sorted and not c.col_t_sorted
    be = dd.batch_assembled(ids, None, sym=False)
    ce = be.csr('edge_index2')
    for nm in ('rowptr', 'col', 'perm', 'rowptr_t', 'col_t', 'perm_t', 'pos_t', 'tpos', 'ginfo128', 'ginfo_t128'):
        assert torch.equal(getattr(c, nm), getattr(ce, nm)), nm
    assert (ce.src_sorted, ce.col_sorted, ce.col_t_sorted) == (c.src_sorted, c.col_sorted, c.col_t_sorted)
    assert ce.sym_index(be.edge_attr2) is None and c.sym_index(b.edge_attr2) is None
    torch.manual_seed(0)
    m = models.zinc_gnnml3().to(dev)
    r = _step(m, b)
    re_ = _step(m, be)
    assert torch.equal(r[0], re_[0]) and torch.equal(r[1], re_[1])
    for n in r[2]:
        assert torch.equal(r[2][n], re_[2][n]), n
    bs = dd.batch_assembled(ids, None, sym=True)
    assert bs.csr('edge_index2')._sym_dev is not None
    rs = _step(m, bs)
    assert torch.equal(r[0], rs[0]) and torch.equal(r[1], rs[1])
    for n in r[2]:
        close(rs[2][n], r[2][n], tol=1e-5, what='sym=True vs sym=False ' + n)
    # the same graphs as designed (rows sorted): the exact batch records a sorted source view, as from_edge_index does
    from gnn_matlang_amd import SpectralDesign, synthetic
    from gnn_matlang_amd.dataset import DeviceDataset
    ds = DeviceDataset.from_graphs(SpectralDesign(recfield=2, dv=2, nfreq=7).design_many(synthetic.make_graphs('zinc', 256, seed=31)), dev)
    ds.y = ds.y.float()
    ds.prepare()
    bd = ds.batch(ids)
    cd = GraphCSR.from_edge_index(bd.edge_index2, int(bd.x.size(0)))
    ced = ds.batch_assembled(ids, None).csr('edge_index2')
    assert cd.col_sorted and cd.col_t_sorted and ced.col_sorted and ced.col_t_sorted
