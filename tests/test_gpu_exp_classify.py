"""The EXP classification experiment (exp_classify.py) on the device: the fused head / BCE / accuracy kernel against float64,
saturated logits, both models on real EXP graphs against a float64 composition of the oracle layers, padded static batches,
evaluation under no_grad, and captured epochs equal to eager ones."""
import copy
import math
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


def _close(got, ref, what):
    e = rel_err(got.detach().cpu().numpy(), ref.detach().cpu().numpy())
    print('%-28s rel err %.2e' % (what, e))
    assert e <= TOL, (what, e)


# ------------------------------------------------------------------ 1. the kernel against float64
def _head_inputs(rows, nin, nh, seed, bias=True, mask=True):
    """float32 inputs on the host; w2 scaled so that the logits' rms is 2.5 (|z| stays far inside 12, and away from 0)"""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(rows, nin, generator=g)
    w1 = torch.randn(nh, nin, generator=g) * (2.0 / math.sqrt(nin))
    b1 = torch.randn(nh, generator=g) * 0.5 if bias else None
    w2 = torch.randn(1, nh, generator=g)
    b2 = torch.randn(1, generator=g) * 0.5 if bias else None
    y = (torch.rand(rows, generator=g) < 0.5).float()
    valid = (torch.rand(rows, generator=g) < 0.7).float() if mask else None
    return p, w1, b1, w2, b2, y, valid


def _head_ref(p, w1, b1, w2, b2, y, valid, act, rows_loss, gscale):
    """float64 composition with autograd: (loss, z, ok, count, gradients p / w1 / b1 / w2 / b2, smallest |fc1 output| under relu)"""
    P, W1, W2 = (t.double().requires_grad_(True) for t in (p, w1, w2))
    B1 = b1.double().requires_grad_(True) if b1 is not None else None
    B2 = b2.double().requires_grad_(True) if b2 is not None else None
    a = F.linear(P, W1, B1)
    z = F.linear(F.relu(a) if act else a, W2, B2)[:, 0]
    v = (valid if valid is not None else torch.ones_like(y)).double()
    l = F.binary_cross_entropy(torch.sigmoid(z), y.double(), reduction='none')       # exp_classify.py:328-329 in float64
    loss = (v * l)[:rows_loss].sum()
    (loss * gscale).backward()
    ok = float((v * ((z > 0) == (y == 1)).double())[:rows_loss].sum())
    cnt = float((v[:rows_loss] != 0).sum())
    grad = lambda t: t.grad if t is not None else None
    return loss.detach(), z.detach(), ok, cnt, (P.grad, W1.grad, grad(B1), W2.grad, grad(B2)), float(a.detach().abs().min())


def _scaled(rows, nin, nh, act, seed, bias=True, mask=True):
    p, w1, b1, w2, b2, y, valid = _head_inputs(rows, nin, nh, seed, bias, mask)
    a = F.linear(p.double(), w1.double(), b1.double() if bias else None)
    s = F.linear(F.relu(a) if act else a, w2.double())
    w2 = (w2.double() * (2.5 / max(float(s.pow(2).mean().sqrt()), 1e-3))).float()
    return p, w1, b1, w2, b2, y, valid


def _run_kernel(dev, inp, act, rows_loss, gscale, stats=None):
    from gnn_matlang_amd import functional as Fn
    p, w1, b1, w2, b2, y, valid = (t.to(dev) if t is not None else None for t in inp)
    leaves = [t.clone().requires_grad_(True) if t is not None else None for t in (p, w1, b1, w2, b2)]
    yl, vl = y[:rows_loss], (valid[:rows_loss] if valid is not None else None)
    loss = Fn.HeadBCEFunction.apply(leaves[0], yl, vl, leaves[1], leaves[2], leaves[3], leaves[4], act, stats)
    (loss * gscale).backward()
    _, pre = Fn.head_bce_logits(p, yl, vl, w1, b1, w2, b2, act)
    return loss.detach(), pre, [t.grad if t is not None else None for t in leaves]


def _check_case(dev, rows, nin, nh, act, rows_loss, seed, bias=True, mask=True):
    inp = _scaled(rows, nin, nh, act, seed, bias, mask)
    valid = inp[6]
    rloss, rz, rok, rcnt, rgrads, amin = _head_ref(*inp, act, rows_loss, 1.5)
    # every row that counts: a logit the reference's own fp32 arithmetic resolves (exp_classify.py:328), away from the class boundary
    counted = torch.arange(rows) < rows_loss
    if valid is not None:
        counted &= valid != 0
    zc = rz[counted].abs()
    if zc.numel():
        assert 1e-3 <= float(zc.min()) and float(zc.max()) <= 12, (float(zc.min()), float(zc.max()))
    # (a relu whose float64 argument is within float32's rounding of a <= 64-term dot product of zero may flip: a jump of the
    #  gradient, not an error of either arithmetic -- such a seed fails here like one outside the window above)
    assert not act or amin >= 2e-6, amin
    stats = torch.zeros(3, device=dev)
    loss, pre, grads = _run_kernel(dev, inp, act, rows_loss, 1.5, stats)
    _close(loss, rloss, 'loss')
    _close(pre, rz, 'pre')
    for g, r, what in zip(grads, rgrads, ('gp', 'dW1', 'db1', 'dw2', 'db2')):
        if r is not None:
            _close(g.reshape(r.shape), r, what)
    _close(stats[0], rloss, 'stats.loss')
    assert float(stats[1]) == rok and float(stats[2]) == rcnt, (stats.tolist(), rok, rcnt)
    gp = grads[0]
    assert not gp[rows_loss:].any()                            # the padding graph's rows: exact zeros
    if valid is not None:
        assert not gp[:rows_loss][valid[:rows_loss].to(dev) == 0].any()
    # fixed-order sums: the same bits again; stats is +=: twice the sums, and a NaN in it stays
    loss2, pre2, grads2 = _run_kernel(dev, inp, act, rows_loss, 1.5, stats)
    assert torch.equal(loss2, loss) and torch.equal(pre2, pre)
    for a, b in zip(grads, grads2):
        assert (a is None and b is None) or torch.equal(a, b)
    assert torch.equal(stats.cpu(), torch.stack([2 * loss.cpu(), torch.tensor(2 * rok), torch.tensor(2 * rcnt)]).float())
    nan = torch.full((3,), float('nan'), device=dev)
    _run_kernel(dev, inp, act, rows_loss, 1.5, nan)
    assert torch.isnan(nan).all()


# seeds: 1000 rows + nin + act unless listed here (the |z| window above must hold for every counted row: checked, not skipped)
_SEEDS = {(1000, 5, 1, 1): 1, (1000, 64, 64, 1): 1, (257, 48, 10, 1, 'none'): 1}


@pytest.mark.parametrize('act', [0, 1])
@pytest.mark.parametrize('nin,nh', [(48, 10), (64, 10), (5, 1), (64, 64)])
@pytest.mark.parametrize('rows', [1, 3, 51, 256, 257, 1000])
def test_head_against_float64(dev, rows, nin, nh, act):
    """loss, logits, every gradient, the correct count and the row count with a padding row (rows_loss = rows - 1), ~30 % of the
    rows invalid, upstream gradient 1.5"""
    _check_case(dev, rows, nin, nh, act, rows - 1, _SEEDS.get((rows, nin, nh, act), 1000 * rows + nin + act))


@pytest.mark.parametrize('rows,nin,nh,act', [(1, 48, 10, 1), (257, 48, 10, 1), (51, 64, 10, 0)])
def test_head_without_a_padding_row(dev, rows, nin, nh, act):
    _check_case(dev, rows, nin, nh, act, rows, _SEEDS.get((rows, nin, nh, act, 'full'), 7000 * rows + nin + act))


@pytest.mark.parametrize('nin,nh,act', [(48, 10, 0), (48, 10, 1), (64, 10, 0), (64, 10, 1), (64, 64, 0), (64, 64, 1), (5, 1, 0)])
@pytest.mark.parametrize('rows', [3, 257])
def test_head_without_biases_and_validity(dev, rows, nin, nh, act):
    """b1 = b2 = valid = None (NULL pointers in the C ABI).  (One relu unit without biases gives z = 0 exactly on half the rows: the
    5 -> 1 shape runs with the identity here.)"""
    _check_case(dev, rows, nin, nh, act, rows - 1, _SEEDS.get((rows, nin, nh, act, 'none'), 3000 * rows + nin + act), bias=False, mask=False)


def test_head_reads_strided_rows(dev):
    """ldp > nin: the pooled rows as a column slice of a wider buffer give the bits of the contiguous copy"""
    from gnn_matlang_amd import functional as Fn
    inp = [t.to(dev) for t in _scaled(51, 48, 10, 1, 99)]
    wide = torch.randn(51, 53, device=dev)
    wide[:, 2:50] = inp[0]
    a = Fn.head_bce_logits(inp[0], inp[5], inp[6], *inp[1:5], 1)
    b = Fn.head_bce_logits(wide[:, 2:50], inp[5], inp[6], *inp[1:5], 1)
    assert Fn.head_bce_supported(wide[:, 2:50], inp[1], inp[3]) and not Fn.head_bce_supported(torch.randn(48, 51, device=dev).t(), inp[1], inp[3])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_head_refuses_what_it_does_not_serve(dev):
    from gnn_matlang_amd import _lib, functional as Fn
    p = torch.randn(4, 65, device=dev)
    w1, w2 = torch.randn(10, 65, device=dev), torch.randn(1, 10, device=dev)
    assert not Fn.head_bce_supported(p, w1, w2)
    assert not Fn.head_bce_supported(p[:, :64].double(), w1[:, :64].double(), w2.double())
    assert not Fn.head_bce_supported(p[:, :64], w1[:, :64].contiguous(), torch.randn(2, 10, device=dev))
    with pytest.raises(ValueError):
        Fn.HeadBCEFunction.apply(p, torch.zeros(4, device=dev), None, w1, None, w2, None, 1, None)
    L = _lib.lib()
    assert L.gml_head_bce_workspace_floats(256, 48, 10) == 0 and L.gml_head_bce_workspace_floats(257, 48, 10) == 2 * (480 + 20 + 4)
    q = torch.randn(300, 48, device=dev)
    v1, v2, y, out = torch.randn(10, 48, device=dev), torch.randn(1, 10, device=dev), torch.zeros(300, device=dev), torch.zeros(1, device=dev)
    ptr = lambda t: t.data_ptr()
    args = lambda rows, nin, nh, ws, nws: (ptr(q), 48, ptr(y), None, ptr(v1), None, ptr(v2), None, rows, rows, nin, nh, 1, ptr(out), None, None, ws, nws, None)
    assert L.gml_head_bce_fwd(*args(300, 48, 10, None, 0)) == _lib.GML_E_WORKSPACE
    assert L.gml_head_bce_fwd(*args(300, 48, 65, None, 0)) == _lib.GML_E_UNSUPPORTED
    assert L.gml_head_bce_fwd(*args(0, 48, 10, None, 0)) == _lib.GML_E_BADARG


# ------------------------------------------------------------------ 2. saturated logits
def test_saturated_logits(dev):
    """z = +-30, +-120 with both labels through nin = nh = 1, identity, unit weights: the loss is min(softplus, 100) and the
    gradient sigmoid(z) - y of float64 -- where the reference's fp32 sigmoid has rounded to 0 / 1 (loss 100, gradient 0)"""
    from gnn_matlang_amd import functional as Fn
    z = torch.tensor([30., 30., -30., -30., 120., 120., -120., -120.])
    y = torch.tensor([0., 1., 0., 1., 0., 1., 0., 1.])
    zd, yd = z.double(), y.double()
    sp = lambda t: torch.clamp(t, min=0) + torch.log1p(torch.exp(-t.abs()))
    lref = yd * torch.clamp(sp(-zd), max=100) + (1 - yd) * torch.clamp(sp(zd), max=100)
    # sigmoid(z) - y without cancellation: y = 1: -sigmoid(-z)
    sig = lambda t: torch.where(t >= 0, 1 / (1 + torch.exp(-t.abs())), torch.exp(-t.abs()) / (1 + torch.exp(-t.abs())))
    dref = torch.where(yd == 1, -sig(-zd), sig(zd))
    assert [round(float(v), 6) for v in lref[[0, 4, 5]]] == [30.0, 100.0, 0.0] and 9.3e-14 < float(lref[1]) < 9.4e-14
    one = torch.ones(1, 1, device=dev)
    p = z.view(-1, 1).to(dev).requires_grad_(True)
    w1, w2 = one.clone().requires_grad_(True), one.clone().requires_grad_(True)
    total = Fn.HeadBCEFunction.apply(p, y.to(dev), None, w1, None, w2, None, 0, None)
    total.backward()
    got_l = torch.stack([Fn.HeadBCEFunction.apply(p.detach(), y.to(dev), torch.eye(8, device=dev)[r].contiguous(), one, None, one, None, 0, None)
                         for r in range(8)]).double().cpu()
    got_d = p.grad[:, 0].double().cpu()
    print('loss per row', got_l.tolist(), lref.tolist())
    print('dz per row', got_d.tolist(), dref.tolist())
    for got, ref in ((got_l, lref), (got_d, dref)):
        assert torch.isfinite(got).all()
        # (1e-37: what float32 cannot hold -- exp(-120) = 8e-53 -- is zero)
        assert bool(((got - ref).abs() <= TOL * ref.abs() + 1e-37).all()), (got.tolist(), ref.tolist())
    assert torch.isfinite(total) and abs(float(total.detach()) - float(lref.sum())) <= TOL * float(lref.sum())
    assert torch.isfinite(w1.grad).all() and torch.isfinite(w2.grad).all()
    _close(w2.grad.view(-1), (dref * zd).sum().view(1), 'dw2')


# ------------------------------------------------------------------ 3. the models on real EXP graphs
NTRAIN, NVAL = 32, 8


@pytest.fixture(scope='module')
def exp_graphs():
    """the first 32 train graphs (ids 400..431) and the first 8 val graphs (ids 0..7) of the fixture, designed as exp_classify.py:16"""
    from gnn_matlang_amd import SpectralDesign, readers
    val, _, train = readers.exp_classify_splits(readers.load_exp(os.path.join(GOLDEN, 'raw', 'exp.npz')))
    ds = SpectralDesign(nmax=64, recfield=1, dv=2, nfreq=5, adddegree=True).design_many(list(train[:NTRAIN]) + list(val[:NVAL]))
    return ds[:NTRAIN], ds[NTRAIN:]


def _model(which, dev=None):
    from gnn_matlang_amd import models
    m = {'gnnml3': models.exp_classify_gnnml3, 'gnnml1': models.exp_classify_gnnml1}[which]()
    return m.to(dev).train() if dev is not None else m


def _oracle_logits(which, P, data, dtype):
    """the reference model (exp_classify.py:244-262 / :284-295) composed from the oracle's layers in `dtype` on data's device"""
    from oracle import spect_conv_oracle as SO
    x = data.x.to(dtype)
    sub = lambda pre: {k[len(pre):]: v for k, v in P.items() if k.startswith(pre)}
    if which == 'gnnml3':
        ea = data.edge_attr2.to(dtype)
        for i in (1, 2, 3):
            x = SO.ml3layer_forward(x, data.edge_index2, ea, sub('conv%d.' % i), True, 16)
    else:
        ones = torch.ones(data.edge_index.size(1), 1, dtype=dtype, device=x.device)
        for i in (1, 2, 3):
            lin = lambda j: F.linear(x, P['fc%d%d.weight' % (i, j)], P['fc%d%d.bias' % (i, j)])
            c = SO.spectconv_forward(x, data.edge_index, ones, P['conv%d1.weight' % i], P['conv%d1.bias' % i], selfconn=False)
            x = F.relu(lin(1) + c + lin(2) * lin(3))
    B = int(data.ptr.numel()) - 1
    cnt = torch.bincount(data.batch, minlength=B).to(dtype).unsqueeze(1)
    x = torch.zeros(B, x.size(1), dtype=dtype, device=x.device).index_add_(0, data.batch, x) / cnt       # global_mean_pool
    h = F.linear(x, P['fc1.weight'], P['fc1.bias'])
    return F.linear(F.relu(h) if which == 'gnnml3' else h, P['fc2.weight'], P['fc2.bias'])


def _oracle(which, P, data, dtype):
    pre = _oracle_logits(which, P, data, dtype)
    loss = F.binary_cross_entropy(torch.sigmoid(pre), data.y.to(dtype).unsqueeze(-1), reduction='sum')   # exp_classify.py:328-329
    return pre, loss


def _params(state, dtype, device='cpu'):
    return {k: v.detach().to(device).to(dtype).requires_grad_(True) for k, v in state.items()}


def _step(m, data, stats=None):
    """one forward + backward through exp_classify_step_loss with the road recorded"""
    from gnn_matlang_amd import functional as Fn, models
    old, Fn.VERBOSE = Fn.VERBOSE, True
    Fn.PATHS.clear()
    try:
        m.zero_grad(set_to_none=True)
        loss = models.exp_classify_step_loss(m, data, stats=stats)
        loss.backward()
        paths = dict(Fn.PATHS)
    finally:
        Fn.VERBOSE = old
        Fn.PATHS.clear()
    return loss.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}, paths


def _assert_fused(paths):
    heads = [k for k in paths if k.startswith('head:')]
    assert heads and all('fused BCE head' in k for k in heads) and not any('torch ops' in k for k in paths), paths


@pytest.mark.parametrize('seed', [0, 1])
@pytest.mark.parametrize('ids', [[0, 1, 2, 3, 4, 5], [0, 3, 4, 7, 8, 11]], ids=['paired', 'unpaired'])
@pytest.mark.parametrize('which', ['gnnml3', 'gnnml1'])
def test_models_against_the_oracle(dev, exp_graphs, which, ids, seed):
    """graphs 400 + ids of the fixture: logits, loss, every parameter gradient and the correct count against the float64 oracle, on
    the fused head; then five Adam steps at lr 1e-3"""
    from gnn_matlang_amd import collate, functional as Fn
    host = collate([exp_graphs[0][i] for i in ids])
    assert host.x.size(1) == 2 and host.edge_attr2.size(1) == 6
    torch.manual_seed(seed)
    m = _model(which)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    # the margin: the reference in ITS arithmetic (fp32, CPU) against float64 on this batch and seed -- a factor of 10 under TOL, and
    # no relu of the reference flips between the two
    P32, P64 = _params(state, torch.float32), _params(state, torch.float64)
    pre32, loss32 = _oracle(which, P32, host, torch.float32)
    pre64, loss64 = _oracle(which, P64, host, torch.float64)
    loss32.backward()
    loss64.backward()
    margins = [('pre', rel_err(pre32.detach().numpy(), pre64.detach().numpy())), ('loss', rel_err(loss32.detach().numpy(), loss64.detach().numpy()))]
    margins += [('grad ' + k, rel_err(P32[k].grad.numpy(), P64[k].grad.numpy())) for k in P64]
    print('fp32 oracle vs float64: worst %.2e (%s), smallest |z| %.3g' % (max(e for _, e in margins), max(margins, key=lambda t: t[1])[0],
                                                                          float(pre64.detach().abs().min())))
    assert all(e <= 1e-5 for _, e in margins), margins
    # the device
    m = m.to(dev).train()
    data = host.to(dev)
    stats = torch.zeros(3, device=dev)
    loss, grads, paths = _step(m, data, stats)
    _assert_fused(paths)
    with torch.no_grad():
        pre = m(data)
        _, pre_k = Fn.head_bce_logits(m.features(data), data.y, None, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, int(which == 'gnnml3'))
    _close(pre, pre64, 'pre')
    _close(pre_k.view(-1, 1), pre64, 'pre (kernel)')
    _close(loss, loss64, 'loss')
    for k, gk in grads.items():
        _close(gk, P64[k].grad, 'grad ' + k)
    ok = float(((pre64[:, 0] > 0) == (host.y == 1)).sum())
    assert stats.tolist() == [float(loss), ok, float(len(ids))]
    # five Adam steps (exp_classify.py:315): the loss trajectory
    from gnn_matlang_amd import models
    D64 = _params(state, torch.float64, dev)
    names = list(D64)
    opt, ropt = torch.optim.Adam(m.parameters(), lr=1e-3), torch.optim.Adam([D64[k] for k in names], lr=1e-3)
    got, want = [], []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        l = models.exp_classify_step_loss(m, data)
        l.backward()
        opt.step()
        got.append(l.detach().double())
        ropt.zero_grad(set_to_none=True)
        _, lr_ = _oracle(which, D64, data, torch.float64)
        lr_.backward()
        ropt.step()
        want.append(lr_.detach())
    got, want = torch.stack(got), torch.stack(want)
    print('trajectory', got.tolist(), want.tolist())
    assert float(((got - want).abs() / want.abs()).max()) <= TOL, (got.tolist(), want.tolist())


# ------------------------------------------------------------------ 4. padded static batch = plain batch
@pytest.fixture(scope='module')
def exp_dd(dev, exp_graphs):
    from gnn_matlang_amd.dataset import DeviceDataset
    out = []
    for gs in exp_graphs:
        dd = DeviceDataset.from_graphs(gs, dev)
        dd.y = dd.y.float()
        out.append(dd)
    return out                                                 # [train (32 graphs), val (8 graphs)]


@pytest.mark.parametrize('which', ['gnnml3', 'gnnml1'])
def test_padded_static_batch_equals_the_plain_batch(dev, exp_graphs, which):
    """16 train graphs; 6 of them + 2 absent slots through batch_assembled against the plain batch of the same 6"""
    from gnn_matlang_amd.dataset import DeviceDataset
    dd = DeviceDataset.from_graphs(exp_graphs[0][:16], dev)
    dd.y = dd.y.float()
    G = len(dd)
    sl = [5, G, 0, 11, 3, G, 14, 2]
    bd = dd.bounds(8)
    bs = dd.batch_assembled(torch.tensor(sl, device=dev), bd, adjacency=(which == 'gnnml1'), groups64=True)
    bp = dd.batch(torch.tensor([i for i in sl if i < G], device=dev))
    torch.manual_seed(4)
    mp = _model(which, dev)
    ms = copy.deepcopy(mp)
    sp, ss = torch.zeros(3, device=dev), torch.zeros(3, device=dev)
    lp, gp, pp = _step(mp, bp, sp)
    ls, gs, ps = _step(ms, bs, ss)
    _assert_fused(pp)
    _assert_fused(ps)
    _close(ls, lp, 'loss')
    for k in gp:
        _close(gs[k], gp[k], 'grad ' + k)
    assert float(ss[1]) == float(sp[1]) and float(ss[2]) == float(sp[2]) == 6.0, (ss.tolist(), sp.tolist())
    _close(ss[0], sp[0], 'stats.loss')


@pytest.mark.parametrize('which', ['gnnml3', 'gnnml1'])
def test_torch_op_road_gives_the_same_step(dev, exp_dd, which, monkeypatch):
    """GML_NO_HEAD_BCE sends the step to the torch-op road (what an unsupported head takes): same loss, gradients and stats on a plain
    and on a padded batch, and the recorded path says so"""
    dd = exp_dd[0]
    G = len(dd)
    plain = dd.batch(torch.arange(6, device=dev))
    padded = dd.batch_assembled(torch.tensor([0, 1, G, 2, 3, 4, 5, G], device=dev), dd.bounds(8), adjacency=(which == 'gnnml1'), groups64=True)
    torch.manual_seed(8)
    m = _model(which, dev)
    for data in (plain, padded):
        sf, st = torch.zeros(3, device=dev), torch.zeros(3, device=dev)
        lf, gf, pf = _step(m, data, sf)
        monkeypatch.setenv('GML_NO_HEAD_BCE', '1')
        lt, gt, pt = _step(m, data, st)
        monkeypatch.delenv('GML_NO_HEAD_BCE')
        _assert_fused(pf)
        assert any(k.startswith('head: torch ops') for k in pt) and not any('fused BCE head' in k for k in pt), pt
        _close(lf, lt, 'loss')
        for k in gf:
            _close(gf[k], gt[k], 'grad ' + k)
        _close(sf[0], st[0], 'stats.loss')
        assert sf[1:].tolist() == st[1:].tolist() and float(sf[2]) == 6.0


# ------------------------------------------------------------------ 5. evaluation
@pytest.mark.parametrize('which', ['gnnml3', 'gnnml1'])
def test_evaluation_under_no_grad(dev, exp_dd, which):
    from gnn_matlang_amd import models
    data = exp_dd[1].batch(torch.arange(8, device=dev))
    torch.manual_seed(6)
    m = _model(which, dev)
    lt = models.exp_classify_step_loss(m, data)
    assert lt.requires_grad
    m.eval()
    stats = torch.zeros(3, device=dev)
    with torch.no_grad():
        le = models.exp_classify_step_loss(m, data, stats=stats)
        pre = m(data)
    assert not le.requires_grad and torch.equal(le, lt.detach()), (float(le), float(lt))
    ok = float(((pre[:, 0] > 0) == (data.y == 1)).sum())
    assert stats.tolist() == [float(le), ok, 8.0]
    assert float(models.accuracy_from_stats(stats)) == ok / 8.0


# ------------------------------------------------------------------ 6. captured epochs = eager epochs
BS = 8


def _epochs(which, dd_train, dd_val, dev, captured, epochs=2):
    """`epochs` epochs of 4 train steps + 1 eval forward at batch 8 (batch_assembled inside the step, OneLaunchAdam), eagerly or as one
    captured train step and one captured eval forward replayed per batch: (per-batch losses, train / val stats per epoch, parameters)"""
    from gnn_matlang_amd import models
    from gnn_matlang_amd.optim import OneLaunchAdam
    torch.manual_seed(13)
    m = _model(which, dev)
    opt = OneLaunchAdam(m.parameters(), lr=1e-3)
    adj = which == 'gnnml1'
    bounds = [dd.bounds(BS) for dd in (dd_train, dd_val)]
    for dd in (dd_train, dd_val):
        dd.prepare()
    ids_t, ids_v = (torch.zeros(BS, dtype=torch.int64, device=dev) for _ in range(2))
    loss_t, loss_v = (torch.zeros((), device=dev) for _ in range(2))
    stats_t, stats_v = (torch.zeros(3, device=dev) for _ in range(2))

    def train_step():
        b = dd_train.batch_assembled(ids_t, bounds[0], adjacency=adj, groups64=True)
        opt.zero_grad(set_to_none=True)
        l = models.exp_classify_step_loss(m, b, stats=stats_t)
        l.backward()
        opt.step()
        loss_t.copy_(l.detach())

    def eval_step():
        with torch.no_grad():
            b = dd_val.batch_assembled(ids_v, bounds[1], adjacency=adj, groups64=True)
            loss_v.copy_(models.exp_classify_step_loss(m, b, stats=stats_v))
    run_t, run_v = train_step, eval_step
    if captured:
        snap = {k: v.clone() for k, v in m.state_dict().items()}
        ids_t.copy_(torch.arange(BS, device=dev))
        ids_v.copy_(torch.arange(BS, device=dev))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                train_step()
                eval_step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        gt, gv = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(gt):
            train_step()
        with torch.cuda.graph(gv):
            eval_step()
        with torch.no_grad():                                  # back to the initial state: the warm-up and capture steps trained
            for k, v in m.state_dict().items():
                v.copy_(snap[k])
            for st in opt.state.values():
                st['exp_avg'].zero_()
                st['exp_avg_sq'].zero_()
                st['step'].zero_()
        torch.cuda.synchronize()
        run_t, run_v = gt.replay, gv.replay
    gen = torch.Generator().manual_seed(5)
    losses, sums = [], []
    for _ in range(epochs):
        stats_t.zero_()
        stats_v.zero_()
        perm = torch.randperm(len(dd_train), generator=gen).to(dev)
        for i in range(0, perm.numel(), BS):
            ids_t.copy_(perm[i:i + BS])
            run_t()
            losses.append(loss_t.clone())
        ids_v.copy_(torch.arange(BS, device=dev))
        run_v()
        losses.append(loss_v.clone())
        sums.append(torch.cat([stats_t, stats_v]).cpu())       # the epoch's one read
    torch.cuda.synchronize()
    return torch.stack(losses).cpu(), torch.stack(sums), {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


@pytest.mark.parametrize('which', ['gnnml3', 'gnnml1'])
def test_captured_epochs_equal_eager_epochs(dev, exp_dd, which):
    """two epochs over 32 train and 8 val graphs: per-batch losses, the epoch sums of train and val and the final parameters, bitwise"""
    le, se, pe = _epochs(which, exp_dd[0], exp_dd[1], dev, captured=False)
    lc, sc, pc = _epochs(which, exp_dd[0], exp_dd[1], dev, captured=True)
    print('eager', le.tolist(), 'captured', lc.tolist(), 'sums', se.tolist())
    assert torch.isfinite(le).all() and le.numel() == 2 * (NTRAIN // BS + 1)
    assert torch.equal(le, lc) and torch.equal(se, sc)
    assert se[:, 2].tolist() == [float(NTRAIN)] * 2 and se[:, 5].tolist() == [float(NVAL)] * 2
    # the sums are the per-batch losses added in order (float32, as the kernel adds them)
    tr = le.view(2, -1)[:, :-1]
    acc = torch.zeros(2)
    for j in range(tr.size(1)):
        acc = acc + tr[:, j]
    assert torch.equal(se[:, 0], acc) and torch.equal(se[:, 3], le.view(2, -1)[:, -1])
    for k in pe:
        assert torch.equal(pe[k], pc[k]), k
