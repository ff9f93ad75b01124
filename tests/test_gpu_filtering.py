"""The 2-D grid filtering experiment (filtering.py) on the device: the node-level readout / masked loss / R^2 kernel against
float64, the node-level GNNML3 on small grids on BOTH roads (large-graph dense blocks, sparse CSR) and on the real 900-node grid
against a float64 composition of the oracle layers, and captured epochs equal to eager ones."""
import os

import numpy as np
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


# ------------------------------------------------------------------ head / loss / R^2 kernel
@pytest.mark.parametrize('N', [1, 63, 900, 4099])
@pytest.mark.parametrize('nin', [1, 32, 48])
def test_node_head_against_float64(dev, N, nin):
    from gnn_matlang_amd import functional as Fn, models
    g = torch.Generator(device='cpu').manual_seed(100 * N + nin)
    x0 = torch.randn(N, nin, generator=g).to(dev)
    w0 = (torch.randn(1, nin, generator=g) * 0.3).to(dev)
    b0 = torch.randn(1, generator=g).to(dev)
    y = (torch.randn(N, 3, generator=g) + 2.0).to(dev)        # a mean well away from zero: ss_tot needs ybar first
    some = (torch.rand(N, 1, generator=g) < 0.7).float()
    for task, mask in ((0, some), (2, torch.ones(N, 1)), (1, torch.zeros(N, 1))):
        mask = mask.to(dev)
        x, w, b = (t.clone().requires_grad_(True) for t in (x0, w0, b0))
        stats = torch.full((4,), float('nan'), device=dev)
        loss, pre = Fn.NodeHeadLossFunction.apply(x, w, b, y, mask, task, stats)
        (loss * 1.5).backward()
        X, W, B = (t.detach().double().requires_grad_(True) for t in (x0, w0, b0))
        P = F.linear(X, W, B)
        yt, m = y.double()[:, task:task + 1], mask.double()
        L = torch.square(m * (P - yt)).sum()                  # filtering.py:320
        (L * 1.5).backward()
        sel = m[:, 0] == 1
        cnt = int(sel.sum())
        ss_res = torch.square(yt[sel] - P[sel]).sum()
        ss_tot = torch.square(yt[sel] - yt[sel].mean()).sum() if cnt else torch.zeros((), dtype=torch.float64)
        assert not pre.requires_grad
        _close(pre, P, 'pre')
        if cnt == 0:                                          # an all-zero mask: loss 0 and zero gradients, exactly
            assert float(loss.detach()) == 0.0 and stats.tolist() == [0.0, 0.0, 0.0, 0.0]
            assert not x.grad.any() and not w.grad.any() and not b.grad.any()
            continue
        _close(loss, L, 'loss')
        _close(stats[0], L, 'stats.loss')
        _close(stats[1], ss_res, 'stats.ss_res')
        if cnt > 1:
            _close(stats[2], ss_tot, 'stats.ss_tot')
            r2 = float((1 - ss_res / ss_tot).detach())
            assert abs(float(models.r2_from_stats(stats)) - r2) <= TOL * max(1.0, abs(r2))
        assert float(stats[3]) == cnt
        _close(x.grad, X.grad, 'dx')
        _close(w.grad, W.grad, 'dw')
        _close(b.grad, B.grad, 'db')
        loss2, pre2 = Fn.NodeHeadLossFunction.apply(x, w, b, y, mask, task, None)      # fixed-order sums: the same bits
        assert torch.equal(loss2, loss) and torch.equal(pre2, pre)


# ------------------------------------------------------------------ the model on both roads
def _grid(a, b):
    idx = np.arange(a * b).reshape(a, b)
    e = np.concatenate([np.stack([idx[:-1].ravel(), idx[1:].ravel()]), np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()])], 1)
    A = np.zeros((a * b, a * b), dtype=np.int64)
    A[e[0], e[1]] = A[e[1], e[0]] = 1
    r, c = np.where(A > 0)
    return np.vstack((r, c)).astype(np.int64)


_CACHE = {}


def _grid_batch(a, b, recfield):
    """a x b grid with random signals: collated host batch (designed once per module)"""
    key = (a, b, recfield)
    if key not in _CACHE:
        from gnn_matlang_amd import SpectralDesign, collate
        n = a * b
        rng = np.random.default_rng(7 * n + recfield)
        d = SpectralDesign(recfield=recfield, dv=10, nfreq=10).design_many([(rng.normal(size=(n, 1)).astype(np.float32), _grid(a, b), 0)])[0]
        d['y'] = rng.normal(size=(n, 3)).astype(np.float32)
        d['mask'] = (rng.random((n, 1)) < 0.75).astype(np.float32)
        _CACHE[key] = collate([d], node_fields=('y', 'mask'))
    return _CACHE[key]


def _oracle(state, data, ntask):
    """float64 composition of oracle.spect_conv_oracle.ml3layer_forward, fc2 and the masked loss on data's device:
    (pre, loss, parameters with requires_grad)"""
    from oracle import spect_conv_oracle as SO
    P = {k: v.detach().to(data.x.device).double().requires_grad_(True) for k, v in state.items()}
    x = data.x.double()
    ea = data.edge_attr2.double()
    for i in (1, 2, 3):
        lp = {k[len('conv%d.' % i):]: v for k, v in P.items() if k.startswith('conv%d.' % i)}
        x = SO.ml3layer_forward(x, data.edge_index2, ea, lp, False, 16)
    pre = F.linear(x, P['fc2.weight'], P['fc2.bias'])
    loss = torch.square(data.mask.double() * (pre - data.y.double()[:, ntask:ntask + 1])).sum()
    return pre, loss, P


def _run_road(m, data, road, ntask=1):
    """(pre, loss, gradients, recorded paths) of one forward + backward of the model on the given road"""
    from gnn_matlang_amd import functional as Fn, models
    old, Fn.VERBOSE = Fn.VERBOSE, True
    Fn.PATHS.clear()
    try:
        m.zero_grad(set_to_none=True)
        pre = m(data, _road=road)
        stats = torch.zeros(4, device=data.x.device)
        loss = models.filtering_step_loss(m, data, ntask, stats, _road=road)
        loss.backward()
        paths = dict(Fn.PATHS)
    finally:
        Fn.VERBOSE = old
        Fn.PATHS.clear()
    return pre.detach(), loss.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}, paths, stats


def _assert_road(paths, road):
    dense = [k for k in paths if k.startswith('dense: support product')]
    sparse = [k for k in paths if k.startswith('conv_fwd') or k.startswith('conv_bwd')]
    if road == 'dense':
        assert dense and not sparse, paths
        assert any('fwd' in k and 'large graph' in k for k in dense) and any('bwd' in k and 'large graph' in k for k in dense), paths
    else:
        assert sparse and not any(k.startswith('dense') for k in paths), paths


@pytest.mark.parametrize('a,b,recfield,fill_lo,fill_hi', [(10, 11, 5, 0.99, 1.0), (13, 13, 3, 0.17, 0.21)])
@pytest.mark.parametrize('road', ['dense', 'sparse'])
def test_model_on_small_grids(dev, a, b, recfield, fill_lo, fill_hi, road):
    from gnn_matlang_amd import models
    host = _grid_batch(a, b, recfield)
    n = a * b
    fill = host.edge_index2.size(1) / float(n * n)
    assert fill_lo <= fill <= fill_hi and host.edge_attr2.size(1) == 11, fill
    data = host.to(dev)
    torch.manual_seed(11)
    m = models.filtering_gnnml3(1, 11).to(dev)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    assert (m._road_of(data).kind == 'big') == (fill >= models.DENSE_BIG_MIN_FILL)         # the road the model takes by itself
    pre, loss, grads, paths, stats = _run_road(m, data, road)
    _assert_road(paths, road)
    pre_ref, loss_ref, P = _oracle(state, data, 1)
    loss_ref.backward()
    _close(pre, pre_ref, 'pre')
    _close(loss, loss_ref, 'loss')
    _close(stats[0], loss_ref, 'stats.loss')
    for k, gk in grads.items():
        _close(gk, P[k].grad, 'grad ' + k)
    # the road the model chooses by itself gives what the forced call gave, bit for bit
    own = 'dense' if m._road_of(data).kind == 'big' else 'sparse'
    if own == road:
        pre2, loss2, _, paths2, _ = _run_road(m, data, None)
        _assert_road(paths2, road)
        assert torch.equal(pre2, pre) and torch.equal(loss2, loss)
    # five Adam steps, lr 1e-3 (filtering.py:299): the loss trajectory
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    names = list(P)
    ropt = torch.optim.Adam([P[k] for k in names], lr=1e-3)
    got, want = [], []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        l = models.filtering_step_loss(m, data, 1, None, _road=road)
        l.backward()
        opt.step()
        got.append(l.detach().double())
        ropt.zero_grad(set_to_none=True)
        _, lr_, _ = _oracle_with(P, data, 1)
        lr_.backward()
        ropt.step()
        want.append(lr_.detach())
    got, want = torch.stack(got), torch.stack(want)
    print('trajectory', got.tolist(), want.tolist())
    assert float(((got - want).abs() / want.abs()).max()) <= TOL, (got.tolist(), want.tolist())


def _oracle_with(P, data, ntask):
    """_oracle on parameters that already exist (the trajectory's float64 copy, updated in place by its optimiser)"""
    from oracle import spect_conv_oracle as SO
    x = data.x.double()
    ea = data.edge_attr2.double()
    for i in (1, 2, 3):
        lp = {k[len('conv%d.' % i):]: v for k, v in P.items() if k.startswith('conv%d.' % i)}
        x = SO.ml3layer_forward(x, data.edge_index2, ea, lp, False, 16)
    pre = F.linear(x, P['fc2.weight'], P['fc2.bias'])
    return pre, torch.square(data.mask.double() * (pre - data.y.double()[:, ntask:ntask + 1])).sum(), P


# ------------------------------------------------------------------ the real grid
@pytest.fixture(scope='module')
def grid30(dev):
    from gnn_matlang_amd import SpectralDesign, collate, readers
    recs = readers.design_twodgrid(readers.load_twodgrid(os.path.join(GOLDEN, 'raw', 'TwoDGrid30.mat')),
                                   SpectralDesign(recfield=5, dv=10, nfreq=10))
    return [collate([r], node_fields=('y', 'mask')).to(dev) for r in recs]


def test_real_grid_forward_backward(dev, grid30):
    """one forward + backward on the 900-node fixture (323,220 mask entries, S = 11) on the dense road against the oracle"""
    from gnn_matlang_amd import models
    data = grid30[0]
    assert tuple(data.x.shape) == (900, 1) and data.edge_index2.size(1) == 323220 and data.edge_attr2.size(1) == 11
    torch.manual_seed(5)
    m = models.filtering_gnnml3(1, 11).to(dev)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    pre, loss, grads, paths, stats = _run_road(m, data, 'dense', ntask=0)
    _assert_road(paths, 'dense')
    pre_ref, loss_ref, P = _oracle(state, data, 0)
    loss_ref.backward()
    _close(pre, pre_ref, 'pre')
    _close(loss, loss_ref, 'loss')
    assert float(stats[3]) == 676
    for k, gk in grads.items():
        _close(gk, P[k].grad, 'grad ' + k)


def test_captured_epochs_equal_eager_epochs(dev, grid30):
    """dist.TrainStep(model, filtering_step_loss, opt).capture(data): five replayed epochs (train step on graph 0) against five
    eager ones from the same state -- losses, the four sums and the final parameters bitwise"""
    from gnn_matlang_amd import models
    from gnn_matlang_amd.dist import TrainStep
    from gnn_matlang_amd.optim import OneLaunchAdam
    data = grid30[0]

    def run(captured):
        torch.manual_seed(9)
        m = models.filtering_gnnml3(1, 11).to(dev).train()
        opt = OneLaunchAdam(m.parameters(), lr=1e-3)
        stats = torch.zeros(4, device=dev)
        ts = TrainStep(m, lambda mod, d: models.filtering_step_loss(mod, d, 0, stats), opt)
        snap = {k: v.clone() for k, v in m.state_dict().items()}
        if captured:
            replay, loss = ts.capture(data)
        else:
            for _ in range(3):                                # (the capture's warm-up steps: the optimiser state exists either way)
                ts.step(data)
        with torch.no_grad():                                 # back to the initial state: parameters and optimiser
            for k, v in m.state_dict().items():
                v.copy_(snap[k])
            for st in opt.state.values():
                st['exp_avg'].zero_()
                st['exp_avg_sq'].zero_()
                st['step'].zero_()
        torch.cuda.synchronize()
        losses, sums = [], []
        for _ in range(5):
            if captured:
                replay()
                losses.append(loss.clone())
            else:
                losses.append(ts.step(data).clone())
            sums.append(stats.clone())
        torch.cuda.synchronize()
        return torch.stack(losses).cpu(), torch.stack(sums).cpu(), {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}

    le, se, pe = run(False)
    lc, sc, pc = run(True)
    print('eager', le.tolist(), 'captured', lc.tolist())
    assert torch.equal(le, lc) and torch.equal(se, sc)
    assert le[-1] < le[0]                                     # it trains
    assert torch.equal(se[:, 0], le)
    for k in pe:
        assert torch.equal(pe[k], pc[k]), k
