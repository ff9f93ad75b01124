"""The road of the head and loss on the device (functional.head_road, models._step_loss): every kind on the smallest batch that
reaches it.  For each case PATHS holds exactly the record's label, and loss, every parameter gradient and stats / loss_sum agree with
the same step on the 'torch' road (the override) within the tolerance the existing test of that head uses:
    L1    loss 1e-5 of its value, gradients 2e-5 (rel_err)      tests/test_gpu_parity.py:1067, :1069
    BCE   1e-4 (rel_err) on loss, gradients and stats.loss      tests/test_gpu_exp_classify.py:16, :25
    node  1e-4 (rel_err) on loss, gradients and stats           tests/test_gpu_filtering.py:15, :24
The fused heads sum in a fixed order: a second run gives the same bits."""
import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


def _cycle(n):
    i = np.arange(n)
    return np.vstack((np.concatenate([i, (i + 1) % n]), np.concatenate([(i + 1) % n, i]))).astype(np.int64) if n > 2 else np.array([[0, 1], [1, 0]])


def _grid(a, b):
    idx = np.arange(a * b).reshape(a, b)
    e = np.concatenate([np.stack([idx[:-1].ravel(), idx[1:].ravel()]), np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()])], 1)
    return np.concatenate([e, e[::-1]], 1).astype(np.int64)


_DESIGNED = {}


def _designed(kind, sizes, seed):
    """designed host graphs (cycles of the given sizes; the pair (2 nodes) is one edge) with random features and labels"""
    from gnn_matlang_amd import SpectralDesign
    key = (kind, tuple(sizes), seed)
    if key not in _DESIGNED:
        rng = np.random.default_rng(seed)
        if kind == 'zinc':                                   # Zinc12k.py: one-hot atom types, a regression target
            raw = [(np.eye(21, dtype=np.float32)[rng.integers(21, size=n)], _cycle(n), np.float32(rng.normal())) for n in sizes]
            design = SpectralDesign(recfield=2, dv=2, nfreq=7)
        elif kind == 'exp':                                  # exp_classify.py: a constant feature + the degree, a 0 / 1 label
            raw = [(np.ones((n, 1), dtype=np.float32), _cycle(n), np.float32(i % 2)) for i, n in enumerate(sizes)]
            design = SpectralDesign(nmax=64, recfield=1, dv=2, nfreq=5, adddegree=True)
        else:                                                # freqclass.py: one signal per node, a 0 / 1 label
            raw = [(rng.normal(size=(n, 1)).astype(np.float32), _cycle(n), np.float32(i % 2)) for i, n in enumerate(sizes)]
            design = SpectralDesign(recfield=2, dv=4, nfreq=5)
        _DESIGNED[key] = design.design_many(raw)
    return _DESIGNED[key]


def _batches(dev, kind, sizes, seed, adjacency=False):
    """(plain batch of all graphs, padded static batch of the same graphs plus one absent slot)"""
    from gnn_matlang_amd.dataset import DeviceDataset
    dd = DeviceDataset.from_graphs(_designed(kind, sizes, seed), dev)
    dd.y = dd.y.float()
    G = len(dd)
    ids = torch.arange(G, device=dev)
    return dd.batch(ids), dd.batch_padded(torch.cat([ids, torch.tensor([G], device=dev)]), dd.bounds(G + 1), adjacency=adjacency)


def _step(fn, m, data, state=None, **kw):
    """(loss, gradients, head PATHS keys) of one forward + backward through the step loss fn"""
    from gnn_matlang_amd import functional as Fn
    if state is not None:
        m.dropout_state.copy_(state)                         # (the same dropout masks for every road)
    old, Fn.VERBOSE = Fn.VERBOSE, True
    Fn.PATHS.clear()
    try:
        m.zero_grad(set_to_none=True)
        loss = fn(m, data, **kw)
        loss.backward()
        heads = sorted(k for k in Fn.PATHS if k.startswith('head:'))
    finally:
        Fn.VERBOSE = old
        Fn.PATHS.clear()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}, heads


def _agree(what, fused, torch_, tol_loss, tol):
    (lf, gf, _), (lt, gt, _) = fused, torch_
    e = abs(float(lf) - float(lt)) / max(abs(float(lt)), 1e-30)
    print('%-22s loss %.8g / %.8g rel %.2e' % (what, float(lf), float(lt), e))
    assert np.isfinite(float(lf)) and e <= tol_loss, (what, float(lf), float(lt))
    assert set(gf) == set(gt)
    for k in gt:
        e = rel_err(gf[k].cpu().numpy(), gt[k].cpu().numpy())
        print('%-22s grad %-18s rel %.2e' % (what, k, e))
        assert e <= tol, (what, k, e)


def _same_bits(a, b):
    assert torch.equal(a[0], b[0]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1]), 'a second run differs'


L1_TOL = dict(tol_loss=1e-5, tol=2e-5)                      # tests/test_gpu_parity.py:1067, :1069
BCE_TOL = dict(tol_loss=1e-4, tol=1e-4)                     # tests/test_gpu_exp_classify.py:16
NODE_TOL = dict(tol_loss=1e-4, tol=1e-4)                    # tests/test_gpu_filtering.py:15


def _zinc(dev, data, seed=1):
    from gnn_matlang_amd import models
    torch.manual_seed(seed)
    return models.zinc_gnnml3(int(data.x.size(1)), int(data.edge_attr2.size(1))).to(dev)


@pytest.mark.parametrize('padded', [False, True])
def test_l1_small(dev, padded):
    """3 graphs of 4-6 nodes: the one workgroup; padded: 4 slots (one absent) + the padding graph, whose feature row gets a zero
    gradient from the head itself (pad_grad_zero)"""
    from gnn_matlang_amd import functional as Fn, models
    data = _batches(dev, 'zinc', (4, 5, 6), 3)[int(padded)]
    m = _zinc(dev, data)
    R, nl = int(data.ptr.numel()) - 1, 4 if padded else 3
    want = Fn.head_road('l1', models._MLP32, True, 32, 32, 1, R, nl, R)
    assert want == ('l1_small', True, 'fused L1 head, one workgroup (32 -> 32 -> 1)') and R == nl + int(padded)
    accf, acct = torch.zeros((), device=dev), torch.zeros((), device=dev)
    fused = _step(models.zinc_step_loss, m, data, loss_sum=accf)
    assert fused[2] == ['head: ' + want.label]
    torch_ = _step(models.zinc_step_loss, m, data, loss_sum=acct, _head_road='torch')
    assert torch_[2] == ['head: torch ops (L1 head outside the fused kernels)']
    _agree('l1_small', fused, torch_, **L1_TOL)
    assert float(accf) == float(fused[0]) and float(acct) == float(torch_[0])
    _same_bits(fused, _step(models.zinc_step_loss, m, data))
    if padded:
        # the padding graph's row: the head writes its zero gradient, the pool was told so and does not mask
        x = m.features(data, pad_grad_zero=True)
        x.retain_grad()
        Fn.HeadL1Function.apply(x, data.y[:nl].float().contiguous(), data.graph_valid, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias).backward()
        assert tuple(x.grad.shape) == (R, 32) and not x.grad[nl:].any() and x.grad[:nl - 1].any() and not x.grad[nl - 1].any()


@pytest.fixture(scope='module')
def many(dev):
    """257 graphs of 2-3 nodes: the first row count the one-workgroup head refuses"""
    return _batches(dev, 'zinc', [2 + i % 2 for i in range(257)], 5)[0]


@pytest.mark.parametrize('masked', [False, True])
def test_l1_big(dev, many, masked):
    from gnn_matlang_amd import functional as Fn, models
    m = _zinc(dev, many)
    assert int(many.ptr.numel()) - 1 == 257
    want = Fn.head_road('l1', models._MLP32, True, 32, 32, 1, 257, 257, 257)
    assert want == ('l1_big', False, 'fused L1 head, one pass + fold (32 -> 32 -> 1)')
    valid = (torch.arange(257, device=dev) % 3 != 0).float() if masked else None
    accf, acct = torch.zeros((), device=dev), torch.zeros((), device=dev)
    fused = _step(models.zinc_step_loss, m, many, valid=valid, loss_sum=accf)
    torch_ = _step(models.zinc_step_loss, m, many, valid=valid, loss_sum=acct, _head_road='torch')
    assert abs(float(accf) - float(fused[0])) <= L1_TOL['tol_loss'] * abs(float(fused[0])) and float(acct) == float(torch_[0])
    assert fused[2] == ['head: ' + want.label] and torch_[2] == ['head: torch ops (L1 head outside the fused kernels)']
    _agree('l1_big', fused, torch_, **L1_TOL)
    _same_bits(fused, _step(models.zinc_step_loss, m, many, valid=valid))


def _stats_agree(sf, st, tol):
    e = abs(float(sf[0]) - float(st[0])) / max(abs(float(st[0])), 1e-30)
    assert e <= tol and sf[1:].tolist() == st[1:].tolist(), (sf.tolist(), st.tolist())



@pytest.mark.parametrize('padded', [False, True])
def test_bce_and_its_torch_roads(dev, padded, monkeypatch):
    """exp_classify_gnnml3 on 3 graphs: the fused head; the torch ops by GML_NO_HEAD_BCE and by the override"""
    from gnn_matlang_amd import functional as Fn, models
    data = _batches(dev, 'exp', (4, 5, 6), 7)[int(padded)]
    torch.manual_seed(2)
    m = models.exp_classify_gnnml3(int(data.x.size(1)), int(data.edge_attr2.size(1))).to(dev)
    R, nl = int(data.ptr.numel()) - 1, 4 if padded else 3
    want = Fn.head_road('bce', models._MLP, True, 48, 10, 1, R, nl, R)
    assert want == ('bce', True, 'fused BCE head (48 -> 10 -> 1, relu)')
    sf, so, se = (torch.zeros(3, device=dev) for _ in range(3))
    fused = _step(models.exp_classify_step_loss, m, data, stats=sf)
    by_override = _step(models.exp_classify_step_loss, m, data, stats=so, _head_road='torch')
    monkeypatch.setenv('GML_NO_HEAD_BCE', '1')
    by_env = _step(models.exp_classify_step_loss, m, data, stats=se)
    monkeypatch.delenv('GML_NO_HEAD_BCE')
    assert fused[2] == ['head: ' + want.label]
    assert by_override[2] == by_env[2] == ['head: torch ops (BCE head outside the fused kernel)']
    _agree('bce', fused, by_override, **BCE_TOL)
    _stats_agree(sf, so, BCE_TOL['tol_loss'])
    assert float(sf[2]) == 3.0 and float(sf[0]) == float(fused[0])
    _same_bits(by_override, by_env)                          # the same ops either way
    assert torch.equal(so, se)
    _same_bits(fused, _step(models.exp_classify_step_loss, m, data))


def test_torch_by_width(dev):
    """freqclass_gnnml3: 66 inputs, beyond the BCE kernel's 64 -- the torch ops with or without the override"""
    from gnn_matlang_amd import functional as Fn, models
    data = _batches(dev, 'freq', (5, 6, 7), 9)[0]
    torch.manual_seed(3)
    m = models.freqclass_gnnml3(int(data.x.size(1)), int(data.edge_attr2.size(1))).to(dev).train()
    want = Fn.head_road('bce', models._MLP, True, 66, 32, 1, 3, 3, 3)
    assert want == ('torch', True, 'torch ops (BCE head outside the fused kernel)')
    state = m.dropout_state.clone()
    sa, sb = torch.zeros(3, device=dev), torch.zeros(3, device=dev)
    a = _step(models.freqclass_step_loss, m, data, state, stats=sa)
    b = _step(models.freqclass_step_loss, m, data, state, stats=sb, _head_road='torch')
    assert a[2] == b[2] == ['head: ' + want.label]
    _same_bits(a, b)
    assert torch.equal(sa, sb) and float(sa[2]) == 3.0 and np.isfinite(float(a[0]))
    assert int(m.dropout_state[1]) == int(state[1]) + 1       # one pass over the layers per step


def test_node(dev):
    """filtering_gnnml3 on a 4 x 4 grid: the node head with its R^2 sums"""
    from gnn_matlang_amd import SpectralDesign, collate, functional as Fn, models
    rng = np.random.default_rng(11)
    d = SpectralDesign(recfield=2, dv=10, nfreq=10).design_many([(rng.normal(size=(16, 1)).astype(np.float32), _grid(4, 4), 0)])[0]
    d['y'] = rng.normal(size=(16, 3)).astype(np.float32)
    d['mask'] = (rng.random((16, 1)) < 0.75).astype(np.float32)
    data = collate([d], node_fields=('y', 'mask')).to(dev)
    torch.manual_seed(4)
    m = models.filtering_gnnml3(1, int(data.edge_attr2.size(1))).to(dev)
    want = Fn.head_road('node_sq', models._NODE, True, 48, 0, 1, 16, 0, 1)
    assert want == ('node', False, 'fused node head (48 -> 1)')
    sf, st = torch.zeros(4, device=dev), torch.zeros(4, device=dev)
    fused = _step(models.filtering_step_loss, m, data, ntask=1, stats=sf)
    torch_ = _step(models.filtering_step_loss, m, data, ntask=1, stats=st, _head_road='torch')
    assert fused[2] == ['head: ' + want.label] and torch_[2] == ['head: torch ops (node head outside the fused kernel)']
    _agree('node', fused, torch_, **NODE_TOL)
    assert rel_err(sf.cpu().numpy(), st.cpu().numpy()) <= 1e-4 and float(sf[3]) == float(st[3]) == float(data.mask.sum())
    _same_bits(fused, _step(models.filtering_step_loss, m, data, ntask=1))


def test_unaligned_fc1_weight_takes_the_torch_ops(dev):
    """fc1.weight as a view 4 bytes into its storage: gml_head_l1_* answer GML_E_UNSUPPORTED for it (the step loss raised before the
    record); the record sends the step to the torch ops, with the loss and gradients of the aligned model on that road"""
    from gnn_matlang_amd import functional as Fn, models
    data = _batches(dev, 'zinc', (4, 5, 6), 3)[0]
    m = _zinc(dev, data)
    ref = _step(models.zinc_step_loss, m, data, _head_road='torch')
    buf = torch.empty(32 * 32 + 1, device=dev)
    w = buf[1:].view(32, 32)
    w.copy_(m.fc1.weight.detach())
    m.fc1.weight = torch.nn.Parameter(w)
    assert m.fc1.weight.data_ptr() % 16 == 4 and Fn.head_flags('l1', data.x, None, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias) == (True, False)
    got = _step(models.zinc_step_loss, m, data)
    assert got[2] == ['head: torch ops (L1 head outside the fused kernels)']
    _agree('unaligned fc1.weight', got, ref, **L1_TOL)
