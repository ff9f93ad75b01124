"""The fused GNNML1 block for inputs up to 144 wide and its tanh-factor form (csrc/gml_gnnml1_wide.hip), and the six GNNML1 models
built on it (Zinc12k.py, counting.py, freqclass.py, ptc.py, enzymes.py, proteins.py): block and models against float64 restatements
written out here in plain torch, bitwise repeatability, the composition outside the kernel's range, dropout, and captured epochs.

Tolerance: the project's 2e-5 of each tensor's scale for exact fp32 products (tests/test_gpu_parity.py: close).  A case listed in
COMPUTED_TOL takes instead 4 x the error of the SAME restatement evaluated by torch in float32 on the CPU against float64 (floor
2e-5; the factor 4: a different summation order) -- a bound from the number format, never from the code under test."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _gnnml1_ref as R
from _gnnml1_ref import TOL, block_case as _block_case, block_cpu as _block_cpu, block_gpu as _block_gpu
from conftest import GOLDEN, rel_err

pytestmark = pytest.mark.gpu

COMPUTED_TOL = set()                                       # ids of the cases whose bound is computed from the float32 restatement


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    from gnn_matlang_amd import _lib
    assert _lib.lib().gml_version() >= 1
    return torch.device('cuda:0')


def _check(got, ref64, ref32, what, case):
    R.check(got, ref64, ref32, what, case, TOL, computed=case in COMPUTED_TOL)


# ------------------------------------------------------------------------------------------------ the block (restated in _gnnml1_ref)
SHAPES = [(130, 65, 16, 16, 16, 1, 1),       # first width past the old limit, unaligned rows
          (300, 96, 32, 32, 32, 1, 1),       # counting / freqclass
          (300, 98, 32, 64, 2, 3, 1),        # ptc: 98 % 4 != 0, n3 = 2
          (300, 144, 64, 64, 16, 2, 1),      # proteins
          (17, 144, 64, 64, 64, 2, 0),       # the LDS limit, one partial tile
          (1, 80, 10, 20, 7, 1, 0)]


@pytest.mark.parametrize('unit', [True, False], ids=['ones', 'values'])
@pytest.mark.parametrize('N,Fin,n1,n2,n3,mode,act', SHAPES)
def test_wide_block_vs_fp64(dev, N, Fin, n1, n2, n3, mode, act, unit):
    """one block forward and backward -- output, dx and all eight parameter gradients -- against the restatement in float64"""
    case = 'block-%d-%d-%d-%d-%d-m%d-%s' % (N, Fin, n1, n2, n3, mode, 'ones' if unit else 'values')
    ei, val, x, W, gout = _block_case(N, Fin, n1, n2, n3, mode, unit)
    y64, dx64, dW64 = _block_cpu(x, ei, val, W, gout, mode, act, torch.float64)
    y32, dx32, dW32 = _block_cpu(x, ei, val, W, gout, mode, act, torch.float32)
    y, dx, dW = _block_gpu(dev, x, ei, val, W, gout, mode, act, unit)
    _check(y, y64, y32, 'out', case)
    _check(dx, dx64, dx32, 'dx', case)
    for k in W:
        _check(dW[k], dW64[k], dW32[k], k, case)


def test_wide_block_without_dx(dev):
    """x.requires_grad == False: the backward's null-dx path (no transposed weight image) still gives the parameter gradients"""
    N, Fin, n1, n2, n3, mode, act = SHAPES[1]
    ei, val, x, W, gout = _block_case(N, Fin, n1, n2, n3, mode, True)
    y64, _, dW64 = _block_cpu(x, ei, val, W, gout, mode, act, torch.float64)
    y32, _, dW32 = _block_cpu(x, ei, val, W, gout, mode, act, torch.float32)
    y, dx, dW = _block_gpu(dev, x, ei, val, W, gout, mode, act, True, need_dx=False)
    assert dx is None
    _check(y, y64, y32, 'out', 'block-nodx')
    for k in W:
        _check(dW[k], dW64[k], dW32[k], k, 'block-nodx')


def test_mode3_is_not_mode2(dev):
    """the ptc shape: mode 3's third part is tanh(f2) tanh(f3) whatever `act` says, and differs from mode 2 / relu there"""
    N, Fin, n1, n2, n3, _, act = SHAPES[2]
    ei, val, x, W, gout = _block_case(N, Fin, n1, n2, n3, 3, True)
    y3, _, _ = _block_gpu(dev, x, ei, val, W, gout, 3, act, True)
    y2, _, _ = _block_gpu(dev, x, ei, val, W, gout, 2, act, True)
    assert torch.equal(y3[:, :n1 + n2], y2[:, :n1 + n2])
    assert not torch.equal(y3[:, n1 + n2:], y2[:, n1 + n2:])
    x64, W64 = x.double(), {k: v.double() for k, v in W.items()}
    f2, f3 = x64 @ W64['w2'].t() + W64['b2'], x64 @ W64['w3'].t() + W64['b3']
    third = torch.tanh(f2) * torch.tanh(f3)
    assert (third < 0).any()                                   # (no relu in it)
    assert rel_err(y3[:, n1 + n2:].cpu().double().numpy(), third.numpy()) <= TOL


def test_wide_block_repeats_bitwise(dev):
    """forward and backward twice on the 144-wide case: identical bits, weight gradients included (ordered folds, no float atomics)"""
    N, Fin, n1, n2, n3, mode, act = SHAPES[3]
    ei, val, x, W, gout = _block_case(N, Fin, n1, n2, n3, mode, False)
    a = _block_gpu(dev, x, ei, val, W, gout, mode, act, False)
    b = _block_gpu(dev, x, ei, val, W, gout, mode, act, False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in W:
        assert torch.equal(a[2][k], b[2][k]), k


# ------------------------------------------------------------------------------------------------ the models, restated
# (blocks, (n1, n2, n3), form, blocks followed by their BatchNorm, pools, head) as the scripts write them
SPEC = dict(zinc=(4, (16, 16, 16), 'product', (), ('add',), 'relu_mlp'),               # Zinc12k.py:294-307
            counting=(5, (32, 32, 32), 'product', (), ('add',), 'lin_mlp'),            # counting.py:318-333
            freqclass=(3, (32, 32, 32), 'product', (), ('mean',), 'relu_mlp'),         # freqclass.py:277-300
            ptc=(2, (32, 64, 2), 'tanh_factors', (1,), ('add', 'max'), 'relu_lsm'),    # ptc.py:310-321
            enzymes=(4, (16, 16, 16), 'factors', (1, 2, 3, 4), ('mean', 'max'), 'lsm'),    # enzymes.py:325-343
            proteins=(2, (64, 64, 16), 'factors', (), ('mean', 'max'), 'lsm'))         # proteins.py:247-257


def _model_ref(P, spec, x, ei, ptr):
    """the script's forward (dropout 0, training mode: BatchNorm on batch statistics) in plain torch, in the dtype of x and P"""
    nblocks, _, form, bn_after, pools, head = spec
    ones = torch.ones(ei.size(1), 1, dtype=x.dtype)
    for i in range(1, nblocks + 1):
        lin = lambda j: F.linear(x, P['fc%d%d.weight' % (i, j)], P['fc%d%d.bias' % (i, j)])
        h = torch.zeros_like(x).index_add_(0, ei[1], ones * x[ei[0]])
        c = h @ P['conv%d1.weight' % i][0] + P['conv%d1.bias' % i]
        f2, f3 = lin(2), lin(3)
        third = {'product': lambda: F.relu(f2 * f3), 'factors': lambda: F.relu(f2) * F.relu(f3),
                 'tanh_factors': lambda: torch.tanh(f2) * torch.tanh(f3)}[form]()
        x = torch.cat([F.relu(lin(1)), F.relu(c), third], 1)
        if i in bn_after:
            x = F.batch_norm(x, None, None, P['bn%d.weight' % i], P['bn%d.bias' % i], training=True)
    seg = [x[ptr[g]:ptr[g + 1]] for g in range(len(ptr) - 1)]
    pool = dict(add=lambda s: s.sum(0), mean=lambda s: s.mean(0), max=lambda s: s.max(0).values)
    x = torch.cat([torch.stack([pool[p](s) for s in seg]) for p in pools], 1)
    if head in ('relu_mlp', 'relu_lsm'):
        x = F.relu(F.linear(x, P['fc1.weight'], P['fc1.bias']))
    elif head == 'lin_mlp':
        x = F.linear(x, P['fc1.weight'], P['fc1.bias'])
    x = F.linear(x, P['fc2.weight'], P['fc2.bias'])
    return F.log_softmax(x, 1) if head.endswith('lsm') else x


def _loss_ref(name, pre, y):
    if name in ('zinc',):
        return (pre[:, 0] - y).abs().sum()                      # Zinc12k.py:365
    if name == 'counting':
        return torch.square(pre - y.view(-1, 1)).sum()          # counting.py:411
    if name == 'freqclass':
        return F.binary_cross_entropy(torch.sigmoid(pre[:, 0]), y, reduction='sum')
    return F.nll_loss(pre, y.long(), reduction='sum')


def _with_degree(graphs):
    """the scripts' DegreeMaxEigTransform(adddegree=True): the node degree as one more feature column"""
    out = []
    for x, ei, y in graphs:
        deg = np.bincount(ei[0], minlength=x.shape[0]).astype(np.float32)
        out.append(dict(x=np.concatenate((x, deg[:, None]), 1), edge_index=ei, y=y))
    return out


_HOST = {}


def _host_batch(name):
    """8 graphs per model, collated once on the host and shared by the tests"""
    from gnn_matlang_amd import collate, readers, synthetic
    key = name
    if key not in _HOST:
        if key in ('ptc', 'enzymes'):
            gs = _with_degree(readers.load_tu(os.path.join(GOLDEN, 'raw', key + '.mat'), key)[:8])
        elif key == 'proteins':                                 # the enzymes batch (4 input features), its six classes folded to two
            gs = [dict(g, y=g['y'] % 2) for g in _with_degree(readers.load_tu(os.path.join(GOLDEN, 'raw', 'enzymes.mat'), 'enzymes')[:8])]
        elif key == 'zinc':
            gs = [dict(x=x, edge_index=ei, y=y) for x, ei, y in synthetic.make_graphs('zinc', 8, seed=3)]
        elif key == 'counting':
            gs = _with_degree(synthetic.make_graphs('counting', 8, seed=3))       # counting.py: a constant feature and the degree
        else:                                                   # freqclass: one feature, a 0 / 1 label
            gs = [dict(x=np.random.default_rng(i).random((x.shape[0], 1), dtype=np.float32), edge_index=ei, y=np.float32(i % 2))
                  for i, (x, ei, y) in enumerate(synthetic.make_graphs('counting', 8, seed=4))]
        _HOST[key] = collate(gs)
    return _HOST[key]


def _factory(name, **kw):
    from gnn_matlang_amd import models
    return getattr(models, name + '_gnnml1')(**kw)


def _model_loss(name, m, data):
    from gnn_matlang_amd import models
    if name == 'zinc':
        return models.zinc_step_loss(m, data)
    if name == 'counting':
        return models.counting_loss(m(data), data.y)
    if name == 'freqclass':
        return models.exp_classify_step_loss(m, data)
    return models.tu_step_loss(m, data)


NINP = dict(zinc=25, counting=2, freqclass=1, ptc=20, enzymes=4, proteins=4)


@pytest.mark.parametrize('name', sorted(SPEC))
def test_models_vs_fp64(dev, name):
    """each factory's output, loss and every parameter gradient (dropout 0, training mode) against the script's forward restated in
    float64; every block after the first reads a concatenation wider than the first block's input and runs on the fused kernel"""
    from gnn_matlang_amd import functional as Fn
    case = 'model-' + name
    host = _host_batch(name)
    assert host.x.size(1) == NINP[name]
    torch.manual_seed(3)
    kw = {} if name in ('zinc', 'counting') else dict(dropout=0.0)
    m = _factory(name, **kw).to(dev).train()
    if name == 'counting':                                      # five add-aggregating blocks with a product each: keep the values in range
        with torch.no_grad():
            for q in m.parameters():
                q.mul_(0.5)
    data = host.to(dev)
    n1, n2, n3 = SPEC[name][1]
    mode = {'product': 1, 'factors': 2, 'tanh_factors': 3}[SPEC[name][2]]
    for fin in (NINP[name], n1 + n2 + n3):                      # the road of every block: fused
        assert Fn.gnnml1_block_supported(data.x, fin, n1, n2, n3, mode), fin
    pre = m(data)
    loss = _model_loss(name, m, data)
    loss.backward()
    ref = {}
    for dt in (torch.float64, torch.float32):
        P = {k: v.detach().cpu().to(dt).requires_grad_(v.dtype.is_floating_point) for k, v in m.state_dict().items()}
        pr = _model_ref(P, SPEC[name], host.x.to(dt), host.edge_index, host.ptr.tolist())
        lr = _loss_ref(name, pr, host.y.to(dt))
        lr.backward()
        ref[dt] = (pr.detach(), lr.detach(), P)
    p64, l64, P64 = ref[torch.float64]
    p32, l32, P32 = ref[torch.float32]
    _check(pre, p64, p32, 'output', case)
    _check(loss.reshape(1), l64.reshape(1), l32.reshape(1), 'loss', case)
    called = [n for n, q in m.named_parameters() if P64[n].grad is not None]
    assert called and all(('bn' in n) for n, q in m.named_parameters() if n not in called)     # only declared-never-called BatchNorms
    for n, q in m.named_parameters():
        if n in called:
            _check(q.grad, P64[n].grad, P32[n].grad, 'grad ' + n, case)
        else:
            assert q.grad is None, n


# ------------------------------------------------------------------------------------------------ outside the kernel's range
@pytest.mark.parametrize('widths', [(64, 64, 17), (16, 16, 65)], ids=['Fin145', 'n3_65'])
def test_outside_the_range_runs_on_the_composition(dev, widths):
    """gml_gnnml1_supported is false for Fin = 145 and for n3 = 65; a model at such widths runs (composition road) and matches the
    restatement.  The composition's conv runs on the general SpectConv kernels: their documented bound, the project's 1e-4."""
    from gnn_matlang_amd import functional as Fn, models
    host = _host_batch('enzymes')
    data = host.to(dev)
    n1, n2, n3 = widths
    assert not Fn.gnnml1_block_supported(data.x, 145, 64, 64, 16, 2)
    assert not Fn.gnnml1_block_supported(data.x, 64, 64, 64, 65, 2)
    assert Fn.gnnml1_block_supported(data.x, 144, 64, 64, 64, 2)
    assert not Fn.gnnml1_block_supported(data.x, n1 + n2 + n3, n1, n2, n3, 2)
    torch.manual_seed(4)
    m = models.GNNML1Blocks(4, widths, 2, form='factors', pool=('mean', 'max'), head='log_softmax', nclass=6).to(dev).train()
    pre = m(data)
    P = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    p64 = _model_ref(P, (2, widths, 'factors', (), ('mean', 'max'), 'lsm'), host.x.double(), host.edge_index, host.ptr.tolist())
    e = rel_err(pre.detach().cpu().double().numpy(), p64.numpy())
    print('outside %s: err %.3e' % (widths, e))
    assert e <= 1e-4


# ------------------------------------------------------------------------------------------------ every form through the one class
_FORMS = ('sum', 'product', 'factors', 'tanh_factors', 'sum_factors')


def _small_batch():
    """3 graphs of 13 nodes, 5 random features (rows not float4-addressable), labels 0 / 1 / 2"""
    from gnn_matlang_amd import collate, synthetic
    if 'small' not in _HOST:
        _HOST['small'] = collate([dict(x=np.random.default_rng(i).standard_normal((x.shape[0], 5)).astype(np.float32), edge_index=ei, y=i % 3)
                                  for i, (x, ei, y) in enumerate(synthetic.make_graphs('counting', 3, seed=5, nmin=13, nmax=13))])
    return _HOST['small']


@pytest.mark.parametrize('act', ['tanh', 'relu'])
@pytest.mark.parametrize('form', _FORMS)
def test_every_form_fused_against_composed(dev, monkeypatch, form, act):
    """GNNML1Blocks of two blocks in each form: loss and every parameter gradient on the fused road (both blocks through
    GNNML1BlockFunction; the second reads 16, 48 or 24 features) against the composition road of the same process
    (GML_NO_GNNML1_FUSED=1, read at call time), at the bound for exact fp32 products"""
    from gnn_matlang_amd import functional as Fn, models
    data = _small_batch().to(dev)
    assert tuple(data.x.shape) == (39, 5)
    widths = (16, 16, 8) if form == 'sum_factors' else (16, 16, 16)
    torch.manual_seed(7)
    m = models.GNNML1Blocks(5, widths, 2, form=form, act=act, pool='add', head='log_softmax', nclass=3).to(dev).train()
    calls, apply = [], Fn.GNNML1BlockFunction.apply
    monkeypatch.setattr(Fn.GNNML1BlockFunction, 'apply', lambda *a: (calls.append(a[11]), apply(*a))[1])

    def run():
        m.zero_grad(set_to_none=True)
        loss = models.tu_step_loss(m, data)
        loss.backward()
        return dict([('loss', loss.detach().reshape(1).clone())] + [(n, q.grad.clone()) for n, q in m.named_parameters()])
    fused = run()
    assert calls == [models.GNNML1Blocks._MODES[form]] * 2
    monkeypatch.setenv('GML_NO_GNNML1_FUSED', '1')
    composed = run()
    assert len(calls) == 2                                      # the composition road: the fused function not at all
    assert len(fused) == 1 + 8 * 2 + 2
    for k in composed:
        e = rel_err(fused[k].cpu().double().numpy(), composed[k].cpu().double().numpy())
        print('%s %s %s: fused against composed %.3e' % (form, act, k, e))
        assert e <= TOL, (form, act, k, e)


# ------------------------------------------------------------------------------------------------ dropout
@pytest.mark.parametrize('name', ['freqclass', 'ptc', 'enzymes'])
def test_dropout_eval_is_the_plain_model_and_training_is_not(dev, name):
    from gnn_matlang_amd import models
    data = _host_batch(name).to(dev)
    torch.manual_seed(6)
    a = _factory(name, dropout=0.0).to(dev)
    b = _factory(name).to(dev)
    assert b.dropout > 0 and 'dropout_state' not in dict(a.named_buffers())
    b.load_state_dict(a.state_dict())
    a.eval()
    b.eval()
    st = b.dropout_state.clone()
    with torch.no_grad():
        assert torch.equal(a(data), b(data))
    assert torch.equal(b.dropout_state, st)                     # eval: the counter does not move
    a.train()
    b.train()
    with torch.no_grad():
        ya, yb = a(data), b(data)
    assert int(b.dropout_state[1]) == int(st[1]) + 1
    assert torch.isfinite(yb).all() and not torch.equal(ya, yb)


# ------------------------------------------------------------------------------------------------ captured epochs
BS = 8


def _enzymes_dataset(dev):
    from gnn_matlang_amd import SpectralDesign, readers
    from gnn_matlang_amd.dataset import DeviceDataset
    raw = readers.load_tu(os.path.join(GOLDEN, 'raw', 'enzymes.mat'), 'enzymes')[:28]
    dd = DeviceDataset.from_graphs(SpectralDesign(recfield=1, dv=2, nfreq=2, adddegree=True).design_many(raw), dev)
    dd.y = dd.y.float()
    return dd


class _Ids(object):
    pass


def _train(dd, dev, captured, epochs=2):
    from gnn_matlang_amd import models
    from gnn_matlang_amd.dist import TrainStep
    from gnn_matlang_amd.optim import OneLaunchAdam
    torch.manual_seed(21)
    m = models.enzymes_gnnml1().to(dev).train()
    assert m.dropout == 0.1
    opt = OneLaunchAdam(m.parameters(), lr=1e-3)
    bd = dd.bounds(BS)
    dd.prepare()
    data = _Ids()
    data.ids = torch.arange(BS, dtype=torch.int64, device=dev)
    ts = TrainStep(m, lambda mod, d: models.tu_step_loss(mod, dd.batch_assembled(d.ids, bd, adjacency=True)), opt)
    snap = {k: v.clone() for k, v in m.state_dict().items()}
    rng = m.dropout_state.clone()
    if captured:
        replay, loss = ts.capture(data)
    else:
        for _ in range(3):                                      # (the capture's warm-up steps: the optimiser state exists either way)
            ts.step(data)
    with torch.no_grad():                                       # back to the initial state: parameters, buffers, optimiser, RNG state
        for k, v in m.state_dict().items():
            v.copy_(snap[k])
        for st in opt.state.values():
            st['exp_avg'].zero_()
            st['exp_avg_sq'].zero_()
            st['step'].zero_()
        m.dropout_state.copy_(rng)
    torch.cuda.synchronize()
    G = len(dd)
    gen = torch.Generator().manual_seed(5)
    losses = []
    for _ in range(epochs):
        perm = torch.cat([torch.randperm(G, generator=gen), torch.full(((-G) % BS,), G, dtype=torch.int64)]).to(dev)
        for i in range(0, perm.numel(), BS):
            data.ids.copy_(perm[i:i + BS])
            if captured:
                replay()
                losses.append(loss.clone())
            else:
                losses.append(ts.step(data).clone())
    torch.cuda.synchronize()
    return torch.stack(losses).cpu(), {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def test_captured_enzymes_epochs_are_bitwise_equal_to_eager_epochs(dev):
    """enzymes_gnnml1 (four fused blocks, masked BatchNorm 48 wide, dropout 0.1) over static batches with the raw adjacency through
    dist.TrainStep: two epochs as ONE captured step replayed per batch equal the same epochs run eagerly -- per-batch losses, final
    parameters and BatchNorm buffers bit for bit (absent slots in the last batch of each epoch)"""
    dd = _enzymes_dataset(dev)
    le, se = _train(dd, dev, captured=False)
    lc, sc = _train(dd, dev, captured=True)
    assert torch.isfinite(le).all() and le.numel() == 2 * ((len(dd) + BS - 1) // BS)
    assert torch.equal(le, lc), (le - lc).abs().max()
    for k in se:
        assert torch.equal(se[k], sc[k]), k
    assert int(se['bn1.num_batches_tracked']) == le.numel()
