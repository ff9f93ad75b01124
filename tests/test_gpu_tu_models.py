"""The TU GNNML3 models (ptc.py, enzymes.py, proteins.py) and GNNML1 with device dropout: a training step against the same layer
modules called by hand with the masks recomputed on the CPU (bitwise) and against a float64 CPU composition of the oracle layers
(1e-4 of each tensor's scale); dropout 0 / eval equal to a model without dropout; captured PTC epochs equal to eager ones."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT, rel_err
import _philox

pytestmark = pytest.mark.gpu

TOL = 1e-4
BS = 32                                                    # ptc.py:398
PTC_SD = dict(nmax=109, adddegree=True, recfield=1, dv=10, nfreq=10)       # ptc.py:16
ENZ_SD = dict(nmax=126, adddegree=True, recfield=1, dv=2, nfreq=4)         # enzymes.py:27
PRO_SD = dict(nmax=0, adddegree=True, recfield=1, dv=4, nfreq=3)           # proteins.py:27


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


def _designed(name):
    from gnn_matlang_amd import SpectralDesign, readers, synthetic
    if name == 'ptc':
        return SpectralDesign(**PTC_SD).design_many(readers.load_tu(os.path.join(GOLDEN, 'raw', 'ptc.mat'), 'ptc'))
    if name == 'enzymes':
        return SpectralDesign(**ENZ_SD).design_many(readers.load_tu(os.path.join(GOLDEN, 'raw', 'enzymes.mat'), 'enzymes')[:60])
    if name == 'proteins':                                 # PROTEINS-like: 3 one-hot feature columns, graphs under and over 80 nodes
        raw = synthetic.make_graphs('counting', 24, seed=11, nmin=12, nmax=150, p=0.05)
        rng = np.random.default_rng(12)
        raw = [(np.eye(3, dtype=np.float32)[rng.integers(3, size=x.shape[0])], ei, np.int64(i % 2)) for i, (x, ei, _) in enumerate(raw)]
        assert min(x.shape[0] for x, _, _ in raw) < 80 < max(x.shape[0] for x, _, _ in raw)
        return SpectralDesign(**PRO_SD).design_many(raw)
    raw = synthetic.make_graphs('mnist75', 16, seed=7)                # GNNML1 (mnist75.py): 2 features, 10 classes
    return [dict(x=x, edge_index=ei, y=y) for x, ei, y in raw]


def _ctor(name, **kw):
    from gnn_matlang_amd import models
    if name == 'gnnml1':
        return models.mnist75_gnnml1(2, dropout=kw.get('dropout', 0.1))
    return getattr(models, name + '_gnnml3')(**kw)


def _where(x, keep, p):
    keep = torch.from_numpy(keep).to(x.device)
    return torch.where(keep, x * torch.tensor(float(_philox.scale(p)), device=x.device), torch.zeros((), device=x.device))


def _by_hand(m, data, masks, p):
    """the model's forward from its own layer modules with the dropout masks applied by torch.where"""
    from gnn_matlang_amd import models
    from gnn_matlang_amd.functional import tall_linear
    x = data.x
    if getattr(m, 'form', None) == 'sum':
        csr = data.csr('edge_index')
        for i in (1, 2, 3):
            g = lambda n: getattr(m, n % i)
            x = _where(x, masks[i - 1], p)
            y = models._gnnml1_block(x, csr, g('fc%d1'), g('conv%d1'), g('fc%d2'), g('fc%d3'), 0, 1)
            assert y is not None
            x = y
        x = models.global_mean_pool(x, data)
        x = F.relu(tall_linear(m.bn1(x), m.fc1))
        return F.log_softmax(tall_linear(x, m.fc2), dim=1)
    for i in range(m.nlayers):
        x = _where(x, masks[i], p)
        x = getattr(m, 'conv%d' % (i + 1))(x, data.edge_index2, data.edge_attr2)
    x = torch.cat([models._POOLS[k](x, data) for k in m.pool], 1)
    if m.pool_bn is not None:
        x = getattr(m, m.pool_bn)(x)
    if hasattr(m, 'fc1'):
        x = F.relu(tall_linear(x, m.fc1))
    return F.log_softmax(tall_linear(x, m.fc2), dim=1)


def _oracle(params, host, masks, p, name, nlayers):
    """float64 CPU composition: oracle ML3 layers (or GNNML1 blocks) with the masks, mean / add pool of oracle/models_oracle.py, a
    max pool per graph, the head"""
    from oracle import spect_conv_oracle as SO, models_oracle as MO
    P = {k: v.detach().cpu().double().requires_grad_(v.dtype.is_floating_point) for k, v in params.items()}
    sc = float(_philox.scale(p))
    x = host.x.double()
    B = int(host.ptr.numel() - 1)
    if name == 'gnnml1':
        ones = torch.ones(host.edge_index.size(1), 1, dtype=torch.float64)
        for i in (1, 2, 3):
            x = torch.where(torch.from_numpy(masks[i - 1]), x * sc, torch.zeros((), dtype=torch.float64))
            lin = lambda j: F.linear(x, P['fc%d%d.weight' % (i, j)], P['fc%d%d.bias' % (i, j)])
            c = SO.spectconv_forward(x, host.edge_index, ones, P['conv%d1.weight' % i], P['conv%d1.bias' % i], selfconn=False)
            x = F.relu(lin(1) + c + lin(2) * lin(3))
        x = MO.global_mean_pool(x, host.batch, B)
        x = F.batch_norm(x, None, None, P['bn1.weight'], P['bn1.bias'], training=True)
        x = F.relu(F.linear(x, P['fc1.weight'], P['fc1.bias']))
        return F.log_softmax(F.linear(x, P['fc2.weight'], P['fc2.bias']), 1), P
    for i in range(nlayers):
        x = torch.where(torch.from_numpy(masks[i]), x * sc, torch.zeros((), dtype=torch.float64))
        lp = {k[len('conv%d.' % (i + 1)):]: v for k, v in P.items() if k.startswith('conv%d.' % (i + 1))}
        x = SO.ml3layer_forward(x, host.edge_index2, host.edge_attr2.double(), lp, 'conv1.fc1_1.weight' in P, lp['fc11.weight'].size(0) if 'fc11.weight' in lp else 0)
    ptr = host.ptr.tolist()
    mx = torch.stack([x[ptr[g]:ptr[g + 1]].max(0).values for g in range(B)])
    first = MO.global_add_pool(x, host.batch, B) if name == 'enzymes' else MO.global_mean_pool(x, host.batch, B)
    x = torch.cat([first, mx], 1)
    if name == 'enzymes':
        x = F.batch_norm(x, None, None, P['bn4.weight'], P['bn4.bias'], training=True)
    if 'fc1.weight' in P:
        x = F.relu(F.linear(x, P['fc1.weight'], P['fc1.bias']))
    return F.log_softmax(F.linear(x, P['fc2.weight'], P['fc2.bias']), 1), P


def _close(got, ref, what, tol=TOL):
    err = rel_err(got.detach().cpu().double().numpy(), ref.detach().double().numpy())
    assert err <= tol, (what, err)


@pytest.fixture(params=['default', 'f32'])
def arith(request):
    """the fused kernels' arithmetic: the default (backward products on the bf16x3 split) or exact f32 products everywhere"""
    from gnn_matlang_amd import functional as Fn
    old = Fn.F32_MFMA
    Fn.F32_MFMA = request.param == 'f32'
    yield request.param
    Fn.F32_MFMA = old


@pytest.mark.parametrize('name', ['ptc', 'enzymes', 'proteins', 'gnnml1'])
def test_training_step_with_dropout_against_the_masks(dev, name, arith):
    """(a) logits, loss and every gradient bitwise equal to the layer modules called by hand with the masks recomputed on the CPU from
    the state (counter read after the forward); (b) the same values within 1e-4 of each tensor's scale of a float64 CPU composition.
    One exception in the default arithmetic: the edge-branch weights' gradients (fc1_*, learnedge: ptc_gnnml3's 11 supports) are sums
    over every edge of bf16x3-split products and come within 3e-4 (1.8e-4 measured); with exact f32 products they meet 1e-4 too."""
    from gnn_matlang_amd import collate, models
    from gnn_matlang_amd.functional import dropout_threshold
    ds = _designed(name)[:BS]
    host = collate(ds)
    data = host.to(dev)
    torch.manual_seed(1)
    m = _ctor(name).to(dev).train()
    p = m.dropout
    assert p > 0
    ref = _ctor(name, dropout=0.0) if name == 'gnnml1' else models.GNNML3(
        m.conv1.conv1.weight.size(1), m.conv1.conv1.weight.size(0), m.conv1.conv1.weight.size(2), m.conv1.nout2, m.nlayers,
        learnedge=m.conv1.learnedge, pool=m.pool, head='log_softmax', nclass=m.fc2.weight.size(0),
        hidden=m.fc1.weight.size(0) if hasattr(m, 'fc1') else 0, pool_bn=m.pool_bn, chain=False)
    ref.load_state_dict(m.state_dict())
    ref = ref.to(dev).train()
    st0 = m.dropout_state.clone()
    pre = m(data)
    seed, ctr = (int(v) for v in m.dropout_state.cpu())
    assert ctr == int(st0[1]) + 1                          # one advance per training forward
    loss = models.tu_loss(pre, data.y)
    loss.backward()
    widths = [int(getattr(m, 'fc%d1' % i).weight.size(1)) for i in (1, 2, 3)] if name == 'gnnml1' else \
        [int(getattr(m, 'conv%d' % (i + 1)).conv1.weight.size(1)) for i in range(m.nlayers)]      # the input width of every layer
    N = int(data.x.size(0))
    masks = [_philox.keep_mask(N, w, p, seed, ctr, i) for i, w in enumerate(widths)]
    assert all(k.any() and (~k).any() for k in masks)
    pre_h = _by_hand(ref, data, masks, p)
    loss_h = models.tu_loss(pre_h, data.y)
    loss_h.backward()
    assert torch.equal(pre, pre_h)
    assert torch.equal(loss, loss_h)
    rp = dict(ref.named_parameters())
    for n, q in m.named_parameters():
        assert torch.equal(q.grad, rp[n].grad), n
    # (b)
    params = {k: v for k, v in m.state_dict().items()}
    pre_o, P = _oracle(params, host, masks, p, name, getattr(m, 'nlayers', 3))
    loss_o = F.nll_loss(pre_o, host.y.long(), reduction='sum')
    loss_o.backward()
    _close(pre, pre_o, 'logits')
    assert abs(loss.item() - loss_o.item()) <= TOL * abs(loss_o.item())
    for n, q in m.named_parameters():
        _close(q.grad, P[n].grad, 'grad ' + n, 3e-4 if arith == 'default' and '.fc1_' in n else TOL)
    assert dropout_threshold(p)[0] > 0


@pytest.mark.parametrize('name', ['ptc', 'enzymes', 'gnnml1'])
def test_dropout_zero_and_eval_match_a_model_without_dropout(dev, name):
    """dropout=0.0 in training, and eval mode with dropout > 0: outputs and gradients bitwise equal to the model built without the
    argument; no RNG state buffer for dropout 0"""
    from gnn_matlang_amd import collate, models
    data = collate(_designed(name)[:BS]).to(dev)
    plain = {'ptc': lambda: models.GNNML3(20, 11, 64, 16, 4, pool=('mean', 'max'), head='log_softmax', hidden=100, nclass=2),
             'enzymes': lambda: models.GNNML3(4, 5, 64, 0, 4, learnedge=False, pool=('add', 'max'), head='log_softmax', nclass=6,
                                              pool_bn='bn4'),
             'gnnml1': lambda: models.mnist75_gnnml1(2)}[name]
    for train, kw in ((True, dict(dropout=0.0)), (False, {})):
        torch.manual_seed(2)
        a = plain().to(dev).train(train)
        b = _ctor(name, **kw).to(dev).train(train)
        b.load_state_dict(a.state_dict())
        if kw:
            assert 'dropout_state' not in dict(b.named_buffers())
        else:
            st = b.dropout_state.clone()
        outs = []
        for mm in (a, b):
            pre = mm(data)
            models.tu_loss(pre, data.y).backward()
            outs.append((pre, {n: q.grad for n, q in mm.named_parameters()}))
        assert torch.equal(outs[0][0], outs[1][0])
        for n in outs[0][1]:
            assert torch.equal(outs[0][1][n], outs[1][1][n]), n
        if not kw:
            assert torch.equal(b.dropout_state, st)        # eval: the counter does not move


def test_padded_batch_readout(dev):
    """mean|max and add|max readouts over a padded static batch: the real graphs' rows equal the plain batch's; bn4 raises on a padded
    batch in training"""
    from gnn_matlang_amd import models
    from gnn_matlang_amd.dataset import DeviceDataset
    dd = DeviceDataset.from_graphs(_designed('ptc')[:40], dev)
    dd.y = dd.y.float()
    bd = dd.bounds(8)
    ids = torch.tensor([3, 1, 4, 1, 5, 9, 2, 40], device=dev)          # 40: an absent slot
    bp = dd.batch_assembled(ids, bd)
    plain = dd.batch(ids[:7])
    torch.manual_seed(5)
    m = models.ptc_gnnml3().to(dev).eval()
    with torch.no_grad():
        a, b = m(bp), m(plain)
    assert rel_err(a[:7].cpu().numpy(), b.cpu().numpy()) <= 1e-5
    l = models.tu_loss(a, bp.y, bp.graph_valid)
    assert torch.isfinite(l) and rel_err(l.item(), models.tu_loss(b, plain.y).item()) <= 1e-5
    e = models.enzymes_gnnml3(ninp=20, ne=11).to(dev).train()
    with pytest.raises(NotImplementedError):
        e(bp)


# ------------------------------------------------------------------ one captured PTC step replayed per batch
def _ptc_dataset(dev):
    from gnn_matlang_amd.dataset import DeviceDataset
    dd = DeviceDataset.from_graphs(_designed('ptc'), dev)
    dd.y = dd.y.float()
    return dd


def _perms(G, epochs, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.cat([torch.randperm(G, generator=gen), torch.full(((-G) % BS,), G, dtype=torch.int64)]) for _ in range(epochs)]


def _train(dd, dev, captured, dropout=0.2, epochs=2, probe=False):
    """(per-batch losses, final parameters) of `epochs` PTC epochs at batch 32 over batch_assembled batches with OneLaunchAdam,
    eagerly or as one captured step replayed per batch.  probe: also the losses of two replays on the same ids (no optimiser
    effect between them is needed: the masks differ)."""
    from gnn_matlang_amd import models
    from gnn_matlang_amd.optim import OneLaunchAdam
    torch.manual_seed(21)
    m = models.ptc_gnnml3(dropout=dropout).to(dev).train()
    opt = OneLaunchAdam(m.parameters(), lr=1e-3)
    bd = dd.bounds(BS)
    dd.prepare()
    ids_buf = torch.zeros(BS, dtype=torch.int64, device=dev)
    loss_buf = torch.zeros((), device=dev)

    def step():
        b = dd.batch_assembled(ids_buf, bd, groups64=True)
        opt.zero_grad(set_to_none=True)
        l = models.tu_step_loss(m, b)
        l.backward()
        opt.step()
        loss_buf.copy_(l.detach())
    run = step
    if captured:
        snap = {k: v.clone() for k, v in m.state_dict().items()}
        rng = m.dropout_state.clone() if dropout > 0 else None
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
        with torch.no_grad():                              # back to the initial state: parameters, optimiser AND the RNG state
            for k, v in m.state_dict().items():
                v.copy_(snap[k])
            for st in opt.state.values():
                st['exp_avg'].zero_()
                st['exp_avg_sq'].zero_()
                st['step'].zero_()
            if rng is not None:
                m.dropout_state.copy_(rng)
        torch.cuda.synchronize()
        run = graph.replay
    losses = []
    for perm in _perms(len(dd), epochs, 5):
        perm = perm.to(dev)
        for i in range(0, perm.numel(), BS):
            ids_buf.copy_(perm[i:i + BS])
            run()
            losses.append(loss_buf.clone())
    torch.cuda.synchronize()
    out = (torch.stack(losses).cpu(), {k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    if not probe:
        return out
    extra = []                                             # (after the final parameters are taken: these steps train too)
    ids_buf.copy_(torch.arange(BS, device=dev))
    for _ in range(2):
        run()
        extra.append(loss_buf.clone())
    return out + (torch.stack(extra).cpu(),)


def test_captured_ptc_epochs_are_bitwise_equal_to_eager_epochs(dev, tmp_path):
    """Two PTC epochs at batch 32, dropout 0.2, as ONE captured step (assembly, counter advance, forward with dropout, masked NLL,
    backward, OneLaunchAdam) replayed per batch vs the same epochs run eagerly: per-batch losses and final parameters bitwise equal,
    and again in a fresh process.  Dropout is active: two replays on the same ids differ, the trajectory differs from dropout 0."""
    dd = _ptc_dataset(dev)
    le, se = _train(dd, dev, captured=False)
    lc, sc, probe = _train(dd, dev, captured=True, probe=True)
    assert torch.isfinite(le).all() and le.numel() == 2 * ((len(dd) + BS - 1) // BS)
    assert torch.equal(le, lc), (le - lc).abs().max()
    for k in se:
        assert torch.equal(se[k], sc[k]), k
    assert probe[0] != probe[1]
    l0, _ = _train(dd, dev, captured=True, dropout=0.0)
    assert not torch.equal(l0, lc)
    out = tmp_path / 'child.pt'
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], cwd=ROOT, timeout=900, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lf, sf = torch.load(str(out))
    assert torch.equal(lf, lc)
    for k in sc:
        assert torch.equal(sf[k], sc[k]), k


if __name__ == '__main__':                                 # the fresh-process repeat of the captured epochs
    sys.path.insert(0, ROOT)
    d = torch.device('cuda:0')
    torch.save(_train(_ptc_dataset(d), d, captured=True), sys.argv[1])
