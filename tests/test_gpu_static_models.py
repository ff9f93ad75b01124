"""Static-shape (padded) batches for the BatchNorm and GNNML1 models: the raw-adjacency assembly (gml_batch_assemble_edges), the
masked BatchNorm kernels (gml_bn_masked_*), padded-vs-plain model steps on the real mutag / sr25 graphs, and one captured training
step replayed per batch against the same epochs run eagerly."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, rel_err

pytestmark = pytest.mark.gpu

BS = 16                                                    # mutag.py:320-351


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


def _dataset(name, dev):
    from gnn_matlang_amd import SpectralDesign, readers, synthetic
    from gnn_matlang_amd.dataset import DeviceDataset
    if name == 'mutag':
        raw = readers.load_mutag(os.path.join(GOLDEN, 'raw', 'mutag.mat'))
    elif name == 'sr25':
        raw = readers.load_sr(os.path.join(GOLDEN, 'raw', 'sr251256.g6'))
    else:                                                  # raw edges NOT sorted by source inside a graph
        rng = np.random.default_rng(5)
        raw = [(x, ei[:, rng.permutation(ei.shape[1])], np.float32(y)) for x, ei, y in synthetic.make_graphs('zinc', 30, seed=4)]
    ds = SpectralDesign(recfield=1, dv=4, nfreq=3, adddegree=True).design_many(raw)
    dd = DeviceDataset.from_graphs(ds, dev)
    dd.y = dd.y.float()
    return dd


@pytest.fixture(scope='module')
def mutag(dev):
    return _dataset('mutag', dev)


# ------------------------------------------------------------------ 2. the raw adjacency of an assembled batch
@pytest.mark.parametrize('name', ['mutag', 'unsorted'])
@pytest.mark.parametrize('ids', [[5, 0, 17, 3, 9, 2, 11, 6], [4, -1, 7, 4, 12, -1, 0, -1], [-1] * 8])
def test_assembled_adjacency_is_bit_identical_to_the_padded_batch_and_its_index(dev, name, ids):
    """batch_assembled(adjacency=True) against batch_padded(adjacency=True) + GraphCSR.from_edge_index: every array of both views of
    the raw adjacency bit-identical and equal to oracle/csr_oracle.py; groups64=True: the 64-row records of the support view equal
    the ones GraphCSR builds, inside bounds()['caps64'].  Absent slots (-1 -> no graph), repeated graphs, the all-absent batch."""
    from gnn_matlang_amd.graph import GraphCSR
    from oracle import csr_oracle
    dd = _dataset(name, dev)
    G = len(dd)
    bd = dd.bounds(8)
    ids = torch.tensor([G if i < 0 else i for i in ids], device=dev)
    bp = dd.batch_padded(ids, bd, adjacency=True)
    ba = dd.batch_assembled(ids, bd, adjacency=True, groups64=True)
    for nm in ('x', 'edge_attr2', 'y', 'graph_valid'):
        assert torch.equal(getattr(bp, nm).float(), getattr(ba, nm)), nm
    cp = GraphCSR.from_edge_index(bp.edge_index, bd['n_pad'])
    ca = ba.csr('edge_index')
    assert (ca.N, ca.E) == (cp.N, cp.E) == (bd['n_pad'], bd['e_pad']) and ca.static_shape
    for nm in ('rowptr', 'col', 'perm', 'rowptr_t', 'col_t', 'perm_t', 'pos_t', 'tpos', 'ginfo128', 'ginfo_t128'):
        assert torch.equal(getattr(cp, nm), getattr(ca, nm)), nm
    assert ca.gmax128[0] >= cp.gmax128[0] and ca.gmax128[1] >= cp.gmax128[1]
    assert ca.gmax_t128[0] >= cp.gmax_t128[0] and ca.gmax_t128[1] >= cp.gmax_t128[1]
    ei = bp.edge_index.cpu().numpy()
    rp, col, perm = csr_oracle.csr_from_coo(ei[0], ei[1], bd['n_pad'])
    assert np.array_equal(rp, ca.rowptr.cpu().numpy()) and np.array_equal(col, ca.col.cpu().numpy()) and np.array_equal(perm, ca.perm.cpu().numpy())
    rpt, colt, post = csr_oracle.transpose_view(ei[0], ei[1], bd['n_pad'], perm)
    assert np.array_equal(rpt, ca.rowptr_t.cpu().numpy()) and np.array_equal(colt, ca.col_t.cpu().numpy()) and np.array_equal(post, ca.pos_t.cpu().numpy())
    # the support view: unchanged by adjacency=True, its 64-row records as GraphCSR builds them (maxima from bounds)
    sp, sa = bp.csr('edge_index2'), ba.csr('edge_index2')
    for nm in ('rowptr', 'col', 'perm', 'rowptr_t', 'col_t', 'pos_t', 'ginfo128', 'ginfo_t128'):
        assert torch.equal(getattr(sp, nm), getattr(sa, nm)), nm
    assert torch.equal(sa._ginfo, sp.ginfo) and torch.equal(sa._ginfo_t, sp.ginfo_t)
    assert all(a >= b for a, b in zip(sa.gmax, sp.gmax)) and all(a >= b for a, b in zip(sa.gmax_t, sp.gmax_t))


# ------------------------------------------------------------------ 3. masked BatchNorm kernels
def _bn_reference(x, idx, w, b, g, eps):
    """float64 BatchNorm over the rows idx: y, dx (zeros elsewhere), dw, db, batch mean and biased variance."""
    xv = x[idx].double().requires_grad_(True)
    wd, bd = w.detach().double().requires_grad_(True), b.detach().double().requires_grad_(True)
    if idx.numel() == 0:
        z = torch.zeros_like(x, dtype=torch.float64)
        zc = torch.zeros_like(w, dtype=torch.float64)
        return z, z, zc, zc, None, None
    m = xv.mean(0)
    v = ((xv - m) ** 2).mean(0)
    yv = (xv - m) / torch.sqrt(v + eps) * wd + bd
    (yv * g[idx].double()).sum().backward()
    y = torch.zeros_like(x, dtype=torch.float64)
    y[idx] = yv.detach()
    dx = torch.zeros_like(x, dtype=torch.float64)
    dx[idx] = xv.grad
    return y, dx, wd.grad, bd.grad, m.detach(), v.detach()


@pytest.mark.parametrize('C', [4, 48, 64])
@pytest.mark.parametrize('nvalid', [0, 1, 2, 200])
def test_masked_batchnorm_vs_batchnorm_of_the_valid_rows(dev, C, nvalid):
    """models.BatchNorm1d(valid=...) (gml_bn_masked_*) against BatchNorm over the valid rows only (float64), two training steps:
    output, dx, d weight, d bias within 1e-5 of their scale, running statistics after each step; invalid rows' y and dx exactly 0;
    running statistics untouched when fewer than two rows are valid."""
    from gnn_matlang_amd import models
    torch.manual_seed(C + nvalid)
    N, eps = 333, 1e-5
    bn = models.BatchNorm1d(C).to(dev).train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C) + 0.5)
        bn.bias.copy_(torch.randn(C))
    rm, rv = bn.running_mean.double().cpu(), bn.running_var.double().cpu()
    for step in range(2):
        x = torch.randn(N, C, device=dev) + 0.3
        valid = torch.zeros(N, device=dev)
        idx = torch.randperm(N, device=dev)[:nvalid].sort()[0]
        if nvalid == 2:
            # two rows: keep every column's spread >= 1 -- like torch's float32 BatchNorm, E[x^2] - mean^2 in float32 cannot resolve a
            # column whose two values nearly coincide (gml.h: the variance form of the BatchNorm kernels)
            x[idx[1]] = x[idx[0]] + (torch.rand(C, device=dev) + 1.0) * torch.sign(torch.randn(C, device=dev))
        x.requires_grad_(True)
        valid[idx] = 1.0
        g = torch.randn(N, C, device=dev)
        bn.weight.grad = bn.bias.grad = None
        y = bn(x, valid=valid)
        y.backward(g)
        ry, rdx, rdw, rdb, m, v = _bn_reference(x.detach(), idx, bn.weight, bn.bias, g, eps)
        inv = valid == 0
        assert bool((y[inv] == 0).all()) and bool((x.grad[inv] == 0).all())
        if nvalid == 0:
            assert bool((y == 0).all()) and bool((x.grad == 0).all())
            assert bool((bn.weight.grad == 0).all()) and bool((bn.bias.grad == 0).all())
        else:
            for got, ref, what in ((y, ry, 'y'), (bn.weight.grad, rdw, 'dweight'), (bn.bias.grad, rdb, 'dbias')):
                err = rel_err(got.detach().cpu().numpy(), ref.cpu().numpy())
                assert err <= 1e-5, (what, step, err)
            # dx = (dy - mean dy - xhat mean(dy xhat)) rstd w cancels almost completely for few rows (two rows: xhat = +-1, dx ~ eps / var):
            # its error is measured against the scale of the terms that cancel, |dy| rstd |w|
            scale = float((g[idx].abs().double().cpu() / torch.sqrt(v.cpu() + eps) * bn.weight.detach().abs().double().cpu()).max())
            err = float((x.grad.double().cpu() - rdx.cpu()).abs().max()) / scale
            assert err <= 1e-5, ('dx', step, err)
        if nvalid >= 2:
            rm = 0.9 * rm + 0.1 * m.cpu()
            rv = 0.9 * rv + 0.1 * v.cpu() * nvalid / (nvalid - 1)
            assert rel_err(bn.running_mean.cpu().numpy(), rm.numpy()) <= 1e-5
            assert rel_err(bn.running_var.cpu().numpy(), rv.numpy()) <= 1e-5
        else:
            assert torch.equal(bn.running_mean.cpu(), rm.float()) and torch.equal(bn.running_var.cpu(), rv.float())
        assert int(bn.num_batches_tracked) == step + 1


# ------------------------------------------------------------------ 4. padded vs plain model steps
def _sr25_loss(pre, nl=None, valid=None):
    w = torch.linspace(-1.0, 1.0, pre.size(1), device=pre.device)
    if valid is None:
        return (pre * w).sum()
    return ((pre[:nl] * w).sum(1) * valid).sum()


@pytest.mark.parametrize('which', ['mutag_gnnml3', 'GNNML1Mutag', 'sr25_gnnml1'])
def test_padded_batch_step_equals_the_plain_batch(dev, mutag, which):
    """The same graphs as a plain batch and as a padded static batch (absent slots included): logits of the real graphs, the (masked)
    loss, every parameter gradient within 2e-5 of its scale, the BatchNorm running statistics after the step."""
    from gnn_matlang_amd import models
    dd = mutag if which != 'sr25_gnnml1' else _dataset('sr25', dev)
    G = len(dd)
    torch.manual_seed(3)
    m = {'mutag_gnnml3': lambda: models.mutag_gnnml3(), 'GNNML1Mutag': lambda: models.mutag_gnnml1(8),
         'sr25_gnnml1': lambda: models.sr25_gnnml1(2)}[which]().to(dev).train()
    mp, ms = m, copy.deepcopy(m)
    sl = [11, 0, G, 7, 3, G, 14, 2, 9, 1, 5, G, 12, 4, 8, 6]
    ids = torch.tensor(sl, device=dev)
    real = torch.tensor([i for i in sl if i < G], device=dev)
    bd = dd.bounds(BS)
    bs = dd.batch_assembled(ids, bd, adjacency=True, groups64=True)
    bpl = dd.batch(real)
    keep = torch.tensor([k for k, i in enumerate(sl) if i < G], device=dev)
    pre_p, pre_s = mp(bpl), ms(bs)
    if which == 'sr25_gnnml1':
        lp, ls = _sr25_loss(pre_p), _sr25_loss(pre_s, BS, bs.graph_valid)
    else:
        lp, ls = models.mutag_loss(pre_p, bpl.y.float()), models.mutag_loss(pre_s, bs.y, bs.graph_valid)
    assert rel_err(pre_s[keep].detach().cpu().numpy(), pre_p.detach().cpu().numpy()) <= 2e-5
    assert abs(ls.item() - lp.item()) <= 2e-5 * abs(lp.item())
    lp.backward()
    ls.backward()
    sp = dict(ms.named_parameters())
    for n, p in mp.named_parameters():
        err = rel_err(sp[n].grad.cpu().numpy(), p.grad.cpu().numpy())
        assert err <= 2e-5, (n, err)
    sb = dict(ms.named_buffers())
    for n, b in mp.named_buffers():
        if 'running' in n:
            assert rel_err(sb[n].cpu().numpy(), b.cpu().numpy()) <= 2e-5, n


# ------------------------------------------------------------------ 5. one captured step replayed per batch
def _perms(G, epochs, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.cat([torch.randperm(G, generator=gen), torch.full(((-G) % BS,), G, dtype=torch.int64)]) for _ in range(epochs)]


def _model(which, dev):
    from gnn_matlang_amd import models
    torch.manual_seed(21)
    return (models.mutag_gnnml3() if which == 'mutag_gnnml3' else models.mutag_gnnml1(8)).to(dev).train()


def _train(which, dd, dev, captured, epochs=2):
    """(per-batch losses [n], final parameters and buffers) of `epochs` epochs of mutag training at batch 16 over
    batch_assembled batches with OneLaunchAdam, eagerly or as one captured step replayed per batch."""
    from gnn_matlang_amd import models
    from gnn_matlang_amd.optim import OneLaunchAdam
    m = _model(which, dev)
    opt = OneLaunchAdam(m.parameters(), lr=1e-3)
    bd = dd.bounds(BS)
    dd.prepare()
    adj = which == 'GNNML1Mutag'
    ids_buf = torch.zeros(BS, dtype=torch.int64, device=dev)
    loss_buf = torch.zeros((), device=dev)

    def step():
        b = dd.batch_assembled(ids_buf, bd, adjacency=adj, groups64=True)
        opt.zero_grad(set_to_none=True)
        l = models.mutag_step_loss(m, b)
        l.backward()
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
        with torch.no_grad():                              # back to the initial state: the warm-up and capture steps trained
            for k, v in m.state_dict().items():
                v.copy_(snap[k])
            for st in opt.state.values():
                st['exp_avg'].zero_()
                st['exp_avg_sq'].zero_()
                st['step'].zero_()
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
    return torch.stack(losses).cpu(), {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


@pytest.mark.parametrize('which', ['mutag_gnnml3', 'GNNML1Mutag'])
def test_captured_epochs_are_bitwise_equal_to_eager_epochs(dev, mutag, which, tmp_path):
    """Two mutag epochs at batch 16 as ONE captured HIP graph replayed per batch (assembly, forward, masked loss, backward, BatchNorm
    running statistics, OneLaunchAdam) vs the same epochs run eagerly over batch_assembled: per-batch losses, final parameters and
    buffers bitwise equal; and once more in a fresh process: bitwise equal again."""
    le, se = _train(which, mutag, dev, captured=False)
    lc, sc = _train(which, mutag, dev, captured=True)
    assert torch.isfinite(le).all() and le.numel() == 2 * ((len(mutag) + BS - 1) // BS)
    assert torch.equal(le, lc), (le - lc).abs().max()
    for k in se:
        assert torch.equal(se[k], sc[k]), k
    out = tmp_path / 'child.pt'
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which, str(out)], cwd=ROOT, timeout=600, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lf, sf = torch.load(str(out))
    assert torch.equal(lf, lc)
    for k in sc:
        assert torch.equal(sf[k], sc[k]), k


if __name__ == '__main__':                                 # the fresh-process repeat of the captured epochs
    sys.path.insert(0, ROOT)
    d = torch.device('cuda:0')
    torch.save(_train(sys.argv[1], _dataset('mutag', d), d, captured=True), sys.argv[2])
