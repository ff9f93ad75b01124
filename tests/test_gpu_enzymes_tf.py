"""The TF GNNML3 of enzymes_contfeats_gnnml3_tf.py on the ragged dense-block road (dense_block.spectconv_ragged, models.DSSGCN) against
the float64 restatement tests/_dssgcn_ref.py, on 8 real ENZYMES graphs of 2 .. 126 nodes (four of them above the 96 nodes of the
equal-size dense kernels).  Tolerance: conftest.rel_err <= 1e-4, the bf16x3 one of every dense test."""
import numpy as np
import pytest
import torch

import _dssgcn_ref as ref
import _philox
from conftest import GOLDEN, rel_err
from gnn_matlang_amd import dense_block, models
from gnn_matlang_amd import functional as Fn
from gnn_matlang_amd.graph import collate

pytestmark = pytest.mark.gpu
TOL = 1e-4
PERM = list(ref.PERM)                    # batch position -> bank slot


@pytest.fixture(scope='module')
def env():
    dev = torch.device('cuda')
    g8 = ref.enzymes8(GOLDEN)
    full = collate(g8).to(dev)
    bank = dense_block.RaggedSupports(full.edge_index2, full.edge_attr2, full.batch, full.ptr)
    graphs = [g8[i] for i in PERM]
    batch = dense_block.attach_bank(collate(graphs).to(dev), bank, torch.tensor(PERM, dtype=torch.int32, device=dev))
    sizes = [g['x'].shape[0] for g in graphs]
    assert bank.sizes == [g['x'].shape[0] for g in g8] and max(sizes) == 126 and min(sizes) == 2
    return dict(dev=dev, bank=bank, graphs=graphs, batch=batch, sizes=sizes, y=[int(g['y']) for g in graphs])


@pytest.fixture(scope='module')
def conv_cases(env):
    """inputs of the layer tests, drawn once: x, weight, upstream gradient per shape"""
    rng = np.random.default_rng(5)
    N = sum(env['sizes'])
    out = {}
    for Fin, Fout in ((22, 200), (200, 200)):
        a = np.sqrt(6.0 / (Fin + Fout))
        out[Fin] = (rng.normal(size=(N, Fin)).astype(np.float32), rng.uniform(-a, a, size=(4, Fin, Fout)).astype(np.float32),
                    rng.normal(size=(Fout,)).astype(np.float32) * 0.1, rng.normal(size=(N, Fout)).astype(np.float32))
    return out


@pytest.mark.parametrize('xgrad', [True, False])
@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('Fin', [22, 200])
def test_spectconv_ragged_autograd(env, conv_cases, monkeypatch, Fin, p, xgrad):
    dev, b = env['dev'], env['batch']
    x0, w0, b0, g0 = conv_cases[Fin]
    x = torch.tensor(x0, device=dev, requires_grad=xgrad)
    w = torch.tensor(w0, device=dev, requires_grad=True)
    bias = torch.tensor(b0, device=dev, requires_grad=True)
    seed, counter, site = 77, 2, 3
    state = Fn.dropout_state(seed, dev)
    state[1] = counter
    calls = []
    real = dense_block.ragged_keep_bits
    monkeypatch.setattr(dense_block, 'ragged_keep_bits', lambda *a, **k: calls.append(k.get('need_bwd')) or real(*a, **k))
    out = dense_block.spectconv_ragged(x, b.bank, b.gid, b.ptr, w, bias, relu=False, p=p, state=state, site=site, training=True)
    assert calls == ([xgrad] if p > 0 else [])              # no mask launch without dropout; no transposed bits without dX
    state[1] = 99                                           # the backward uses the bits the forward saved
    out.backward(torch.tensor(g0, device=dev))
    kk = _philox.keep_mask(len(env['sizes']) * 4 * 128, 128, p, seed, counter, site).reshape(-1, 4, 128, 128) if p > 0 else None
    r_out, r_dx, r_dw, r_db = ref.conv(env['graphs'], x0, w0, b0, False, g0, kk, _philox.scale(p) if p > 0 else 1.0)
    errs = dict(out=rel_err(out.detach().cpu().numpy(), r_out), dw=rel_err(w.grad.cpu().numpy(), r_dw), db=rel_err(bias.grad.cpu().numpy(), r_db))
    if xgrad:
        errs['dx'] = rel_err(x.grad.cpu().numpy(), r_dx)
    else:
        assert x.grad is None
    print('rel_err', Fin, p, xgrad, errs)
    assert max(errs.values()) <= TOL, errs
    # evaluation: the same call with training off is the layer without dropout, and launches no mask
    calls.clear()
    ev = dense_block.spectconv_ragged(x.detach(), b.bank, b.gid, b.ptr, w.detach(), bias.detach(), p=p, state=state, site=site, training=False)
    assert calls == [] and rel_err(ev.cpu().numpy(), ref.conv(env['graphs'], x0, w0, b0)) <= TOL


def _run(env, m, training, seed=ref.DROP_SEED):
    m.train(training)
    m.zero_grad(set_to_none=True)
    with torch.no_grad():
        m.dropout_state.copy_(torch.tensor([seed, 0], dtype=torch.int64))
    logits = m(env['batch'])
    loss = models.dssgcn_loss(m, logits, env['batch'].y)
    loss.backward()
    return (logits.detach().cpu().numpy().astype(np.float64), float(loss.detach()),
            dict((k, v.grad.detach().cpu().numpy().astype(np.float64)) for k, v in m.named_parameters()))


def _check(got, want, what):
    errs = dict(logits=rel_err(got[0], want[0]), loss=abs(got[1] - want[1]) / abs(want[1]))
    for k in want[2]:
        errs[k] = rel_err(got[2][k], want[2][k])
    print('rel_err', what, errs)
    assert max(errs.values()) <= TOL, errs


@pytest.fixture(scope='module')
def model_and_params(env):
    m, P = ref.new_model()
    return m.to(env['dev']), P


def test_model_eval_mode(env, model_and_params):
    m, P = model_and_params
    _check(_run(env, m, False), ref.model(env['graphs'], P, env['y']), 'eval')


def test_model_training_mode(env, model_and_params):
    m, P = model_and_params
    masks = ref.philox_masks(env['sizes'], 4, ref.DIMS, ref.DROP_P, ref.DROP_SEED, 1)      # (the counter steps to 1 before the draws)
    want = ref.model(env['graphs'], P, env['y'], masks, ref.DROP_P)
    _check(_run(env, m, True), want, 'training')
    assert rel_err(want[0], ref.model(env['graphs'], P, env['y'])[0]) > 100 * TOL           # the masks matter


def test_same_bits_on_both_roads(env, model_and_params):
    m, _ = model_and_params
    hip = _run(env, m, True)
    with Fn.exact_products():
        lib = _run(env, m, True)
    _check(hip, lib, 'HIP road against the library road')


def test_stateful_draws(env, model_and_params):
    m, _ = model_and_params
    m.train()
    with torch.no_grad():
        m.dropout_state.copy_(torch.tensor([ref.DROP_SEED, 0], dtype=torch.int64))
        a = m(env['batch']).cpu().numpy()
        b = m(env['batch']).cpu().numpy()
        assert int(m.dropout_state[1]) == 2
        m.dropout_state.copy_(torch.tensor([ref.DROP_SEED, 0], dtype=torch.int64))
        c = m(env['batch']).cpu().numpy()
    assert not np.array_equal(a, b) and np.array_equal(a, c)


def test_training_smoke(env):
    torch.manual_seed(3)
    m = models.enzymes_contfeat_gnnml3(dropout=0.0).to(env['dev']).train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    losses = []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        loss = models.dssgcn_loss(m, m(env['batch']), env['batch'].y)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print('losses', losses)
    assert np.isfinite(losses).all() and all(b < a for a, b in zip(losses, losses[1:]))
