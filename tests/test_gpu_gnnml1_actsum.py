"""GNNML1 block mode 5 (form 'act_sum': relu(a) + relu(c) + relu(f2 f3), csrc/gml_gnnml1_act.hip) and the node-level filtering GNNML1
built on it, on the device: the block against its float64 restatement (tests/_gnnml1_actsum_ref.py), the recorded patterns, the
variants, the C ABI outside its range, the model on small grids and on the real 900-node grid on both roads, and captured epochs."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _gnnml1_actsum_ref as A
from _gnnml1_ref import check as _check
from conftest import GOLDEN, ROOT, rel_err

pytestmark = pytest.mark.gpu

MODEL_TOL = 1e-4                                                 # tests/test_gpu_filtering.py
_ID = lambda c: '%dx%d-%d%s' % (c[0], c[1], c[2], '' if c[3] else '-vals')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


_REF = {}


def _case(c):
    """(arguments, float64 restatement, float32 restatement) of a case, computed once and shared"""
    if c not in _REF:
        args = A.case(*c)
        _REF[c] = (args, A.block(*args, torch.float64), A.block(*args, torch.float32))
    return _REF[c]


def _block_gpu(dev, x, ei, val, W, gout, unit, need_dx=True, strided=False):
    """the fused block forward + backward: (out, dx, gradients, recorded pattern bytes)"""
    from gnn_matlang_amd import functional as Fn
    from gnn_matlang_amd.graph import GraphCSR
    N, Fin = x.shape
    n = W['w1'].size(0)
    csr = GraphCSR.from_edge_index(ei.to(dev), N)
    if strided:                                                  # x: rows of a wider buffer (ldx > Fin); gout: a column slice
        buf = torch.zeros(N, Fin + 5, device=dev)
        buf[:, :Fin] = x.to(dev)
        xl = buf.requires_grad_(need_dx)
        xd = xl[:, :Fin]
        gbuf = torch.randn(N, n + 7, device=dev)
        gbuf[:, 3:3 + n] = gout.to(dev)
        gd = gbuf[:, 3:3 + n]
        assert xd.stride(0) > Fin and gd.stride(0) > n and not gd.is_contiguous()
    else:
        xl = xd = x.detach().to(dev).requires_grad_(need_dx)
        gd = gout.to(dev)
    Wd = {k: v.detach().to(dev).requires_grad_(True) for k, v in W.items()}
    vs = None if unit else csr.sort_values(val.to(dev).view(-1, 1)).view(-1)
    assert Fn.gnnml1_block_supported(xd, Fin, n, n, n, 5) and Fn.gnnml1_block_supported(xd, Fin, n, n, n, 5, 1)
    assert not Fn.gnnml1_block_supported(xd, Fin, n, n, n, 5, 0)                  # tanh: the composition
    y = Fn.GNNML1BlockFunction.apply(xd, csr, vs, Wd['w1'], Wd['b1'], Wd['wc'], Wd['bc'], Wd['w2'], Wd['b2'], Wd['w3'], Wd['b3'], 5, 1)
    assert y.shape == (N, n)
    pat = [t for t in y.grad_fn.saved_tensors if t is not None and t.dtype == torch.uint8]
    assert len(pat) == 1 and not any(t is not None and t.data_ptr() == y.data_ptr() for t in y.grad_fn.saved_tensors)   # `out` is not saved
    pat = pat[0].clone()
    y.backward(gd)
    dx = (xl.grad[:, :Fin] if strided else xl.grad) if need_dx else None
    assert need_dx or xl.grad is None
    return y.detach(), dx, {k: v.grad for k, v in Wd.items()}, pat


def _check_all(got, r64, r32, tag, dx=True):
    _check(got[0], r64['out'], r32['out'], 'output', tag, computed=True)
    if dx:
        _check(got[1], r64['dx'], r32['dx'], 'dx', tag, computed=True)
    assert len(got[2]) == 8
    for k in r64['grads']:
        _check(got[2][k], r64['grads'][k], r32['grads'][k], 'd' + k, tag, computed=True)


# ------------------------------------------------------------------------------------------------ the block
@pytest.mark.parametrize('c', A.CASES, ids=_ID)
def test_block_against_float64(dev, c):
    """output, dx and all eight parameter gradients; bound: the project's 2e-5, or 4 x the float32 restatement's own error"""
    args, r64, r32 = _case(c)
    assert A.patterns_agree(r32, r64)                            # no bit of any pattern hangs on the number format
    _check_all(_block_gpu(dev, *args, c[3]), r64, r32, _ID(c))


def test_the_three_patterns_are_kept_apart(dev):
    """every sign combination of (a, c, f2 f3) covers more than 5 % of the entries, so a kernel that mixes up two patterns (or applies
    one relu to the sum, mode 0) misses the weight and bias gradients of the parts"""
    c = A.SEPARATION
    args, r64, r32 = _case(c)
    shares = A.combination_shares(r64)
    print('shares of the eight sign combinations', shares.tolist())
    assert shares.min() > 0.05
    got = _block_gpu(dev, *args, c[3])
    for k in ('w1', 'b1', 'wc', 'bc', 'w2', 'b2', 'w3', 'b3'):
        _check(got[2][k], r64['grads'][k], r32['grads'][k], 'd' + k, 'separation', computed=True)


@pytest.mark.parametrize('c', [A.SEPARATION, A.CASES[4], A.CASES[0]], ids=_ID)
def test_recorded_bytes(dev, c):
    """the bytes the forward records are the bits of the float32 restatement (which equal the float64 ones), padding columns zero"""
    args, r64, r32 = _case(c)
    assert A.patterns_agree(r32, r64)
    pat = _block_gpu(dev, *args, c[3])[3].cpu()
    want = A.pattern_bytes(r32)
    assert pat.shape == want.shape and pat.dtype == torch.uint8
    assert torch.equal(pat, want), int((pat != want).sum())


def test_block_without_dx(dev):
    c = A.CASES[2]
    args, r64, r32 = _case(c)
    got = _block_gpu(dev, *args, c[3], need_dx=False)
    assert got[1] is None
    _check_all(got, r64, r32, 'no dx', dx=False)
    full = _block_gpu(dev, *args, c[3])
    for k in full[2]:                                            # the weight gradients do not depend on whether dx is formed
        assert torch.equal(full[2][k], got[2][k]), k


@pytest.mark.parametrize('c', [A.CASES[1], A.CASES[3], A.CASES[4]], ids=_ID)
def test_block_on_strided_views(dev, c):
    args, r64, r32 = _case(c)
    got = _block_gpu(dev, *args, c[3], strided=True)
    _check_all(got, r64, r32, 'strided ' + _ID(c))
    plain = _block_gpu(dev, *args, c[3])
    assert torch.equal(plain[0], got[0]) and torch.equal(plain[1], got[1]) and torch.equal(plain[3], got[3])


def test_block_repeats_bitwise(dev):
    c = A.CASES[3]
    args = _case(c)[0]
    a = _block_gpu(dev, *args, c[3])
    for _ in range(3):
        b = _block_gpu(dev, *args, c[3])
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
        for k in a[2]:
            assert torch.equal(a[2][k], b[2][k]), k


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_answers_outside_the_range(dev):
    """GML_E_UNSUPPORTED (-2): widths past the limit, tanh; GML_E_BADARG (-1): unequal parts, no pattern in the backward -- and nothing
    is launched: buffers filled with NaN stay NaN"""
    from gnn_matlang_amd import _lib
    from gnn_matlang_amd.graph import GraphCSR
    L = _lib.lib()
    N = 40
    x, ei, val, W, gout = A.case(*A.CASES[6])
    csr = GraphCSR.from_edge_index(ei.to(dev), N)
    big = lambda *s: torch.randn(*s, device=dev)
    xd, w, b, g = big(N, 160), big(80 * 160), big(80), big(N, 80)
    nan = lambda *s: torch.full(s, float('nan'), device=dev)
    out, dx, g4, q = nan(N, 80), nan(N, 160), nan(N, 4 * 80), nan(N, 80)
    pat = torch.zeros(N, 20, dtype=torch.uint8, device=dev)
    P = lambda t: t.data_ptr()

    def fwd(Fin, n1, n2, n3, act):
        return L.gml_gnnml1_actsum_fwd(P(csr.rowptr), P(csr.col), None, P(xd), 160, N, Fin, P(w), P(b), n1, P(w), P(b), n2, P(w), P(b), P(w),
                                       P(b), n3, act, P(out), 80, P(pat), 20, None)

    def bwd(Fin, n1, n2, n3, act, pattern=pat):
        return L.gml_gnnml1_actsum_bwd(P(csr.rowptr_t), P(csr.col_t), None, P(xd), 160, P(g), 80, N, Fin, P(w), n1, P(w), n2, P(w), P(b), P(w),
                                       P(b), n3, act, P(pattern) if pattern is not None else None, 20, P(dx), 160, P(g4), 320, P(q), 80, None)

    for call in (fwd, bwd):
        assert call(145, 64, 64, 64, 1) == -2 and call(144, 65, 65, 65, 1) == -2 and call(1, 80, 80, 80, 1) == -2      # past the widths
        assert call(32, 32, 32, 32, 0) == -2                                                                         # tanh
        assert call(32, 32, 16, 32, 1) == -1 and call(32, 32, 32, 16, 1) == -1 and call(32, 16, 32, 32, 1) == -1      # unequal parts
        assert call(32, 32, 32, 32, 2) == -1 and call(0, 32, 32, 32, 1) == -1
    assert bwd(32, 32, 32, 32, 1, pattern=None) == -1
    assert bwd(144, 64, 64, 64, 1, pattern=None) == -1
    torch.cuda.synchronize()
    for t in (out, dx, g4, q):
        assert bool(torch.isnan(t).all())
    assert not bool(pat.any())
    sup = L.gml_gnnml1_actsum_supported
    assert sup(144, 64, 64, 64, 1) == 1 and sup(1, 1, 1, 1, 1) == 1
    assert [sup(145, 64, 64, 64, 1), sup(1, 65, 65, 65, 1), sup(32, 32, 32, 32, 0), sup(32, 32, 16, 32, 1), sup(32, 32, 32, 16, 1)] == [0] * 5


# gml_gnnml1_supported for mode = -1, 0, 1, 2, 3, 4, 5, 6 and gml_gnnml1_sum_supported, recorded from the library before mode 5 existed
_BEFORE = [(1, 32, 32, 32, '01111000', 1), (1, 64, 64, 64, '01111000', 1), (1, 65, 65, 65, '00000000', 0), (1, 32, 16, 32, '00111000', 0),
           (1, 32, 32, 16, '00111000', 1), (64, 32, 32, 32, '01111000', 1), (64, 64, 64, 64, '01111000', 1), (64, 65, 65, 65, '00000000', 0),
           (64, 32, 16, 32, '00111000', 0), (64, 32, 32, 16, '00111000', 1), (144, 32, 32, 32, '01111000', 1),
           (144, 64, 64, 64, '01111000', 1), (144, 65, 65, 65, '00000000', 0), (144, 32, 16, 32, '00111000', 0),
           (144, 32, 32, 16, '00111000', 1), (145, 32, 32, 32, '00000000', 1), (145, 64, 64, 64, '00000000', 1),
           (145, 65, 65, 65, '00000000', 0), (145, 32, 16, 32, '00000000', 0), (145, 32, 32, 16, '00000000', 1),
           (192, 128, 128, 64, '00000000', 1), (193, 128, 128, 64, '00000000', 0), (192, 128, 64, 64, '00000000', 0)]


def test_existing_predicates_answer_as_before(dev):
    from gnn_matlang_amd import _lib
    L = _lib.lib()
    for Fin, n1, n2, n3, modes, s in _BEFORE:
        got = ''.join(str(L.gml_gnnml1_supported(Fin, n1, n2, n3, m)) for m in (-1, 0, 1, 2, 3, 4, 5, 6))
        assert got == modes and L.gml_gnnml1_sum_supported(Fin, n1, n2, n3) == s, (Fin, n1, n2, n3, got)


# ------------------------------------------------------------------------------------------------ the model
_HOST = {}


def _grid_batch(a, b):
    """a x b grid with random signals, y and mask (75 % ones), the raw grid adjacency as data.edge_index; collated once"""
    from gnn_matlang_amd import collate
    if (a, b) not in _HOST:
        n = a * b
        rng = np.random.default_rng(7 * n)
        d = dict(x=rng.normal(size=(n, 1)).astype(np.float32), edge_index=A.grid_edges(a, b), y=rng.normal(size=(n, 3)).astype(np.float32),
                 mask=(rng.random((n, 1)) < 0.75).astype(np.float32))
        _HOST[(a, b)] = collate([d], node_fields=('y', 'mask'))
    return _HOST[(a, b)]


def _run_model(m, data, ntask):
    """pre, loss, the four sums, the gradients and the launches recorded under functional.PROFILE of one forward + backward"""
    from gnn_matlang_amd import functional as Fn, models
    assert Fn.PROFILE is None
    Fn.PROFILE = {}
    try:
        m.zero_grad(set_to_none=True)
        with torch.no_grad():
            pre = m(data, _road='dense')                         # (_road: accepted, one road)
        Fn.PROFILE.clear()
        stats = torch.zeros(4, device=data.x.device)
        loss = models.filtering_step_loss(m, data, ntask, stats)
        loss.backward()
        torch.cuda.synchronize()
        tags = {k: len(v) for k, v in Fn.PROFILE.items()}
    finally:
        Fn.PROFILE = None
    return dict(pre=pre.detach().cpu(), loss=loss.detach().cpu(), stats=stats.cpu(), tags=tags,
                grads={k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()})


def _reference(state, host, ntask, concat=False, act=F.relu):
    P = {k: v.detach().cpu().double().requires_grad_(True) for k, v in state.items()}
    pre, loss, stats = A.model_ref(P, host.x.double(), host.edge_index, host.y.double(), host.mask.double(), ntask, concat=concat, act=act)
    loss.backward()
    return pre.detach(), loss.detach(), stats, {k: v.grad for k, v in P.items()}


def _close(got, ref, what):
    e = rel_err(got.detach().cpu().double().numpy(), ref.detach().cpu().double().numpy())
    print('%-28s rel err %.2e' % (what, e))
    assert e <= MODEL_TOL, (what, e)


def _against_reference(run, ref, nparams=26):
    pre, loss, stats, grads = ref
    _close(run['pre'], pre, 'pre')
    _close(run['loss'], loss, 'loss')
    for i, k in enumerate(('loss', 'ss_res', 'ss_tot', 'count')):
        _close(run['stats'][i], stats[i], 'stats.' + k)
    assert float(run['stats'][3]) == float(stats[3])
    assert len(run['grads']) == nparams == len(grads)
    for k, g in run['grads'].items():
        _close(g, grads[k], 'grad ' + k)


_FUSED = ('gnnml1_actsum_fwd', 'gnnml1_actsum_bwd', 'gnnml1_actsum_dw')


@pytest.mark.parametrize('a,b', [(5, 7), (17, 3)])
def test_model_on_small_grids(dev, a, b, tmp_path):
    """filtering_gnnml1 against the float64 composition: all three blocks on the fused kernel; GML_NO_GNNML1_FUSED=1 in a fresh process
    gives the composition, within the same bound"""
    from gnn_matlang_amd import models
    host = _grid_batch(a, b)
    data = host.to(dev)
    torch.manual_seed(11)
    m = models.filtering_gnnml1().to(dev).train()
    state = {k: v.clone() for k, v in m.state_dict().items()}
    run = _run_model(m, data, 1)
    assert [run['tags'].get(t) for t in _FUSED] == [3, 3, 3], run['tags']             # the fused road, three blocks each way
    assert 'conv_fwd' not in run['tags'] and 'gnnml1_fwd' not in run['tags'], run['tags']
    ref = _reference(state, host, 1)
    _against_reference(run, ref)
    assert abs(float(models.r2_from_stats(run['stats'])) - float(1 - ref[2][1] / ref[2][2])) <= MODEL_TOL * max(1.0, abs(float(1 - ref[2][1] / ref[2][2])))
    out = str(tmp_path / 'composition.pt')
    code = ("import sys, torch\n"
            "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_gnnml1_actsum as T\n"
            "from gnn_matlang_amd import functional as Fn, models\n"
            "d = torch.device('cuda:0')\n"
            "data = T._grid_batch(%d, %d).to(d)\n"
            "assert not Fn.gnnml1_block_supported(data.x, 1, 32, 32, 32, 5, 1)\n"
            "torch.manual_seed(11)\n"
            "m = models.filtering_gnnml1().to(d).train()\n"
            "torch.save(T._run_model(m, data, 1), %r)\n" % (ROOT, os.path.join(ROOT, 'tests'), a, b, out))
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, GML_NO_GNNML1_FUSED='1'), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    comp = torch.load(out)
    assert not any(t in comp['tags'] for t in _FUSED), comp['tags']
    _against_reference(comp, ref)


def test_concat_runs_on_the_product_form(dev):
    from gnn_matlang_amd import models
    host = _grid_batch(5, 7)
    torch.manual_seed(12)
    m = models.filtering_gnnml1(concat=True).to(dev).train()
    state = {k: v.clone() for k, v in m.state_dict().items()}
    run = _run_model(m, host.to(dev), 2)
    assert run['tags'].get('gnnml1_fwd') == 3 and not any(t in run['tags'] for t in _FUSED), run['tags']
    _against_reference(run, _reference(state, host, 2, concat=True))


def test_tanh_act_sum_runs_on_the_composition(dev):
    from gnn_matlang_amd import models
    host = _grid_batch(17, 3)
    torch.manual_seed(13)
    m = models.GNNML1Blocks(1, (32, 32, 32), 3, form='act_sum', act='tanh', pool=None, head='node').to(dev).train()
    state = {k: v.clone() for k, v in m.state_dict().items()}
    run = _run_model(m, host.to(dev), 0)
    assert not any(t in run['tags'] for t in _FUSED) and 'gnnml1_fwd' not in run['tags'], run['tags']
    _against_reference(run, _reference(state, host, 0, act=torch.tanh))


# ------------------------------------------------------------------------------------------------ the real grid
@pytest.fixture(scope='module')
def grid30():
    from gnn_matlang_amd import collate, readers
    recs = readers.load_twodgrid(os.path.join(GOLDEN, 'raw', 'TwoDGrid30.mat'))
    return [collate([r], node_fields=('y', 'mask')) for r in recs]


def test_real_grid_forward_backward(dev, grid30):
    """one forward + backward on the 900-node fixture at ntask = 0 against float64"""
    from gnn_matlang_amd import models
    host = grid30[0]
    assert tuple(host.x.shape) == (900, 1) and tuple(host.y.shape) == (900, 3) and host.edge_index.size(1) == 2 * 2 * 30 * 29
    torch.manual_seed(5)
    m = models.filtering_gnnml1().to(dev).train()
    state = {k: v.clone() for k, v in m.state_dict().items()}
    run = _run_model(m, host.to(dev), 0)
    assert [run['tags'].get(t) for t in _FUSED] == [3, 3, 3], run['tags']
    assert float(run['stats'][3]) == 676
    _against_reference(run, _reference(state, host, 0))


def test_captured_epochs_equal_eager_epochs(dev, grid30):
    """dist.TrainStep(model, filtering_step_loss, opt).capture(data): five replayed epochs (train step on graph 0) against five
    eager ones from the same state -- losses, the four sums and the final parameters bitwise"""
    from gnn_matlang_amd import models
    from gnn_matlang_amd.dist import TrainStep
    from gnn_matlang_amd.optim import OneLaunchAdam
    data = grid30[0].to(dev)

    def run(captured):
        torch.manual_seed(9)
        m = models.filtering_gnnml1().to(dev).train()
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
