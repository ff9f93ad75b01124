"""The fused GNNML1 block in the sum-and-factors form (csrc/gml_gnnml1_sum.hip: [act(fc1 x) + act(conv x) | act(fc2 x) * act(fc3 x)],
inputs up to 192 wide, n1 = n2 <= 128, n3 <= 64) and the model built on it, enzymes_contfeat_gnnml1 (enzymes_contfeat.py:284-346):
block and model against float64 restatements written out here in plain torch, the two relu patterns of the sum, strided inputs,
bitwise repeatability, the composition outside the kernel's range and under GML_NO_GNNML1_FUSED, dropout.

Tolerance: the project's bound for exact fp32 products, max|got - ref64| <= 2e-5 max|ref64| per tensor (tests/test_gpu_gnnml1_wide.py:
TOL).  The float32 restatement's own error against float64 is printed beside every measured figure (CPU: at most 2.0e-6 for the
blocks, 3.0e-6 for the model)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _gnnml1_ref as R
from _gnnml1_ref import TOL, check as _check
from conftest import GOLDEN, ROOT, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    from gnn_matlang_amd import _lib
    assert _lib.lib().gml_version() >= 1
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------ the block (restated in _gnnml1_ref)
def _parts_ref(x, ei, v, W):
    return R.parts_ref(x, ei, v, W)


def _block_ref(x, ei, v, W, act):
    return R.block_ref(x, ei, v, W, 4, act)


def _block_case(N, Fin, n1, n3, unit):
    return R.block_case(N, Fin, n1, n1, n3, 4, unit)


def _block_cpu(x, ei, val, W, gout, act, dtype):
    return R.block_cpu(x, ei, val, W, gout, 4, act, dtype)


def _block_gpu(dev, x, ei, val, W, gout, act, unit, **kw):
    return R.block_gpu(dev, x, ei, val, W, gout, 4, act, unit, **kw)


# (N, Fin, n1 = n2, n3, act)
SECOND = (300, 192, 128, 64, 1)             # the script's second block
SHAPES = [SECOND,
          (130, 22, 128, 64, 1),            # the first block: rows not float4-addressable, one group, 130 not a multiple of 16
          (17, 192, 128, 64, 0),            # one partial tile at the limit, the tanh derivative
          (1, 30, 10, 7, 1),                # one row, one self loop, parts that are no multiples of 16
          (300, 145, 64, 17, 1),            # first input width past the other modes' limit, n3 one past a block
          (40, 64, 16, 16, 0)]              # narrow
CASES = [s + (True,) for s in SHAPES] + [SECOND + (False,)]


@pytest.mark.parametrize('N,Fin,n1,n3,act,unit', CASES)
def test_sum_block_vs_fp64(dev, N, Fin, n1, n3, act, unit):
    """one block forward and backward -- output, dx and all eight parameter gradients -- against the restatement in float64"""
    case = 'sum-%d-%d-%d-%d-a%d-%s' % (N, Fin, n1, n3, act, 'ones' if unit else 'values')
    ei, val, x, W, gout = _block_case(N, Fin, n1, n3, unit)
    y64, dx64, dW64 = _block_cpu(x, ei, val, W, gout, act, torch.float64)
    y32, dx32, dW32 = _block_cpu(x, ei, val, W, gout, act, torch.float32)
    y, dx, dW = _block_gpu(dev, x, ei, val, W, gout, act, unit)
    _check(y, y64, y32, 'out', case)
    _check(dx, dx64, dx32, 'dx', case)
    for k in W:
        _check(dW[k], dW64[k], dW32[k], k, case)


def test_the_two_relu_patterns_are_kept_apart(dev):
    """the script's second block: each of the four sign combinations of (a, c) covers a good share of the entries and the block is
    NOT relu(a + c) -- a swapped or shared activation pattern in the backward cannot pass the gradient checks on this case"""
    N, Fin, n1, n3, act = SECOND
    ei, val, x, W, gout = _block_case(N, Fin, n1, n3, True)
    x64, W64 = x.double(), {k: v.double() for k, v in W.items()}
    a, c, _, _ = _parts_ref(x64, ei, val.double(), W64)
    for sa in (True, False):
        for sc in (True, False):
            share = float((((a > 0) == sa) & ((c > 0) == sc)).double().mean())
            print('a > 0: %s, c > 0: %s: %.3f of the entries' % (sa, sc, share))
            assert share > 0.15, (sa, sc, share)
    ref = _block_ref(x64, ei, val.double(), W64, act)
    assert rel_err(torch.relu(a + c).numpy(), ref[:, :n1].numpy()) > 0.05
    # the gradients at a and at c differ where exactly one of them is positive: dW1 and dWc see different rows
    y, dx, dW = _block_gpu(dev, x, ei, val, W, gout, act, True)
    _, _, dW64 = _block_cpu(x, ei, val, W, gout, act, torch.float64)
    _, _, dW32 = _block_cpu(x, ei, val, W, gout, act, torch.float32)
    _check(y[:, :n1], ref[:, :n1], _block_ref(x, ei, val, W, act)[:, :n1], 'sum part', 'patterns')
    for k in ('w1', 'b1', 'wc', 'bc'):
        _check(dW[k], dW64[k], dW32[k], k, 'patterns')


def test_sum_block_without_dx(dev):
    """x.requires_grad == False: no dx launch, the parameter gradients still hold"""
    N, Fin, n1, n3, act = SECOND
    ei, val, x, W, gout = _block_case(N, Fin, n1, n3, True)
    y64, _, dW64 = _block_cpu(x, ei, val, W, gout, act, torch.float64)
    y32, _, dW32 = _block_cpu(x, ei, val, W, gout, act, torch.float32)
    y, dx, dW = _block_gpu(dev, x, ei, val, W, gout, act, True, need_dx=False)
    assert dx is None
    _check(y, y64, y32, 'out', 'sum-nodx')
    for k in W:
        _check(dW[k], dW64[k], dW32[k], k, 'sum-nodx')


@pytest.mark.parametrize('shape', [SECOND, SHAPES[1]], ids=['192', '22'])
def test_sum_block_on_strided_views(dev, shape):
    """x as a row-strided view (ldx > Fin) and gout as a column slice of a wider tensor: the same results"""
    N, Fin, n1, n3, act = shape
    ei, val, x, W, gout = _block_case(N, Fin, n1, n3, False)
    y64, dx64, dW64 = _block_cpu(x, ei, val, W, gout, act, torch.float64)
    y32, dx32, dW32 = _block_cpu(x, ei, val, W, gout, act, torch.float32)
    y, dx, dW = _block_gpu(dev, x, ei, val, W, gout, act, False, strided=True)
    _check(y, y64, y32, 'out', 'sum-strided')
    _check(dx, dx64, dx32, 'dx', 'sum-strided')
    for k in W:
        _check(dW[k], dW64[k], dW32[k], k, 'sum-strided')


def test_sum_block_repeats_bitwise(dev):
    """forward and backward twice on the second block with edge values: identical bits, weight gradients included"""
    N, Fin, n1, n3, act = SECOND
    ei, val, x, W, gout = _block_case(N, Fin, n1, n3, False)
    a = _block_gpu(dev, x, ei, val, W, gout, act, False)
    b = _block_gpu(dev, x, ei, val, W, gout, act, False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in W:
        assert torch.equal(a[2][k], b[2][k]), k


@pytest.mark.parametrize('shape', [SECOND, SHAPES[1], SHAPES[3], SHAPES[4]], ids=['192', '22', 'one_row', '145'])
def test_recorded_pattern_equals_the_recomputed_one(dev, shape):
    """relu: phase 1 of the backward from the pattern the forward recorded (the default) and from recomputed a, c (record=False, the
    road tanh takes): the same g4, so every gradient is equal bit for bit"""
    N, Fin, n1, n3, act = shape
    assert act == 1
    ei, val, x, W, gout = _block_case(N, Fin, n1, n3, False)
    a = _block_gpu(dev, x, ei, val, W, gout, act, False)
    b = _block_gpu(dev, x, ei, val, W, gout, act, False, record=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in W:
        assert torch.equal(a[2][k], b[2][k]), k


def test_abi_answers_outside_the_range(dev):
    """GML_E_UNSUPPORTED (-2) past the widths, GML_E_BADARG (-1) for n1 != n2 -- before anything is launched"""
    from gnn_matlang_amd import _lib
    L = _lib.lib()
    z = torch.zeros(64, device=dev)
    zi = torch.zeros(4, dtype=torch.int32, device=dev)
    p, pi = z.data_ptr(), zi.data_ptr()
    call = lambda Fin, n1, n2, n3: L.gml_gnnml1_sum_fwd(pi, pi, None, p, Fin, 0, Fin, p, None, n1, p, None, n2, p, None, p, None, n3, 1,
                                                        p, n1 + n3, None, 0, None)
    assert call(192, 128, 128, 64) == 0                          # (no rows: nothing to do)
    assert call(193, 128, 128, 64) == -2 and call(192, 129, 129, 64) == -2 and call(192, 128, 128, 65) == -2
    assert call(192, 128, 64, 64) == -1


# ------------------------------------------------------------------------------------------------ the model, restated
def _model_ref(P, nblocks, x, ei, ptr):
    """enzymes_contfeat.py:318-346 (dropout 0, training mode: BatchNorm on batch statistics) in plain torch, in the dtype of x and P"""
    ones = torch.ones(ei.size(1), 1, dtype=x.dtype)
    for i in range(1, nblocks + 1):
        lin = lambda j: F.linear(x, P['fc%d%d.weight' % (i, j)], P['fc%d%d.bias' % (i, j)])
        h = torch.zeros_like(x).index_add_(0, ei[1], ones * x[ei[0]])
        c = h @ P['conv%d1.weight' % i][0] + P['conv%d1.bias' % i]
        x = torch.cat([F.relu(lin(1)) + F.relu(c), F.relu(lin(2)) * F.relu(lin(3))], 1)
        x = F.batch_norm(x, None, None, P['bn%d.weight' % i], P['bn%d.bias' % i], training=True)
    seg = [x[ptr[g]:ptr[g + 1]] for g in range(len(ptr) - 1)]
    x = torch.cat([torch.stack([s.mean(0) for s in seg]), torch.stack([s.max(0).values for s in seg])], 1)
    return F.log_softmax(F.linear(x, P['fc2.weight'], P['fc2.bias']), 1)


_HOST = {}


def _host_batch():
    """16 real ENZYMES graphs (0, 37, 74, ...) with all 21 features and the degree, standardised by the graphs with index % 10 != 0;
    collated once and shared by the tests"""
    from gnn_matlang_amd import collate, readers
    if 'b' not in _HOST:
        raw = readers.load_tu(os.path.join(GOLDEN, 'raw', 'enzymes.mat'), 'enzymes', contfeat=True)
        gs = []
        for x, ei, y in raw:                                     # SpectralDesign(adddegree=True): the degree as one more column
            deg = np.bincount(ei[0], minlength=x.shape[0]).astype(np.float32)
            gs.append(dict(x=np.concatenate((x, deg[:, None]), 1), edge_index=ei, y=y))
        gs, _ = readers.standardize_tu(gs, [i for i in range(len(gs)) if i % 10 != 0])
        _HOST['b'] = collate([gs[i] for i in range(0, 16 * 37, 37)])
    return _HOST['b']


def test_model_vs_fp64(dev):
    """enzymes_contfeat_gnnml1 (dropout 0, training mode) on 16 real graphs: logits, tu_step_loss and every parameter gradient against
    the script's forward restated in float64; both blocks run on the fused kernel"""
    from gnn_matlang_amd import functional as Fn, models
    host = _host_batch()
    assert tuple(host.x.shape) == (657, 22) and host.edge_index.size(1) == 2024 and host.y.numel() == 16
    torch.manual_seed(3)
    m = models.enzymes_contfeat_gnnml1(dropout=0.0).to(dev).train()
    data = host.to(dev)
    for fin in (22, 192):
        assert Fn.gnnml1_block_supported(data.x, fin, 128, 128, 64, 4), fin
    pre = m(data)
    loss = models.tu_step_loss(m, data)
    loss.backward()
    ref = {}
    for dt in (torch.float64, torch.float32):
        P = {k: v.detach().cpu().to(dt).requires_grad_(v.dtype.is_floating_point) for k, v in m.state_dict().items()}
        pr = _model_ref(P, 2, host.x.to(dt), host.edge_index, host.ptr.tolist())
        lr = F.nll_loss(pr, host.y.long(), reduction='sum')
        lr.backward()
        ref[dt] = (pr.detach(), lr.detach(), P)
    p64, l64, P64 = ref[torch.float64]
    p32, l32, P32 = ref[torch.float32]
    _check(pre, p64, p32, 'output', 'model')
    _check(loss.reshape(1), l64.reshape(1), l32.reshape(1), 'loss', 'model')
    names = [n for n, _ in m.named_parameters()]
    assert len(names) == 22
    for n, q in m.named_parameters():
        _check(q.grad, P64[n].grad, P32[n].grad, 'grad ' + n, 'model')


# ------------------------------------------------------------------------------------------------ the remaining roads
def test_outside_the_range_runs_on_the_composition(dev):
    """n1 = n2 = 129 is past the kernel: the model runs on the composition and matches the restatement at the general conv kernels'
    documented bound, the project's 1e-4; n1 != n2 is no sum form at all"""
    from gnn_matlang_amd import functional as Fn, models
    host = _host_batch()
    data = host.to(dev)
    assert not Fn.gnnml1_block_supported(data.x, 22, 129, 129, 64, 4) and not Fn.gnnml1_block_supported(data.x, 193, 128, 128, 64, 4)
    torch.manual_seed(4)
    m = models.GNNML1Blocks(22, (129, 129, 64), 2, form='sum_factors', bn_after=(1, 2), nbn=2, pool=('mean', 'max'), head='log_softmax',
                            nclass=6).to(dev).train()
    pre = m(data)
    P = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    p64 = _model_ref(P, 2, host.x.double(), host.edge_index, host.ptr.tolist())
    e = rel_err(pre.detach().cpu().double().numpy(), p64.numpy())
    print('outside (129, 129, 64): err %.3e' % e)
    assert e <= 1e-4
    with pytest.raises(ValueError):
        models.GNNML1Blocks(22, (128, 64, 64), 2, form='sum_factors')


def test_composition_via_environment_equals_the_fused_road(dev, tmp_path):
    """GML_NO_GNNML1_FUSED=1 in a fresh process: the same model on the composition, its output within 2e-5 of the fused road's"""
    from gnn_matlang_amd import models
    torch.manual_seed(3)
    m = models.enzymes_contfeat_gnnml1(dropout=0.0).to(dev).train()
    with torch.no_grad():
        fused = m(_host_batch().to(dev)).cpu()
    out = str(tmp_path / 'composition.pt')
    code = ("import sys, torch\n"
            "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_gnnml1_sum as T\n"
            "from gnn_matlang_amd import functional as Fn, models\n"
            "d = torch.device('cuda:0')\n"
            "data = T._host_batch().to(d)\n"
            "assert not Fn.gnnml1_block_supported(data.x, 22, 128, 128, 64, 4)\n"
            "torch.manual_seed(3)\n"
            "m = models.enzymes_contfeat_gnnml1(dropout=0.0).to(d).train()\n"
            "with torch.no_grad():\n"
            "    torch.save(m(data).cpu(), %r)\n" % (ROOT, os.path.join(ROOT, 'tests'), out))
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, GML_NO_GNNML1_FUSED='1'), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    comp = torch.load(out)
    e = rel_err(comp.double().numpy(), fused.double().numpy())
    print('composition against fused: %.3e' % e)
    assert e <= TOL


def test_dropout_eval_is_the_plain_model_and_training_is_not(dev):
    from gnn_matlang_amd import models
    data = _host_batch().to(dev)
    torch.manual_seed(6)
    a = models.enzymes_contfeat_gnnml1(dropout=0.0).to(dev)
    b = models.enzymes_contfeat_gnnml1().to(dev)
    assert b.dropout == 0.2 and 'dropout_state' not in dict(a.named_buffers())
    b.load_state_dict(a.state_dict())                            # (dropout_state is a non-persistent buffer)
    a.eval()
    b.eval()
    with torch.no_grad():
        assert torch.equal(a(data), b(data))
    a.train()
    b.train()
    with torch.no_grad():
        ya, yb = a(data), b(data)
    assert torch.isfinite(yb).all() and not torch.equal(ya, yb)
