"""gml_dropout_fwd / gml_dropout_bwd (csrc/gml_dropout.hip) against the CPU restatement of the mask contract (tests/_philox.py):
mask bits and outputs bitwise, the backward, the keep fraction, and the no-launch cases."""
import numpy as np
import pytest
import torch

import _philox

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


def _mask_bits(mask, n):
    """bool [n] of a packed device mask"""
    w = mask.cpu().numpy().view(np.uint32)
    assert w.size == (n + 31) // 32
    return ((w[:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(-1)[:n]


def _state(seed, counter, dev):
    from gnn_matlang_amd import functional as Fn
    st = Fn.dropout_state(seed, dev)
    st[1] = counter if counter < 2 ** 63 else counter - 2 ** 64
    return st


@pytest.mark.parametrize('C', [1, 3, 4, 20, 80])
@pytest.mark.parametrize('seed,counter,site,p', [(0, 0, 0, 0.2), (0x0123456789abcdef, 5, 3, 0.1),
                                                 (2 ** 64 - 1, 2 ** 32 + 7, 7, 0.5), (17, 1, 0, 0.9)])
def test_mask_and_output_bitwise_equal_to_the_restatement(dev, C, seed, counter, site, p):
    from gnn_matlang_amd import functional as Fn
    N = 1037                                               # N C is not a multiple of 32 for C = 1, 3, 20
    torch.manual_seed(C)
    x = torch.randn(N, C, device=dev) * 3
    st = _state(seed, counter, dev)
    y, mask = Fn.dropout_fwd(x, p, st, site)
    keep = _philox.keep_mask(N, C, p, seed, counter, site)
    assert np.array_equal(_mask_bits(mask, N * C), keep.reshape(-1))
    assert np.array_equal(mask.cpu().numpy().view(np.uint32), _philox.pack(keep))          # unused high bits are 0
    want = _philox.apply(x.cpu().numpy(), keep, p)
    assert np.array_equal(y.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert st.cpu().tolist() == _state(seed, counter, 'cpu').tolist()                       # the kernel does not touch the state


@pytest.mark.parametrize('C,ldx', [(4, 12), (20, 24), (3, 7), (20, 21)])
def test_strided_rows(dev, C, ldx):
    """row-strided inputs (float4-addressable or not): the mask depends on the logical index only"""
    from gnn_matlang_amd import functional as Fn
    N = 301
    base = torch.randn(N, ldx, device=dev)
    x = base[:, :C]
    st = _state(99, 4, dev)
    y, mask = Fn.dropout_fwd(x, 0.3, st, 2)
    y2, mask2 = Fn.dropout_fwd(x.contiguous(), 0.3, st, 2)
    keep = _philox.keep_mask(N, C, 0.3, 99, 4, 2)
    assert torch.equal(mask, mask2)
    assert np.array_equal(_mask_bits(mask, N * C), keep.reshape(-1))
    want = _philox.apply(x.cpu().numpy(), keep, 0.3)
    assert np.array_equal(y.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert torch.equal(y, y2)


def test_dropped_elements_are_plus_zero_and_p_one(dev):
    from gnn_matlang_amd import functional as Fn
    x = torch.tensor([[float('nan'), float('inf'), -0.0, -2.0]] * 64, device=dev)
    st = _state(5, 1, dev)
    y, mask = Fn.dropout_fwd(x, 0.5, st, 0)
    keep = _philox.keep_mask(64, 4, 0.5, 5, 1, 0)
    assert keep.any() and (~keep).any()
    yb = y.cpu().numpy().view(np.uint32)
    assert (yb[~keep] == 0).all()                          # +0.0 bit pattern, not NaN / -0.0
    y1, m1 = Fn.dropout_fwd(x, 1.0, st, 0)
    assert (y1.cpu().numpy().view(np.uint32) == 0).all() and int(m1.abs().sum()) == 0
    with pytest.raises(ValueError):
        Fn.dropout(x, -0.5, True, st)


def test_empty_inputs(dev):
    from gnn_matlang_amd import functional as Fn
    st = _state(1, 1, dev)
    for shape in ((0, 4), (0, 3), (5, 0)):
        x = torch.empty(*shape, device=dev)
        y, mask = Fn.dropout_fwd(x, 0.4, st, 0)
        assert tuple(y.shape) == shape and mask.numel() == 0
        assert tuple(Fn.dropout_bwd(x, mask, 0.4).shape) == shape


@pytest.mark.parametrize('C', [1, 3, 4, 20, 80])
def test_backward_is_the_masked_scaled_gradient(dev, C):
    from gnn_matlang_amd import functional as Fn
    N, p = 777, 0.2
    x = torch.randn(N, C, device=dev, requires_grad=True)
    st = _state(1234, 9, dev)
    y = Fn.dropout(x, p, True, st, site=1)
    _, mask = Fn.dropout_fwd(x.detach(), p, st, 1)
    st[1] += 1                                             # a later change of the state does not affect the backward
    g = torch.randn(N, C, device=dev)
    y.backward(g)
    keep = torch.from_numpy(_mask_bits(mask, N * C).reshape(N, C)).to(dev)
    scale = torch.tensor(float(_philox.scale(p)), device=dev)
    want = torch.where(keep, g * scale, torch.zeros((), device=dev))
    assert torch.equal(x.grad.view(torch.int32), want.view(torch.int32))
    gs = torch.randn(N, C + 5, device=dev)[:, :C]          # a row-strided gradient
    dx = Fn.dropout_bwd(gs, mask, p)
    assert torch.equal(dx, torch.where(keep, gs * scale, torch.zeros((), device=dev)))


def test_eval_and_p_zero_return_the_input_and_launch_nothing(dev):
    from gnn_matlang_amd import functional as Fn
    x = torch.randn(64, 20, device=dev, requires_grad=True)
    st = _state(3, 0, dev)
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        a = Fn.dropout(x, 0.5, False, st)
        b = Fn.dropout(x, 0.0, True, st)
        torch.cuda.synchronize()
    assert a is x and b is x
    assert not [e for e in prof.events() if 'dropout' in e.name]
    c = Fn.dropout(x, 0.5, True, st)
    assert c is not x and c.data_ptr() != x.data_ptr()


@pytest.mark.parametrize('p', [0.1, 0.2, 0.5])
def test_keep_fraction(dev, p):
    """2^26 elements: the kept fraction within 6 sigma of 1 - p; different sites / counters give different masks"""
    from gnn_matlang_amd import functional as Fn
    N, C = 2 ** 20, 64
    x = torch.ones(N, C, device=dev)
    st = _state(2024, 3, dev)
    y, mask = Fn.dropout_fwd(x, p, st, 0)
    n = N * C
    kept = int((y != 0).sum())
    sigma = (n * p * (1 - p)) ** 0.5
    assert abs(kept - n * (1 - p)) <= 6 * sigma, (kept, n * (1 - p), sigma)
    bits = int(np.unpackbits(mask.cpu().numpy().view(np.uint8)).sum())
    assert bits == kept
    _, m_site = Fn.dropout_fwd(x, p, st, 1)
    st2 = _state(2024, 4, dev)
    _, m_ctr = Fn.dropout_fwd(x, p, st2, 0)
    _, m_same = Fn.dropout_fwd(x, p, _state(2024, 3, dev), 0)
    assert torch.equal(mask, m_same)
    for other in (m_site, m_ctr):
        assert float((mask != other).float().mean()) > 0.5
