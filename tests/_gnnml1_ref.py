"""One GNNML1 block restated in plain torch for all five forms (kernel modes 0..4 of functional.GNNML1BlockFunction), the random
cases the GPU tests hold the fused block to, and the checker.  Shared by tests/test_gpu_gnnml1_wide.py (modes 0..3) and
tests/test_gpu_gnnml1_sum.py (mode 4); no device is touched on import.

Tolerance: the project's bound for exact fp32 products, max|got - ref64| <= 2e-5 max|ref64| per tensor (TOL).  check(computed=True)
takes instead 4 x the error of the SAME restatement evaluated by torch in float32 on the CPU against float64 (floor TOL; the factor
4: a different summation order) -- a bound from the number format, never from the code under test."""
import numpy as np
import torch

from conftest import rel_err

TOL = 2e-5


def check(got, ref64, ref32, what, case, tol=TOL, computed=False):
    """max|got - ref64| <= tol max|ref64|, with the figures printed first"""
    g = got.detach().cpu().double().numpy()
    r = ref64.detach().double().numpy()
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert np.isfinite(g).all(), what
    e, e32 = rel_err(g, r), rel_err(ref32.detach().double().numpy(), r)
    if computed:
        tol = max(tol, 4 * e32)
    print('%s %s: err %.3e (float32 restatement %.3e, tol %.1e)' % (case, what, e, e32, tol))
    assert e <= tol, '%s %s: rel err %.3e > %.1e (float32 restatement: %.3e)' % (case, what, e, tol, e32)


def parts_ref(x, ei, v, W):
    """libs/spect_conv.py:98-99 aggregates at the TARGET; the four linears"""
    h = torch.zeros_like(x).index_add_(0, ei[1], v.unsqueeze(1) * x[ei[0]])
    a, c = x @ W['w1'].t() + W['b1'], h @ W['wc'][0] + W['bc']
    f2, f3 = x @ W['w2'].t() + W['b2'], x @ W['w3'].t() + W['b3']
    return a, c, f2, f3


def block_ref(x, ei, v, W, mode, act):
    """the forms (mode 0: sr25.py:231-240; 3: ptc.py:311; 4: enzymes_contfeat.py:336)"""
    A = torch.tanh if act == 0 else torch.relu
    a, c, f2, f3 = parts_ref(x, ei, v, W)
    if mode == 0:
        return A(a + c + f2 * f3)
    if mode == 4:
        return torch.cat([A(a) + A(c), A(f2) * A(f3)], 1)
    third = A(f2 * f3) if mode == 1 else (A(f2) * A(f3) if mode == 2 else torch.tanh(f2) * torch.tanh(f3))
    return torch.cat([A(a), A(c), third], 1)


def out_cols(n1, n2, n3, mode):
    return n1 if mode == 0 else (n1 + n3 if mode == 4 else n1 + n2 + n3)


def graph(N, seed):
    """a directed random graph (its transposed view is another matrix) with node 0 without in-edge, node 1 without out-edge and
    node 2 of in-degree >= 40 (as many as N allows below 42 nodes); N = 1: one self loop"""
    if N == 1:
        return torch.zeros(2, 1, dtype=torch.int64)
    rng = np.random.default_rng(seed)
    src = rng.integers(0, N, size=N * 5)
    dst = np.clip(src + rng.integers(-20, 21, size=src.shape), 0, N - 1)
    hub = rng.permutation(np.arange(2, N))[:min(48, N - 2)]
    src, dst = np.concatenate((src, hub)), np.concatenate((dst, np.full(hub.shape, 2)))
    keep = (dst != 0) & (src != 1)
    ei = np.unique(np.vstack((src[keep], dst[keep])), axis=1).astype(np.int64)
    assert not (ei[1] == 0).any() and not (ei[0] == 1).any() and (ei[1] == 2).sum() >= min(40, N - 3)
    assert not np.array_equal(ei, np.unique(ei[::-1], axis=1))
    return torch.from_numpy(ei)


def block_case(N, Fin, n1, n2, n3, mode, unit):
    torch.manual_seed(N + Fin)
    ei = graph(N, N + Fin)
    E = ei.size(1)
    val = torch.ones(E) if unit else torch.randn(E)
    x = torch.randn(N, Fin)
    W = dict(w1=torch.randn(n1, Fin) * 0.3, b1=torch.randn(n1) * 0.1, wc=torch.randn(1, Fin, n2) * 0.2, bc=torch.randn(n2) * 0.1,
             w2=torch.randn(n3, Fin) * 0.3, b2=torch.randn(n3) * 0.1, w3=torch.randn(n3, Fin) * 0.3, b3=torch.randn(n3) * 0.1)
    gout = torch.randn(N, out_cols(n1, n2, n3, mode))
    return ei, val, x, W, gout


def block_cpu(x, ei, val, W, gout, mode, act, dtype):
    xr = x.detach().to(dtype).clone().requires_grad_(True)      # (fresh leaves: .to() of the same dtype returns its argument)
    Wr = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in W.items()}
    y = block_ref(xr, ei, val.to(dtype), Wr, mode, act)
    (y * gout.to(dtype)).sum().backward()
    return y.detach(), xr.grad, {k: v.grad for k, v in Wr.items()}


def block_gpu(dev, x, ei, val, W, gout, mode, act, unit, need_dx=True, strided=False, record=True):
    from gnn_matlang_amd import functional as Fn
    from gnn_matlang_amd.graph import GraphCSR
    N, Fin = x.shape
    n1, n2, n3 = W['w1'].size(0), W['wc'].size(2), W['w2'].size(0)
    C = out_cols(n1, n2, n3, mode)
    csr = GraphCSR.from_edge_index(ei.to(dev), N)
    if strided:                                                  # x: rows of a wider buffer (ldx > Fin); gout: a column slice
        buf = torch.zeros(N, Fin + 5, device=dev)
        buf[:, :Fin] = x.to(dev)
        xl = buf.requires_grad_(need_dx)
        xd = xl[:, :Fin]
        gbuf = torch.randn(N, C + 7, device=dev)
        gbuf[:, 3:3 + C] = gout.to(dev)
        gd = gbuf[:, 3:3 + C]
        assert xd.stride(0) > Fin and gd.stride(0) > C and not xd.is_contiguous()
    else:
        xl = xd = x.detach().to(dev).requires_grad_(need_dx)
        gd = gout.to(dev)
    Wd = {k: v.detach().to(dev).requires_grad_(True) for k, v in W.items()}
    vs = None if unit else csr.sort_values(val.to(dev).view(-1, 1)).view(-1)
    assert Fn.gnnml1_block_supported(xd, Fin, n1, n2, n3, mode)
    y = Fn.GNNML1BlockFunction.apply(xd, csr, vs, Wd['w1'], Wd['b1'], Wd['wc'], Wd['bc'], Wd['w2'], Wd['b2'], Wd['w3'], Wd['b3'], mode, act,
                                     record)
    assert y.shape == (N, C)
    y.backward(gd)
    dx = xl.grad[:, :Fin] if (strided and need_dx) else xl.grad
    return y.detach(), dx, {k: v.grad for k, v in Wd.items()}
