"""GNNML1 block mode 5 (form 'act_sum', filtering.py:246-248) restated in plain torch WITH its gradients written out, the cases the
GPU tests hold the fused block to, and the filtering GNNML1 as a composition.  Shared by tests/test_filtering_gnnml1_cpu.py (which
checks this restatement against autograd) and tests/test_gpu_gnnml1_actsum.py; no device is touched on import.

    out = relu(a) + relu(c) + relu(f2 f3),   a = fc_i1 x, c = (A^T x) Wc + bc, f2 = fc_i2 x, f3 = fc_i3 x

The seeds of CASES are chosen so that the float32 and the float64 evaluation agree on all three relu patterns (no pre-activation so
close to zero that the number format decides a bit); SEPARATION's seed so that each of the eight sign combinations of (a, c, f2 f3)
covers more than 5 % of the entries.  Both conditions are asserted where the cases are used."""
import numpy as np
import torch
import torch.nn.functional as F

from _gnnml1_ref import graph

# (N, Fin, n, unit edge values, seed)
CASES = [(1, 1, 32, True, 1),        # one row, a self loop
         (77, 1, 32, True, 2),       # the first block's width, a partial tile
         (130, 32, 32, True, 3),     # the later blocks
         (130, 32, 32, False, 4),    # ... with random edge values
         (97, 20, 24, True, 5),      # widths that are no multiples of 16 or 4
         (64, 64, 64, True, 6),      # the limit of the 64-feature instantiation
         (40, 144, 64, True, 7),     # the limit of the kernel
         (50, 96, 32, True, 8),      # the 96- and the 112-feature instantiations
         (50, 112, 48, True, 9)]
SEPARATION = (130, 32, 32, True, 3)


def case(N, Fin, n, unit, seed):
    g = torch.Generator().manual_seed(1000 * seed + N + Fin)
    ei = graph(N, seed)
    E = ei.size(1)
    r = lambda *s: torch.randn(*s, generator=g)
    val = torch.ones(E) if unit else r(E)
    x = r(N, Fin)
    s = 1.0 / np.sqrt(Fin)
    W = dict(w1=r(n, Fin) * s, b1=r(n) * 0.1, wc=r(1, Fin, n) * s * 0.5, bc=r(n) * 0.1,
             w2=r(n, Fin) * s, b2=r(n) * 0.1, w3=r(n, Fin) * s, b3=r(n) * 0.1)
    return x, ei, val, W, r(N, n)                              # (the argument order of block / block_autograd)


def block(x, ei, val, W, gout, dtype):
    """forward and backward by their formulas in `dtype`: dict(out, dx, grads, pa, pc, pp) -- pa, pc, pp: the patterns a > 0, c > 0,
    f2 f3 > 0 (relu'(0) = 0)"""
    x, val, gout = x.to(dtype), val.to(dtype), gout.to(dtype)
    W = {k: v.to(dtype) for k, v in W.items()}
    h = torch.zeros_like(x).index_add_(0, ei[1], val.unsqueeze(1) * x[ei[0]])      # aggregation at the TARGET (libs/spect_conv.py:98-99)
    a, c = x @ W['w1'].t() + W['b1'], h @ W['wc'][0] + W['bc']
    f2, f3 = x @ W['w2'].t() + W['b2'], x @ W['w3'].t() + W['b3']
    pa, pc, pp = a > 0, c > 0, f2 * f3 > 0
    zero = torch.zeros((), dtype=dtype)
    out = torch.where(pa, a, zero) + torch.where(pc, c, zero) + torch.where(pp, f2 * f3, zero)
    da, dc, g = torch.where(pa, gout, zero), torch.where(pc, gout, zero), torch.where(pp, gout, zero)
    d2, d3 = g * f3, g * f2
    q = torch.zeros_like(dc).index_add_(0, ei[0], val.unsqueeze(1) * dc[ei[1]])      # q = A dc
    dx = da @ W['w1'] + q @ W['wc'][0].t() + d2 @ W['w2'] + d3 @ W['w3']
    grads = dict(w1=da.t() @ x, b1=da.sum(0), wc=(h.t() @ dc).unsqueeze(0), bc=dc.sum(0), w2=d2.t() @ x, b2=d2.sum(0),
                 w3=d3.t() @ x, b3=d3.sum(0))
    return dict(out=out, dx=dx, grads=grads, pa=pa, pc=pc, pp=pp)


def block_autograd(x, ei, val, W, gout, dtype, form='act_sum'):
    """the same block from torch.nn.functional and autograd (form 'sum': relu(a + c + f2 f3), kernel mode 0, for contrast)"""
    xr = x.detach().to(dtype).clone().requires_grad_(True)
    P = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in W.items()}
    msg = val.to(dtype).unsqueeze(1) * xr[ei[0]]
    h = torch.zeros(xr.shape, dtype=dtype).index_add_(0, ei[1], msg)
    a, c = F.linear(xr, P['w1'], P['b1']), h @ P['wc'][0] + P['bc']
    f2, f3 = F.linear(xr, P['w2'], P['b2']), F.linear(xr, P['w3'], P['b3'])
    y = F.relu(a) + F.relu(c) + F.relu(f2 * f3) if form == 'act_sum' else F.relu(a + c + f2 * f3)
    (y * gout.to(dtype)).sum().backward()
    return y.detach(), xr.grad, {k: v.grad for k, v in P.items()}


def patterns_agree(r32, r64):
    return all(torch.equal(r32[k], r64[k]) for k in ('pa', 'pc', 'pp'))


def combination_shares(r):
    """share of the entries in each of the eight sign combinations of (a, c, f2 f3)"""
    code = r['pa'].long() * 4 + r['pc'].long() * 2 + r['pp'].long()
    return np.bincount(code.reshape(-1).numpy(), minlength=8) / float(code.numel())


def pattern_bytes(r):
    """the bytes the forward records: [N, 4 ceil(n / 16)], byte j: bit u = a > 0, bit 4 + u = c > 0 of column 4 j + u"""
    N, n = r['pa'].shape
    npad = (n + 15) // 16 * 16
    pa, pc = torch.zeros(N, npad, dtype=torch.int64), torch.zeros(N, npad, dtype=torch.int64)
    pa[:, :n], pc[:, :n] = r['pa'], r['pc']
    w = torch.tensor([1, 2, 4, 8])
    return ((pa.view(N, -1, 4) * w).sum(2) + 16 * (pc.view(N, -1, 4) * w).sum(2)).to(torch.uint8)


# ------------------------------------------------------------------------------------------------ the model, restated
def grid_edges(a, b):
    """the raw adjacency of an a x b grid, np.where(A > 0) as libs/utils.py builds it"""
    idx = np.arange(a * b).reshape(a, b)
    e = np.concatenate([np.stack([idx[:-1].ravel(), idx[1:].ravel()]), np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()])], 1)
    A = np.zeros((a * b, a * b), dtype=np.int64)
    A[e[0], e[1]] = A[e[1], e[0]] = 1
    r, c = np.where(A > 0)
    return np.vstack((r, c)).astype(np.int64)


def model_ref(P, x, ei, y, mask, ntask, concat=False, act=F.relu):
    """filtering.py:234-250 and its masked square loss (:320) in the dtype of x and P: (pre, loss, [loss, ss_res, ss_tot, count])"""
    for i in (1, 2, 3):
        lin = lambda j: F.linear(x, P['fc%d%d.weight' % (i, j)], P['fc%d%d.bias' % (i, j)])
        h = torch.zeros_like(x).index_add_(0, ei[1], x[ei[0]])
        c = h @ P['conv%d1.weight' % i][0] + P['conv%d1.bias' % i]
        parts = [act(lin(1)), act(c), act(lin(2) * lin(3))]
        x = torch.cat(parts, 1) if concat else parts[0] + parts[1] + parts[2]
    pre = F.linear(x, P['fc2.weight'], P['fc2.bias'])
    yt = y[:, ntask:ntask + 1]
    loss = torch.square(mask * (pre - yt)).sum()
    sel = mask[:, 0] == 1
    ss_res = torch.square(yt[sel] - pre[sel]).sum()
    ss_tot = torch.square(yt[sel] - yt[sel].mean()).sum()
    return pre, loss, torch.stack([loss.detach(), ss_res.detach(), ss_tot.detach(), sel.sum().to(x.dtype)])
