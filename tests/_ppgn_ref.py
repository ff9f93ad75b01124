"""PPGN restated in plain torch (inputs, one block, the whole model), run in float64 and float32, and the random block cases the
GPU tests hold the fused block to.  Shared by tests/test_ppgn_cpu.py and tests/test_gpu_ppgn.py; no device is touched on import.

A block case is redrawn until (a) no pre-activation of the float64 restatement lies within 1e-4 of its tensor's max-abs from zero
on a real pixel -- a condition, not a measurement: the relu patterns must not hang on the number format -- and (b) the float32 and
float64 patterns agree."""
import numpy as np
import torch

READOUTS = ('sum', 'mean', 'diag')
MARGIN = 1e-4


def mask(n, nmax, dtype):
    """[B, 1, nmax, nmax]: 1 where i < n_g and j < n_g"""
    inside = torch.arange(nmax).view(1, -1) < torch.as_tensor(n).view(-1, 1)
    return (inside.unsqueeze(2) & inside.unsqueeze(1)).to(dtype).unsqueeze(1)


def block_parts(x, n, W):
    """pre-activations z1, z2, z3 (masked) and the block output; W: w1, w2 [C, Cin], w3 [C, C + Cin], b1..b3 [C] or None"""
    m = mask(n, x.size(-1), x.dtype)
    lin = lambda t, w, b: torch.einsum('oc,bcij->boij', w, t) + (0 if b is None else b.view(1, -1, 1, 1))
    z1 = lin(x, W['w1'], W['b1']) * m
    z2 = lin(x, W['w2'], W['b2']) * m
    p = torch.matmul(torch.relu(z1), torch.relu(z2)) * m
    z3 = lin(torch.cat([p, x], 1), W['w3'], W['b3']) * m
    return z1, z2, z3, torch.relu(z3), m


def readout_of(y, m, readout):
    nmax = y.size(-1)
    eye = torch.eye(nmax, dtype=y.dtype)
    m0, m1 = m * eye, m * (1 - eye)
    r0, r1 = (y * m0).sum((2, 3)), (y * m1).sum((2, 3))
    if readout == 'diag':
        return r0
    if readout == 'mean':
        return torch.cat([r0 / m0.sum((2, 3)), r1 / m1.sum((2, 3))], 1)         # n = 1: 0 / 0, as exp_classify.py:60
    return torch.cat([r0, r1], 1)


def readout_rows_then_cols(y, m):
    """sr25.py:52, 70: sum over rows per block, then over columns after the concatenation"""
    nmax = y.size(-1)
    eye = torch.eye(nmax, dtype=y.dtype)
    return torch.cat([torch.sum(y * (m * eye), 2), torch.sum(y * (m * (1 - eye)), 2)], 1).sum(2)


def block_ref(x, n, W, readout='sum'):
    _, _, _, y, m = block_parts(x, n, W)
    return y, readout_of(y, m, readout)


def block_cpu(x, n, W, gy, gr, readout, dtype, need_dx=True):
    """the restatement with autograd: (y, r, dx, grads of W) for the loss sum(y gy) + sum(r gr)"""
    xr = x.detach().to(dtype).clone().requires_grad_(need_dx)
    Wr = {k: (None if v is None else v.detach().to(dtype).clone().requires_grad_(True)) for k, v in W.items()}
    y, r = block_ref(xr, n, Wr, readout)
    ((y * gy.to(dtype)).sum() + (r * gr.to(dtype)[:, :r.size(1)]).sum()).backward()
    return y.detach(), r.detach(), xr.grad, {k: (None if v is None else v.grad) for k, v in Wr.items()}


def _margins_ok(x, n, W):
    z64 = block_parts(x.double(), n, {k: (None if v is None else v.double()) for k, v in W.items()})
    z32 = block_parts(x, n, W)
    m = z64[4].bool()
    for a, b in zip(z64[:3], z32[:3]):
        mm = m.expand_as(a)
        va = a[mm]
        if va.numel() == 0:
            continue
        if float(va.abs().min()) <= MARGIN * float(va.abs().max()):
            return False
        if not torch.equal(va > 0, b[mm] > 0):
            return False
    return True


def block_case(B, nmax, nlist, Cin, C, bias, seed=0):
    """x [B, Cin, nmax, nmax] random, not symmetric, with random NON-ZERO values in the padding; weights, biases (or None) and the
    output gradients gy [B, C, nmax, nmax] (non-zero in the padding too) and gr [B, 2C]"""
    if nlist == 'random':
        nlist = np.random.default_rng(1000 + seed).integers(1, nmax + 1, B).tolist()
    assert len(nlist) == B and all(1 <= v <= nmax for v in nlist)
    n = torch.tensor(nlist, dtype=torch.int32)
    inside = mask(n, nmax, torch.float32)
    for attempt in range(200):
        g = torch.Generator().manual_seed(7919 * seed + 31 * attempt + B + nmax + Cin + C)
        # Continuous random data cannot meet the margin at these sizes (10^5 .. 10^6 pre-activations per case: some always fall
        # within 1e-4 of zero), so the case lives on a grid that keeps every pre-activation an odd multiple of 1/2: channel 0 of x
        # is +-1/2 and meets weights +-1, every other input, weight and bias is an integer, and the weights on the product p (whose
        # quantum is 1/4) are multiples of 4.  The values stay random, sparse like the real inputs, and not symmetric; the
        # conditions are still verified below, and the gradients gy, gr are continuous.
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
        sign = lambda *s: ri(0, 1, *s) * 2 - 1
        sparse = lambda dens, *s: sign(*s) * (torch.rand(*s, generator=g) < dens).float()
        x = sparse(0.5, B, Cin, nmax, nmax)
        pad = sign(B, Cin, nmax, nmax) * ri(1, 2, B, Cin, nmax, nmax)                # the padding: random, never zero
        x = x * inside + pad * (1 - inside)
        x[:, 0] = sign(B, nmax, nmax) * 0.5
        dw = min(1.0, 6.0 / Cin)
        W = dict(w1=sparse(dw, C, Cin), w2=sparse(dw, C, Cin), w3=torch.cat([4 * sparse(min(1.0, 3.0 / C), C, C), sparse(dw, C, Cin)], 1))
        W['w1'][:, 0], W['w2'][:, 0], W['w3'][:, C] = sign(C), sign(C), sign(C)
        for k in ('b1', 'b2', 'b3'):
            W[k] = ri(-1, 1, C) if bias else None
        gy = torch.randn(B, C, nmax, nmax, generator=g)
        gr = torch.randn(B, 2 * C, generator=g)
        if _margins_ok(x, n, W):
            return x, n, W, gy, gr
    raise AssertionError('no block case with relu margins found')


def inputs_ref(graphs, nmax, nfeat):
    """ppgn_inputs_host per graph, stacked: X2 [B, nfeat + 2, nmax, nmax], M [B, 2, nmax, nmax], n [B]"""
    from gnn_matlang_amd.ppgn import ppgn_inputs_host
    X2, M, n = zip(*(ppgn_inputs_host(g['x'], g['edge_index'], nmax, nfeat) for g in graphs))
    return np.stack(X2), np.stack(M), np.asarray(n, dtype=np.int32)


def state_W(sd, b, dtype):
    """the weights of block b of a models.PPGN state_dict as block_parts takes them"""
    g = lambda k: sd[k].detach().cpu().to(dtype) if k in sd else None
    out = {}
    for i in (1, 2, 3):
        w = g('mlp%d_%d.weight' % (b, i))
        out['w%d' % i] = w.reshape(w.size(0), w.size(1))
        out['b%d' % i] = g('mlp%d_%d.bias' % (b, i))
    return out


def model_ref(params, nblocks, X2, n, readout, head_act, dtype):
    """the whole model on the CPU from a dict of parameters (leaves that may require grad): (pooled readouts, output)"""
    x = torch.as_tensor(X2).to(dtype)
    outs = []
    for b in range(1, nblocks + 1):
        W = {}
        for i in (1, 2, 3):
            w = params['mlp%d_%d.weight' % (b, i)]
            W['w%d' % i] = w.reshape(w.size(0), w.size(1))
            W['b%d' % i] = params.get('mlp%d_%d.bias' % (b, i))
        x, r = block_ref(x, n, W, readout)
        outs.append(r)
    pooled = torch.cat(outs, 1)
    h = pooled @ params['h1.weight'].t() + params['h1.bias']
    if head_act is not None:
        h = torch.tanh(h) if head_act == 'tanh' else torch.relu(h)
    if 'h2.weight' in params:
        h = h @ params['h2.weight'].t() + params['h2.bias']
    return pooled, h
