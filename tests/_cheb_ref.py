"""ChebConv restated in plain torch, dtype-generic and dense per node (no scatter): the arithmetic of torch_geometric 1.6.1's ChebConv
at normalization='sym' as include/gml.h states it for gml_cheb_*.  torch_geometric itself is not available to these tests: this is a
restatement of its arithmetic, not a run of the library.

    A[i, j]  = number of edges (j -> i) with j != i (self loops dropped, repeats counted)
    deg[j]   = sum_i A[i, j] (a node's edges as a SOURCE);  dis = deg^-1/2, 0 where deg = 0
    s[i]     = 2 / lambda_max[batch[i]]   (lambda_max None: 2.0)
    L^[i, j] = -s[i] dis[i] A[i, j] dis[j],  L^[i, i] = s[i] - 1
    Tx_0 = x, Tx_1 = L^ x, Tx_k = 2 L^ Tx_{k-1} - Tx_{k-2};  y = act(bias + sum_k Tx_k W_k)

forward(): the above; backward(): the adjoint recurrence of the issue (g = dy act'(y), dW_k = Tx_k^T g, db = sum g, G_{K-1} = g W_{K-1}^T,
G_k = g W_k^T + c_k L^T G_{k+1} - G_{k+2} with c_0 = 1 and c_k = 2 otherwise, dx = G_0); chebnet_ref(): the ChebNet of the experiment
scripts on top.  The cases of the GPU layer matrix and their kink margins live here so that tests/test_cheb_cpu.py can verify the
margins without a device."""
import numpy as np
import torch

import _gat_ref as G
import _gin_ref as GI

ACTS = (None, 'relu', 'tanh')
MARGIN = G.MARGIN                 # kink margin: for relu every pre-activation >= MARGIN x max-abs away from 0
act_fn, dact_from_y = GI.act_fn, GI.dact_from_y


def adjacency(ei, N, dtype):
    """A [N target, N source]: edge multiplicities, self loops DROPPED"""
    ei = torch.as_tensor(ei, dtype=torch.int64)
    keep = ei[0] != ei[1]
    A = torch.zeros(N, N, dtype=dtype)
    A.index_put_((ei[1][keep], ei[0][keep]), torch.ones(int(keep.sum()), dtype=dtype), accumulate=True)
    return A


def laplacian(ei, N, batch, lam, dtype):
    """L^ [N, N] of the docstring; batch [N] int64 or None, lam: None, a float or a tensor [B]"""
    A = adjacency(ei, N, dtype)
    deg = A.sum(0)
    dis = torch.where(deg > 0, deg.clamp(min=1).pow(-0.5), torch.zeros_like(deg))
    if lam is None:
        s = torch.ones(N, dtype=dtype)
    elif isinstance(lam, torch.Tensor):
        s = 2.0 / lam.to(dtype)[torch.as_tensor(batch, dtype=torch.int64)]
    else:
        s = torch.full((N,), 2.0 / float(lam), dtype=dtype)
    return -(s * dis).unsqueeze(1) * A * dis.unsqueeze(0) + torch.diag(s - 1)


def recurrence(x, L, K):
    tx = [x]
    if K > 1:
        tx.append(L @ x)
    for _ in range(2, K):
        tx.append(2 * (L @ tx[-1]) - tx[-2])
    return tx


def forward(x, L, W, b, act, parts=False):
    """W [K, Fin, Fout], b [Fout] or None; parts: (y, [Tx_0 .. Tx_{K-1}], pre)"""
    tx = recurrence(x, L, W.size(0))
    pre = sum(t @ W[k] for k, t in enumerate(tx))
    if b is not None:
        pre = pre + b
    y = act_fn(pre, act)
    return (y, tx, pre) if parts else y


def backward(x, L, W, b, act, dy):
    """dict(dx, dW, db) by the adjoint recurrence"""
    y, tx, _ = forward(x, L, W, b, act, parts=True)
    K = W.size(0)
    g = dy * dact_from_y(y, act)
    Gs = [None] * (K + 2)
    for k in range(K - 1, -1, -1):
        v = g @ W[k].t()
        if Gs[k + 1] is not None:
            v = v + (1 if k == 0 else 2) * (L.t() @ Gs[k + 1])
        if Gs[k + 2] is not None:
            v = v - Gs[k + 2]
        Gs[k] = v
    return dict(dx=Gs[0], dW=torch.stack([t.t() @ g for t in tx]), db=g.sum(0))


class AnalyticCheb(torch.autograd.Function):
    """forward() with backward() as its gradient: what gradcheck holds against finite differences.  leaves: x, W, b"""

    @staticmethod
    def forward(ctx, L, act, x, W, b):
        ctx.save_for_backward(L, x, W, b)
        ctx.act = act
        return forward(x, L, W, b, act)

    @staticmethod
    def backward(ctx, dy):
        L, x, W, b = ctx.saved_tensors
        d = backward(x, L, W, b, ctx.act, dy)
        return None, None, d['dx'], d['dW'], d['db']


# ---------------------------------------------------------------------------------------------------------------- graphs
GRAPHS = dict(G.GRAPHS, loops=GI.self_loops)
NO_LAMBDA = 'hand'                 # the graph whose cases pass lambda_max=None
SHAPES = [(3, 1, 1), (25, 64, 2), (7, 33, 3), (2, 32, 4), (32, 64, 5), (48, 48, 5), (1, 64, 7), (64, 64, 8)]    # (Fin, Fout, K)
_GRAPH_CACHE = {}


def lambda_of(ei, n):
    """the largest eigenvalue of the graph's own I - D^-1/2 A D^-1/2 in float64 (eigvalsh; a graph that is not symmetric: the largest
    singular value, which bounds |L^| the same way and is the same number on a symmetric graph)"""
    A = adjacency(ei, n, torch.float64)
    deg = A.sum(0)
    dis = torch.where(deg > 0, deg.clamp(min=1).pow(-0.5), torch.zeros_like(deg))
    Ln = torch.eye(n, dtype=torch.float64) - dis.unsqueeze(1) * A * dis.unsqueeze(0)
    if torch.equal(Ln, Ln.t()):
        return float(torch.linalg.eigvalsh(Ln).max())
    return float(torch.linalg.matrix_norm(Ln, 2))


def _segments(name, N):
    """the node ranges of the graphs of a named batch: mutag16 its 16 molecules, star the star and the path, else one graph"""
    if name == 'mutag16':
        import os
        from conftest import GOLDEN
        from gnn_matlang_amd import readers
        sizes = [x.shape[0] for x, _, _ in readers.load_mutag(os.path.join(GOLDEN, 'raw', 'mutag.mat'))[:16]]
        return np.cumsum([0] + sizes)
    if name == 'star':
        return np.array([0, N - 3, N])
    return np.array([0, N])


def get_graph(name):
    """(edge_index, N, batch int64 [N], lambda_max float64 [B] or None)"""
    if name not in _GRAPH_CACHE:
        ei, N = GRAPHS[name]()
        ptr = _segments(name, N)
        batch = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
        lam = None
        if name != NO_LAMBDA:
            lams = []
            for a, b in zip(ptr[:-1], ptr[1:]):
                m = (ei[0] >= a) & (ei[0] < b)
                assert ((ei[1][m] >= a) & (ei[1][m] < b)).all()
                lams.append(lambda_of(ei[:, m] - a, int(b - a)))
            lam = torch.tensor(lams, dtype=torch.float64).float().double()     # the float32 values the device gets, in every dtype
        _GRAPH_CACHE[name] = (ei, N, torch.from_numpy(batch), lam)
    return _GRAPH_CACHE[name]


def draw_case(shape, N, seed):
    Fin, Fout, K = shape
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=r(N, Fin), W=r(K, Fin, Fout) * (0.5 / (K * Fin) ** 0.5), b=r(Fout) * 0.1, dy=r(N, Fout))


def margin(case, L, act):
    """smallest |pre-activation| / max (relu only; else inf) on the float64 restatement"""
    if act != 'relu':
        return float('inf')
    d = {k: v.double() for k, v in case.items()}
    pre = forward(d['x'], L.double(), d['W'], d['b'], act, parts=True)[2]
    return float(pre.abs().min() / pre.abs().max())


_CASES = {}


def layer_case(shape_idx, act, gname, max_seeds=400):
    """The case of the GPU matrix: the first seed (CPU search, ascending from a base that differs per case) whose float64 restatement
    keeps the kink margin -- no element is excluded; cached.  Returns (case dict, graph tuple of get_graph, L float64, seed)."""
    key = (shape_idx, act, gname)
    if key not in _CASES:
        gr = get_graph(gname)
        ei, N, batch, lam = gr
        L = laplacian(ei, N, batch, lam, torch.float64)
        base = 1000 * shape_idx + 100 * ACTS.index(act) + 10 * sorted(GRAPHS).index(gname)
        for seed in range(base, base + max_seeds):
            case = draw_case(SHAPES[shape_idx], N, seed)
            if margin(case, L, act) >= MARGIN:
                break
        else:
            raise AssertionError('no seed keeps the kink margin for %s' % (key,))
        _CASES[key] = (case, gr, L, seed)
    return _CASES[key]


_REFS = {}


def layer_ref(key, case, gr, act, bias=True):
    """(float64, float32) restatements: dict(y, dx, dW, db, T [N, (K - 1) Fin]) each; computed once per case.  Each builds its own L^ in its dtype."""
    if key not in _REFS:
        ei, N, batch, lam = gr
        out = []
        for dt in (torch.float64, torch.float32):
            d = {k: v.to(dt) for k, v in case.items()}
            L = laplacian(ei, N, batch, None if lam is None else lam.to(dt), dt)
            b = d['b'] if bias else None
            r = backward(d['x'], L, d['W'], b, act, d['dy'])
            r['y'], tx, _ = forward(d['x'], L, d['W'], b, act, parts=True)
            r['T'] = torch.cat(tx[1:], 1) if len(tx) > 1 else torch.zeros(N, 0, dtype=dt)
            out.append(r)
        _REFS[key] = tuple(out)
    return _REFS[key]


# ---------------------------------------------------------------------------------------------------------------- ChebNet
def chebnet_ref(p, model, x, ei, ptr, lam, features=False):
    """the ChebNet of the scripts with parameters p (name -> tensor of the working dtype) and the structure of `model` (a models.Cheb:
    nlayers, act, pool, head, bn_after, lmax); lam: lambda_max per graph (read when model.lmax).  BatchNorms in training mode (batch
    statistics), no dropout"""
    dt = p['conv1.weight'].dtype
    x = torch.as_tensor(x).to(dt)
    ptr = [int(v) for v in ptr]
    batch = torch.repeat_interleave(torch.arange(len(ptr) - 1), torch.tensor(np.diff(ptr)))
    L = laplacian(ei, x.size(0), batch, torch.as_tensor(lam).to(dt) if model.lmax else None, dt)
    for i in range(1, model.nlayers + 1):
        x = forward(x, L, p['conv%d.weight' % i], p['conv%d.bias' % i], model.act)
        if i in model.bn_after:
            x = G._bn_train(x, p['bn%d.weight' % i], p['bn%d.bias' % i])
    if model.pool is not None:
        x = G.pool_ref(x, ptr, model.pool)
    if features:
        return x
    lin = lambda v, n: v @ p[n + '.weight'].t() + p[n + '.bias']
    if model.head == 'node':
        return lin(x, 'fc2')
    if model.head == 'tanh':
        return torch.tanh(lin(x, 'fc1'))
    if model.head == 'bn_mlp':
        x = G._bn_train(x, p['bn1.weight'], p['bn1.bias'])
    if 'fc1.weight' in p:
        x = torch.relu(lin(x, 'fc1'))
    x = lin(x, 'fc2')
    return x if model.head == 'mlp' else torch.log_softmax(x, dim=1)


def graph_lambdas(gs):
    """lambda_of for every graph dict (x, edge_index), float32 as a data set stores it"""
    return [np.float32(lambda_of(np.asarray(g['edge_index'], np.int64), g['x'].shape[0])) for g in gs]


FACTORIES = ['zinc_cheb', 'sr25_cheb', 'graph8c_cheb', 'exp_cheb', 'exp_classify_cheb', 'counting_cheb', 'mutag_cheb', 'freqclass_cheb',
             'filtering_cheb', 'mnist75_cheb', 'enzymes_cheb', 'ptc_cheb', 'proteins_cheb', 'enzymes_contfeat_cheb']
WIDE = ('enzymes_cheb', 'ptc_cheb', 'proteins_cheb', 'enzymes_contfeat_cheb')        # 128 / 200 wide: on the composition
