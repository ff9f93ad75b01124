"""GINConv restated in plain torch, dtype-generic and dense per node (no scatter): the arithmetic of torch_geometric 1.6.1's GINConv with
nn = Sequential(Linear) or Sequential(Linear, ReLU, Linear) as include/gml.h states it for gml_gin_*.  torch_geometric itself is not
available to these tests: this is a restatement of its arithmetic, not a run of the library.

    A[i, j] = number of edges (j -> i), the diagonal INCLUDED (a self loop is an edge like any other; nothing is dropped or added)
    h       = A x + (1 + eps) x
    depth 2: t = relu(h W1^T + b1), pre = t W2^T + b2;   depth 1: pre = h W1^T + b1
    y       = act(pre)

forward(): the above; backward(): the analytic gradient formulas of the issue (g2 = dy act'(y), dW2 = g2^T t, db2 = sum g2,
g1 = (g2 W2) [t > 0] or g2, dW1 = g1^T h, db1 = sum g1, dh = g1 W1, deps = sum_i <dh[i], x[i]>, dx = (1 + eps) dh + A^T dh) and the
term sum of deps; ginnet_ref(): the GinNet of the experiment scripts on top.  The cases of the GPU layer matrix and their kink
margins live here so that tests/test_gin_cpu.py can verify the margins without a device."""
import numpy as np
import torch

import _gat_ref as G

ACTS = (None, 'relu', 'tanh')
MARGIN = G.MARGIN                 # kink margin: every hidden (and, for relu, every outer) pre-activation >= MARGIN x max-abs away from 0


def adjacency(ei, N, dtype):
    """A [N target, N source]: edge multiplicities, self loops included"""
    ei = torch.as_tensor(ei, dtype=torch.int64)
    A = torch.zeros(N, N, dtype=dtype)
    A.index_put_((ei[1], ei[0]), torch.ones(ei.size(1), dtype=dtype), accumulate=True)
    return A


def act_fn(v, act):
    return torch.relu(v) if act == 'relu' else (torch.tanh(v) if act == 'tanh' else v)


def dact_from_y(y, act):
    if act == 'relu':
        return (y > 0).to(y.dtype)
    return 1 - y * y if act == 'tanh' else torch.ones_like(y)


def forward(x, A, eps, lins, act, parts=False):
    """lins = [(W1, b1 or None)] or [(W1, b1), (W2, b2)]; parts: (y, h, hidden pre-activation or None, t or None, pre)"""
    lin = lambda v, wb: v @ wb[0].t() + (0 if wb[1] is None else wb[1])
    h = A @ x + (1 + eps) * x
    pre1 = lin(h, lins[0])
    if len(lins) == 2:
        t = torch.relu(pre1)
        pre = lin(t, lins[1])
    else:
        t, pre, pre1 = None, pre1, None
    y = act_fn(pre, act)
    return (y, h, pre1, t, pre) if parts else y


def backward(x, A, eps, lins, act, dy):
    """dict(dx, deps, dW1, db1[, dW2, db2], dh) and teps = sum_i sum_c |dh[i, c]| |x[i, c]|: the term sum of deps, the scale an fp32
    evaluation's error is measured against where the signed sum cancels"""
    y, h, _, t, _ = forward(x, A, eps, lins, act, parts=True)
    g2 = dy * dact_from_y(y, act)
    out = {}
    if len(lins) == 2:
        out['dW2'], out['db2'] = g2.t() @ t, g2.sum(0)
        g1 = (g2 @ lins[1][0]) * (t > 0).to(x.dtype)
    else:
        g1 = g2
    dh = g1 @ lins[0][0]
    out.update(dW1=g1.t() @ h, db1=g1.sum(0), dh=dh, deps=(dh * x).sum().reshape(1), teps=(dh.abs() * x.abs()).sum(),
               dx=(1 + eps) * dh + A.t() @ dh)
    return out


class AnalyticGIN(torch.autograd.Function):
    """forward() with backward() as its gradient: what gradcheck holds against finite differences.  leaves: x, eps, W1, b1[, W2, b2]"""

    @staticmethod
    def forward(ctx, A, act, x, eps, *wb):
        ctx.save_for_backward(A, x, eps, *wb)
        ctx.act = act
        return forward(x, A, eps, [tuple(wb[:2]), tuple(wb[2:])][:len(wb) // 2], act)

    @staticmethod
    def backward(ctx, dy):
        A, x, eps, *wb = ctx.saved_tensors
        d = backward(x, A, eps, [tuple(wb[:2]), tuple(wb[2:])][:len(wb) // 2], ctx.act, dy)
        return (None, None, d['dx'], d['deps'], d['dW1'], d['db1']) + ((d['dW2'], d['db2']) if len(wb) == 4 else ())


# ---------------------------------------------------------------------------------------------------------------- graphs
def self_loops():
    """9 nodes: self loops on 0, 2 (twice), 5 and 7; node 7's row holds ONLY its own self loop (it sends one edge to 6), node 8 is
    isolated; the rest ordinary edges with a repeat (1 -> 0 twice)"""
    src = [0, 1, 1, 2, 2, 2, 3, 4, 5, 5, 6, 7, 7, 3]
    dst = [0, 0, 0, 2, 2, 1, 2, 3, 5, 4, 5, 7, 6, 1]
    return np.array([src, dst], np.int64), 9


GRAPHS = dict(G.GRAPHS, loops=self_loops)
SHAPES = [(1, 64, 64, 2), (2, 64, 64, 1), (3, 20, 36, 2), (25, 64, 64, 2), (64, 64, 64, 1), (64, 64, 64, 2), (7, 33, 1, 2)]    # (Fin, Fh, Fout, depth)
_GRAPH_CACHE = {}


def get_graph(name):
    if name not in _GRAPH_CACHE:
        _GRAPH_CACHE[name] = GRAPHS[name]()
    return _GRAPH_CACHE[name]


def out_width(shape):
    Fin, Fh, Fout, depth = shape
    return Fout if depth == 2 else Fh


def draw_case(shape, N, seed):
    Fin, Fh, Fout, depth = shape
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    c = dict(x=r(N, Fin), eps=torch.rand(1, generator=g), W1=r(Fh, Fin) * (0.5 / Fin ** 0.5), b1=r(Fh) * 0.1)
    if depth == 2:
        c.update(W2=r(Fout, Fh) * (0.5 / Fh ** 0.5), b2=r(Fout) * 0.1)
    c['dy'] = r(N, out_width(shape))
    return c


def lins_of(c):
    return [(c['W1'], c['b1'])] + ([(c['W2'], c['b2'])] if 'W2' in c else [])


def margins(case, A, act):
    """(smallest |hidden pre-activation| / max: depth 2 only, smallest |outer pre-activation| / max: relu only; else inf), float64"""
    d = {k: v.double() for k, v in case.items()}
    _, _, pre1, _, pre = forward(d['x'], A.double(), d['eps'], lins_of(d), act, parts=True)
    mh = float(pre1.abs().min() / pre1.abs().max()) if pre1 is not None else float('inf')
    mo = float(pre.abs().min() / pre.abs().max()) if act == 'relu' else float('inf')
    return mh, mo


_CASES = {}


def layer_case(shape_idx, act, gname, max_seeds=400):
    """The case of the GPU matrix: the first seed (CPU search, ascending from a base that differs per case) whose float64 restatement
    keeps the kink margin; cached.  Returns (case dict, edge_index, N, A float64, seed)."""
    key = (shape_idx, act, gname)
    if key not in _CASES:
        ei, N = get_graph(gname)
        A = adjacency(ei, N, torch.float64)
        base = 1000 * shape_idx + 100 * ACTS.index(act) + 10 * sorted(GRAPHS).index(gname)
        for seed in range(base, base + max_seeds):
            case = draw_case(SHAPES[shape_idx], N, seed)
            if min(margins(case, A, act)) >= MARGIN:
                break
        else:
            raise AssertionError('no seed keeps the kink margin for %s' % (key,))
        _CASES[key] = (case, ei, N, A, seed)
    return _CASES[key]


_REFS = {}


def layer_ref(key, case, A, act):
    """(float64, float32) restatements: dict(y, dx, deps, teps, dW1, db1[, dW2, db2], dh, h[, t]) each; computed once per case"""
    if key not in _REFS:
        out = []
        for dt in (torch.float64, torch.float32):
            d = {k: v.to(dt) for k, v in case.items()}
            r = backward(d['x'], A.to(dt), d['eps'], lins_of(d), act, d['dy'])
            r['y'], r['h'], _, t, _ = forward(d['x'], A.to(dt), d['eps'], lins_of(d), act, parts=True)
            if t is not None:
                r['t'] = t
            out.append(r)
        _REFS[key] = tuple(out)
    return _REFS[key]


# ---------------------------------------------------------------------------------------------------------------- GinNet
def ginnet_ref(p, model, x, ei, ptr, features=False, taps=None):
    """the GinNet of the scripts with parameters p (name -> tensor of the working dtype) and the structure of `model` (a models.GIN:
    nlayers, depth, act, pool, head, bn_after, share_nn); a layer built on another layer's nn reads that layer's keys when its own are
    not in p (named_parameters() lists a shared tensor once).  BatchNorms in training mode (batch statistics), no dropout.
    taps: a list that receives (layer input, h with its gradient retained) per layer -- after a backward, sum |h.grad| |input| is the
    term sum of that layer's deps"""
    dt = p['conv1.eps'].dtype
    x = torch.as_tensor(x).to(dt)
    A = adjacency(ei, x.size(0), dt)
    for i in range(1, model.nlayers + 1):
        c = 'conv%d.nn.' % i
        if c + '0.weight' not in p:
            c = 'conv%d.nn.' % model.share_nn[i]
        lins = [(p[c + '0.weight'], p[c + '0.bias'])] + ([(p[c + '2.weight'], p[c + '2.bias'])] if model.depth == 2 else [])
        xin = x
        x, h = forward(x, A, p['conv%d.eps' % i], lins, model.act, parts=True)[:2]
        if taps is not None:
            h.retain_grad()
            taps.append((xin.detach(), h))
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
    if 'fc1.weight' in p:
        x = torch.relu(lin(x, 'fc1'))
    x = lin(x, 'fc2')
    return x if model.head == 'mlp' else torch.log_softmax(x, dim=1)


def embed_sparse(p, model, x, ei, batch, num_graphs):
    """ginnet_ref for a whole data set at once (add / mean pools, heads 'tanh' / 'mlp'): the same arithmetic with index_add_ in place
    of the dense A (tests/test_gin_cpu.py holds it against ginnet_ref), for the expressivity counts over hundreds of graphs"""
    dt = p['conv1.eps'].dtype
    x, ei, batch = torch.as_tensor(x).to(dt), torch.as_tensor(ei, dtype=torch.int64), torch.as_tensor(batch, dtype=torch.int64)
    for i in range(1, model.nlayers + 1):
        c = 'conv%d.nn.' % i
        h = torch.zeros_like(x).index_add_(0, ei[1], x[ei[0]]) + (1 + p['conv%d.eps' % i]) * x
        v = h @ p[c + '0.weight'].t() + p[c + '0.bias']
        if model.depth == 2:
            v = torch.relu(v) @ p[c + '2.weight'].t() + p[c + '2.bias']
        x = act_fn(v, model.act)
    assert model.pool in ('add', 'mean') and not model.bn_after and not model.share_nn
    g = torch.zeros(num_graphs, x.size(1), dtype=dt).index_add_(0, batch, x)
    if model.pool == 'mean':
        g = g / torch.bincount(batch, minlength=num_graphs).to(dt).unsqueeze(1)
    lin = lambda v, n: v @ p[n + '.weight'].t() + p[n + '.bias']
    if model.head == 'tanh':
        return torch.tanh(lin(g, 'fc1'))
    return lin(torch.relu(lin(g, 'fc1')), 'fc2')


FACTORIES = ['sr25_gin', 'graph8c_gin', 'exp_gin', 'exp_classify_gin', 'zinc_gin', 'counting_gin', 'mutag_gin', 'freqclass_gin',
             'filtering_gin', 'enzymes_gin', 'ptc_gin', 'proteins_gin', 'enzymes_contfeat_gin']
WIDE = ('ptc_gin', 'proteins_gin', 'enzymes_contfeat_gin')            # 200 wide: on the composition
