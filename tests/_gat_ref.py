"""GATConv restated in plain torch, dtype-generic and dense per node (no scatter): the arithmetic of torch_geometric 1.6.1's GATConv
(heads concatenated, negative_slope 0.2, no attention dropout) as include/gml.h states it for gml_gat_*.  torch_geometric itself is
not available to these tests: this is a restatement of its arithmetic, not a run of the library.

    A[i, j]  = number of edges (j -> i) with j != i, plus 1 on the diagonal           (self edges dropped, one self edge added)
    xl       = x W^T [N, H, C];  al = <xl, att_l>,  ar = <xl, att_r>                   [N, H]
    s[i, j]  = al[j] + ar[i];   e = s > 0 ? s : 0.2 s   (slope 0.2 at s == 0: torch's leaky_relu)
    m[i]     = max over A[i, j] > 0 of e;  p = A exp(e - m);  z = sum_j p;  alpha = p / (z + 1e-16)
    y        = act(sum_j alpha[i, j] xl[j] + bias)

forward(): the above; backward(): the analytic gradient formulas of the issue (g = dy act'(y), dalpha = <g[i], xl[j]>, de = alpha
(dalpha - <g, out>), ds = de slope, dar / dal = row / column sums of ds, dxl = alpha^T g + dal att_l + dar att_r, ...);
gatnet_ref(): the GatNet of the experiment scripts on top.  The cases of the GPU layer matrix and their kink margins live here so
that tests/test_gat_cpu.py can verify the margins without a device."""
import os

import numpy as np
import torch

ACTS = (None, 'relu', 'tanh', 'elu')
SLOPE = 0.2
MARGIN = 1e-5                     # kink margin: every edge logit (and, for relu, every pre-activation) >= MARGIN x max-abs away from 0


def adjacency(ei, N, dtype):
    """A [N target, N source]: edge multiplicities without the diagonal, plus the identity"""
    ei = torch.as_tensor(ei, dtype=torch.int64)
    A = torch.zeros(N, N, dtype=dtype)
    keep = ei[0] != ei[1]
    A.index_put_((ei[1][keep], ei[0][keep]), torch.ones(int(keep.sum()), dtype=dtype), accumulate=True)
    return A + torch.eye(N, dtype=dtype)


def act_fn(v, act):
    if act == 'relu':
        return torch.relu(v)
    if act == 'tanh':
        return torch.tanh(v)
    if act == 'elu':
        return torch.where(v > 0, v, torch.expm1(v))
    return v


def dact_from_y(y, act):
    if act == 'relu':
        return (y > 0).to(y.dtype)
    if act == 'tanh':
        return 1 - y * y
    if act == 'elu':
        return torch.where(y > 0, torch.ones_like(y), y + 1)
    return torch.ones_like(y)


def attention(xl, att_l, att_r, A):
    """(s, alpha) [N, N, H] (target, source, head); s is meaningful where A > 0"""
    H, C = att_l.shape[-2], att_l.shape[-1]
    al = (xl * att_l.reshape(1, H, C)).sum(-1)
    ar = (xl * att_r.reshape(1, H, C)).sum(-1)
    s = al.unsqueeze(0) + ar.unsqueeze(1)
    e = torch.where(s > 0, s, SLOPE * s)
    on = (A > 0).unsqueeze(-1)
    em = torch.where(on, e, torch.full_like(e, float('-inf')))                    # (exp(-inf) = 0 off the graph, in value and gradient)
    m = em.max(1, keepdim=True)[0]
    p = A.unsqueeze(-1) * torch.exp(em - m)
    return s, p / (p.sum(1, keepdim=True) + 1e-16)


def forward(x, A, W, att_l, att_r, bias, act, parts=False):
    N = x.size(0)
    H, C = att_l.shape[-2], att_l.shape[-1]
    xl = (x @ W.t()).view(N, H, C)
    s, alpha = attention(xl, att_l, att_r, A)
    out = torch.einsum('ijh,jhc->ihc', alpha, xl).reshape(N, H * C)
    pre = out if bias is None else out + bias
    y = act_fn(pre, act)
    return (y, xl, s, alpha, out, pre) if parts else y


def backward(x, A, W, att_l, att_r, bias, act, dy):
    """the analytic gradients: dict(dx, dW, datt_l, datt_r, dbias, dxl), and the term sums tl / tr of datt_l / datt_r (the same sums over
    alpha (|dalpha| + |<g, out>|) |xl|: the scale an fp32 evaluation's error is measured against where the gradient itself cancels to
    zero -- a graph whose rows hold their self edge only has de = alpha (dalpha - <g, out>) = 0 exactly)"""
    N = x.size(0)
    H, C = att_l.shape[-2], att_l.shape[-1]
    y, xl, s, alpha, out, _ = forward(x, A, W, att_l, att_r, bias, act, parts=True)
    g = (dy * dact_from_y(y, act)).view(N, H, C)
    dalpha = torch.einsum('ihc,jhc->ijh', g, xl)
    gout = (g * out.view(N, H, C)).sum(-1)                                        # <g[i, h], out[i, h]> = sum_j alpha dalpha
    de = alpha * (dalpha - gout.unsqueeze(1))
    ds = de * torch.where(s > 0, torch.ones_like(s), torch.full_like(s, SLOPE))
    dar, dal = ds.sum(1), ds.sum(0)
    dxl = torch.einsum('ijh,ihc->jhc', alpha, g) + dal.unsqueeze(-1) * att_l.reshape(1, H, C) + dar.unsqueeze(-1) * att_r.reshape(1, H, C)
    dxl2 = dxl.reshape(N, H * C)
    ts = alpha * (dalpha.abs() + gout.abs().unsqueeze(1))
    tl = (ts.sum(0).unsqueeze(-1) * xl.abs()).sum(0).reshape(att_l.shape)
    tr = (ts.sum(1).unsqueeze(-1) * xl.abs()).sum(0).reshape(att_r.shape)
    return dict(tl=tl, tr=tr, dx=dxl2 @ W, dW=dxl2.t() @ x, datt_l=(dal.unsqueeze(-1) * xl).sum(0).reshape(att_l.shape),
                datt_r=(dar.unsqueeze(-1) * xl).sum(0).reshape(att_r.shape), dbias=g.reshape(N, H * C).sum(0), dxl=dxl2)


class AnalyticGAT(torch.autograd.Function):
    """forward() with backward() as its gradient: what gradcheck holds against finite differences"""

    @staticmethod
    def forward(ctx, x, W, att_l, att_r, bias, A, act):
        ctx.save_for_backward(x, W, att_l, att_r, bias, A)
        ctx.act = act
        return forward(x, A, W, att_l, att_r, bias, act)

    @staticmethod
    def backward(ctx, dy):
        x, W, att_l, att_r, bias, A = ctx.saved_tensors
        d = backward(x, A, W, att_l, att_r, bias, ctx.act, dy)
        return d['dx'], d['dW'], d['datt_l'], d['datt_r'], d['dbias'], None, None


# ---------------------------------------------------------------------------------------------------------------- graphs
def hand_made():
    """6 nodes: a self loop (2 -> 2, dropped), a repeated edge (0 -> 1 twice), a one-way edge (3 -> 4), an isolated node (5)"""
    return np.array([[0, 0, 1, 2, 2, 1, 3, 3, 4], [1, 1, 0, 2, 1, 2, 4, 0, 0]], np.int64), 6


def star_and_path(leaves=200):
    """a star (centre 0, `leaves` leaves, both directions) beside a path of 3: one row far above any wave or chunk width"""
    l = np.arange(1, leaves + 1)
    a = leaves + 1
    src = np.concatenate([l, np.zeros(leaves, np.int64), [a, a + 1, a + 1, a + 2]])
    dst = np.concatenate([np.zeros(leaves, np.int64), l, [a + 1, a, a + 2, a + 1]])
    return np.stack([src, dst]).astype(np.int64), leaves + 4


def random_graph(N, seed, mean_degree=4):
    rng = np.random.default_rng(seed)
    E = N * mean_degree
    return np.stack([rng.integers(0, N, E), rng.integers(0, N, E)]).astype(np.int64), N    # directed, self loops and repeats included


def mutag16():
    from conftest import GOLDEN
    from gnn_matlang_amd import readers
    gs = readers.load_mutag(os.path.join(GOLDEN, 'raw', 'mutag.mat'))[:16]
    off, eis = 0, []
    for x, ei, _ in gs:
        eis.append(np.asarray(ei, np.int64) + off)
        off += x.shape[0]
    return np.concatenate(eis, 1), off


GRAPHS = {'one': lambda: (np.zeros((2, 0), np.int64), 1), 'hand': hand_made, 'star': star_and_path,
          'rand67': lambda: random_graph(67, 67), 'rand129': lambda: random_graph(129, 129), 'mutag16': mutag16}
SHAPES = [(1, 16), (2, 16), (25, 8), (64, 12), (96, 12), (128, 16)]               # (Fin, C); H = 8
H = 8
_GRAPH_CACHE = {}


def get_graph(name):
    if name not in _GRAPH_CACHE:
        _GRAPH_CACHE[name] = GRAPHS[name]()
    return _GRAPH_CACHE[name]


def draw_case(Fin, C, N, seed, att_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=r(N, Fin), W=r(H * C, Fin) * (0.5 / Fin ** 0.5), att_l=r(1, H, C) * (0.5 * att_scale), att_r=r(1, H, C) * (0.5 * att_scale),
                bias=r(H * C) * 0.1, dy=r(N, H * C))


def margins(case, A, act):
    """(smallest |s| over the edges / max |s|, smallest |pre-activation| / max: relu only, else inf) on the float64 restatement"""
    d = {k: v.double() for k, v in case.items()}
    _, _, s, _, _, pre = forward(d['x'], A.double(), d['W'], d['att_l'], d['att_r'], d['bias'], act, parts=True)
    sv = s[A > 0].abs()
    ms = float(sv.min() / sv.max())
    mp = float(pre.abs().min() / pre.abs().max()) if act == 'relu' else float('inf')
    return ms, mp


_CASES = {}


def layer_case(shape_idx, act, gname, max_seeds=200):
    """The case of the GPU matrix: the first seed (CPU search, ascending from a base that differs per case) whose float64 restatement
    keeps the kink margin; cached.  Returns (case dict, edge_index, N, A float64, seed)."""
    key = (shape_idx, act, gname)
    if key not in _CASES:
        Fin, C = SHAPES[shape_idx]
        ei, N = get_graph(gname)
        A = adjacency(ei, N, torch.float64)
        base = 1000 * shape_idx + 100 * ACTS.index(act) + 10 * sorted(GRAPHS).index(gname)
        for seed in range(base, base + max_seeds):
            case = draw_case(Fin, C, N, seed)
            ms, mp = margins(case, A, act)
            if ms >= MARGIN and mp >= MARGIN:
                break
        else:
            raise AssertionError('no seed keeps the kink margin for %s' % (key,))
        _CASES[key] = (case, ei, N, A, seed)
    return _CASES[key]


def range_case():
    """the star case with att scaled so that the logits inside the centre's row pass +-80"""
    ei, N = get_graph('star')
    A = adjacency(ei, N, torch.float64)
    for seed in range(5000, 5200):
        case = draw_case(64, 12, N, seed, att_scale=60.0)
        if margins(case, A, None)[0] >= MARGIN:
            return case, A
    raise AssertionError('no seed')


_REFS = {}


def layer_ref(key, case, A, act):
    """(float64, float32) restatements: dict(y, dx, dW, datt_l, datt_r, dbias, dxl) each; computed once per case"""
    if key not in _REFS:
        out = []
        for dt in (torch.float64, torch.float32):
            d = {k: v.to(dt) for k, v in case.items()}
            r = backward(d['x'], A.to(dt), d['W'], d['att_l'], d['att_r'], d['bias'], act, d['dy'])
            r['y'] = forward(d['x'], A.to(dt), d['W'], d['att_l'], d['att_r'], d['bias'], act)
            out.append(r)
        _REFS[key] = tuple(out)
    return _REFS[key]


# ---------------------------------------------------------------------------------------------------------------- GatNet
def _bn_train(x, w, b, eps=1e-5):
    mu, var = x.mean(0), x.var(0, unbiased=False)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def pool_ref(x, ptr, pool):
    if isinstance(pool, tuple):
        return torch.cat([pool_ref(x, ptr, p) for p in pool], 1)
    rows = []
    for g in range(len(ptr) - 1):
        seg = x[int(ptr[g]):int(ptr[g + 1])]
        rows.append(seg.sum(0) if pool == 'add' else (seg.mean(0) if pool == 'mean' else seg.max(0)[0]))
    return torch.stack(rows)


def gatnet_ref(p, model, x, ei, ptr, features=False):
    """the GatNet of the scripts with parameters p (name -> tensor of the working dtype) and the structure of `model` (a models.GAT:
    nlayers, act, pool, head, bn_after); BatchNorms in training mode (batch statistics), no dropout"""
    dt = p['conv1.lin_l.weight'].dtype
    x = torch.as_tensor(x).to(dt)
    A = adjacency(ei, x.size(0), dt)
    for i in range(1, model.nlayers + 1):
        c = 'conv%d.' % i
        x = forward(x, A, p[c + 'lin_l.weight'], p[c + 'att_l'], p[c + 'att_r'], p[c + 'bias'], model.act)
        if i in model.bn_after:
            x = _bn_train(x, p['bn%d.weight' % i], p['bn%d.bias' % i])
    if model.pool is not None:
        x = pool_ref(x, ptr, model.pool)
    if features:
        return x
    lin = lambda v, n: v @ p[n + '.weight'].t() + p[n + '.bias']
    if model.head == 'node':
        return lin(x, 'fc2')
    if model.head == 'tanh':
        return torch.tanh(lin(x, 'fc1'))
    if model.head == 'bn_mlp':
        x = _bn_train(x, p['bn1.weight'], p['bn1.bias'])
    if 'fc1.weight' in p:
        x = torch.relu(lin(x, 'fc1'))
    x = lin(x, 'fc2')
    return x if model.head == 'mlp' else torch.log_softmax(x, dim=1)


FACTORIES = ['sr25_gat', 'graph8c_gat', 'exp_gat', 'exp_classify_gat', 'zinc_gat', 'counting_gat', 'mutag_gat', 'ptc_gat', 'enzymes_gat',
             'proteins_gat', 'enzymes_contfeat_gat', 'freqclass_gat', 'filtering_gat', 'mnist75_gat']
