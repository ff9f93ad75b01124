"""GAT without a device: the restatement of tests/_gat_ref.py (its analytic backward against finite differences of its forward), the
torch-op composition functional.gat_conv_torch against it, the module's parameters and initialisation, every factory's state_dict,
the arguments that raise, and the kink margins of every case of the GPU layer matrix (tests/test_gpu_gat.py)."""
import math

import numpy as np
import pytest
import torch

import _gat_ref as R
from conftest import rel_err


def small_case(act, dtype, seed=0, Fin=3, C=4, margin=0.0):
    """the hand-made graph with the first seed from `seed` upwards whose kink margins reach `margin`"""
    ei, N = R.hand_made()
    A = R.adjacency(ei, N, dtype)
    while min(R.margins(R.draw_case(Fin, C, N, seed), A, act)) < margin:
        seed += 1
    c = {k: v.to(dtype) for k, v in R.draw_case(Fin, C, N, seed).items()}
    return c, torch.from_numpy(ei), N, A


def test_hand_made_graph_has_the_four_features():
    ei, N = R.hand_made()
    pairs = list(zip(ei[0].tolist(), ei[1].tolist()))
    assert (2, 2) in pairs and pairs.count((0, 1)) == 2 and (3, 4) in pairs and (4, 3) not in pairs
    assert 5 not in ei and N == 6
    A = R.adjacency(ei, N, torch.float64)
    assert A[1, 0] == 2 and A[2, 2] == 1 and A[5].sum() == 1 and torch.equal(A.diagonal(), torch.ones(6, dtype=torch.float64))


@pytest.mark.parametrize('act', R.ACTS)
def test_analytic_backward_against_gradcheck(act):
    c, _, _, A = small_case(act, torch.float64, seed=3, margin=2e-3)
    ms, mp = R.margins(c, A, act)
    assert ms > 1e-3 and mp > 1e-3                      # finite differences of 1e-6 stay on one side of every kink
    leaves = [c[k].clone().requires_grad_(True) for k in ('x', 'W', 'att_l', 'att_r', 'bias')]
    assert torch.autograd.gradcheck(lambda *a: R.AnalyticGAT.apply(*a, A, act), leaves, eps=1e-6, atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize('act', R.ACTS)
def test_analytic_backward_equals_autograd(act):
    c, _, _, A = small_case(act, torch.float64, seed=4, Fin=5, C=8)
    leaves = {k: c[k].clone().requires_grad_(True) for k in ('x', 'W', 'att_l', 'att_r', 'bias')}
    y = R.forward(leaves['x'], A, leaves['W'], leaves['att_l'], leaves['att_r'], leaves['bias'], act)
    y.backward(c['dy'])
    d = R.backward(c['x'], A, c['W'], c['att_l'], c['att_r'], c['bias'], act, c['dy'])
    for k, name in (('x', 'dx'), ('W', 'dW'), ('att_l', 'datt_l'), ('att_r', 'datt_r'), ('bias', 'dbias')):
        assert rel_err(d[name].numpy(), leaves[k].grad.numpy()) <= 1e-12, name


def test_isolated_node_is_act_of_its_own_row():
    c, _, N, A = small_case('tanh', torch.float64)
    y = R.forward(c['x'], A, c['W'], c['att_l'], c['att_r'], c['bias'], 'tanh')
    want = torch.tanh(c['x'][5] @ c['W'].t() + c['bias'])
    assert rel_err(y[5].numpy(), want.numpy()) <= 1e-15


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
@pytest.mark.parametrize('act', R.ACTS)
def test_gat_conv_torch_against_restatement(act, dtype):
    from gnn_matlang_amd import functional as Fn
    c, ei, N, A = small_case(act, dtype, seed=5, Fin=7, C=12)
    leaves = {k: c[k].clone().requires_grad_(True) for k in ('x', 'W', 'att_l', 'att_r', 'bias')}
    y = Fn.gat_conv_torch(leaves['x'], ei, leaves['W'], leaves['att_l'], leaves['att_r'], leaves['bias'], act)
    y.backward(c['dy'])
    d = R.backward(c['x'], A, c['W'], c['att_l'], c['att_r'], c['bias'], act, c['dy'])
    d['y'] = R.forward(c['x'], A, c['W'], c['att_l'], c['att_r'], c['bias'], act)
    tol = 1e-12 if dtype == torch.float64 else 2e-5
    assert rel_err(y.detach().numpy(), d['y'].numpy()) <= tol
    for k, name in (('x', 'dx'), ('W', 'dW'), ('att_l', 'datt_l'), ('att_r', 'datt_r'), ('bias', 'dbias')):
        assert rel_err(leaves[k].grad.numpy(), d[name].numpy()) <= tol, name


def test_gat_conv_torch_without_edges_and_without_bias():
    from gnn_matlang_amd import functional as Fn
    c = {k: v.double() for k, v in R.draw_case(3, 4, 2, 0).items()}
    y = Fn.gat_conv_torch(c['x'], torch.zeros(2, 0, dtype=torch.int64), c['W'], c['att_l'], c['att_r'], None, 'elu')
    assert rel_err(y.numpy(), torch.nn.functional.elu(c['x'] @ c['W'].t()).numpy()) <= 1e-15


def test_module_parameters_and_init():
    from gnn_matlang_amd import GATConv
    torch.manual_seed(0)
    m = GATConv(25, 12, heads=8, concat=True, dropout=0.0)
    shapes = {k: tuple(v.shape) for k, v in m.named_parameters()}
    assert shapes == {'att_l': (1, 8, 12), 'att_r': (1, 8, 12), 'bias': (96,), 'lin_l.weight': (96, 25)}
    assert sum(v.numel() for v in m.parameters()) == (25 + 3) * 8 * 12
    assert m.lin_r is m.lin_l
    sd = m.state_dict()
    assert list(sd) == ['att_l', 'att_r', 'bias', 'lin_l.weight', 'lin_r.weight']
    assert sd['lin_l.weight'].data_ptr() == sd['lin_r.weight'].data_ptr()
    bw, ba = math.sqrt(6.0 / (96 + 25)), math.sqrt(6.0 / (8 + 12))
    wmax = float(m.lin_l.weight.detach().abs().max())
    assert 0.9 * bw < wmax <= bw
    for a in (m.att_l, m.att_r):
        assert 0.8 * ba < float(a.detach().abs().max()) <= ba
    assert float(m.bias.detach().abs().max()) == 0
    m2 = GATConv(25, 12, heads=8)
    m2.load_state_dict(sd, strict=True)
    assert torch.equal(m2.lin_l.weight, m.lin_l.weight) and torch.equal(m2.att_r, m.att_r)
    assert GATConv(4, 8, heads=8, bias=False).bias is None


@pytest.mark.parametrize('kw,name', [(dict(concat=False), 'concat'), (dict(dropout=0.5), 'dropout'), (dict(add_self_loops=False), 'add_self_loops')])
def test_unsupported_arguments_raise(kw, name):
    from gnn_matlang_amd import GATConv
    with pytest.raises(NotImplementedError, match=name):
        GATConv(4, 8, heads=8, **kw)


def test_tuple_inputs_raise():
    from gnn_matlang_amd import GATConv
    with pytest.raises(NotImplementedError, match='tuple'):
        GATConv((4, 4), 8, heads=8)
    m = GATConv(4, 8, heads=8)
    with pytest.raises(NotImplementedError, match='tuple'):
        m((torch.zeros(2, 4), torch.zeros(2, 4)), torch.zeros(2, 0, dtype=torch.int64))


# the scripts' classes: (conv widths, BatchNorms declared, (fc1, fc2) as (in, out) or None), H = 8
SCRIPTS = {'zinc_gat': (25, (8, 12, 12, 12), 0, (96, 64), (64, 1)), 'mutag_gat': (8, (8, 16, 16), 0, (128, 10), (10, 1)),
           'enzymes_gat': (4, (8, 16, 16, 16), 0, None, (256, 6)), 'freqclass_gat': (1, (8, 16, 16), 0, (128, 32), (32, 1)),
           'ptc_gat': (20, (16, 16, 16, 16), 2, (256, 100), (100, 2)), 'proteins_gat': (4, (16, 16), 2, (256, 100), (100, 2)),
           'enzymes_contfeat_gat': (22, (16, 16), 2, (256, 100), (100, 6)), 'sr25_gat': (2, (16, 16, 16), 0, (128, 10), None),
           'graph8c_gat': (2, (16, 16, 16), 0, (128, 10), None), 'exp_gat': (2, (16, 16, 16), 0, (128, 10), None),
           'exp_classify_gat': (2, (16, 16, 16), 0, (128, 10), (10, 1)), 'counting_gat': (2, (16,) * 5, 0, (128, 32), (32, 1)),
           'filtering_gat': (1, (16, 16, 16), 0, None, (128, 1)), 'mnist75_gat': (3, (8, 16, 16), 1, (128, 32), (32, 10))}


def script_shaped(name):
    """a module with the attributes the script's GatNet declares, in its order (GATConv's own keys as torch_geometric 1.6.1 names them)"""
    ninp, widths, nbn, fc1, fc2 = SCRIPTS[name]
    ref = torch.nn.Module()
    fin = ninp
    for i, w in enumerate(widths, start=1):
        conv = torch.nn.Module()
        conv.att_l = torch.nn.Parameter(torch.randn(1, 8, w))
        conv.att_r = torch.nn.Parameter(torch.randn(1, 8, w))
        conv.bias = torch.nn.Parameter(torch.randn(8 * w))
        conv.lin_l = torch.nn.Linear(fin, 8 * w, bias=False)
        conv.lin_r = conv.lin_l
        setattr(ref, 'conv%d' % i, conv)
        fin = 8 * w
    for i in range(1, nbn + 1):
        setattr(ref, 'bn%d' % i, torch.nn.BatchNorm1d(128))
    if fc1:
        ref.fc1 = torch.nn.Linear(*fc1)
    if fc2:
        ref.fc2 = torch.nn.Linear(*fc2)
    return ref


@pytest.mark.parametrize('name', R.FACTORIES)
def test_factory_state_dict(name):
    from gnn_matlang_amd import models
    assert sorted(SCRIPTS) == sorted(R.FACTORIES)
    torch.manual_seed(1)
    sd = script_shaped(name).state_dict()
    m = getattr(models, name)()
    own = m.state_dict()
    assert list(own) == list(sd)
    assert all(own[k].shape == sd[k].shape for k in sd)
    m.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    convs = [getattr(m, 'conv%d' % i) for i in range(1, m.nlayers + 1)]
    assert all(c.heads == 8 for c in convs)
    nconv = sum((c.in_channels + 3) * 8 * c.out_channels for c in convs)           # the scripts' "(in+3)*head*out"
    assert sum(v.numel() for n, v in m.named_parameters() if n.startswith('conv')) == nconv


def test_matrix_cases_keep_the_kink_margin():
    """every case of the GPU layer matrix: all edge logits (and, for relu, all pre-activations) of the float64 restatement lie at
    least MARGIN x max-abs away from 0, so no leaky-relu / relu decision can differ between fp32 and float64 -- no element is ever
    excluded from a comparison.  The float32 restatement's own error on the logits is printed: the margin must stay 3 x above it."""
    worst_s, worst_p, worst_e32, seeds = float('inf'), float('inf'), 0.0, set()
    for si in range(len(R.SHAPES)):
        for act in R.ACTS:
            for g in sorted(R.GRAPHS):
                case, ei, N, A, seed = R.layer_case(si, act, g)
                ms, mp = R.margins(case, A, act)
                worst_s, worst_p = min(worst_s, ms), min(worst_p, mp)
                seeds.add(seed - (1000 * si + 100 * R.ACTS.index(act) + 10 * sorted(R.GRAPHS).index(g)))
                if g in ('hand', 'rand67'):                              # the fp32 restatement's error on the logits, a sample of cases
                    d32 = {k: v.float() for k, v in case.items()}
                    d64 = {k: v.double() for k, v in case.items()}
                    s32 = R.forward(d32['x'], A.float(), d32['W'], d32['att_l'], d32['att_r'], d32['bias'], act, parts=True)[2]
                    s64 = R.forward(d64['x'], A, d64['W'], d64['att_l'], d64['att_r'], d64['bias'], act, parts=True)[2]
                    on = A > 0
                    worst_e32 = max(worst_e32, float((s32.double() - s64)[on].abs().max() / s64[on].abs().max()))
    print('smallest logit margin %.2e, pre-activation margin %.2e, float32 logit error %.2e, seed offsets used %s'
          % (worst_s, worst_p, worst_e32, sorted(seeds)))
    assert worst_s >= R.MARGIN and worst_p >= R.MARGIN
    assert 3 * worst_e32 < R.MARGIN


def test_softmax_range_case_reaches_80():
    case, A = R.range_case()
    d = {k: v.double() for k, v in case.items()}
    s = R.forward(d['x'], A, d['W'], d['att_l'], d['att_r'], d['bias'], None, parts=True)[2]
    row = torch.where(A[0] > 0)[0]                       # the star's centre: 201 edges
    assert row.numel() == 201
    assert float(s[0, row].max()) >= 80 and float(s[0, row].min()) <= -80
    assert R.margins(case, A, None)[0] >= R.MARGIN
