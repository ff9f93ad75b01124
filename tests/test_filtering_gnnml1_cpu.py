"""The filtering GNNML1 (filtering.py:200-250) and the EXP GNNML1 (exp_iso.py:195-247) without a device: the factories against the
reference classes' parameters written out by hand, the constructor's refusals, and the restatement of block mode 5 that the GPU tests
use (tests/_gnnml1_actsum_ref.py) against autograd."""
import numpy as np
import pytest
import torch

import _gnnml1_actsum_ref as A
from conftest import rel_err


def _gnnml1_shapes(ninp, nout, concat, head):
    """the state_dict of the reference GNNML1 -- filtering.py:214-231 / exp_iso.py:208-226: SpectConv(in, out, K=1) holds weight
    [1, in, out] and bias [out]; `head` = (name, outputs)"""
    nin = 3 * nout if concat else nout
    s = {}
    for i, fin in ((1, ninp), (2, nin), (3, nin)):
        s['conv%d1.weight' % i], s['conv%d1.bias' % i] = (1, fin, nout), (nout,)
        for j in (1, 2, 3):
            s['fc%d%d.weight' % (i, j)], s['fc%d%d.bias' % (i, j)] = (nout, fin), (nout,)
    s[head[0] + '.weight'], s[head[0] + '.bias'] = (head[1], nin), (head[1],)
    return s


FACTORIES = [('filtering_gnnml1', {}, _gnnml1_shapes(1, 32, False, ('fc2', 1))),
             ('filtering_gnnml1', dict(concat=True), _gnnml1_shapes(1, 32, True, ('fc2', 1))),
             ('exp_gnnml1', {}, _gnnml1_shapes(2, 64, False, ('fc1', 10)))]


@pytest.mark.parametrize('name,kw,want', FACTORIES, ids=['filtering', 'filtering_concat', 'exp'])
def test_factory_matches_the_reference_class(name, kw, want):
    from gnn_matlang_amd import models
    m = getattr(models, name)(**kw)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == want
    assert len(want) == 26                                       # 3 x (conv + three Linears) + the head, weight and bias each
    assert sum(p.numel() for p in m.parameters()) == sum(int(np.prod(s)) for s in want.values())
    g = torch.Generator().manual_seed(1)
    ckpt = {k: torch.randn(*s, generator=g) for k, s in want.items()}
    m.load_state_dict(ckpt, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, ckpt[k]), k


def test_filtering_factory_forms():
    from gnn_matlang_amd import models
    m = models.filtering_gnnml1()
    assert (m.form, m.act, m.pool, m.head, m.nblocks) == ('act_sum', 'relu', None, 'node', 3) and not hasattr(m, 'fc1')
    c = models.filtering_gnnml1(concat=True)
    assert (c.form, c.pool, c.head) == ('product', None, 'node') and c.fc2.in_features == 96
    e = models.exp_gnnml1()
    assert (e.form, e.act, e.pool, e.head) == ('sum', 'tanh', 'add', 'lin10') and not hasattr(e, 'fc2')


def test_constructor_errors():
    from gnn_matlang_amd.models import GNNML1Blocks
    with pytest.raises(ValueError):
        GNNML1Blocks(1, (32, 32, 16), 3, form='act_sum', pool=None, head='node')
    with pytest.raises(ValueError):
        GNNML1Blocks(1, (32, 16, 32), 3, form='act_sum', pool=None, head='node')
    with pytest.raises(ValueError):
        GNNML1Blocks(1, (32, 32, 32), 3, form='act_sum', pool='add', head='node')
    with pytest.raises(ValueError):
        GNNML1Blocks(1, (32, 32, 32), 3, form='act_sum', pool=None, head='mlp32')
    GNNML1Blocks(1, (32, 32, 32), 3, form='act_sum', pool='add', head='mlp32')      # (the form does not need the node head)


@pytest.mark.parametrize('c', A.CASES, ids=lambda c: '%dx%d-%d%s' % (c[0], c[1], c[2], '' if c[3] else '-vals'))
def test_restatement_against_autograd(c):
    """the written-out forward and backward equal autograd's, in float64 to rounding; the float32 and float64 evaluations agree on
    every relu pattern (the condition on the seeds)"""
    args = A.case(*c)
    r64, r32 = A.block(*args, torch.float64), A.block(*args, torch.float32)
    assert A.patterns_agree(r32, r64)
    y, dx, g = A.block_autograd(*args, torch.float64)
    assert rel_err(r64['out'].numpy(), y.numpy()) <= 1e-13 and rel_err(r64['dx'].numpy(), dx.numpy()) <= 1e-12
    assert set(g) == set(r64['grads']) and len(g) == 8
    for k in g:
        assert r64['grads'][k].shape == g[k].shape and rel_err(r64['grads'][k].numpy(), g[k].numpy()) <= 1e-12, k


def test_restatement_is_not_the_sum_form():
    """relu(a) + relu(c) + relu(f2 f3) against relu(a + c + f2 f3), kernel mode 0: output and gradients differ by more than 5 % on the
    separation case, whose eight sign combinations each cover more than 5 % of the entries -- a mode-0 kernel cannot pass for mode 5"""
    args = A.case(*A.SEPARATION)
    r64 = A.block(*args, torch.float64)
    shares = A.combination_shares(r64)
    assert shares.min() > 0.05, shares
    y0, dx0, g0 = A.block_autograd(*args, torch.float64, form='sum')
    assert rel_err(y0.numpy(), r64['out'].numpy()) > 0.05
    assert rel_err(dx0.numpy(), r64['dx'].numpy()) > 0.05
    for k in g0:
        assert rel_err(g0[k].numpy(), r64['grads'][k].numpy()) > 0.05, k
    b = A.pattern_bytes(r64)
    assert b.shape == (130, 8) and b.dtype == torch.uint8
    assert int(b[5, 3]) == sum(int(r64['pa'][5, 12 + u]) << u | int(r64['pc'][5, 12 + u]) << (4 + u) for u in range(4))
