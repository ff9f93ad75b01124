"""tests/_edge_ref.py, the float64 restatement the edge-branch ABI tests hold the kernels to, against float64 autograd of
oracle.spect_conv_oracle.edge_mlp_forward: values and all five gradients to 1e-12, the unique-row form against the plain form on a
list whose mirrored rows are bitwise equal, every term sum >= the absolute value of its element, exact zeros for zero rows.
No device."""
import numpy as np
import pytest
import torch

import _edge_ref as ER
from oracle import spect_conv_oracle as O

SHAPES = [(1, 1), (3, 3), (8, 8), (12, 12), (16, 16), (24, 24), (20, 47)]     # (S, Sout); the last: the wide kernels' S != Sout
E = 41


def _case(S, So, seed=0):
    g = torch.Generator().manual_seed(100 * S + So + seed)
    ea = torch.randn(E, S, generator=g, dtype=torch.float64) * 0.7
    ws = [torch.randn(2 * S, S, generator=g, dtype=torch.float64) * 0.7 for _ in range(3)] + \
         [torch.randn(So, 4 * S, generator=g, dtype=torch.float64) * 0.5]
    gout = torch.randn(E, So, generator=g, dtype=torch.float64)
    return ea, ws, gout


def _autograd(ea, ws, gout):
    e = ea.clone().requires_grad_(True)
    w = [t.clone().requires_grad_(True) for t in ws]
    out = O.edge_mlp_forward(e, *w)
    (out * gout).sum().backward()
    return out.detach().numpy(), e.grad.numpy(), [t.grad.numpy() for t in w]


def _close(got, ref, what):
    assert got.shape == ref.shape, what
    assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), (what, np.abs(got - ref).max())


@pytest.mark.parametrize('S,So', SHAPES)
def test_values_and_gradients_match_float64_autograd(S, So):
    ea, ws, gout = _case(S, So)
    out, gin, dws = _autograd(ea, ws, gout)
    w = [t.numpy() for t in ws]
    f = ER.edge_fwd_ref(ea.numpy(), *w)
    b = ER.edge_bwd_ref(ea.numpy(), *w, gout.numpy(), wide=True)
    _close(f.v, out, 'out')
    _close(b['gin'].v, gin, 'gin')
    for i in range(4):
        _close(b['dw%d' % (i + 1)].v, dws[i], 'dw%d' % (i + 1))
    # the wide backward's per-edge outputs give the same weight gradients through the contractions gml.h names
    go, hid, gz = b['go'].v, b['hid'].v, b['gz'].v
    _close(go, gout.numpy() * (out > 0), 'go')
    for m in range(3):
        _close(gz[:, m].T @ ea.numpy(), dws[m], 'gz -> dw%d' % (m + 1))
    _close(np.concatenate([hid[:, 0].T @ go, hid[:, 1].T @ go], 0).T, dws[3], 'hid -> dw4')
    _close(sum(gz[:, m] @ w[m] for m in range(3)), gin, 'gz -> gin')


@pytest.mark.parametrize('S,So', SHAPES)
def test_term_sums_bound_their_elements(S, So):
    ea, ws, gout = _case(S, So, 1)
    w = [t.numpy() for t in ws]
    refs = dict(ER.edge_bwd_ref(ea.numpy(), *w, gout.numpy(), wide=True), out=ER.edge_fwd_ref(ea.numpy(), *w))
    uid, mir = np.arange(0, E, 2), np.where(np.arange(0, E, 2) + 1 < E, np.arange(0, E, 2) + 1, -1)
    for k, r in ER.edge_bwd_ref(ea.numpy(), *w, gout.numpy(), uid=uid, mir=mir).items():
        refs['sym ' + k] = r
    for k, r in refs.items():
        if r is None:
            assert k == 'sym gin'
            continue
        assert r.v.shape == r.t.shape and np.isfinite(r.t).all() and (r.t >= 0).all(), k
        assert (r.t >= np.abs(r.v)).all(), (k, float((np.abs(r.v) - r.t).max()))


@pytest.mark.parametrize('S,So', SHAPES)
def test_unique_row_form_equals_the_plain_form(S, So):
    """edges [0, P) and their mirrors [P, 2P) carry bitwise the same row, the rest are one-sided: the entries' sums over
    gout[uid] + gout[mir] are the plain form's sums over all edges"""
    ea, ws, gout = _case(S, So, 2)
    P = E // 3
    ea[P:2 * P] = ea[:P]
    order = np.random.default_rng(S).permutation(E - P)
    uid = np.concatenate([np.arange(P), np.arange(2 * P, E)])[order]
    mir = np.concatenate([np.arange(P, 2 * P), np.full(E - 2 * P, -1)])[order]
    w = [t.numpy() for t in ws]
    plain = ER.edge_bwd_ref(ea.numpy(), *w, gout.numpy())
    sym = ER.edge_bwd_ref(ea.numpy(), *w, gout.numpy(), uid=uid, mir=mir)
    assert sym['gin'] is None
    for k in ('dw1', 'dw2', 'dw3', 'dw4'):
        _close(sym[k].v, plain[k].v, k)
        assert np.abs(sym[k].t - plain[k].t).max() <= 1e-12 * plain[k].t.max(), k


@pytest.mark.parametrize('S,So', SHAPES)
def test_zero_rows_give_exact_zeros(S, So):
    ea, ws, gout = _case(S, So, 3)
    zero = [0, E // 2, E - 1]
    ea[zero] = 0.0
    w = [t.numpy() for t in ws]
    f = ER.edge_fwd_ref(ea.numpy(), *w)
    b = ER.edge_bwd_ref(ea.numpy(), *w, gout.numpy(), wide=True)
    assert not f.v[zero].any() and not np.signbit(f.v[zero]).any()
    for k in ('gin', 'go', 'hid', 'gz'):
        assert not b[k].v[zero].any(), k
    z = ER.edge_bwd_ref(ea.numpy()[zero], *w, gout.numpy()[zero])           # a batch made only of zero rows
    for k in ('gin', 'dw1', 'dw2', 'dw3', 'dw4'):
        assert not z[k].v.any(), k


def test_checker_catches_an_overrun_and_a_small_wrong_element():
    """what tests/test_gpu_edge_abi.py relies on, on host arrays: a store range one row too long lands in the guard rows and fails the
    guard assertion (before any value is looked at); an element of small magnitude that is wrong by 3 tol of its own term sum
    passes the max-norm and fails the term-sum assertion"""
    import _conv_ref as R
    S = 4
    ea, ws, gout = _case(S, S, 4)
    f = ER.edge_fwd_ref(ea.numpy(), *[t.numpy() for t in ws])
    buf, off = R.alloc(E, S, S)
    rows = buf.reshape(E + R.GUARD_ROWS, S)
    rows[:E] = f.v
    assert off == 0 and R.check(buf, f.v, f.t, E, S, S, 1e-4)[0] < 1e-6
    over = buf.copy()
    over.reshape(E + R.GUARD_ROWS, S)[E] = 0.0                                # the row behind the last one
    with pytest.raises(AssertionError, match='guard words overwritten'):
        R.check(over, f.v, f.t, E, S, S, 1e-4)
    g = ER.edge_bwd_ref(ea.numpy(), *[t.numpy() for t in ws], gout.numpy())['gin']      # gin: term sums from 0 (closed masks) upwards
    buf, _ = R.alloc(E, S, S)
    buf.reshape(E + R.GUARD_ROWS, S)[:E] = g.v
    R.check(buf, g.v, g.t, E, S, S, 1e-4)
    i = np.unravel_index(np.argmin(np.where(g.t > 0, g.t, np.inf)), g.t.shape)
    buf.reshape(E + R.GUARD_ROWS, S)[i] += 3e-4 * g.t[i]
    assert 3e-4 * g.t[i] < 0.5e-4 * np.abs(g.v).max()                        # invisible on the max-norm
    with pytest.raises(AssertionError, match='term sum'):
        R.check(buf, g.v, g.t, E, S, S, 1e-4)
