"""tests/_conv_ref.py itself: the float64 restatement against the oracle, and the checker against planted faults."""
import numpy as np
import pytest
import torch

import _conv_ref as R
from conftest import rel_err


def _graph(rng, N, deg):
    src = np.repeat(np.arange(N), deg)
    dst = np.clip(src + rng.integers(-6, 7, size=src.shape), 0, N - 1)
    return np.unique(np.vstack((src, dst)), axis=1).astype(np.int64)


@pytest.mark.parametrize('N,deg,S,fin,fout,relu', [(37, 3, 3, 5, 7, False), (130, 6, 8, 12, 9, True)])
def test_conv_ref_agrees_with_the_oracle(N, deg, S, fin, fout, relu):
    from oracle.spect_conv_oracle import spectconv_forward, propagate_add
    rng = np.random.default_rng(N)
    ei = _graph(rng, N, deg)
    ei = ei[:, ei[1] != 5]                                         # an empty row
    E = ei.shape[1]
    ea, x = rng.standard_normal((E, S)), rng.standard_normal((N, fin))
    w, b, out0 = rng.standard_normal((S, fin, fout)), rng.standard_normal(fout), rng.standard_normal((N, fout))
    D = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    yo = spectconv_forward(D(x), torch.tensor(ei), D(ea), D(w), D(b), False)
    yo = (torch.relu(yo) if relu else yo).numpy()
    to = spectconv_forward(D(np.abs(x)), torch.tensor(ei), D(np.abs(ea)), D(np.abs(w)), D(np.abs(b)), False).numpy()
    rowptr, perm = R.csr_order(ei, N)
    assert rowptr[-1] == E and (np.diff(ei[1][perm]) >= 0).all() and rowptr[6] == rowptr[5]
    out, t = R.conv_ref(ei[:, perm], ea[perm], x, w, b, relu, None)
    assert np.abs(out - yo).max() <= 1e-12 * max(np.abs(yo).max(), 1.0)
    assert np.abs(t - to).max() <= 1e-12 * np.abs(to).max()
    # accumulate: the old values join the sum (and its term sum) in front of the activation
    out2, t2 = R.conv_ref(ei[:, perm], ea[perm], x, w, None, False, out0)
    yo2 = spectconv_forward(D(x), torch.tensor(ei), D(ea), D(w), None, False).numpy() + out0
    assert np.abs(out2 - yo2).max() <= 1e-12 * np.abs(yo2).max()
    assert np.abs(t2 - (to - np.abs(b) + np.abs(out0))).max() <= 1e-12 * np.abs(to).max()
    # H and the Hadamard columns
    H, _ = R.spmm_ref(ei[:, perm], ea[perm], x)
    for s in range(S):
        hs = propagate_add(D(x), torch.tensor(ei), D(ea[:, s])).numpy()
        assert np.abs(H[:, s, :] - hs).max() <= 1e-12 * max(np.abs(hs).max(), 1.0)
    w11, w12, b11, b12 = rng.standard_normal((2, fin)), rng.standard_normal((2, fin)), rng.standard_normal(2), rng.standard_normal(2)
    mo = (torch.tanh(D(x) @ D(w11).t() + D(b11)) * torch.tanh(D(x) @ D(w12).t() + D(b12))).numpy()
    m, mt = R.mix_ref(x, w11, b11, w12, b12)
    assert np.abs(m - mo).max() <= 1e-12 and (mt >= 1.0).all()


def _clean(N=70, fout=9, ldo=12, head=True, seed=3):
    rng = np.random.default_rng(seed)
    ref = rng.standard_normal((N, fout))
    ref[11, 4] = 1e-3                                              # a small element whose terms cancel ...
    t = np.abs(ref) + 1.0
    t[11, 4] = 2e-3                                                # ... from terms of its own size
    buf, off = R.alloc(N, fout, ldo, head)
    buf[off:].reshape(N + R.GUARD_ROWS, ldo)[:N, :fout] = ref.astype(np.float32)
    return buf, off, ref, t


def test_check_accepts_the_clean_buffer():
    for head in (False, True):
        buf, off, ref, t = _clean(head=head)
        assert off == (R.GUARD_HEAD if head else 0)
        e_max, e_ts = R.check(buf, ref, t, 70, 9, 12, 1e-4)
        assert e_max <= 1e-7 and e_ts <= 1e-7
    buf, off, ref, t = _clean(ldo=9, head=False)                   # exact width: no guard columns, the guard rows remain
    R.check(buf, ref, t, 70, 9, 9, 1e-4)


def test_check_rejects_a_small_element_the_max_norm_passes():
    buf, off, ref, t = _clean()
    rows = buf[off:].reshape(-1, 12)
    rows[11, 4] = np.float32(ref[11, 4] + 2e-4 * t[11, 4])         # 2e-4 of its term sum = 4e-7 absolute
    got, _ = R.split(buf, 70, 9, 12)
    assert rel_err(got, ref) < 1e-4                                # the project's max-norm bar does not see it
    with pytest.raises(AssertionError, match='term sum'):
        R.check(buf, ref, t, 70, 9, 12, 1e-4)


def test_check_rejects_an_overwritten_guard_column():
    buf, off, ref, t = _clean()
    buf[off:].reshape(-1, 12)[33, 9] = 0.0                         # column Fout of a row in the middle
    with pytest.raises(AssertionError, match='guard'):
        R.check(buf, ref, t, 70, 9, 12, 1e-4)
    buf, off, ref, t = _clean()
    buf[off:].reshape(-1, 12)[69, 11] = np.float32(np.nan)         # another NaN than the sentinel is an overwrite too
    with pytest.raises(AssertionError, match='guard'):
        R.check(buf, ref, t, 70, 9, 12, 1e-4)


def test_check_rejects_an_overwritten_guard_row():
    buf, off, ref, t = _clean()
    buf[off:].reshape(-1, 12)[70, 0] = 1.0                         # row N, what a store past the last partial group hits first
    with pytest.raises(AssertionError, match='guard'):
        R.check(buf, ref, t, 70, 9, 12, 1e-4)
    buf, off, ref, t = _clean()
    buf[off - 1] = 1.0                                             # the float in front of an offset output
    with pytest.raises(AssertionError, match='guard'):
        R.check(buf, ref, t, 70, 9, 12, 1e-4)


def test_check_rejects_a_nan_inside_the_output():
    buf, off, ref, t = _clean()
    buf[off:].reshape(-1, 12)[5, 2] = np.float32(np.nan)
    with pytest.raises(AssertionError, match='finite'):
        R.check(buf, ref, t, 70, 9, 12, 1e-4)
    buf, off, ref, t = _clean()                                    # a row the kernel never wrote still holds the sentinel
    buf[off:].reshape(-1, 12)[69, :9] = np.full(9, R.SENTINEL, np.int32).view(np.float32)
    with pytest.raises(AssertionError, match='finite'):
        R.check(buf, ref, t, 70, 9, 12, 1e-4)


# ---------------------------------------------------------------------------------------------------------------------- the backward
def _bwd_graph(rng, N):
    """source-keyed edges [2, E] with an empty source row (5), a duplicate edge (7 -> 9 twice) and a self loop (11 -> 11)"""
    ei = _graph(rng, N, 3)
    ei = ei[:, (ei[0] != 5) & ~((ei[0] == 11) & (ei[1] == 11))]
    ei = np.concatenate([ei, np.array([[7, 7, 11], [9, 9, 11]])], 1)
    ei = ei[:, np.argsort(ei[0], kind='stable')]
    assert not (ei[0] == 5).any() and ((ei[0] == 7) & (ei[1] == 9)).sum() >= 2 and ((ei[0] == 11) & (ei[1] == 11)).sum() == 1
    return ei.astype(np.int64)


def _fwd_torch(ei, val, x, w, relu):
    """conv_ref's own forward formula in torch: out[c] = sum_s (sum_{e into c} val[e, s] x[r_e]) W_s"""
    src, dst = torch.tensor(ei[0]), torch.tensor(ei[1])
    out = 0
    for s in range(val.shape[1]):
        H = torch.zeros_like(x).index_add(0, dst, val[:, s:s + 1] * x[src])
        out = out + H @ w[s]
    return torch.relu(out) if relu else out


@pytest.mark.parametrize('relu,had', [(False, False), (True, False), (True, True)], ids=['plain', 'relu', 'relu+hadamard'])
def test_conv_bwd_ref_agrees_with_autograd(relu, had):
    """float64 autograd of the forward formula (and, for `had`, of the ML3Layer output cat[relu(conv), tanh(fc11 x) tanh(fc12 x)])
    on an input x = cat[relu(u), v] of a layer below: the restated dx with relu_cols = width of u is the gradient at (u, v)"""
    N, S, fin, fout, ucols = 41, 3, 7, 5, 4
    rng = np.random.default_rng(77 + relu + 2 * had)
    ei = _bwd_graph(rng, N)
    E = ei.shape[1]
    D = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    u, v = D(rng.standard_normal((N, ucols))).requires_grad_(), D(rng.standard_normal((N, fin - ucols))).requires_grad_()
    val, w = D(rng.standard_normal((E, S))).requires_grad_(), D(rng.standard_normal((S, fin, fout))).requires_grad_()
    w11, w12 = (D(rng.standard_normal((2, fin))).requires_grad_() for _ in range(2))
    b11, b12 = (D(rng.standard_normal(2)).requires_grad_() for _ in range(2))
    cb = D(rng.standard_normal(fout)).requires_grad_()
    gout = rng.standard_normal((N, fout + 2))
    x = torch.cat([torch.relu(u), v], 1)
    conv = _fwd_torch(ei, val, x, w, False) + cb
    y = torch.relu(conv) if relu else conv
    if had:
        y = torch.cat([y, torch.tanh(x @ w11.t() + b11) * torch.tanh(x @ w12.t() + b12)], 1)
        loss = (y * D(gout)).sum()
    else:
        loss = (y * D(gout[:, :fout])).sum()
    loss.backward()
    g = gout.copy()                                                # the ABI's g arrives masked by this layer's relu
    if relu:
        g[:, :fout] *= (conv.detach().numpy() > 0)
    xn = x.detach().numpy()
    if had:
        dz, dzt, hr = R.had_ref(xn, g, fout, w11.detach().numpy(), b11.detach().numpy(), w12.detach().numpy(), b12.detach().numpy())
        wmix = np.concatenate([w11.detach().numpy(), w12.detach().numpy()])
        r = R.conv_bwd_ref(ei, val.detach().numpy(), xn, g[:, :fout], w.detach().numpy(), dz=dz, wmix=wmix, relu_cols=ucols, dz_t=dzt)
        for k, t in (('dw11', w11), ('dw12', w12), ('db11', b11), ('db12', b12), ('dcb', cb)):
            assert np.abs(hr[k].v - t.grad.numpy()).max() <= 1e-12 * max(np.abs(t.grad.numpy()).max(), 1.0), k
            assert (hr[k].t >= np.abs(hr[k].v) - 1e-12).all() and hr[k].n == N
        assert (dzt >= np.abs(dz)).all()
    else:
        r = R.conv_bwd_ref(ei, val.detach().numpy(), xn, g[:, :fout], w.detach().numpy(), relu_cols=ucols)
    want = {'dx': torch.cat([u.grad, v.grad], 1).numpy(), 'dval': val.grad.numpy(), 'dw': w.grad.numpy()}
    for k in want:
        assert r[k].v.shape == want[k].shape == r[k].t.shape
        assert np.abs(r[k].v - want[k]).max() <= 1e-12 * max(np.abs(want[k]).max(), 1.0), k
        assert (r[k].t >= np.abs(r[k].v) - 1e-12).all(), k
    # masked elements have no terms; the empty source row has neither terms nor value
    assert (r['dx'].t[:, :ucols][xn[:, :ucols] <= 0] == 0).all() and (xn[:, :ucols] <= 0).any()
    assert (r['dx'].v[5, ucols:] == (dz @ wmix)[5, ucols:] if had else r['dx'].v[5] == 0).all()


def test_conv_bwd_ref_term_sums_counts_and_old_values():
    N, S, fin, fout = 41, 3, 7, 5
    rng = np.random.default_rng(5)
    ei = _bwd_graph(rng, N)
    E = ei.shape[1]
    val, x, g, w = rng.standard_normal((E, S)), rng.standard_normal((N, fin)), rng.standard_normal((N, fout)), rng.standard_normal((S, fin, fout))
    dz, wmix = rng.standard_normal((N, 3)), rng.standard_normal((3, fin))
    dx0, dval0 = rng.standard_normal((N, fin)), rng.standard_normal((E, S))
    r = R.conv_bwd_ref(ei, val, x, g, w, dx0, dval0, dz, wmix)
    ra = R.conv_bwd_ref(ei, np.abs(val), np.abs(x), np.abs(g), np.abs(w), np.abs(dx0), np.abs(dval0), np.abs(dz), np.abs(wmix))
    r0 = R.conv_bwd_ref(ei, val, x, g, w)
    for k in ('dx', 'dval', 'dw'):                                 # the term sum IS the formula over absolute values
        assert np.abs(r[k].t - ra[k].v).max() <= 1e-12 * ra[k].v.max(), k
    assert np.abs(r['dx'].v - (r0['dx'].v + dx0 + dz @ wmix)).max() <= 1e-12 * np.abs(r['dx'].v).max()
    assert np.abs(r['dval'].v - (r0['dval'].v + dval0)).max() <= 1e-12 * np.abs(r['dval'].v).max()
    assert np.array_equal(r['dw'].v, r0['dw'].v)
    deg = np.bincount(ei[0], minlength=N)
    assert deg[5] == 0 and np.array_equal(r0['dx'].n, np.repeat(deg[:, None] * S * fout, fin, 1))
    assert np.array_equal(r['dx'].n, r0['dx'].n + 3 + 1) and (r0['dval'].n == fin * fout).all() and (r['dval'].n == fin * fout + 1).all()
    assert (r['dw'].n == E).all()
    b = R.f32_bound(r['dw'])
    assert b.shape == r['dw'].v.shape and np.allclose(b, 2 * (E + 8) * 2.0 ** -24 * r['dw'].t)
    # the duplicate edge counts twice, the self loop once: against a dense restatement
    A = np.zeros((S, N, N))
    np.add.at(A, (slice(None), ei[0], ei[1]), val.T)
    assert np.abs(r0['dx'].v - np.einsum('src,co,sfo->rf', A, g, w)).max() <= 1e-12 * np.abs(r0['dx'].v).max()
    assert np.abs(r0['dw'].v - np.einsum('rf,src,co->sfo', x, A, g)).max() <= 1e-12 * np.abs(r0['dw'].v).max()


def _filled(n, ncols, ld, seed, **kw):
    ref = np.random.default_rng(seed).standard_normal((n, ncols))
    buf, off = R.alloc(n, ncols, ld, out0=ref.astype(np.float32), **kw)
    return buf, off, ref, np.abs(ref) + 1.0


def test_check_serves_the_backward_buffers_and_trips_on_one_guard_word_in_each():
    N, fin, lddx, E, S, fout = 70, 9, 12, 200, 6, 5
    # dx [N, Fin] in rows of lddx: a padding column
    buf, off, ref, t = _filled(N, fin, lddx, 1)
    R.check(buf, ref, t, N, fin, lddx, 1e-4)
    buf[off:].reshape(-1, lddx)[40, fin + 2] = 0.0
    with pytest.raises(AssertionError, match='guard'):
        R.check(buf, ref, t, N, fin, lddx, 1e-4)
    # dval [E, S]: the row behind edge E - 1
    buf, off, ref, t = _filled(E, S, S, 2)
    R.check(buf, ref, t, E, S, S, 1e-4)
    buf[off:].reshape(-1, S)[E, 0] = 1.0
    with pytest.raises(AssertionError, match='guard'):
        R.check(buf, ref, t, E, S, S, 1e-4)
    # a dw [S Fin, Fout] that a GML_NO_FOLD call promises not to write: no columns of its own, every word a guard
    none = np.zeros((S * fin, 0))
    buf, off = R.alloc(S * fin, 0, fout)
    R.check(buf, none, none, S * fin, 0, fout, 1e-4)
    buf[off:].reshape(-1, fout)[17, 3] = 0.0
    with pytest.raises(AssertionError, match='guard'):
        R.check(buf, none, none, S * fin, 0, fout, 1e-4)
    # a flat workspace of n floats with 16 floats behind it, no guard rows
    n = S * fin * fout * 3
    buf, off, ref, t = _filled(1, n, n + 16, 3, guard_rows=0)
    assert buf.size == n + 16
    R.check(buf, ref, t, 1, n, n + 16, 1e-4, guard_rows=0)
    buf[n] = 0.0
    with pytest.raises(AssertionError, match='guard'):
        R.check(buf, ref, t, 1, n, n + 16, 1e-4, guard_rows=0)


def test_check_holds_a_derived_bound_beside_the_tolerance():
    buf, off, ref, t = _filled(30, 4, 4, 4)
    bound = np.full(ref.shape, 1e-6)
    R.check(buf, ref, t, 30, 4, 4, 1e-4, bound=bound)
    buf[off:].reshape(-1, 4)[3, 1] += np.float32(1e-5)              # inside 1e-4 of its term sum, outside the bound
    R.check(buf, ref, t, 30, 4, 4, 1e-4)
    with pytest.raises(AssertionError, match='derived bound'):
        R.check(buf, ref, t, 30, 4, 4, 1e-4, bound=bound)
