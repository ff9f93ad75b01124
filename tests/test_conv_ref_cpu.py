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
