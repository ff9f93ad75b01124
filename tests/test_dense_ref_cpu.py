"""CPU companion of tests/test_gpu_dense_abi.py: every case of the equal-size dense-block matrix, evaluated by the numpy emulation of
the kernels' arithmetic (tests/_dense_ref.py: operands split to bf16 pairs, three products, float32 accumulation) and held to the
bars the device is held to -- TOL on the max-norm and on every element's own term sum.  A case whose data correct arithmetic could
not hold fails here, without a GPU.  Also: the relu "either side" share stays at or below 1 % of an output, no case is degenerate (no
all-zero output, no term sum of zero where something is written), the case tables reach every template and road the matrix lists,
the restatement itself is checked against an independent formulation, and the launchers' plan (gml_dense_plan: answered on the
host, the library loads without a GPU) is held to the road every case names for each of its operands -- the float4 road needs the
width, the leading dimension, the column stride AND the pointer on the 16-byte grid; a misaligned float4 access gave the same
bits where it was tried, so only the plan shows a launcher that forgets one of the four."""
import numpy as np
import pytest

import _conv_ref as R
import _dense_ref as Q


def _meets(got, ref, what):
    assert np.isfinite(got).all(), what
    e_max, e_ts = R.errors(got, ref.v, ref.t)
    assert e_max <= Q.TOL, '%s: emulated max-norm figure %.3e' % (what, e_max)
    assert e_ts <= Q.TOL, '%s: emulated term-sum figure %.3e' % (what, e_ts)
    return e_max, e_ts


def _alive(ref, what, written=None):
    v, t = (ref.v, ref.t) if written is None else (ref.v[:, written], ref.t[:, written])
    assert v.size and np.abs(v).max() > 0, what + ': all-zero output'
    assert (t > 0).all(), what + ': an element without terms'


def _blocks_of(c, transposed):
    D = Q.blocks(c['B'], c['S'], c['n'])
    return np.ascontiguousarray(D.transpose(0, 1, 3, 2)) if transposed else D


@pytest.mark.parametrize('c', Q.MM_CASES, ids=lambda c: c['name'])
def test_support_mm_emulation_meets_the_bar(c):
    i = Q.inputs(c['B'], c['S'], c['n'], c['F'], act_cols=c['acols'])
    D = _blocks_of(c, c['form'] == 'a')
    ref, written = Q.support_mm_ref(D, i['act'], c['sa'], c['so'], c['sum_s'], c['F'])
    assert ref.v.shape == (c['B'] * c['n'], c['width'])
    _alive(ref, c['name'], written)
    _meets(Q.emu_support_mm(D, i['act'], c['sa'], c['so'], c['sum_s'], c['F']), ref, c['name'])


@pytest.mark.parametrize('c', Q.CF_CASES, ids=lambda c: c['name'])
def test_conv_fwd_emulation_meets_the_bar_and_relu_share(c):
    i = Q.inputs(c['B'], c['S'], c['n'], c['Fin'], c['Fout'])
    D = _blocks_of(c, False)
    bias = i['bias'] if c['bias'] else None
    ref = Q.conv_fwd_ref(D, i['x'], i['w'], bias, c['relu'])
    _alive(ref['out2'], c['name'])
    _alive(ref['hcat'], c['name'] + ' hcat')
    _meets(Q.emu_conv_fwd(D, i['x'], i['w'], bias, c['relu']), ref['out2'], c['name'])
    hc = Q.emu_H(D, i['x']).transpose(0, 2, 1, 3).reshape(ref['hcat'].v.shape)
    _meets(hc, ref['hcat'], c['name'] + ' hcat')
    if c['relu']:
        share = ref['near'].mean()
        assert share <= 0.01, '%s: %.2f %% of the output within the bar of zero' % (c['name'], 100 * share)
        assert (ref['pre'] < 0).mean() >= 0.05 and (ref['pre'] > 0).mean() >= 0.05, c['name'] + ': relu selects (almost) nothing'
    else:
        assert not ref['near'].any()


@pytest.mark.parametrize('c', Q.BX_CASES, ids=lambda c: c['name'])
def test_conv_bwd_x_emulation_meets_the_bar(c):
    i = Q.inputs(c['B'], c['S'], c['n'], c['Fin'], c['Fout'])
    D = _blocks_of(c, False)
    ref = Q.conv_bwd_x_ref(D, i['g'], i['w'])
    _alive(ref, c['name'])
    _meets(Q.emu_conv_bwd_x(D, i['g'], i['w']), ref, c['name'])


@pytest.mark.parametrize('c', Q.BW_CASES, ids=lambda c: c['name'])
def test_conv_bwd_w_emulation_meets_the_bar(c):
    i = Q.inputs(c['B'], c['S'], c['n'], c['Fin'], c['Fout'])
    D = _blocks_of(c, False)
    ref = Q.conv_bwd_w_ref(D, i['x'], i['g'])
    _alive(ref['dw'], c['name'])
    slices, per = Q.dw_slices(c['B']), ref['per']
    assert ref['partials'].v.shape == (slices, c['S'], c['Fin'], c['Fout'])
    used = -(-c['B'] // per)
    assert (ref['partials'].t[:used] > 0).all() and not ref['partials'].v[used:].any() and not ref['partials'].t[used:].any()
    np.testing.assert_allclose(ref['partials'].v.sum(0), ref['dw'].v, rtol=0, atol=1e-12 * ref['dw'].t.max())
    _meets(Q.emu_conv_bwd_w(D, i['x'], i['g']), ref['dw'], c['name'])


@pytest.mark.parametrize('c', Q.XW_CASES, ids=lambda c: c['name'])
def test_xty_wide_emulation_meets_the_bar(c):
    A, Bm = Q.xw_inputs(c)
    ref = Q.xty_ref(A, Bm)
    _alive(ref, c['name'])
    _meets(Q.emu_xty(A, Bm), ref, c['name'])


def test_slices_of_the_weight_gradient():
    """B = 65 and B = 129 leave trailing slices without a graph"""
    got = {c['B']: (Q.dw_slices(c['B']), -(-c['B'] // Q.dw_slices(c['B']))) for c in Q.BW_CASES}
    assert got[1] == (1, 1) and got[2] == (2, 1) and got[63] == (63, 1) and got[64] == (64, 1) and got[65] == (64, 2) and got[129] == (64, 3)
    assert -(-65 // 2) == 33 and -(-129 // 3) == 43                        # slices that own a graph: 31 and 21 stay empty


def test_bf16_rounding_and_pack_layout():
    """round-to-nearest-even on the float32 bits, against hand-worked patterns; the pair reproduces the value to 2^-17; the layout"""
    v = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23, -0.0, 0.0, -2.0 ** -126, 65280.0], np.float32)
    assert [hex(int(b)) for b in Q.bf16_bits(v)] == ['0x3f80', '0x3f80', '0x3f82', '0x3f81', '0x8000', '0x0', '0x8080', '0x477f']
    hi, lo = Q.split_bf16(Q.PACK_SPECIALS)
    assert np.array_equal(Q.bf16_rne(hi), hi) and np.array_equal(Q.bf16_rne(lo), lo)
    assert lo[0] == 0 and lo[1] == 0 and lo[4] != 0                                            # exactly bf16 / both pieces
    sub = Q.PACK_SPECIALS[9]                                                                   # 2^-120 (1 + 2^-9): residual 2^-129
    assert Q.split_bf16(np.array([sub]))[1][0] == np.float32(2.0 ** -129) and 0 < 2.0 ** -129 < np.finfo(np.float32).tiny
    assert np.signbit(hi[12]) and not np.signbit(lo[12]) and lo[12] == 0                         # -0.0 -> (0x8000, 0x0000)
    x = Q.rng('split').standard_normal(4096).astype(np.float32)
    h, l = Q.split_bf16(x)
    assert (np.abs(x.astype(np.float64) - h - l) <= 2.0 ** -17 * np.abs(x)).all()
    b = Q.pack_blocks(3, 5)
    for tr in (0, 1):
        img = Q.pack_ref(b, 32, tr)
        assert img.shape == (3, 2, 5, 32) and img.dtype == np.uint16 and not img[:, :, :, 5:].any()
        src = b.transpose(0, 2, 1) if tr else b
        assert np.array_equal(img[:, 0, :, :5], Q.bf16_bits(src)) and img[1, 0, 2, 3] == Q.bf16_bits(src[1, 2, 3])
    assert not np.array_equal(Q.pack_ref(b, 32, 0), Q.pack_ref(b, 32, 1))
    assert all((Q.pack_blocks(2, 9).reshape(-1)[:, None] == Q.PACK_SPECIALS[None, :]).any(0) | np.isnan(Q.PACK_SPECIALS))


def test_restatement_against_an_independent_formulation():
    """the einsum restatement against explicit per-graph matrix products: the chained forward, both gradients as the adjoints of
    the forward (<out, g> differentiated by finite structure: linearity makes them exact), and the Hcat layout"""
    B, S, n, Fin, Fout = 2, 3, 5, 4, 6
    i = Q.inputs(B, S, n, Fin, Fout)
    D = i['D'].astype(np.float64)
    x, w, g = i['x'].astype(np.float64), i['w'].astype(np.float64), i['g'].astype(np.float64)
    out = np.zeros((B * n, Fout))
    hcat = np.zeros((B * n, S * Fin))
    for b in range(B):
        for s in range(S):
            h = D[b, s] @ x[b * n:(b + 1) * n]
            hcat[b * n:(b + 1) * n, s * Fin:(s + 1) * Fin] = h
            out[b * n:(b + 1) * n] += h @ w[s]
    ref = Q.conv_fwd_ref(i['D'], i['x'], i['w'], None, False)
    assert np.allclose(ref['out2'].v, out, rtol=0, atol=1e-12) and np.allclose(ref['hcat'].v, hcat, rtol=0, atol=1e-12)
    mm, written = Q.support_mm_ref(i['D'], i['x'], 0, Fin, 0, Fin)
    assert written.all() and np.allclose(mm.v, hcat, rtol=0, atol=1e-12)
    # <out(x, w), g> is bilinear: its gradients are dx and dw
    dx = Q.conv_bwd_x_ref(i['D'], i['g'], i['w']).v
    dw = Q.conv_bwd_w_ref(i['D'], i['x'], i['g'])['dw'].v
    assert np.isclose((dx * x).sum(), (out * g).sum(), rtol=1e-12) and np.isclose((dw * w).sum(), (out * g).sum(), rtol=1e-12)
    e = np.zeros_like(x)
    e[7, 2] = 1.0
    assert np.isclose((Q.conv_fwd_ref(i['D'], e, i['w'], None, False)['out2'].v * g).sum(), dx[7, 2], rtol=1e-12)
    # the adjoint form of the support product on the transposed blocks is the adjoint of the forward form
    gh = Q.rng('gh').standard_normal((B * n, S * Fin))
    adj, _ = Q.support_mm_ref(i['D'].transpose(0, 1, 3, 2), gh, Fin, 0, 1, Fin)
    assert np.isclose((adj.v * x).sum(), (hcat * gh).sum(), rtol=1e-12)
    # a gap between the supports' column slices (so > F) is not written
    gap, written = Q.support_mm_ref(i['D'], i['x'], 0, Fin + 2, 0, Fin)
    assert written.tolist() == ([True] * Fin + [False] * 2) * 2 + [True] * Fin and np.allclose(gap.v[:, written], hcat, rtol=0, atol=1e-12)


def test_case_tables_reach_every_template_and_road():
    """what the matrix's last test requires to have run is reachable from the tables; the issue's sizes are all present"""
    ns = {c['n'] for c in Q.MM_CASES}
    assert ns >= {1, 15, 16, 17, 32, 33, 64, 65, 75, 96}
    assert {c['F'] for c in Q.MM_CASES} >= {1, 3, 4, 16, 17, 32, 33, 64, 65, 128}
    assert {(c['n'], c['KP']) for c in Q.MM_CASES} >= {(17, 64), (17, 96), (33, 96)}
    for tab in (Q.CF_CASES, Q.BX_CASES, Q.BW_CASES):
        assert {c['n'] for c in tab} >= {1, 15, 16, 17, 32, 33, 64, 65, 75, 96}
        assert {c['Fin'] for c in tab} >= {1, 3, 4, 16, 17, 32, 33, 64, 65, 128}
        assert {c['Fout'] for c in tab} >= {1, 4, 63, 64, 65, 128}
        assert {(c['n'], c['KP']) for c in tab} >= {(17, 64), (17, 96), (33, 96)}
    for tab in (Q.CF_CASES, Q.BX_CASES):
        assert {(Q.nft_of(c['Fin']), Q.not_of(c['Fout'])) for c in tab} == {(a, b) for a in (1, 2, 4, 8) for b in (4, 8)}
    assert {c['Fout'] for c in Q.BW_CASES} >= {144} and {c['B'] for c in Q.BW_CASES} >= {1, 2, 63, 64, 65, 129}
    assert all(c['n'] <= 17 for c in Q.BW_CASES if c['B'] >= 63)
    for form in 'fa':                                       # every condition of every road on its own
        mm = [c for c in Q.MM_CASES if c['form'] == form]
        assert {c['road_in'] for c in mm if c['road_out'] == 'vec'} >= {'vec', 'scalar:ld', 'scalar:ptr'}
        assert {c['road_out'] for c in mm if c['road_in'] == 'vec'} >= {'vec', 'scalar:ld', 'scalar:ptr'}
    assert {c['road_in'] for c in Q.MM_CASES} >= {'scalar:F', 'scalar:sa'} and {c['road_out'] for c in Q.MM_CASES} >= {'scalar:F', 'scalar:so'}
    assert {c['road_x'] for c in Q.CF_CASES} >= {'vec', 'scalar:F', 'scalar:ld', 'scalar:ptr'}
    assert {c['road_h'] for c in Q.CF_CASES} >= {'vec', 'scalar:F', 'scalar:ptr'}
    assert {c['road_o'] for c in Q.CF_CASES} >= {'vec', 'scalar:F', 'scalar:ld', 'scalar:ptr'}
    assert {c['road_o'] for c in Q.BX_CASES} >= {'vec', 'scalar:F', 'scalar:ld', 'scalar:ptr'}
    assert {c['road_x'] for c in Q.BW_CASES} >= {'vec', 'scalar:F', 'scalar:ld', 'scalar:ptr'}
    assert {(c['bias'], c['relu']) for c in Q.CF_CASES} == {(a, b) for a in (True, False) for b in (True, False)}
    for tab in (Q.MM_CASES, Q.CF_CASES, Q.BX_CASES, Q.BW_CASES):
        names = [c['name'] for c in tab]
        assert len(set(names)) == len(names)
        for c in tab:
            assert c['KP'] % 32 == 0 and c['n'] <= c['KP'] <= 96
            if c['same']:
                o = next(d for d in tab if d['name'] == c['same'])
                assert all(o[k] == c[k] for k in ('n', 'S', 'B') + (('F', 'form', 'sa', 'so') if 'F' in c else ('Fin', 'Fout'))), c['name']
                if 'relu' in c:
                    assert (o['bias'], o['relu']) == (c['bias'], c['relu']), c['name']


def test_plan_takes_the_road_every_case_names():
    """gml_dense_plan, the function the launchers themselves decide by, for every case of the four tables with its operands at
    synthetic addresses: 16-byte aligned, or 4 bytes past where the case says so"""
    from gnn_matlang_amd import _lib
    L = _lib.lib()
    at = lambda off: 0x7f0000100000 + (4 if off else 0)
    for c in Q.MM_CASES:
        assert Q.plan_ask(L, Q.MM, c, at(c['alead']), at(c['off4'])) == Q.plan_want(Q.MM, c), c['name']
    for c in Q.CF_CASES:
        assert Q.plan_ask(L, Q.CF, c, at(c['xlead']), at(c['hoff4']), at(c['off4'])) == Q.plan_want(Q.CF, c), c['name']
        assert Q.plan_ask(L, Q.CF, c, at(c['xlead']), 0, at(c['off4'])) == Q.plan_want(Q.CF, c, with_h=False), c['name']
    for c in Q.BX_CASES:
        assert Q.plan_ask(L, Q.BX, c, 0, at(c['off4'])) == Q.plan_want(Q.BX, c), c['name']
    for c in Q.BW_CASES:
        assert Q.plan_ask(L, Q.BW, c, at(c['xlead'])) == Q.plan_want(Q.BW, c), c['name']
    # each of the four conditions on its own takes each operand off the float4 road, every other address offset does too
    base = _lib.GML_DENSE_VEC_IN | _lib.GML_DENSE_VEC_OUT | 2 << 8
    mm = lambda pi=at(0), lda=36, sa=32, po=at(0), ldo=100, so=32, F=32: int(L.gml_dense_plan(0, pi, lda, sa, po, ldo, so, None, 0, F, 0))
    assert mm() == base
    for kw in (dict(pi=at(0) + 4), dict(pi=at(0) + 8), dict(pi=at(0) + 12), dict(lda=37), dict(sa=33), dict(sa=34)):
        assert mm(**kw) == base & ~_lib.GML_DENSE_VEC_IN, kw
    for kw in (dict(po=at(0) + 4), dict(po=at(0) + 8), dict(po=at(0) + 12), dict(ldo=101), dict(so=33), dict(so=34)):
        assert mm(**kw) == base & ~_lib.GML_DENSE_VEC_OUT, kw
    assert mm(F=30, lda=32, ldo=96) == 2 << 8 and mm(F=128) == base & 0xff | 8 << 8 and mm(pi=at(0) + 16, po=at(0) + 32) == base
    cf = lambda px=at(0), ldx=36, ph=at(0), po=at(0), ldo2=68, Fin=32, Fout=64: int(L.gml_dense_plan(1, px, ldx, 0, ph, 0, 0, po, ldo2, Fin, Fout))
    assert cf() == 7 | 2 << 8 | 4 << 16 and cf(ph=None) == 5 | 2 << 8 | 4 << 16
    assert cf(po=at(0) + 4) == 3 | 2 << 8 | 4 << 16 and cf(ldo2=67) == 3 | 2 << 8 | 4 << 16 and cf(Fout=62, ldo2=64) == 3 | 2 << 8 | 4 << 16
    assert cf(ph=at(0) + 4) == 5 | 2 << 8 | 4 << 16 and cf(px=at(0) + 4) == 6 | 2 << 8 | 4 << 16 and cf(Fout=65, ldo2=68) == 3 | 2 << 8 | 8 << 16
    assert [(int(L.gml_dense_plan(1, at(0), 128, 0, None, 0, 0, at(0), 128, F, 64)) >> 8) & 0xff for F in (1, 16, 17, 32, 33, 64, 65, 96, 97, 128)] == \
        [1, 1, 2, 2, 4, 4, 8, 8, 8, 8]
    assert [int(L.gml_dense_plan(3, at(0), 16, 0, None, 0, 0, None, 0, 16, Fo)) >> 16 for Fo in (1, 64, 65, 128, 129, 144, 1000, 16257, 16320)] == \
        [1, 1, 2, 2, 3, 3, 16, 255, 255]
    # the weight gradient's bound: 255 workgroups along Fout is what the plan word holds; beyond it both the plan and the launcher refuse
    assert all(int(L.gml_dense_plan(3, at(0), 16, 0, None, 0, 0, None, 0, 16, Fo)) == _lib.GML_E_UNSUPPORTED for Fo in (16321, 16384, 16385, 1 << 21, 2 ** 31 - 1))
    assert all(int(L.gml_dense_plan(3, at(0), 16, 0, None, 0, 0, None, 0, F, 16320)) > 0 for F in (1, 128))
    U, B_ = _lib.GML_E_UNSUPPORTED, _lib.GML_E_BADARG
    ask = lambda e, F, Fo: int(L.gml_dense_plan(e, at(0), 256, 0, at(0), 256, 0, at(0), 256, F, Fo))
    assert [ask(-1, 32, 32), ask(4, 32, 32)] == [B_, B_] and all(ask(e, F, 32) == U for e in range(4) for F in (0, 129))
    assert all(ask(e, 32, Fo) == U for e in (1, 2) for Fo in (0, 129)) and ask(3, 32, 0) == U and ask(3, 32, 129) > 0 and ask(0, 32, 0) > 0
