"""The fused conv backward at the level of its C ABI (include/gml.h): gml_spectconv_bwd, _bwd_mix, _bwd_mix_relu, _bwd_mix_relu2 and
_bwd_had on every kernel family and launch mode against the float64 restatement of tests/_conv_ref.py -- one launch and one numpy
reference per case, through _lib.lib() directly, so that a case decides everything functional.py never varies: which of dx / dval /
dw are NULL, GML_ACCUM, GML_DVAL_ACCUM and GML_NO_FOLD, ldx > Fin, lddx > Fin, x / dx / g four bytes off a 16-byte boundary, padded g
rows, nmix and the two-array wmix forms, relu_cols strictly inside (0, Fin), the output stage with and without dx, and the error
answers callers fall back on.

Which kernel a case reaches is read off the dispatch (csrc/gml_spectconv_bwd.hip, plan_bwd / spectconv_bwd_impl): 64-row records with
GML_F32_MFMA (or a shape only that kernel has) -> the 64-row f32-MFMA kernel; 128-row records -> the 8-wave bf16x3 kernel bwd3, or
with GML_DMA_RING its ring form bwd4 while every group fits the ring and nothing asks for an accumulate -- else bwd3 again (labelled
"bwd4>bwd3").  The graphs' roles (inside every staging / beyond the staged edges / windows beyond the staged rows / refused by the
LDS plan) are asserted in the fixture against gml_spectconv_bwd_stage_edges / _stage_window / _workspace_bytes.

Every output sits in a buffer of _conv_ref.alloc(): dx columns Fin .. lddx - 1, 8 rows behind dx, dval and dw, 4 floats in front of
an offset dx and 16 floats behind the workspace hold a NaN sentinel and must still hold it; an output the call promises not to write
(NULL pointers aside: a dw under GML_NO_FOLD, everything after an error answer) must be bit-unchanged.  Values are held to TOL = 1e-4
on the max-norm (conftest.rel_err) AND elementwise on each element's own term sum.

The 64-row kernel is also held to a derived bound.  gml.h documents its arithmetic as an fmaf chain: every product and every
addition is one fp32 rounding, relative error at most u = 2^-24.  A sum of n rounded products, accumulated in ANY order (a chain, the
MFMA's 4-deep blocks, per-workgroup partials folded later), therefore lies within ((1 + u)^n - 1) T ~ n u T of the exact sum, T the
sum of the terms' absolute values.  Every output is formed in two chained stages -- Z = x W_s or P = sum val g first, then the
contraction with g or the projection with W / x -- so each outer term carries an inner relative error of at most n u as well: the
figure doubles.  With n = the number of terms the reference counts for the element (deg S Fout for dx, Fin Fout for dval, E for dw)
and c = 8 for the roundings outside the sums, |got - ref| <= 2 (n + 8) u T (_conv_ref.f32_bound).  A correct fp32 kernel cannot exceed
it; an excess is a finding.

The worst figures per (family, arithmetic, output) are printed by the last test (pytest -rP) and recorded in DESIGN.md s4.2a."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _conv_ref as R
from gnn_matlang_amd import _lib
from test_gpu_conv_fwd_abi import _Out, _done, _f32, _p, _rng, _up

# the library reads these once per process; each silently changes which kernel a label below means
assert not [k for k in ('GML_BWD_DMA', 'GML_BWD_WIDE48', 'GML_BWD_HAD') if k in os.environ], 'run without the backward A/B switches'

pytestmark = pytest.mark.gpu

TOL = 1e-4
N = 300
OK, BAD, UNS, WSP = _lib.GML_OK, _lib.GML_E_BADARG, _lib.GML_E_UNSUPPORTED, _lib.GML_E_WORKSPACE
F32, RING, ACC, DACC, NOFOLD = _lib.GML_F32_MFMA, _lib.GML_DMA_RING, _lib.GML_ACCUM, _lib.GML_DVAL_ACCUM, _lib.GML_NO_FOLD
WORST = {}                                                  # (family, arithmetic, output) -> [cases, worst max-norm, worst term-sum figure]
RAN = set()                                                 # (kernel, S, NFB[, NOB]) instantiations that ran
ROLES = {}                                                  # (family, graph) -> [ran, refused]
# the compiled instantiations (csrc/gml_spectconv_bwd.hip: GML_BWD_SHAPES / GML_BWD3_SHAPES / GML_BWD4_SHAPES)
BWD_SHAPES = [(8, 2, 2), (8, 1, 2), (4, 2, 2), (4, 1, 2), (12, 2, 1), (12, 1, 1), (6, 3, 2), (6, 1, 2), (4, 3, 2), (6, 2, 2), (8, 2, 1), (4, 4, 2)]
BWD3_SHAPES = [(8, 2, 2), (8, 1, 2), (6, 2, 2), (6, 1, 2), (4, 2, 2), (4, 1, 2), (2, 2, 2), (2, 1, 2), (6, 3, 2), (4, 3, 2), (12, 2, 1), (12, 1, 1),
               (8, 2, 1), (8, 1, 1)]
BWD4_SHAPES = [(8, 2), (8, 1), (4, 2), (4, 1)]


def _r4(n):
    return (n + 3) // 4 * 4


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    assert _lib.lib().gml_version() >= 1
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------------------------------- graphs
def _band_src(rng, n, half, deg):
    """every SOURCE row sends `deg` edges to distinct targets within +-half of itself: [2, E] (source, target), sorted by (source,
    target) -- the source-keyed CSR order is the input order, and a group of r rows holds exactly r deg edges"""
    src, dst = [], []
    for r in range(n):
        lo, hi = max(r - half, 0), min(r + half, n - 1)
        dst.append(np.sort(rng.choice(np.arange(lo, hi + 1), size=min(deg, hi - lo + 1), replace=False)))
        src.append(np.full(dst[-1].size, r))
    return np.stack([np.concatenate(src), np.concatenate(dst)]).astype(np.int64)


def _with(ei, src, dst):
    e = np.concatenate([ei, np.array([src, dst], np.int64)], 1)
    return e[:, np.lexsort((e[1], e[0]))]


def _records(ei, n, rows):
    """{first edge, edges, smallest target, window width} per group of `rows` source rows, as gml_csr_group_info defines them"""
    rowptr = np.zeros(n + 1, np.int64)
    np.add.at(rowptr, ei[0] + 1, 1)
    rowptr = np.cumsum(rowptr)
    rec = []
    for r0 in range(0, n, rows):
        kb, ke = rowptr[r0], rowptr[min(r0 + rows, n)]
        c = ei[1][kb:ke]
        rec.append([kb, ke - kb, c.min() if ke > kb else 0, c.max() - c.min() + 1 if ke > kb else 0])
    return rowptr, np.array(rec, np.int64)


class _Graph(object):
    def __init__(self, dev, name, ei, n):
        from gnn_matlang_amd.graph import GraphCSR
        self.name, self.N, self.E, self.eis = name, n, ei.shape[1], ei       # eis: (source, target) in the source-keyed CSR order
        assert (np.diff(ei[0]) >= 0).all()
        self.csr = GraphCSR.from_edge_index(torch.from_numpy(ei).to(dev), n)
        rowptr, self.rec128 = _records(ei, n, 128)
        _, self.rec64 = _records(ei, n, 64)
        assert np.array_equal(self.csr.rowptr_t.cpu().numpy(), rowptr) and np.array_equal(self.csr.col_t.cpu().numpy(), ei[1])
        assert np.array_equal(self.csr.ginfo_t128.cpu().numpy()[:, :4], self.rec128), name
        assert np.array_equal(self.csr.ginfo_t.cpu().numpy()[:, :4], self.rec64), name

    def rec(self, rows):
        """(device records, host records, (max edges, max window)) of the `rows`-row groups of the source-keyed view"""
        h = self.rec128 if rows == 128 else self.rec64
        return (self.csr.ginfo_t128 if rows == 128 else self.csr.ginfo_t), h, (int(h[:, 1].max()), int(h[:, 3].max()))


@pytest.fixture(scope='module')
def graphs(dev):
    L = _lib.lib()
    rng = np.random.default_rng(20241)
    a = _band_src(rng, N, 6, 5)
    a = a[:, a[0] != 77]                                    # one empty source row
    # C: a few edges from the first 60 rows to rows 236 .. 247 and from row 290 back to row 55
    c = _with(a, [3, 17, 31, 44, 59, 290], [240, 236, 247, 238, 244, 55])
    eis = {'A': (a, N), 'H': (_band_src(rng, N, 12, 17), N), 'H12': (_band_src(rng, N, 12, 13), N), 'C': (c, N),
           'B': (_band_src(rng, N, 30, 48), N), 'D7': (_band_src(rng, 7, 3, 2), 7), 'D129': (_band_src(rng, 129, 6, 5), 129)}
    g = {k: _Graph(dev, k[:1] if k[0] == 'H' else k, ei, n) for k, (ei, n) in eis.items()}
    A, H, H12, C, B = g['A'], g['H'], g['H12'], g['C'], g['B']
    se = lambda S, fin, fout, fl: int(L.gml_spectconv_bwd_stage_edges(S, fin, fout, fl))
    sw = lambda S, fin, fout, fl: int(L.gml_spectconv_bwd_stage_window(S, fin, fout, fl))
    ws = lambda gr, rows, S, fin, fout, fl: int(L.gml_spectconv_bwd_workspace_bytes(gr.N, S, fin, fout, *gr.rec(rows)[2], fl))
    k128 = [(8, 32, 32, 0), (4, 32, 32, 0), (6, 32, 32, 0), (2, 32, 32, 0), (12, 32, 16, 0), (8, 32, 16, 0), (4, 48, 32, 0), (6, 48, 32, 0),
            (8, 32, 32, RING), (4, 32, 32, RING)]                            # every staging of the 8-wave kernel and of its ring form
    k64 = [(8, 32, 32, F32), (4, 64, 32, 0), (12, 32, 16, F32)]              # the 64-row kernel's one staging (S = 6 has none: 0)
    assert all(se(*k) > 0 and sw(*k) > 0 for k in k128 + k64) and se(6, 32, 32, F32) == 0
    assert not (A.eis[0] == 77).any() and (A.eis[0] == 0).any() and (A.eis[0] == N - 1).any()
    assert [r[1] for r in A.rec128.tolist()] == [128 * 5 - 5, 128 * 5, 44 * 5]
    # A: every group inside every staging of every family
    assert all(A.rec(128)[2][0] <= se(*k) and A.rec(128)[2][1] <= sw(*k) for k in k128), A.rec(128)[2]
    assert all(A.rec(64)[2][0] <= se(*k) and A.rec(64)[2][1] <= sw(*k) for k in k64), A.rec(64)[2]
    # H: full groups beyond the staged edges of each family (17 per row: 2,176 per 128 rows, 1,088 per 64), the last partial group
    # inside; still served
    assert all(H.rec128[:2, 1].min() > se(*k) and H.rec128[-1, 1] <= se(*k) and H.rec(128)[2][1] <= sw(*k) for k in k128 if k[0] != 12), H.rec128[:, :4]
    assert all(H.rec64[:4, 1].min() > se(*k) and H.rec64[-1, 1] <= se(*k) for k in k64), H.rec64[:, :4]
    assert all(ws(H, 128, *k) > 0 for k in k128 if k[0] != 12) and all(ws(H, 64, *k) > 0 for k in k64)
    # (the 160 KB plan refuses 2,176-edge groups at S = 12, whose value rows are staged in LDS: that class takes the role on H12, 13 per
    # row = 1,664 per 128 rows against its 1,536)
    k12 = (12, 32, 16, 0)
    assert ws(H, 128, *k12) == 0 and ws(H12, 128, *k12) > 0 and H12.rec128[:2, 1].min() > se(*k12) >= H12.rec128[-1, 1] and H12.rec(128)[2][1] <= sw(*k12)
    # C: some windows just beyond the staged rows of each family, beside groups that stay staged; still served
    # (but for the 33 .. 48-feature class of the 8-wave kernel: its second X and W images leave the plan room for 208 window rows at
    # these edge counts, fewer than the 224 its staging would take -- the plan refuses C there and the 64-row kernel serves it)
    wide = [k for k in k128 if k[1] > 32]
    k128c = [k for k in k128 if k[1] <= 32]
    assert all(C.rec128[:, 3].max() > sw(*k) >= C.rec128[:, 3].min() and C.rec(128)[2][0] <= se(*k) for k in k128), C.rec128[:, :4]
    assert len(wide) == 2 and all(ws(C, 128, *k) == 0 and ws(C, 64, *k[:3], F32) > 0 for k in wide)
    assert all(C.rec64[:, 3].max() > sw(*k) >= C.rec64[:, 3].min() for k in k64), C.rec64[:, :4]
    assert 225 <= C.rec128[:, 3].max() <= 250 and 225 <= C.rec64[:, 3].max() <= 250
    assert all(ws(C, 128, *k) > 0 for k in k128c) and all(ws(C, 64, *k) > 0 for k in k64)
    # B: the LDS plan refuses the 128-row kernel at S = 8 and S = 4; the 64-row kernel takes the same shapes with its records
    # (where workspace_bytes says so: asserted per case)
    assert ws(B, 128, 8, 32, 32, 0) == 0 and ws(B, 128, 4, 32, 32, 0) == 0 and ws(B, 128, 8, 32, 32, RING) == 0, B.rec(128)[2]
    assert ws(B, 64, 4, 32, 32, F32) > 0, B.rec(64)[2]
    assert g['D7'].rec128.shape[0] == 1 and g['D129'].rec128.shape[0] == 2 and g['D129'].rec64.shape[0] == 3
    return g


# ------------------------------------------------------------------------------------------------------------------------- one launch
def _note(fam, arith, out, e_max, e_ts):
    w = WORST.setdefault((fam, arith, out), [0, 0.0, 0.0])
    w[0] += 1
    w[1], w[2] = max(w[1], e_max), max(w[2], e_ts)


def _flat(dev, n, out0=None, tail=16):
    """a flat buffer of n floats with `tail` sentinel floats behind it"""
    return _Out(dev, 1, n, n + tail, False, out0, guard_rows=0)


def _ring_runs(L, S, fin, fout, fl, ldx, xlead, dxvec, has_dx, has_dz, me, mw):
    """the dispatch's own conditions for the ring form, capacities from the stage queries"""
    if not (fl & RING) or S not in (4, 8) or fin > 32 or fl & (ACC | DACC) or fin % 4 or ldx % 4 or xlead:
        return False
    if has_dx and has_dz and not dxvec:
        return False
    return me <= int(L.gml_spectconv_bwd_stage_edges(S, fin, fout, RING)) and mw <= int(L.gml_spectconv_bwd_stage_window(S, fin, fout, RING))


def run_bwd(dev, g, fam, S, fin, fout, conds=(), ldx=None, mix=None, had=None, expect=OK, f32flag=True, over=None):
    """One backward launch and its check.  fam: '64' (64-row records; GML_F32_MFMA unless f32flag = False: a shape only that kernel
    has), 'bwd3' (128-row records), 'bwd4' (128-row records, GML_DMA_RING).  conds:
      nodx / nodval / nodw (NULL pointers), accum (GML_ACCUM, dx pre-filled), dvalacc (GML_DVAL_ACCUM, dval pre-filled), nofold
      (GML_NO_FOLD), ldxpad (ldx = roundup4(Fin) + 4, junk padding), xoff (x 4 bytes past a 16-byte boundary), lddx3 / lddx4
      (lddx = Fin + 3 / + 4), dxoff (dx 4 bytes off), ldg8 (ldg = roundup4(columns) + 8, junk behind the zero padding), ldgodd
      (ldg = Fout), goff (g 4 bytes off), wsbig (ws_bytes 64 more than asked), wsshort (one byte less), valoff / dvaloff.
    mix = {'na', 'nb' (None: the one-array entries), 'relu' (None: gml_spectconv_bwd_mix)}; had = {'dx', 'relu', 'bias', 'fold'}.
    expect: the return code; anything but GML_OK must leave every output bit-unchanged.  over: ldx / ldg / lddx / num_rows as passed."""
    from gnn_matlang_amd.graph import _stream
    L = _lib.lib()
    conds, over = tuple(conds), dict(over or {})
    rows = 64 if fam == '64' else 128
    gi, rec, (me, mw) = g.rec(rows)
    fl = (F32 if fam == '64' and f32flag else 0) | (RING if fam == 'bwd4' else 0) | (ACC if 'accum' in conds else 0) | \
        (DACC if 'dvalacc' in conds else 0) | (NOFOLD if 'nofold' in conds else 0)
    nd = g.N
    gcols = fout + (2 if had else 0)
    ldx = (_r4(fin) + 4 if 'ldxpad' in conds else fin) if ldx is None else ldx
    ldg = fout if 'ldgodd' in conds else _r4(gcols) + (8 if 'ldg8' in conds else 0)
    lddx = fin + (3 if 'lddx3' in conds else 4 if 'lddx4' in conds else 0)
    rng = _rng('bwd', fam, S, fin, fout, conds, ldx, sorted((mix or {}).items()), sorted((had or {}).items()), g.name, f32flag)
    val, x = _f32(rng.standard_normal((g.E, S))), _f32(rng.standard_normal((nd, ldx)))
    w = _f32(rng.standard_normal((S, fin, fout)) * fin ** -0.5)
    ga = _f32(rng.standard_normal((nd, ldg)))
    ga[:, gcols:min(_r4(gcols), ldg)] = 0                    # gml.h: the padding columns up to roundup4 are zero; behind them: junk
    dx0 = _f32(rng.standard_normal((nd, fin))) if 'accum' in conds else None
    dval0 = _f32(rng.standard_normal((g.E, S))) if 'dvalacc' in conds else None
    relu_cols, dz, dzt, wmix, hr = 0, None, None, None, None
    if mix is not None:
        relu_cols = mix.get('relu') or 0
        x[::3, :relu_cols], x[1::7, :relu_cols] = 0.0, -0.0  # the mask's edge: exact zeros of both signs
        nmix = mix['na'] + (mix['nb'] or 0)
        dz4 = _f32(rng.standard_normal((nd, 4)))             # columns >= nmix: junk the kernel must ignore
        wma, wmb = _f32(rng.standard_normal((max(mix['na'], 1), fin)) * 0.5), _f32(rng.standard_normal((max(mix['nb'] or 0, 1), fin)) * 0.5)
        dz, wmix = dz4[:, :nmix], np.concatenate([wma[:mix['na']], wmb[:mix['nb'] or 0]])
    if had is not None:
        relu_cols = had['relu']
        x[::3, :relu_cols], x[1::7, :relu_cols] = 0.0, -0.0
        w11, w12 = (_f32(rng.standard_normal((2, fin)) * fin ** -0.5) for _ in range(2))
        b11, b12 = (_f32(rng.random(2) - 0.5) if had['bias'] else None for _ in range(2))
        dz, dzt, hr = R.had_ref(x[:, :fin], ga, fout, w11, b11, w12, b12)
        wmix = np.concatenate([w11, w12])
    ldx_p, ldg_p, lddx_p, n_p = over.get('ldx', ldx), over.get('ldg', ldg), over.get('lddx', lddx), over.get('num_rows', nd)
    want_dx = 'nodx' not in conds and (had is None or had['dx'])

    xl, gl, vl = int('xoff' in conds), int('goff' in conds), int('valoff' in conds)
    xd, gd, vd, wd = _up(x, dev, xl), _up(ga, dev, gl), _up(val, dev, vl), _up(w, dev)
    dx = _Out(dev, nd, fin, lddx, 'dxoff' in conds, dx0) if want_dx else None
    dval = _Out(dev, g.E, S, S, 'dvaloff' in conds, dval0) if 'nodval' not in conds else None
    dw = _Out(dev, S * fin, fout, fout) if 'nodw' not in conds else None
    need = int(L.gml_spectconv_bwd_workspace_bytes(nd, S, fin, fout, me, mw, fl))
    nws = max(need // 4, 64)
    ws = _flat(dev, nws)
    ws_bytes = need + (64 if 'wsbig' in conds else -1 if 'wsshort' in conds else 0)
    outs = [o for o in (dx, dval, dw, ws) if o is not None]
    tail = (n_p, S, fin, fout, me, mw, fl, ws.ptr(), ws_bytes)
    head = (_p(g.csr.rowptr_t), _p(g.csr.col_t), _p(gi), _p(vd, vl), _p(xd, xl), ldx_p, _p(gd, gl), ldg_p, _p(wd),
            dx.ptr() if dx else _p(None), lddx_p, dval.ptr() if dval else _p(None), dw.ptr() if dw else _p(None))
    if had is not None:
        parts = int(L.gml_spectconv_bwd_had_parts(nd, S, fin, fout, 2, int(had['dx']), me, mw, fl))
        npart = 4 * fin + 4 + fout
        hws = _flat(dev, max(parts, 1) * npart)
        hd = [_up(a, dev) if a is not None else None for a in (w11, b11, w12, b12)]
        ho = {}
        if had['fold']:
            ho = {'dcb': _Out(dev, 1, fout, fout), 'dw11': _Out(dev, 2, fin, fin), 'dw12': _Out(dev, 2, fin, fin)}
            if had['bias']:
                ho.update({'db11': _Out(dev, 1, 2, 2), 'db12': _Out(dev, 1, 2, 2)})
        outs += [hws] + list(ho.values())
        hp = lambda k: ho[k].ptr() if k in ho else _p(None)
        rc = L.gml_spectconv_bwd_had(*head, _p(hd[0]), _p(hd[1]), _p(hd[2]), _p(hd[3]), relu_cols, hp('dcb'), hp('dw11'), hp('db11'),
                                     hp('dw12'), hp('db12'), n_p, S, fin, fout, 2, me, mw, fl, ws.ptr(), ws_bytes, hws.ptr(),
                                     max(parts, 1) * npart * 4, _stream(dev))
    elif mix is not None:
        dzd, wad, wbd = _up(dz4, dev), _up(wma, dev), _up(wmb, dev)
        if mix['nb'] is not None:
            rc = L.gml_spectconv_bwd_mix_relu2(*head, _p(dzd), _p(wad), mix['na'], _p(wbd) if mix['nb'] else _p(None), mix['nb'], relu_cols, *tail,
                                               _stream(dev))
        elif mix.get('relu') is not None:
            rc = L.gml_spectconv_bwd_mix_relu(*head, _p(dzd), _p(wad), mix['na'], relu_cols, *tail, _stream(dev))
        else:
            rc = L.gml_spectconv_bwd_mix(*head, _p(dzd), _p(wad), mix['na'], *tail, _stream(dev))
    else:
        rc = L.gml_spectconv_bwd(*head, *tail, _stream(dev))
    rc = _done(rc)

    dxvec = want_dx and fin % 4 == 0 and lddx % 4 == 0 and 'dxoff' not in conds
    ring = fam == 'bwd4' and had is None and _ring_runs(L, S, fin, fout, fl, ldx, xl, dxvec, want_dx, mix is not None, me, mw)
    label = {'64': '64', 'bwd3': 'bwd3', 'bwd4': 'bwd4' if ring else 'bwd4>bwd3'}[fam] + (' DZ' if mix is not None else ' HAD' if had else '')
    what = '%s graph %s S=%d Fin=%d(ld %d) Fout=%d(ld %d) lddx=%d %s%s%s flags=%#x' % (
        label, g.name, S, fin, ldx, fout, ldg, lddx, '+'.join(conds) or 'plain', ' mix=%s' % sorted(mix.items()) if mix else '',
        ' had=%s' % sorted(had.items()) if had else '', fl)
    role = ROLES.setdefault((fam + (' DZ' if mix is not None else ' HAD' if had else ''), g.name), [0, 0])
    assert rc == expect, '%s: return code %d, expected %d' % (what, rc, expect)
    if expect != OK:
        for o in outs:
            assert o.unchanged(), what + ': a refused call wrote to an output'
        role[1] += 1
        return None
    role[0] += 1
    nfb, nob = (fin + 15) // 16, (fout + 15) // 16
    RAN.add(('bwd4', S, nfb) if ring else ('bwd', S, nfb, nob) if fam == '64' else ('bwd3', S, nfb, nob))
    arith = 'f32' if fam == '64' else 'bf16'
    ref = R.conv_bwd_ref(g.eis, val, x[:, :fin], ga[:, :fout], w, dx0, dval0, dz, wmix, relu_cols, dzt)
    bound = (lambda r: R.f32_bound(r)) if fam == '64' else (lambda r: None)
    raw = {}

    def held(name, buf, r, n, ncols, ld, **kw):
        raw[name] = np.array(buf, np.float32)
        e = R.check(raw[name], r.v.reshape(n, ncols), r.t.reshape(n, ncols), n, ncols, ld, TOL, what + ' ' + name,
                    bound=None if bound(r) is None else np.broadcast_to(bound(r), r.v.shape).reshape(n, ncols), **kw)
        print('%-150s %-5s max-norm %.2e  term-sum %.2e' % (what, name, e[0], e[1]))
        _note(label, arith, name, *e)

    if dx is not None:
        held('dx', dx.get(), ref['dx'], nd, fin, lddx)
    if dval is not None:
        held('dval', dval.get(), ref['dval'], g.E, S, S)
    nw = S * fin * fout
    if dw is None:
        assert ws.unchanged(), what + ': no dw wanted, the workspace was written'
    else:
        wsb = ws.get().copy()
        _, guards = R.split(wsb, 1, nws, nws + 16, 0)
        assert (guards == R.SENTINEL).all(), what + ': the floats behind the workspace were written'
        if 'nofold' in conds:
            R.check(dw.get(), np.zeros((S * fin, 0)), np.zeros((S * fin, 0)), S * fin, 0, fout, TOL, what + ' dw (must stay unwritten)')
            assert need % (4 * nw) == 0
            part = wsb[:need // 4].reshape(need // (4 * nw), nw).astype(np.float64).sum(0).astype(np.float32)
            held('dw', R.alloc(S * fin, fout, fout, out0=part.reshape(S * fin, fout))[0], ref['dw'], S * fin, fout, fout)
        else:
            held('dw', dw.get(), ref['dw'], S * fin, fout, fout)
    if had is not None:
        hb = hws.get().copy()
        _, guards = R.split(hb, 1, parts * npart, parts * npart + 16, 0)
        assert parts > 0 and (guards == R.SENTINEL).all(), what + ': the floats behind hws were written'
        psum = hb[:parts * npart].reshape(parts, npart).astype(np.float64).sum(0).astype(np.float32)
        seg = {'dw11': (0, 2, fin), 'dw12': (2 * fin, 2, fin), 'db11': (4 * fin, 1, 2), 'db12': (4 * fin + 2, 1, 2), 'dcb': (4 * fin + 4, 1, fout)}
        for k, (o0, r_, c_) in seg.items():
            if k in ('db11', 'db12') and not had['bias']:
                continue
            buf = ho[k].get() if had['fold'] else R.alloc(r_, c_, c_, out0=psum[o0:o0 + r_ * c_].reshape(r_, c_))[0]
            held(k, buf, R.Ref(hr[k].v.reshape(r_, c_), hr[k].t.reshape(r_, c_), hr[k].n), r_, c_, c_)
    return raw


def _pick(graphs, gname, fam, S):
    """the graph that takes role `gname` for this kernel class (H: H12 for the 8-wave kernel at S = 12, see the fixture)"""
    return graphs['H12' if gname == 'H' and S == 12 and fam != '64' else gname]


def _f32_native(S, fin, fout):
    return int(_lib.lib().gml_spectconv_bwd_group_rows(S, fin, fout, 0)) == 64


# ------------------------------------------------------------------------------------------------------------------------- 64-row kernel
# every (S, NFB, NOB) of GML_BWD_SHAPES: Fin in {3, 16, 17, 20, 32, 33, 48, 64}, Fout in {1, 9, 16, 17, 30, 32}
FAM64 = [(8, 32, 32), (8, 17, 30), (8, 20, 17), (8, 16, 32), (8, 3, 17), (4, 32, 30), (4, 20, 32), (4, 16, 17), (4, 3, 30), (12, 32, 16), (12, 17, 9),
         (12, 16, 1), (12, 3, 16), (6, 48, 32), (6, 33, 17), (6, 16, 30), (6, 3, 32), (4, 48, 30), (4, 33, 32), (6, 32, 32), (6, 20, 17), (8, 32, 9),
         (8, 20, 1), (8, 17, 16), (4, 64, 32), (4, 49, 17)]
FAM64_DIAG = [(8, 32, 32), (8, 16, 30), (4, 20, 17), (4, 3, 32), (12, 32, 9), (12, 16, 16), (6, 48, 17), (6, 16, 32), (4, 33, 30), (6, 20, 32),
              (8, 17, 1), (4, 64, 17)]                      # one per instantiation


@pytest.mark.parametrize('S,fin,fout', FAM64)
def test_family64_shapes(dev, graphs, S, fin, fout):
    """S = 6 has no staged road (float2 value rows), S in {4, 8, 12} take it on this graph"""
    run_bwd(dev, graphs['A'], '64', S, fin, fout)


@pytest.mark.parametrize('S,fin,fout', [(4, 64, 32), (4, 49, 17), (4, 64, 17)])
def test_family64_shapes_that_reach_it_without_the_flag(dev, graphs, S, fin, fout):
    assert _f32_native(S, fin, fout)
    run_bwd(dev, graphs['A'], '64', S, fin, fout, f32flag=False)


@pytest.mark.parametrize('gname', ['H', 'C', 'D7', 'D129'])
@pytest.mark.parametrize('S,fin,fout', FAM64_DIAG)
def test_family64_graphs(dev, graphs, gname, S, fin, fout):
    """H: groups beyond the staged edges, C: windows beyond the staged rows (both: the rolled loops), D: partial groups"""
    run_bwd(dev, graphs[gname], '64', S, fin, fout)


NULLS = [('nodx',), ('nodval',), ('nodw',), ('nodx', 'nodval'), ('nodx', 'nodw'), ('nodval', 'nodw'), ('nodx', 'nodval', 'nodw')]
COMMON = [('accum',), ('nofold',), ('ldxpad',), ('xoff',), ('lddx3',), ('lddx4',), ('dxoff',), ('ldg8',), ('wsbig',)]
TOGETHER = ('accum', 'nofold', 'ldxpad', 'xoff', 'lddx3', 'dxoff', 'ldg8', 'wsbig')
TOGETHER4 = ('accum', 'nofold', 'ldxpad', 'lddx4', 'ldg8', 'wsbig')           # the float4 roads kept
_ids = lambda c: '+'.join(c) if isinstance(c, tuple) else str(c)


@pytest.mark.parametrize('conds', NULLS + COMMON + [('goff',), TOGETHER, TOGETHER4, TOGETHER + ('goff',)], ids=_ids)
@pytest.mark.parametrize('S,fin,fout,gname', [(8, 32, 32, 'A'), (6, 33, 17, 'C'), (12, 17, 9, 'H'), (4, 64, 32, 'A')])
def test_family64_conditions(dev, graphs, conds, S, fin, fout, gname):
    run_bwd(dev, graphs[gname], '64', S, fin, fout, conds)


@pytest.mark.parametrize('conds', [('ldgodd',), ('ldgodd', 'goff'), TOGETHER[:-2] + ('ldgodd', 'goff', 'wsbig')], ids=_ids)
@pytest.mark.parametrize('S,fin,fout,gname', [(8, 32, 17, 'A'), (6, 20, 31, 'C'), (12, 17, 9, 'H'), (4, 64, 29, 'A')])
def test_family64_unpadded_gradient_rows(dev, graphs, conds, S, fin, fout, gname):
    """ldg = Fout odd and g 4 bytes off: no float4 road for g, hence no staged road either"""
    run_bwd(dev, graphs[gname], '64', S, fin, fout, conds)


def test_family64_dval_accumulate_is_refused_untouched(dev, graphs):
    for S, fin, fout in [(8, 32, 32), (4, 64, 32), (12, 17, 9)]:
        run_bwd(dev, graphs['A'], '64', S, fin, fout, ('dvalacc',), expect=UNS)


# ------------------------------------------------------------------------------------------------------------------------- bwd3
BWD3_FIN = [(4, 4), (16, 16), (17, 17), (25, 28), (32, 32)]  # (Fin, ldx): 25 features in float4-addressable rows of 28; 17: the scalar x road
BWD3_WIDE = [(33, 36), (36, 36), (44, 44), (48, 48), (33, 33)]
BWD3_DIAG = [(8, 32, 32, 32), (8, 16, 16, 17), (6, 25, 28, 30), (6, 4, 4, 32), (4, 17, 17, 17), (4, 16, 16, 30), (2, 32, 32, 30), (2, 4, 4, 17),
             (6, 44, 44, 32), (4, 33, 36, 17), (12, 32, 32, 16), (12, 16, 16, 9), (8, 25, 28, 1), (8, 4, 4, 16)]      # one per instantiation


@pytest.mark.parametrize('fout', [17, 30, 32])
@pytest.mark.parametrize('fin,ldx', BWD3_FIN)
@pytest.mark.parametrize('S', [2, 4, 6, 8])
def test_bwd3_shapes(dev, graphs, S, fin, ldx, fout):
    run_bwd(dev, graphs['A'], 'bwd3', S, fin, fout, ldx=ldx)


@pytest.mark.parametrize('fout', [1, 9, 16])
@pytest.mark.parametrize('fin,ldx', [(16, 16), (25, 28), (32, 32)])
@pytest.mark.parametrize('S', [8, 12])
def test_bwd3_one_output_block(dev, graphs, S, fin, ldx, fout):
    run_bwd(dev, graphs['A'], 'bwd3', S, fin, fout, ldx=ldx)


@pytest.mark.parametrize('fout', [17, 32])
@pytest.mark.parametrize('fin,ldx', BWD3_WIDE)
@pytest.mark.parametrize('S', [4, 6])
def test_bwd3_wide_rows_in_one_launch(dev, graphs, S, fin, ldx, fout):
    run_bwd(dev, graphs['A'], 'bwd3', S, fin, fout, ldx=ldx)


@pytest.mark.parametrize('gname', ['H', 'C', 'D7', 'D129'])
@pytest.mark.parametrize('S,fin,ldx,fout', BWD3_DIAG)
def test_bwd3_graphs(dev, graphs, gname, S, fin, ldx, fout):
    if gname == 'C' and fin > 32:                            # the plan refuses C's windows for this class (see the fixture)
        run_bwd(dev, graphs['C'], 'bwd3', S, fin, fout, ldx=ldx, expect=UNS)
        run_bwd(dev, graphs['C'], '64', S, fin, fout, ldx=ldx)
        return
    run_bwd(dev, _pick(graphs, gname, 'bwd3', S), 'bwd3', S, fin, fout, ldx=ldx)


BWD3_COND_SHAPES = [(8, 32, 32, 'A'), (4, 25, 30, 'C'), (6, 17, 17, 'H'), (12, 32, 9, 'A'), (4, 44, 32, 'H')]


def _dvalacc_served(S, fin, fout):
    """gml.h, GML_DVAL_ACCUM: not S = 8 with two output blocks, not 33 .. 48 input features in one launch"""
    return not (S == 8 and fout > 16) and fin <= 32


@pytest.mark.parametrize('conds', NULLS + COMMON + [('dvalacc',), TOGETHER, TOGETHER4], ids=_ids)
@pytest.mark.parametrize('S,fin,fout,gname', BWD3_COND_SHAPES)
def test_bwd3_conditions(dev, graphs, conds, S, fin, fout, gname):
    if conds == ('dvalacc',):
        run_bwd(dev, _pick(graphs, gname, 'bwd3', S), 'bwd3', S, fin, fout, conds, expect=OK if _dvalacc_served(S, fin, fout) else UNS)
        return
    if len(conds) > 3 and _dvalacc_served(S, fin, fout):
        conds = conds + ('dvalacc',)
    run_bwd(dev, _pick(graphs, gname, 'bwd3', S), 'bwd3', S, fin, fout, conds, ldx=28 if fin == 25 and 'ldxpad' not in conds else None)


# ------------------------------------------------------------------------------------------------------------------------- bwd4
@pytest.mark.parametrize('fout', [17, 30, 32, 1, 9, 16])
@pytest.mark.parametrize('fin', [16, 20, 32])
@pytest.mark.parametrize('S', [4, 8])
def test_bwd4_shapes(dev, graphs, S, fin, fout):
    if S == 4 and fout <= 16:
        assert int(_lib.lib().gml_spectconv_bwd_group_rows(S, fin, fout, RING)) == 0
        run_bwd(dev, graphs['A'], 'bwd4', S, fin, fout, expect=UNS)                 # no 128-row kernel has this class
        return
    run_bwd(dev, graphs['A'], 'bwd4', S, fin, fout)
    assert ('bwd4', S, (fin + 15) // 16) in RAN


@pytest.mark.parametrize('gname', ['H', 'C', 'D7', 'D129'])
@pytest.mark.parametrize('S,fin,fout', [(8, 32, 32), (8, 16, 17), (4, 20, 30), (4, 16, 32), (8, 20, 9), (4, 32, 17)])
def test_bwd4_graphs(dev, graphs, gname, S, fin, fout):
    """H and C: a group beyond the ring's capacities sends the whole launch to bwd3 (fallback); the numbers are the same"""
    run_bwd(dev, graphs[gname], 'bwd4', S, fin, fout)


@pytest.mark.parametrize('conds', NULLS + COMMON + [('dvalacc',), TOGETHER, TOGETHER4], ids=_ids)
@pytest.mark.parametrize('S,fin,fout,gname', [(8, 32, 32, 'A'), (4, 20, 30, 'D129'), (8, 16, 9, 'A')])
def test_bwd4_conditions(dev, graphs, conds, S, fin, fout, gname):
    """accum, dvalacc and xoff fall back to bwd3; the NULL subsets, padded rows and an unaligned dx stay on the ring"""
    if conds == ('dvalacc',):
        run_bwd(dev, graphs[gname], 'bwd4', S, fin, fout, conds, expect=OK if _dvalacc_served(S, fin, fout) else UNS)
        return
    run_bwd(dev, graphs[gname], 'bwd4', S, fin, fout, conds)


# ------------------------------------------------------------------------------------------------------------------------- DZ
@pytest.mark.parametrize('relu', [0, 1, 17, -1, -2])
@pytest.mark.parametrize('nmix', [1, 2, 3, 4])
@pytest.mark.parametrize('fin', [20, 24, 28, 32])
def test_dz_mask_and_widths(dev, graphs, fin, nmix, relu):
    """gml_spectconv_bwd_mix_relu on bwd3: relu_cols in {0, 1, 17, Fin - 1, Fin}"""
    relu = {-1: fin - 1, -2: fin}.get(relu, relu)
    run_bwd(dev, graphs['A'], 'bwd3', 8, fin, (30, 32, 17, 25)[nmix - 1], mix={'na': nmix, 'nb': None, 'relu': relu})


@pytest.mark.parametrize('fam', ['bwd3', 'bwd4'])
@pytest.mark.parametrize('nmix', [1, 2, 3, 4])
@pytest.mark.parametrize('fin', [20, 24, 28, 32])
def test_dz_plain_entry(dev, graphs, fam, fin, nmix):
    """gml_spectconv_bwd_mix, on bwd3 and on the ring (which has no mask: relu_cols = 0 only)"""
    run_bwd(dev, graphs['A'], fam, 8, fin, 30, mix={'na': nmix, 'nb': None, 'relu': None})
    assert fam == 'bwd3' or ('bwd4', 8, 2) in RAN


@pytest.mark.parametrize('relu', [0, 17, -2])
@pytest.mark.parametrize('na,nb', [(2, 2), (4, 0), (1, 2), (0, 3)])
@pytest.mark.parametrize('fin', [20, 32])
def test_dz_two_weight_arrays(dev, graphs, fin, na, nb, relu):
    run_bwd(dev, graphs['A'], 'bwd3', 8, fin, 30, mix={'na': na, 'nb': nb, 'relu': fin if relu < 0 else relu})


@pytest.mark.parametrize('gname', ['H', 'C', 'D7', 'D129'])
@pytest.mark.parametrize('fam,fin,na,nb,relu,conds', [('bwd3', 32, 2, 2, 30, ()), ('bwd3', 20, 3, None, 19, ('nodval', 'lddx4')),
                                                      ('bwd4', 24, 2, 2, 0, ('nofold',)), ('bwd3', 28, 1, 2, 17, ('nodw', 'ldg8', 'ldxpad'))], ids=_ids)
def test_dz_graphs_and_conditions(dev, graphs, gname, fam, fin, na, nb, relu, conds):
    run_bwd(dev, graphs[gname], fam, 8, fin, 30, conds, mix={'na': na, 'nb': nb, 'relu': relu})


# ------------------------------------------------------------------------------------------------------------------------- HAD
@pytest.mark.parametrize('fold', [True, False], ids=['folded', 'partials'])
@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('fin,relu', [(20, 0), (20, 20), (32, 0), (32, 30), (32, 32)])
def test_had_with_dx(dev, graphs, fin, relu, bias, fold):
    run_bwd(dev, graphs['A'], 'bwd3', 8, fin, 30, had={'dx': True, 'relu': relu, 'bias': bias, 'fold': fold})


@pytest.mark.parametrize('fold', [True, False], ids=['folded', 'partials'])
@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('fin,ldx', [(17, 20), (25, 28), (30, 32)])
def test_had_without_dx(dev, graphs, fin, ldx, bias, fold):
    """the model's first layer: any input width in 17 .. 32 in float4-readable rows"""
    run_bwd(dev, graphs['A'], 'bwd3', 8, fin, 30, ldx=ldx, had={'dx': False, 'relu': 0, 'bias': bias, 'fold': fold})


@pytest.mark.parametrize('gname', ['H', 'C', 'D7', 'D129'])
@pytest.mark.parametrize('fin,ldx,dxw,relu,conds', [(32, 32, True, 30, ()), (25, 28, False, 0, ('nodval',)), (20, 20, True, 7, ('nofold', 'lddx4', 'ldg8'))],
                         ids=_ids)
def test_had_graphs_and_conditions(dev, graphs, gname, fin, ldx, dxw, relu, conds):
    run_bwd(dev, graphs[gname], 'bwd3', 8, fin, 30, conds, ldx=ldx, had={'dx': dxw, 'relu': relu, 'bias': True, 'fold': gname != 'C'})


# ------------------------------------------------------------------------------------------------------------------------- contracts
def test_graph_b_is_refused_by_the_128_row_plan_and_served_by_the_64_row_kernel(dev, graphs):
    B, L = graphs['B'], _lib.lib()
    served = 0
    for S, fin, fout in [(8, 32, 32), (4, 32, 32), (4, 20, 17), (8, 16, 30)]:
        for fam in ('bwd3', 'bwd4'):
            run_bwd(dev, B, fam, S, fin, fout, expect=UNS)
        if int(L.gml_spectconv_bwd_workspace_bytes(B.N, S, fin, fout, *B.rec(64)[2], F32)) > 0:
            run_bwd(dev, B, '64', S, fin, fout)
            served += 1
        else:
            run_bwd(dev, B, '64', S, fin, fout, expect=UNS)
    assert served >= 2                                       # (the fixture asserts S = 4, 32 x 32)


def test_contract_error_answers(dev, graphs):
    A, L = graphs['A'], _lib.lib()
    for fam in ('64', 'bwd3', 'bwd4'):
        run_bwd(dev, A, fam, 8, 32, 32, expect=BAD, over={'ldx': 28})
        run_bwd(dev, A, fam, 8, 32, 32, expect=BAD, over={'ldg': 28})
        run_bwd(dev, A, fam, 8, 32, 32, expect=BAD, over={'lddx': 31})
        run_bwd(dev, A, fam, 8, 32, 32, ('valoff',), expect=BAD)
        run_bwd(dev, A, fam, 8, 32, 32, ('dvaloff',), expect=BAD)
        run_bwd(dev, A, fam, 8, 32, 32, ('wsshort',), expect=WSP)
    for fam in ('bwd3', 'bwd4'):                             # the 8-wave kernel prefetches g as float4 whatever it does with it
        run_bwd(dev, A, fam, 8, 32, 32, ('goff',), expect=BAD)
        run_bwd(dev, A, fam, 8, 32, 30, ('ldgodd',), expect=BAD)
        run_bwd(dev, A, fam, 4, 32, 17, ('ldgodd',), expect=BAD)
    for S, fin, fout, fl in [(5, 32, 32, 0), (12, 32, 32, 0), (8, 48, 32, 0), (2, 32, 32, F32), (4, 65, 32, 0), (8, 32, 33, F32)]:
        assert int(L.gml_spectconv_bwd_group_rows(S, fin, fout, fl)) == 0
        assert int(L.gml_spectconv_bwd_workspace_bytes(A.N, S, fin, fout, *A.rec(128)[2], fl)) == 0
        run_bwd(dev, A, '64' if fl else 'bwd3', S, fin, fout, expect=UNS)
    dz = {'na': 2, 'nb': 2, 'relu': 0}
    run_bwd(dev, A, 'bwd3', 8, 32, 30, ('accum',), mix=dz, expect=UNS)
    run_bwd(dev, A, 'bwd3', 8, 32, 30, ('nodx',), mix=dz, expect=UNS)
    run_bwd(dev, A, 'bwd3', 8, 32, 30, mix={'na': 2, 'nb': 2, 'relu': 33}, expect=BAD)
    run_bwd(dev, A, 'bwd3', 8, 32, 30, mix={'na': 2, 'nb': None, 'relu': 33}, expect=BAD)
    run_bwd(dev, A, 'bwd4', 8, 32, 30, mix={'na': 2, 'nb': 2, 'relu': 1}, expect=UNS)
    run_bwd(dev, A, 'bwd4', 8, 32, 30, mix={'na': 4, 'nb': None, 'relu': 32}, expect=UNS)
    for S, fin, nmix in [(4, 32, 2), (8, 16, 2), (8, 30, 2), (8, 32, 5)]:        # outside gml_spectconv_bwd_mix_supported
        assert not L.gml_spectconv_bwd_mix_supported(S, fin, 30, nmix, 0)
        run_bwd(dev, A, 'bwd3', S, fin, 30, mix={'na': nmix, 'nb': None, 'relu': None}, expect=UNS)
    hd = {'dx': True, 'relu': 0, 'bias': True, 'fold': True}
    run_bwd(dev, A, 'bwd3', 8, 32, 30, ('accum',), had=hd, expect=UNS)
    run_bwd(dev, A, 'bwd3', 8, 32, 30, ('dvalacc',), had=hd, expect=UNS)
    run_bwd(dev, A, 'bwd4', 8, 32, 30, had=hd, expect=UNS)
    run_bwd(dev, A, 'bwd3', 8, 32, 30, ('nodw',), had=hd, expect=UNS)
    run_bwd(dev, A, 'bwd3', 8, 32, 30, had=dict(hd, relu=33), expect=BAD)
    run_bwd(dev, A, 'bwd3', 8, 30, 30, ldx=32, had=dict(hd, dx=False, relu=4), expect=BAD)          # a mask without dx


@pytest.mark.parametrize('fam', ['64', 'bwd3', 'bwd4'])
def test_contract_no_rows_zeroes_dw(dev, graphs, fam):
    """num_rows = 0: GML_OK, dw = 0 (an optimizer step over an empty batch adds nothing), dx and dval not touched"""
    from gnn_matlang_amd.graph import _stream
    A, L = graphs['A'], _lib.lib()
    S, fin, fout = 8, 32, 32
    gi, _, (me, mw) = A.rec(64 if fam == '64' else 128)
    fl = F32 if fam == '64' else RING if fam == 'bwd4' else 0
    val, x, ga, w = (_up(np.ones(s, np.float32), dev) for s in ((A.E, S), (N, fin), (N, fout), (S, fin, fout)))
    dx, dval, dw, ws = _Out(dev, N, fin, fin), _Out(dev, A.E, S, S), _Out(dev, S * fin, fout, fout), _flat(dev, 3 * S * fin * fout)
    rc = _done(L.gml_spectconv_bwd(_p(A.csr.rowptr_t), _p(A.csr.col_t), _p(gi), _p(val), _p(x), fin, _p(ga), fout, _p(w), dx.ptr(), fin,
                                   dval.ptr(), dw.ptr(), 0, S, fin, fout, me, mw, fl, ws.ptr(), 3 * S * fin * fout * 4, _stream(dev)))
    assert rc == OK and dx.unchanged() and dval.unchanged() and ws.unchanged()
    zero = np.zeros((S * fin, fout))
    R.check(dw.get(), zero, zero + 1.0, S * fin, fout, fout, TOL, 'num_rows = 0: dw')
    assert not dw.get()[:S * fin * fout].any()


# ------------------------------------------------------------------------------------------------------------------------- repeatability
@pytest.mark.parametrize('fam,S,fin,fout,gname,kw', [
    ('64', 8, 32, 32, 'H', {}), ('bwd3', 8, 32, 32, 'H', {}), ('bwd3', 6, 44, 32, 'H', {}), ('bwd4', 8, 32, 32, 'A', {}),
    ('bwd3', 8, 32, 30, 'A', {'mix': {'na': 2, 'nb': 2, 'relu': 30}}), ('bwd3', 8, 32, 30, 'H', {'had': {'dx': True, 'relu': 30, 'bias': True, 'fold': True}})],
    ids=lambda v: str(v) if not isinstance(v, dict) else '+'.join(sorted(v)) or 'plain')
def test_two_launches_are_bitwise_equal(dev, graphs, fam, S, fin, fout, gname, kw):
    """no atomics, a fixed fold order (gml.h: "bitwise deterministic"): fresh buffers, the same bits"""
    a = run_bwd(dev, graphs[gname], fam, S, fin, fout, **kw)
    b = run_bwd(dev, graphs[gname], fam, S, fin, fout, **kw)
    assert sorted(a) == sorted(b) and len(a) >= 3
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), (fam, k)


# ------------------------------------------------------------------------------------------------------------------------- report
def test_worst_figures_and_coverage_report():
    """prints what the matrix measured (pytest -rP): per kernel family, arithmetic and output, the worst max-norm figure and the worst
    |got - ref| / term sum (each already asserted <= 1e-4 by its own case), the refused cases per (family, graph), and asserts the
    coverage: every (family, graph role) pair ran, every compiled instantiation ran"""
    assert WORST, 'no case ran'
    print('%-14s %-5s %-5s %6s %12s %12s' % ('family', 'arith', 'out', 'cases', 'max-norm', 'term-sum'))
    for (fam, arith, out), (n, e_max, e_ts) in sorted(WORST.items()):
        print('%-14s %-5s %-5s %6d %12.2e %12.2e' % (fam, arith, out, n, e_max, e_ts))
        assert e_max <= TOL and e_ts <= TOL
    print('%-14s %-6s %6s %8s' % ('family', 'graph', 'ran', 'refused'))
    for (fam, gname), (ran, refused) in sorted(ROLES.items()):
        print('%-14s %-6s %6d %8d' % (fam, gname, ran, refused))
    for fam in ('64', 'bwd3', 'bwd4', 'bwd3 DZ', 'bwd3 HAD'):
        for gname in ('A', 'H', 'C', 'D7', 'D129'):
            assert ROLES.get((fam, gname), [0, 0])[0] > 0, 'no case of %s ran on graph %s' % (fam, gname)
    assert ROLES[('bwd3', 'B')][1] > 0 and ROLES[('bwd4', 'B')][1] > 0 and ROLES[('64', 'B')][0] > 0
    assert ROLES.get(('bwd4 DZ', 'A'), [0, 0])[0] > 0
    missing = [('bwd',) + s for s in BWD_SHAPES if ('bwd',) + s not in RAN] + [('bwd3',) + s for s in BWD3_SHAPES if ('bwd3',) + s not in RAN] + \
              [('bwd4',) + s for s in BWD4_SHAPES if ('bwd4',) + s not in RAN]
    assert not missing, 'compiled instantiations no case reached: %s' % missing
    for k in ('64', 'bwd3', 'bwd4', 'bwd4>bwd3', 'bwd3 DZ', 'bwd4 DZ', 'bwd3 HAD'):
        assert any(f == k for f, _, _ in WORST), 'no case was labelled %s' % k
