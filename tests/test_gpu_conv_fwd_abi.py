"""The conv forward at the level of its C ABI (include/gml.h): every kernel family and launch mode against the float64 restatement
of tests/_conv_ref.py -- one launch and one numpy reference per case, through _lib.lib() directly so that each case sets its own
arithmetic flag and everything functional.py never passes: accumulate and relu, ldo > Fout, outputs that are not 16-byte aligned,
transposed weight strides, no bias, a position map on a plain conv, Hadamard widths other than 2, GML_FWD_ONEWIN where no batch
needs it, and the error answers callers fall back on.

Which kernel a case reaches is read off the dispatch (csrc/gml_spectconv.hip, plan_fwd / fwd_kernel): 64-row records and no
GML_GROUPS128 -> the 64-row family for ANY shape; GML_GROUPS128 with S in {4, 8}, float4-addressable x rows, no GML_ACCUM -> fwd3;
S = 12, or S in {4, 8} with unaligned x rows or GML_ACCUM -> fwd2; the chunked-only shapes, or GML_FWD_CHUNKED -> fwd4.  The graphs'
roles (fits every staging / beyond it / window beyond it) are asserted against the library's own stage queries in the fixture.

Every output sits in a buffer of _conv_ref.alloc(): columns Fout .. ldo - 1, 8 rows after row N - 1 and 4 floats in front of an
offset output hold a NaN sentinel and must still hold it afterwards.  Values are held to tol = 1e-4 on the max-norm (conftest.rel_err)
AND elementwise on each element's own term sum; GML_F32_MFMA cases with S Fin <= 256 also to the 2e-6 max-norm that
test_exact_fp32_mode_is_closer_to_the_oracle applies at that size.  The worst figures per family and arithmetic are printed by the
last test (pytest -rP) and recorded in DESIGN.md s4.1d."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import _conv_ref as R
from gnn_matlang_amd import _lib

pytestmark = pytest.mark.gpu

TOL = 1e-4
TOL_F32 = 2e-6
N = 300
G128, CHK, ONEWIN = _lib.GML_GROUPS128, _lib.GML_FWD_CHUNKED, _lib.GML_FWD_ONEWIN
ARITH128 = {'bf16': 0, 'f16': _lib.GML_F16X3}              # the 128-row kernels: bf16 pairs / f16 pieces
ARITH64 = {'bf16': 0, 'f32': _lib.GML_F32_MFMA}             # the 64-row family: bf16 pairs (exact products up to 16 features) / f32 MFMA
WORST = {}                                                  # (family, arithmetic) -> [cases, worst max-norm, worst term-sum figure]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    assert _lib.lib().gml_version() >= 1
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------------------------------- graphs
def _band(rng, n, half, deg):
    """each row takes `deg` distinct sources within +-half of itself; [2, E] (source, target), sorted by source"""
    src, dst = [], []
    for r in range(n):
        lo, hi = max(r - half, 0), min(r + half, n - 1)
        src.append(rng.choice(np.arange(lo, hi + 1), size=min(deg, hi - lo + 1), replace=False))
        dst.append(np.full(src[-1].size, r))
    return _sorted(np.concatenate(src), np.concatenate(dst))


def _sorted(src, dst):
    o = np.lexsort((dst, src))
    return np.stack([src[o], dst[o]]).astype(np.int64)


class _Graph(object):
    def __init__(self, dev, name, ei, n):
        from gnn_matlang_amd.graph import GraphCSR
        self.name, self.N, self.E, self.ei = name, n, ei.shape[1], ei
        self.csr = GraphCSR.from_edge_index(torch.from_numpy(ei).to(dev), n)
        rowptr, perm = R.csr_order(ei, n)
        self.eis = ei[:, perm]                              # the edges in the order the kernels read them
        assert np.array_equal(self.csr.rowptr.cpu().numpy(), rowptr) and np.array_equal(self.csr.col.cpu().numpy(), self.eis[0])
        self.g128, self.g64 = self.csr.ginfo128.cpu().numpy(), self.csr.ginfo.cpu().numpy()
        self.e128, self.w128 = int(self.g128[:, 1].max()), int(self.g128[:, 3].max())
        self.e64, self.w64 = int(self.g64[:, 1].max()), int(self.g64[:, 3].max())


@pytest.fixture(scope='module')
def graphs(dev):
    L = _lib.lib()
    rng = np.random.default_rng(20240)
    a = _band(rng, N, 6, 5)
    a = a[:, a[1] != 77]                                    # one empty row
    far_d = np.array([3, 17, 31, 44, 59, 262, 271, 280, 291, 299])
    far_s = np.array([255, 290, 270, 299, 251, 40, 2, 33, 18, 49])
    eis = {'A': (a, N), 'B': (_band(rng, N, 25, 40), N),
           'C': (_sorted(np.concatenate([a[0], far_s]), np.concatenate([a[1], far_d])), N),
           'D7': (_band(rng, 7, 3, 2), 7), 'D129': (_band(rng, 129, 6, 5), 129), 'E': (_band(rng, N, 8, 10), N),
           'F': (_band(rng, N, 6, 3), N)}
    g = {k: _Graph(dev, k, ei, n) for k, (ei, n) in eis.items()}
    caps = [int(L.gml_spectconv_fwd_stage_edges(S, fin, 32, 0)) for S, fin in ((4, 32), (8, 32), (6, 32))]
    caps48 = [int(L.gml_spectconv_fwd_stage_edges(S, fin, 32, 0)) for S, fin in ((6, 48), (4, 48), (4, 33))]
    wins = [int(L.gml_spectconv_fwd_stage_window(S, fin, 32, CHK)) for S, fin in ((8, 32), (6, 48))]
    assert min(caps) > 0 and min(caps48) > 0 and min(wins) > 0
    A, B, C, E = g['A'], g['B'], g['C'], g['E']
    # F: light enough for one work item of the chunked kernel at 33 .. 48 features too (two X windows: half the edges; A needs
    # two chunks there without GML_FWD_ONEWIN and one with it)
    assert g['F'].e128 <= min(caps48) < A.e128 and g['F'].w128 <= min(wins), (g['F'].e128, caps48, A.e128)
    assert (A.eis[1] == 0).any() and (A.eis[1] == N - 1).any() and not (A.eis[1] == 77).any()
    assert [int(v) for v in np.diff(np.append(np.arange(0, N, 128), N))] == [128, 128, 44]
    # A: every group inside every kernel's staging (64-row family: 512 edges, 144 window rows, DESIGN s4.1b)
    assert A.e128 <= min(caps) and A.w128 <= min(wins) and A.e64 <= 512 and A.w64 <= 144, (A.e128, A.w128, A.e64, A.w64)
    # B: beyond every edge capacity (fwd2: 1,024; S = 6 of the 64-row family: 1,024), inside the chunked kernel's window
    assert B.g128[:, 1].min() > 1024 and B.g64[:, 1].min() > 1024 and B.w128 <= min(wins), (B.g128[:, 1], B.g64[:, 1], B.w128)
    # C: windows beyond 200 rows in both group sizes, beside groups that stay staged
    assert C.w128 > 200 and C.w64 > 200 and C.g128[:, 3].min() <= min(wins) and C.g64[:, 3].min() <= 144, (C.g128[:, 3], C.g64[:, 3])
    # E: fwd2's S = 12 staging (1,536 edges) beyond the 1,024 of its S in {4, 8} form
    assert 1024 < E.g128[:2, 1].min() and E.e128 <= 1536, E.g128[:, 1]
    assert g['D7'].g128.shape[0] == 1 and g['D129'].g128.shape[0] == 2
    return g


# ------------------------------------------------------------------------------------------------------------------------- one launch
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _up(a, dev, lead=0):
    """array -> device, behind `lead` extra floats (an address 4 * lead bytes past the allocation's alignment)"""
    a = np.ascontiguousarray(a)
    if lead:
        a = np.concatenate([np.zeros(lead, a.dtype), a.ravel()])
    return torch.from_numpy(a).to(dev)


def _p(t, lead=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * lead) if t is not None else ctypes.c_void_p(0)


def _done(rc):
    """wait for the launch; a HIP error (return code > 0, or a failed synchronize) ends the session: nothing more runs on a device
    that has faulted"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit('device error after a launch: %s' % e, returncode=3)
    if rc > 0:
        pytest.exit('HIP error %d from a launch' % rc, returncode=3)
    return rc


def _note(fam, arith, e_max, e_ts):
    w = WORST.setdefault((fam, arith), [0, 0.0, 0.0])
    w[0] += 1
    w[1], w[2] = max(w[1], e_max), max(w[2], e_ts)


class _Out(object):
    """an output buffer of _conv_ref.alloc() on the device; `off4`: the output starts 4 bytes past a 16-byte boundary, behind its
    4 guard floats"""

    def __init__(self, dev, n, ncols, ldo, off4=False, out0=None, guard_rows=R.GUARD_ROWS):
        self.n, self.ncols, self.ldo, self.lead, self.guard_rows = n, ncols, ldo, 1 if off4 else 0, guard_rows
        self.host, self.off = R.alloc(n, ncols, ldo, off4, out0, guard_rows)
        self.t = _up(self.host, dev, self.lead)
        assert (self.t.data_ptr() + 4 * (self.lead + self.off)) % 16 == (4 if off4 else 0)

    def ptr(self):
        return _p(self.t, self.lead + self.off)

    def get(self):
        b = self.t.cpu().numpy()
        assert self.lead == 0 or b[0] == 0.0
        return b[self.lead:]

    def unchanged(self):
        return np.array_equal(self.get().view(np.int32), self.host.view(np.int32))


def _inputs(g, S, fin, fout, key, conds, ldx, F2):
    """host-side operands of one case: values in CSR order, x with junk (finite) padding columns, W scaled by Fin ** -0.5"""
    rng = _rng(key)
    c = {'val': _f32(rng.standard_normal((g.E, S))), 'x': _f32(rng.standard_normal((g.N, ldx))),
         'w': _f32(rng.standard_normal((S, fin, fout)) * fin ** -0.5),
         'bias': None if 'nobias' in conds else _f32(rng.random(fout) - 0.5),
         'out0': _f32(rng.standard_normal((g.N, fout + F2))) if 'accum' in conds else None, 'epos': None}
    if 'epos' in conds:
        c['epos'] = rng.permutation(g.E).astype(np.int32)
    if F2:
        c['w11'], c['w12'] = (_f32(rng.standard_normal((F2, fin)) * fin ** -0.5) for _ in range(2))
        c['b11'], c['b12'] = (_f32(rng.random(F2) - 0.5) for _ in range(2))
    return c


def run_conv(dev, g, fam, arith, aflag, S, fin, fout, conds=(), flags=0, ldx=None, F2=0):
    """One gml_spectconv_fwd (F2 = 0) / gml_ml3_fwd launch and its check.  `fam`: the kernel family the dispatch source sends the case
    to (a label for the report; '64' passes 64-row records, the others 128-row records and GML_GROUPS128).  conds:
      relu, accum (out pre-filled with out0), nobias, ldo3 (ldo = columns + 3: scalar stores), wide (ldo = columns + 4, aligned: the
      float4 stores of fwd3 / fwd4 where the columns are a multiple of 4), off4 (output 4 bytes past a 16-byte boundary), wT (weights stored [S, Fout, Fin]: w_si = 1),
      epos (values through a random position map), xoff (x 4 bytes past a 16-byte boundary)."""
    from gnn_matlang_amd.graph import _stream
    conds = tuple(conds)
    ldx = fin if ldx is None else ldx
    ncols = fout + F2
    c = _inputs(g, S, fin, fout, (fam, arith, S, fin, fout, conds, flags, ldx, F2, g.N, g.E), conds, ldx, F2)
    ldo = ncols + (3 if 'ldo3' in conds else 4 if 'wide' in conds else 0)
    out = _Out(dev, g.N, ncols, ldo, 'off4' in conds, c['out0'])
    val = c['val']
    if c['epos'] is not None:                                # the kernel reads val[epos[k]] for CSR position k
        val = np.empty_like(c['val'])
        val[c['epos']] = c['val']
    if 'wT' in conds:
        wd, ws = _up(c['w'].transpose(0, 2, 1), dev), (fin * fout, 1, fin)
    else:
        wd, ws = _up(c['w'], dev), (fin * fout, fout, 1)
    xl = 1 if 'xoff' in conds else 0
    xd, vd = _up(c['x'], dev, xl), _up(val, dev)
    bd = _up(c['bias'], dev) if c['bias'] is not None else None
    ed = _up(c['epos'], dev) if c['epos'] is not None else None
    gi = g.csr.ginfo if fam == '64' else g.csr.ginfo128
    fl = aflag | flags | (0 if fam == '64' else G128) | (_lib.GML_RELU if 'relu' in conds else 0) | (_lib.GML_ACCUM if 'accum' in conds else 0)
    L = _lib.lib()
    head = (_p(g.csr.rowptr), _p(g.csr.col), _p(gi), _p(ed), _p(vd), _p(xd, xl), ldx, _p(wd), ws[0], ws[1], ws[2], _p(bd))
    if F2:
        mix = [_up(c[k], dev) for k in ('w11', 'b11', 'w12', 'b12')]
        rc = L.gml_ml3_fwd(*head, _p(mix[0]), _p(mix[1]), _p(mix[2]), _p(mix[3]), out.ptr(), ldo, g.N, S, fin, fout, F2, fl, _stream(dev))
    else:
        rc = L.gml_spectconv_fwd(*head, out.ptr(), ldo, g.N, S, fin, fout, fl, _stream(dev))
    rc = _done(rc)
    what = '%s/%s graph %s S=%d Fin=%d(ld %d) Fout=%d F2=%d %s flags=%#x' % (fam, arith, g.name, S, fin, ldx, fout, F2,
                                                                               '+'.join(conds) or 'plain', fl)
    assert rc == _lib.GML_OK, '%s: return code %d' % (what, rc)
    x = c['x'][:, :fin]
    ref, ts = R.conv_ref(g.eis, c['val'], x, c['w'], c['bias'], 'relu' in conds, None if c['out0'] is None else c['out0'][:, :fout])
    if F2:
        m, mt = R.mix_ref(x, c['w11'], c['b11'], c['w12'], c['b12'])
        ref, ts = np.concatenate([ref, m], 1), np.concatenate([ts, mt], 1)
    e_max, e_ts = R.check(out.get(), ref, ts, g.N, ncols, ldo, TOL, what)
    print('%-110s max-norm %.2e  term-sum %.2e' % (what, e_max, e_ts))
    if (aflag & _lib.GML_F32_MFMA) and S * fin <= 256:
        assert e_max <= TOL_F32, '%s: exact-fp32 mode at %.3e > %.1e' % (what, e_max, TOL_F32)
    _note(fam, arith, e_max, e_ts)
    return e_max, e_ts


# ------------------------------------------------------------------------------------------------------------------------- 64-row family
CONDS64 = ('relu', 'accum', 'nobias', 'ldo3', 'off4', 'wT', 'epos')
# (S, Fin, Fout, graph, ldx).  The family picks 4 features per lane up to Fin = 16 (and up to 48 in the f32 mode), else 8, and
# the largest compiled support count SC dividing S (SC >= 4 or SC = S) -- so Fin = 12 / 20 with these S reach every compiled pair
FAM64_PAIRS = [(S, 20, 30, 'A', 20) for S in (1, 2, 3, 4, 6, 8)] + [(S, 12, 30, 'A', 12) for S in (1, 2, 3, 4, 6, 8, 12, 16)]
FAM64_SHAPES = [
    (5, 20, 30, 'A', 24), (7, 3, 5, 'B', 3), (9, 40, 50, 'A', 40), (11, 20, 100, 'C', 20),          # greedy splits: 4+1, 6+1, 8+1, 8+3
    (12, 20, 30, 'B', 20), (16, 40, 130, 'A', 40), (24, 70, 30, 'A', 70),                           # several passes of one SC
    (3, 3, 5, 'A', 3), (4, 40, 50, 'B', 44), (2, 70, 100, 'A', 70), (8, 20, 130, 'C', 20),          # Fin 3 / 20 / 40 / 70 x Fout 5 .. 130
    (6, 40, 30, 'C', 40), (8, 70, 5, 'B', 71), (4, 32, 32, 'C', 32), (8, 32, 30, 'B', 32), (6, 48, 32, 'A', 48)]
# the conditions, one at a time and all together, on: a greedy split, passes on the heavy graph, two column groups with a wide
# window, rows that are not float4-addressable
FAM64_COND_SHAPES = [(5, 20, 30, 'A', 20), (12, 20, 50, 'B', 20), (8, 40, 130, 'C', 40), (3, 3, 5, 'A', 3)]


@pytest.mark.parametrize('arith', sorted(ARITH64))
@pytest.mark.parametrize('S,fin,fout,gname,ldx', FAM64_PAIRS + FAM64_SHAPES)
def test_family64_shapes(dev, graphs, arith, S, fin, fout, gname, ldx):
    run_conv(dev, graphs[gname], '64', arith, ARITH64[arith], S, fin, fout, ldx=ldx)


@pytest.mark.parametrize('arith', sorted(ARITH64))
@pytest.mark.parametrize('conds', [(c,) for c in CONDS64] + [CONDS64], ids=lambda c: '+'.join(c))
@pytest.mark.parametrize('S,fin,fout,gname,ldx', FAM64_COND_SHAPES)
def test_family64_conditions(dev, graphs, arith, conds, S, fin, fout, gname, ldx):
    run_conv(dev, graphs[gname], '64', arith, ARITH64[arith], S, fin, fout, conds, ldx=ldx)


# ------------------------------------------------------------------------------------------------------------------------- fwd3
FWD3_FIN = [(4, 4), (25, 28), (32, 32)]                     # (Fin, ldx): 25 features in float4-addressable rows of 28
FWD3_FOUT = [9, 16, 17, 30, 32]
FWD3_DIAG = [(8, 4, 4, 9), (4, 25, 28, 16), (8, 32, 32, 17), (4, 4, 4, 30), (8, 25, 28, 32), (4, 32, 32, 9)]
CONDS3 = ('relu', 'nobias', 'epos', 'ldo3', 'off4', 'wT')


@pytest.mark.parametrize('arith', sorted(ARITH128))
@pytest.mark.parametrize('fout', FWD3_FOUT)
@pytest.mark.parametrize('fin,ldx', FWD3_FIN)
@pytest.mark.parametrize('S', [4, 8])
def test_fwd3_shapes(dev, graphs, arith, S, fin, ldx, fout):
    run_conv(dev, graphs['A'], 'fwd3', arith, ARITH128[arith], S, fin, fout, ldx=ldx)


@pytest.mark.parametrize('arith', sorted(ARITH128))
@pytest.mark.parametrize('S,fin,ldx,fout', FWD3_DIAG)
@pytest.mark.parametrize('gname', ['B', 'C', 'D7', 'D129'])
def test_fwd3_graphs(dev, graphs, arith, gname, S, fin, ldx, fout):
    """B: every group beyond the staged edges, C: windows beyond the staged rows (both: the global-gather road), D: partial groups"""
    run_conv(dev, graphs[gname], 'fwd3', arith, ARITH128[arith], S, fin, fout, ldx=ldx)


@pytest.mark.parametrize('arith', sorted(ARITH128))
@pytest.mark.parametrize('conds', [(c,) for c in CONDS3] + [('wide',), ('wide', 'relu', 'epos', 'wT'), CONDS3], ids=lambda c: '+'.join(c))
@pytest.mark.parametrize('S,fin,ldx,fout,gname', [(8, 32, 32, 32, 'A'), (4, 25, 28, 16, 'C'), (8, 4, 4, 28, 'B')])
def test_fwd3_conditions(dev, graphs, arith, conds, S, fin, ldx, fout, gname):
    run_conv(dev, graphs[gname], 'fwd3', arith, ARITH128[arith], S, fin, fout, conds, ldx=ldx)


# (S, Fin, ldx, nout1, F2): 30 + 2 and 24 + 8 complete float4 rows (the merged wide stores), the others take the scalar stores
ML3_SHAPES = [(8, 32, 32, 30, 2), (8, 32, 32, 24, 8), (4, 25, 28, 9, 1), (4, 32, 32, 16, 8), (8, 4, 4, 31, 1), (4, 32, 32, 17, 2)]


@pytest.mark.parametrize('arith', sorted(ARITH128))
@pytest.mark.parametrize('conds', [(), ('epos',), ('wide', 'relu'), ('ldo3', 'epos', 'relu')], ids=lambda c: '+'.join(c) or 'plain')
@pytest.mark.parametrize('S,fin,ldx,nout1,F2', ML3_SHAPES)
def test_fwd3_hadamard_branch(dev, graphs, arith, conds, S, fin, ldx, nout1, F2):
    """gml_ml3_fwd on the ring kernel: F2 in {1, 2, 8}, with and without the position map; ldo = columns + 4 keeps the merged wide
    stores for the 32- and 24-column rows and the scalar ones for 10 and 19 columns"""
    run_conv(dev, graphs['C' if 'epos' in conds else 'A'], 'fwd3', arith, ARITH128[arith], S, fin, nout1, conds, ldx=ldx, F2=F2)


def _epi_ref(g, c, S, fin, fout, epilogue, self_term):
    """float64 of gml.h's two epilogues.  1: support s -> column block s + self_term (+ that block's bias; block 0 of a self-term
    layer is the caller's); 2: out = (sum_s ds_s . H_s + ds_self . x) W + bias"""
    x = c['x'][:, :fin].astype(np.float64)
    H, Ht = R.spmm_ref(g.eis, c['val'], x)
    if epilogue == 1:
        nb = S + self_term
        ref, ts = np.zeros((g.N, nb * fout)), np.zeros((g.N, nb * fout))
        for s in range(S):
            sl = slice((s + self_term) * fout, (s + self_term + 1) * fout)
            ref[:, sl] = H[:, s, :] @ c['w'][s].astype(np.float64) + c['bias'][sl]
            ts[:, sl] = Ht[:, s, :] @ np.abs(c['w'][s]).astype(np.float64) + np.abs(c['bias'][sl])
        return ref, ts
    ds = c['ds'].astype(np.float64)
    a = np.einsum('nsf,sf->nf', H, ds[:S]) + (ds[S] * x if self_term else 0)
    at = np.einsum('nsf,sf->nf', Ht, np.abs(ds[:S])) + (np.abs(ds[S]) * np.abs(x) if self_term else 0)
    w = c['w'][0].astype(np.float64)
    return a @ w + c['bias'][:fout], at @ np.abs(w) + np.abs(c['bias'][:fout])


@pytest.mark.parametrize('extra', [3, 4])
@pytest.mark.parametrize('epilogue,self_term', [(1, 0), (1, 1), (2, 0), (2, 1)])
@pytest.mark.parametrize('S,fin,ldx,fout,gname', [(8, 32, 32, 16, 'A'), (4, 25, 28, 30, 'B'), (4, 4, 4, 9, 'D129')])
def test_fwd3_epilogues_keep_to_their_columns(dev, graphs, S, fin, ldx, fout, gname, epilogue, self_term, extra):
    """gml_spectconv_fwd_epi with ldo beyond the written columns (test_ring_kernel_epilogues_vs_oracle keeps the numerics of the
    modules; here: the guards, and block 0 of a self-term ConCat call, which the kernel must leave to the caller)"""
    from gnn_matlang_amd.graph import _stream
    g = graphs[gname]
    nb = S + self_term
    ncols = nb * fout if epilogue == 1 else fout
    c = _inputs(g, S, fin, fout, ('epi', S, fin, fout, gname, epilogue, self_term, extra), (), ldx, 0)
    rng = _rng('epi-extra', S, fin, fout, epilogue, self_term)
    c['bias'] = _f32(rng.random(ncols) - 0.5)
    c['ds'] = _f32(rng.standard_normal((nb, fin)) * 0.5)
    ldo = ncols + extra
    out = _Out(dev, g.N, ncols, ldo)
    wd = _up(c['w'] if epilogue == 1 else c['w'][0], dev)
    xd, vd, bd, dsd = _up(c['x'], dev), _up(c['val'], dev), _up(c['bias'], dev), _up(c['ds'], dev)
    rc = _lib.lib().gml_spectconv_fwd_epi(_p(g.csr.rowptr), _p(g.csr.col), _p(g.csr.ginfo128), _p(vd), _p(xd), ldx, _p(wd), fin * fout, fout, 1,
                                          _p(bd), out.ptr(), ldo, g.N, S, fin, fout, 0, epilogue, _p(dsd) if epilogue == 2 else _p(None),
                                          self_term, _stream(dev))
    rc = _done(rc)
    what = 'epilogue %d self %d S=%d Fin=%d Fout=%d ldo=%d graph %s' % (epilogue, self_term, S, fin, fout, ldo, gname)
    assert rc == _lib.GML_OK, (what, rc)
    ref, ts = _epi_ref(g, c, S, fin, fout, epilogue, self_term)
    buf = out.get().copy()
    if epilogue == 1 and self_term:                          # block 0 is the caller's GEMM: untouched, then zero for the value check
        blk = buf[out.off:].reshape(g.N + R.GUARD_ROWS, ldo)[:g.N, :fout]
        assert (blk.view(np.int32) == R.SENTINEL).all(), what + ': block 0 of a self-term ConCat call was written'
        blk[:] = 0
        ts[:, :fout] = 1
    e_max, e_ts = R.check(buf, ref, ts, g.N, ncols, ldo, TOL, what)
    print('%-110s max-norm %.2e  term-sum %.2e' % (what, e_max, e_ts))
    _note('fwd3 epilogues', 'bf16', e_max, e_ts)


# ------------------------------------------------------------------------------------------------------------------------- fwd2
CONDS2 = CONDS3
# (S, Fin, ldx, Fout, conds that select fwd2): S = 12 always; S in {4, 8} by rows of 25 floats, by an x 4 bytes off, by GML_ACCUM
FWD2_SHAPES = [(12, 32, 32, 32, ()), (12, 25, 25, 17, ()), (12, 4, 4, 9, ()), (12, 20, 20, 30, ('accum',)), (12, 32, 32, 16, ('xoff',)),
               (8, 25, 25, 30, ()), (4, 25, 25, 9, ()), (8, 32, 32, 32, ('accum',)), (4, 32, 32, 17, ('accum',)), (8, 4, 4, 16, ('accum',)),
               (4, 32, 32, 30, ('xoff',)), (8, 20, 21, 9, ())]


@pytest.mark.parametrize('arith', sorted(ARITH128))
@pytest.mark.parametrize('gname', ['A', 'B', 'C'])
@pytest.mark.parametrize('S,fin,ldx,fout,sel', FWD2_SHAPES, ids=lambda v: ('+'.join(v) or 'plain') if isinstance(v, tuple) else str(v))
def test_fwd2_shapes(dev, graphs, arith, gname, S, fin, ldx, fout, sel):
    run_conv(dev, graphs[gname], 'fwd2', arith, ARITH128[arith], S, fin, fout, sel, ldx=ldx)


@pytest.mark.parametrize('arith', sorted(ARITH128))
@pytest.mark.parametrize('conds', [(c,) for c in CONDS2] + [('wide',), CONDS2, CONDS2 + ('accum',)], ids=lambda c: '+'.join(c))
@pytest.mark.parametrize('S,fin,ldx,fout,gname', [(12, 32, 32, 32, 'A'), (8, 25, 25, 16, 'C'), (4, 25, 25, 28, 'B'), (12, 20, 20, 12, 'E')])
def test_fwd2_conditions(dev, graphs, arith, conds, S, fin, ldx, fout, gname):
    run_conv(dev, graphs[gname], 'fwd2', arith, ARITH128[arith], S, fin, fout, conds, ldx=ldx)


@pytest.mark.parametrize('arith', sorted(ARITH128))
@pytest.mark.parametrize('fin,ldx,fout', [(32, 32, 32), (32, 32, 9), (25, 25, 17), (4, 4, 30)])
def test_fwd2_twelve_supports_between_the_two_edge_capacities(dev, graphs, arith, fin, ldx, fout):
    """S = 12 stages up to 1,536 edges per group (graph E: 1,280), the S in {4, 8} form 1,024"""
    run_conv(dev, graphs['E'], 'fwd2', arith, ARITH128[arith], 12, fin, fout, ldx=ldx)


@pytest.mark.parametrize('arith', sorted(ARITH128))
@pytest.mark.parametrize('conds', [(), ('epos', 'relu')], ids=lambda c: '+'.join(c) or 'plain')
@pytest.mark.parametrize('S,fin,ldx,nout1,F2', [(12, 32, 32, 30, 2), (12, 32, 32, 24, 8), (12, 20, 20, 15, 1), (12, 25, 25, 30, 2),
                                                (8, 25, 25, 24, 8), (4, 25, 25, 9, 1), (12, 30, 30, 16, 8)])
def test_fwd2_hadamard_branch(dev, graphs, arith, conds, S, fin, ldx, nout1, F2):
    """gml_ml3_fwd on the register-staged kernel: F2 in {1, 2, 8}, float4-addressable x rows (ldx 32, 20) and not (25, 30)"""
    run_conv(dev, graphs['B' if conds else 'A'], 'fwd2', arith, ARITH128[arith], S, fin, nout1, conds, ldx=ldx, F2=F2)


# ------------------------------------------------------------------------------------------------------------------------- fwd4
FWD4_ONLY = [(6, 20), (6, 48), (4, 40), (4, 48)]            # no other 128-row kernel
FWD4_ASKED = [(8, 32), (4, 32)]                             # fwd3's shapes under GML_FWD_CHUNKED
CONDS4 = ('epos', 'relu', 'nobias', 'ldo3', 'off4')


@pytest.mark.parametrize('arith', sorted(ARITH128))
@pytest.mark.parametrize('gname', ['A', 'B'])
@pytest.mark.parametrize('fout', [9, 24, 32])
@pytest.mark.parametrize('S,fin', FWD4_ONLY + FWD4_ASKED)
def test_fwd4_shapes(dev, graphs, arith, S, fin, fout, gname):
    """A: one chunk per group; B: 5,000-edge groups walked in chunks"""
    run_conv(dev, graphs[gname], 'fwd4', arith, ARITH128[arith], S, fin, fout, flags=CHK if (S, fin) in FWD4_ASKED else 0)


@pytest.mark.parametrize('arith', sorted(ARITH128))
@pytest.mark.parametrize('gname', ['F', 'A', 'B'])
@pytest.mark.parametrize('onewin', [0, ONEWIN])
@pytest.mark.parametrize('S,fin,fout', [(6, 48, 32), (4, 40, 24), (4, 48, 9), (6, 36, 17)])
def test_fwd4_wide_rows_one_and_two_windows(dev, graphs, arith, S, fin, fout, onewin, gname):
    """Fin > 32 with and without GML_FWD_ONEWIN: on a batch that needs no chunks in either form (F), one that needs them with two
    X windows only (A) and one that needs them in both (B)"""
    run_conv(dev, graphs[gname], 'fwd4', arith, ARITH128[arith], S, fin, fout, flags=onewin)


@pytest.mark.parametrize('arith', sorted(ARITH128))
@pytest.mark.parametrize('conds', [(c,) for c in CONDS4] + [('wide',), CONDS4], ids=lambda c: '+'.join(c))
@pytest.mark.parametrize('S,fin,fout,gname,flags', [(6, 48, 32, 'B', ONEWIN), (4, 40, 24, 'A', 0), (8, 32, 32, 'B', CHK), (6, 20, 28, 'B', 0)])
def test_fwd4_conditions(dev, graphs, arith, conds, S, fin, fout, gname, flags):
    run_conv(dev, graphs[gname], 'fwd4', arith, ARITH128[arith], S, fin, fout, conds, flags=flags)


# ------------------------------------------------------------------------------------------------------------------------- contracts
def _refused(dev, g, want, S, fin, fout, flags, ldx=None, ldo=None, xlead=0, vlead=0, epi=0):
    """a call the host code answers without a launch: the return code, and the output buffer (guards included) bit for bit as before"""
    from gnn_matlang_amd.graph import _stream
    ldx = fin if ldx is None else ldx
    c = _inputs(g, S, fin, fout, ('refused', S, fin, fout, flags), ('accum',), max(ldx, fin), 0)
    out = _Out(dev, g.N, fout, max(ldo or fout, fout), False, c['out0'])
    xd, vd, wd, bd = _up(c['x'], dev, xlead), _up(c['val'], dev, vlead), _up(c['w'], dev), _up(c['bias'], dev)
    gi = g.csr.ginfo128 if (flags & G128) or epi else g.csr.ginfo
    L = _lib.lib()
    if epi:
        dsd = _up(np.ones((S + 1, fin), np.float32), dev)
        rc = L.gml_spectconv_fwd_epi(_p(g.csr.rowptr), _p(g.csr.col), _p(gi), _p(vd, vlead), _p(xd, xlead), ldx, _p(wd), fin * fout, fout, 1,
                                     _p(bd), out.ptr(), ldo or fout, g.N, S, fin, fout, flags, epi, _p(dsd), 0, _stream(dev))
    else:
        rc = L.gml_spectconv_fwd(_p(g.csr.rowptr), _p(g.csr.col), _p(gi), _p(None), _p(vd, vlead), _p(xd, xlead), ldx, _p(wd),
                                 fin * fout, fout, 1, _p(bd), out.ptr(), ldo or fout, g.N, S, fin, fout, flags, _stream(dev))
    rc = _done(rc)
    assert rc == want, (S, fin, fout, hex(flags), ldx, ldo, xlead, vlead, epi, rc)
    assert out.unchanged(), (S, fin, fout, hex(flags), 'the refused call wrote to the output')


def test_contract_error_answers(dev, graphs):
    g = graphs['A']
    BAD, UNS = _lib.GML_E_BADARG, _lib.GML_E_UNSUPPORTED
    for S, fin in FWD4_ONLY:                                 # only fwd4 serves them on 128-row records, and fwd4 is a ring kernel
        _refused(dev, g, UNS, S, fin, 24, G128, xlead=1)                         # x not 16-byte aligned
        _refused(dev, g, UNS, S, fin, 24, G128 | _lib.GML_ACCUM)
    _refused(dev, g, UNS, 6, 21, 24, G128, ldx=21)                               # x rows not float4-addressable
    for S, fin, fout, fl in [(5, 32, 32, 0), (8, 33, 32, 0), (8, 32, 33, 0), (8, 32, 32, _lib.GML_F32_MFMA), (12, 48, 16, 0), (6, 49, 16, 0)]:
        _refused(dev, g, BAD, S, fin, fout, G128 | fl)                           # 128-row records for a 64-row shape
    for S, fin in [(8, 32), (12, 32), (6, 48), (4, 40)]:
        _refused(dev, g, BAD, S, fin, 16, G128, vlead=1)                         # value rows 4 bytes off
    _refused(dev, g, BAD, 7, 20, 16, 0, vlead=1)                                 # (the 64-row family wants them 16-byte aligned too)
    for fl in (0, G128):
        _refused(dev, g, BAD, 8, 32, 16, fl, ldx=28)                             # ldx < Fin
        _refused(dev, g, BAD, 8, 32, 16, fl, ldo=12)                             # ldo < Fout
    for epi in (1, 2):
        _refused(dev, g, UNS, 12, 32, 16, 0, epi=epi, ldo=12 * 16)               # the epilogues are fwd3's alone
        _refused(dev, g, UNS, 8, 32, 16, _lib.GML_F32_MFMA, epi=epi, ldo=8 * 16)
        _refused(dev, g, UNS, 8, 32, 16, 0, epi=epi, ldo=8 * 16, xlead=1)
        _refused(dev, g, UNS, 8, 25, 16, 0, epi=epi, ldo=8 * 16, ldx=25)


@pytest.mark.parametrize('arith', sorted(ARITH128))
@pytest.mark.parametrize('gname', ['D7', 'D129'])
def test_contract_every_128_row_shape_of_the_plan_grid_is_served(dev, graphs, arith, gname):
    """every shape of tests/test_conv_fwd_plan_cpu.py's grid that answers group_rows = 128: an aligned GML_GROUPS128 call returns
    GML_OK and the right numbers"""
    L = _lib.lib()
    served = 0
    for S in list(range(1, 17)) + [24]:
        for fin in [1, 16, 17, 32, 33, 48, 49, 64]:
            for fout in [1, 16, 17, 32, 33]:
                if int(L.gml_spectconv_fwd_group_rows(S, fin, fout, 0)) != 128:
                    continue
                win = int(L.gml_spectconv_fwd_stage_window(S, fin, fout, 0))
                fam = 'fwd4' if win else ('fwd2' if S == 12 else 'fwd3')
                run_conv(dev, graphs[gname], fam, arith, ARITH128[arith], S, fin, fout, ldx=(fin + 3) // 4 * 4)
                served += 1
    assert served == 3 * 4 * 4 + 6 * 4 + 2 * 4               # S in {4, 8, 12} x Fin <= 32; S = 6 x Fin <= 48; S = 4 x Fin in {33, 48}


# ------------------------------------------------------------------------------------------------------------------------- SpMM
def run_spmm(dev, g, fam, S, fin, ldx, hint, ginfo=True):
    """gml_spmm_fwd_ex -> H [N, S, Fin] (rows of S Fin floats, 8 guard rows behind) against spmm_ref"""
    from gnn_matlang_amd.graph import _stream
    rng = _rng('spmm', fam, S, fin, ldx, g.N, g.E)
    val, x = _f32(rng.standard_normal((g.E, S))), _f32(rng.standard_normal((g.N, ldx)))
    out = _Out(dev, g.N, S * fin, S * fin)
    xd, vd = _up(x, dev), _up(val, dev)
    rc = _lib.lib().gml_spmm_fwd_ex(_p(g.csr.rowptr), _p(g.csr.col), _p(g.csr.ginfo128 if ginfo else None), _p(None), _p(vd), _p(xd), ldx,
                                    out.ptr(), g.N, S, fin, hint, _stream(dev))
    rc = _done(rc)
    what = 'spmm %s S=%d Fin=%d(ld %d) hint=%d N=%d E=%d' % (fam, S, fin, ldx, hint, g.N, g.E)
    assert rc == _lib.GML_OK, (what, rc)
    H, Ht = R.spmm_ref(g.eis, val, x[:, :fin])
    e_max, e_ts = R.check(out.get(), H.reshape(g.N, -1), Ht.reshape(g.N, -1), g.N, S * fin, S * fin, TOL, what)
    print('%-110s max-norm %.2e  term-sum %.2e' % (what, e_max, e_ts))
    _note('spmm ' + fam, 'f32', e_max, e_ts)


@pytest.mark.parametrize('fin,ldx', [(32, 36), (48, 52), (40, 44), (64, 68), (80, 84), (20, 24)])
@pytest.mark.parametrize('S', [8, 6, 5])
def test_spmm_ring(dev, graphs, S, fin, ldx):
    """spmm3 in its 4-, 2- and 1-support forms; 32-feature launches, the 36 .. 48-feature form, and both in one call (80 = 32 + 48).
    Shapes of the conv's 128-row class reach the ring through the hint max_group_edges > 1,024 (graph B)"""
    g = graphs['B']
    run_spmm(dev, g, 'ring', S, fin, ldx, g.e128)


@pytest.mark.parametrize('gname', ['A', 'D129'])
@pytest.mark.parametrize('fin,ldx', [(32, 36), (20, 24), (20, 23)])
@pytest.mark.parametrize('S', [4, 8, 12])
def test_spmm_register_staged(dev, graphs, S, fin, ldx, gname):
    """fwd2's NOB = 0 form: the 32-feature float4 stores, the element stores, rows that are not float4-addressable"""
    g = graphs[gname]
    run_spmm(dev, g, 'fwd2', S, fin, ldx, g.e128 if ldx == 36 else -1)


@pytest.mark.parametrize('S,fin,ldx,ginfo', [(6, 20, 24, True), (6, 48, 52, True), (4, 40, 44, True), (4, 48, 52, True), (4, 36, 39, True),
                                             (8, 32, 36, False), (5, 17, 19, False), (3, 70, 72, False), (13, 4, 5, False)])
def test_spmm_row_loop(dev, graphs, S, fin, ldx, ginfo):
    """gml_k_spmm: no group records, and the 128-row shapes fwd2 has no NOB = 0 form for -- 6 supports, and S = 4 with 33 .. 48
    features (which the S = 4 instantiation once took: a lane holds 8 of 32 features there, H[:, :, 32:] stayed unwritten)"""
    g = graphs['A']
    run_spmm(dev, g, 'loop', S, fin, ldx, g.e128 if ginfo else -1, ginfo)


# ------------------------------------------------------------------------------------------------------------------------- report
def test_worst_figures_report():
    """prints what the matrix measured (pytest -rP): per kernel family and arithmetic, the worst max-norm figure and the worst
    |got - ref| / term sum.  Every figure was already asserted <= 1e-4 by its own case."""
    assert WORST, 'no case ran'
    print('%-18s %-6s %6s %12s %12s' % ('family', 'arith', 'cases', 'max-norm', 'term-sum'))
    for (fam, arith), (n, e_max, e_ts) in sorted(WORST.items()):
        print('%-18s %-6s %6d %12.2e %12.2e' % (fam, arith, n, e_max, e_ts))
        assert e_max <= TOL and e_ts <= TOL
