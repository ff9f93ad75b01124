"""The ML3Layer node side at the level of its C ABI (include/gml.h): gml_ml3_split_bwd / _ex, gml_node_mix_fwd / _bwd, gml_relu_bwd,
gml_xty and the pools gml_segment_sum / _sum_mask / _bcast / _bcast_mask / _max / _max_bwd, against the float64 restatement of
tests/_node_ref.py: one launch and one numpy reference per case, through _lib.lib() directly, so that a case decides what
functional.py never varies -- an unaligned base or an odd leading dimension, Fin in (48, 64], gy_seg, the pre-masked and the no-fold
form, NULL outputs, a workspace of the exact size, the grid cap and the first row past it, and the error answers.

Which instantiation a case reaches is restated from the launchers (split_inst, mix_inst below, with the source lines they were read
off) and recorded; the last test asserts that every reachable one ran.  The row counts walk the kernels' boundaries: 64 (a wave),
128 (a tile of gml_k_ml3_split_bwd), 256 (a tile of gml_k_node_mix and gml_k_xty), each +- 1, 1000 (several workgroups, a partial
last tile), and the row count at which each persistent grid stops growing and that count + 1, where exactly one workgroup takes a
second trip of its stride loop -- for the pipelined DZO form the trip whose prefetch was issued for a one-row tile.

Every output sits in a buffer of _conv_ref.alloc(): 8 rows behind it, and the columns between its width and its leading dimension,
hold a NaN sentinel and must still hold it; G of gml_ml3_split_bwd and g of gml_relu_bwd are zero-filled up to ldg by contract
(bitwise +0.0 asserted), dz beyond 2 F2 likewise.  The workspace is passed at exactly the size the size query returns with 16
sentinel floats behind it; after an error answer every output must be bit-unchanged.  Inputs carry 8 readable rows behind row N - 1
and every index a case passes stays inside an allocation it owns.  Values are held to TOL_F32 = 2e-5 on the max-norm AND
elementwise on each element's own term sum, the sums (dcb, dw*, db*, dx, xty) also to _conv_ref.f32_bound; selects and the pools'
sums bit-exact.  tests/test_node_ref_cpu.py shows that plain fp32 meets these figures on the same inputs.

The worst figures per (kernel, instantiation, output) are printed by the last test (pytest -rP) and recorded in DESIGN.md s4.4a.
That test reads what the tests before it recorded in this module: run the file whole -- under -k or --lf it reports instantiations
as "not run" that merely were not selected."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import _conv_ref as R
import _node_ref as NR
from gnn_matlang_amd import _lib as G
from test_gpu_conv_fwd_abi import _Out, _done, _f32, _p, _rng, _up

for _k in ('GML_SPLIT_WGS', 'GML_SPLIT_PIPE', 'GML_SPLIT_MM'):
    assert _k not in os.environ, 'run without %s: it is read once per process and changes the dispatch of gml_ml3_split_bwd' % _k

pytestmark = pytest.mark.gpu

TOL_F32 = 2e-5
OK, BAD, UNS, WSP = G.GML_OK, G.GML_E_BADARG, G.GML_E_UNSUPPORTED, G.GML_E_WORKSPACE
N_SMALL = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000)
PAD = R.GUARD_ROWS
NCU = 256                                                   # GML_NUM_CU (csrc/gml_common.h); asserted against the size queries
# launch geometry, read off the launchers: kernel -> (rows per workgroup trip, workgroups at the cap)
CAPS = {'split': (128, 4 * NCU),                            # sb_grid, csrc/gml_ml3_bwd.hip:482-486: SB_ROWS, SB_WGS_PER_CU = 4
        'mix': (256, 2 * NCU),                              # node_mix_grid, csrc/gml_misc.hip:217-220: NM_ROWS
        'xty': (256, 2 * NCU)}                              # xty_grid, csrc/gml_ml3_bwd.hip:706-709: XTY_ROWS
CAP = {k: r * w for k, (r, w) in CAPS.items()}
assert set(CAP.values()) == {131072}
WORST = {}                                                  # (kernel, instantiation, output) -> [cases, worst max-norm, worst term-sum figure]
RAN = set()                                                 # instantiations that ran
TRIPS = set()                                               # kernel classes whose cap + 1 case ran
MEANS = {'cases': 0, 'bit-equal': 0}
SPLIT_ALL = {('rpl', f, va, vx) for f in (16, 32, 48, 64) for va in (1, 4) for vx in (1, 4)} | {('rpl', 0, 1, 4), ('rpl', 0, 4, 4)} | \
            {('dzo', 16), ('dzo', 32)} | {('mm', 32), ('mm', 48), ('mm', 64)}
# 23 of the 24 compiled instantiations: <16, 4, 4, false, MM> is compiled (SB_GO_MM(16)) but `mm` asks FINP >= 32, so no argument
# list reaches it (below 32 inputs the row-per-lane form is faster) -- split_inst asserts that it never names it
MIX_ALL = {(f, d) for f in (16, 32, 48, 64) for d in ('fwd', 'bwd')}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    assert G.lib().gml_version() >= 1
    return torch.device('cuda:0')


def _st(dev):
    from gnn_matlang_amd.graph import _stream
    return _stream(dev)


def _note(kern, inst, out, e):
    w = WORST.setdefault((kern, str(inst), out), [0, 0.0, 0.0])
    w[0] += 1
    w[1], w[2] = max(w[1], e[0]), max(w[2], e[1])


def _flat(dev, n, tail=16):
    """a workspace of n floats with `tail` sentinel floats behind it"""
    return _Out(dev, 1, n, n + tail, guard_rows=0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _ws_exact(ws, n, what):
    """the size query is exact: every one of its n floats was written (one partial row per workgroup the query counts, every
    element of a row), and nothing behind them"""
    w = ws.get().view(np.int32)
    assert (w[n:] == R.SENTINEL).all(), what + ': wrote behind the workspace'
    left = np.flatnonzero(w[:n] == R.SENTINEL)
    assert left.size == 0, '%s: %d workspace floats never written, first at %d of %d' % (what, left.size, left[0], n)


def _up4(n):
    return (n + 3) // 4 * 4


def _odd(n):
    return n | 1


def _ld(width, kind):
    """leading dimension of an operand of `width` columns: al / off -> the next multiple of 4 (off: the base sits 4 bytes past a
    16-byte boundary instead), odd -> the next odd number (never float4-addressable), pad -> 4 more than al"""
    return _odd(width) if kind == 'odd' else _up4(width) + (4 if kind == 'pad' else 0)


def _wide(a, ld, rows=None):
    """a [n, w] -> float32 [rows or n, ld] with finite junk in the padding columns and rows"""
    a = np.asarray(a, np.float32)
    out = np.full((a.shape[0] if rows is None else rows, ld), 7.0, np.float32)
    out[:a.shape[0], :a.shape[1]] = a
    return out


def _hold(o, ref, what, key, bound=True):
    """an _Out against a Ref: TOL_F32 on the max-norm and on each element's term sum, f32_bound, guards"""
    v = np.asarray(ref.v, np.float64).reshape(o.n, o.ncols)
    t = np.asarray(ref.t, np.float64).reshape(o.n, o.ncols)
    b = np.broadcast_to(R.f32_bound(ref), np.asarray(ref.v).shape).reshape(o.n, o.ncols) if bound else None
    e = R.check(o.get(), v, t, o.n, o.ncols, o.ldo, TOL_F32, what, o.guard_rows, bound=b)
    _note(key[0], key[1], key[2], e)


def _exact(o, want, what):
    """an _Out against float32 values, bit for bit; guards intact"""
    got, guards = R.split(o.get(), o.n, o.ncols, o.ldo, o.guard_rows)
    assert (guards == R.SENTINEL).all(), what + ': guard words overwritten'
    want = np.asarray(want, np.float32).reshape(o.n, o.ncols)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, '%s: %d elements differ, first at %s: got %r want %r' % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


# --------------------------------------------------------------------------------------------------------- gml_ml3_split_bwd / _ex
def split_inst(Fin, F2, nout1, ldgy, ldy, ldg, ldx, lddx, a16, x16, dz, dx, premasked):
    """(instantiation, CP) as split_bwd_impl decides them, csrc/gml_ml3_bwd.hip:532-578 (sb_finp :477-480, sb_cp :481, sb_lds
    :488-501).  a16 / x16: the bases of gy, y, G / of x, dx are 16-byte aligned."""
    if premasked:
        ldy = ldg = ldgy
    finp = 0 if F2 == 0 else next(f for f in (16, 32, 48, 64) if Fin <= f)
    w = max(ldg, nout1 + F2)
    cp = 32 if w <= 32 else (64 if w <= 64 else 128)
    va = 4 if ((ldgy | ldy | ldg) & 3) == 0 and a16 else 1
    vx = 4 if F2 == 0 or (((ldx | (lddx if dx else 0)) & 3) == 0 and x16) else 1
    f2p = (F2 + 15) // 16 * 16
    ldxm = finp + (4 if finp % 32 == 16 else 20)
    lds_mm = 4 * max(2 * 128 * 4 + 128 * ldxm + 2 * f2p * ldxm + 2 * f2p + 128 * (2 * f2p + 4), 2 * 2 * 4 * (finp // 16 + 1) * 4 * 64)
    mm = 16 <= F2 <= 32 and finp >= 32 and va == 4 and vx == 4 and not dz and lds_mm <= 160 * 1024
    dzo = bool(dz) and not dx and 2 * F2 <= 4 and va == 4 and vx == 4 and finp in (16, 32) and cp == 32
    inst = ('dzo', finp) if dzo else (('mm', finp) if mm else ('rpl', finp, va, vx if finp else 4))
    assert inst in SPLIT_ALL, inst
    return inst, cp


def _seg_sizes(N):
    """segment sizes 3, 1, 0, 7, 64, 2, 129, ... cut off at N rows"""
    out, tot, k = [], 0, 0
    pat = (3, 1, 0, 7, 64, 2, 129, 5, 0, 0, 33)
    while tot < N:
        s = min(pat[k % len(pat)], N - tot)
        out.append(s)
        tot += s
        k += 1
    return out


def _split_case(N, Fin, F2, nout1, seg, pre, bias, special):
    """(host operands, float64 reference) of one output-stage case"""
    c = dict(NR.stage_inputs(N, Fin, F2, nout1, PAD))
    c['gy'], c['y'] = c['gy'].copy(), c['y'].copy()
    if not bias:
        c['b11'] = c['b12'] = None
    c['where'] = []
    if special:                                              # +0.0, -0.0, a positive denormal and a NaN in the saved output
        vals = np.array([0.0, -0.0, 1e-45, np.nan], np.float32)[:nout1]
        for r in sorted({0, N // 2, N - 1}):
            c['y'][r, :vals.size] = vals
            c['gy'][r, :vals.size] = np.float32(1.5) + np.arange(vals.size, dtype=np.float32)
            c['where'].append(r)
    gseg = None
    if seg:
        sizes = _seg_sizes(N)
        assert len(sizes) <= N + PAD
        gseg = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
        c['nseg'] = len(sizes)
        c['seg'] = np.concatenate([gseg, np.full(PAD, len(sizes) - 1, np.int32)])      # the guard rows' entries stay inside gy
    if pre:
        c['gy'][:, :nout1] = NR.relu_bwd_ref(c['gy'][:, :nout1], c['y'])
    gyr = c['gy'][:c['nseg']] if seg else c['gy'][:N]
    ref = NR.split_bwd_ref(gyr, gseg, None if pre else c['y'][:N], c['x'][:N] if F2 else None, c['w11'], c['b11'], c['w12'], c['b12'],
                           nout1, F2, premasked=pre)
    return c, ref


_small_case = functools.lru_cache(maxsize=64)(_split_case)
_large_case = functools.lru_cache(maxsize=1)(_split_case)


def split_case(N, *a):
    return (_small_case if N <= 4096 else _large_case)(N, *a)


class _Split(object):
    """one output-stage case on the device: operands, outputs in guarded buffers, the workspace at its exact size"""

    def __init__(self, dev, N, Fin, F2, nout1, a='al', x='al', dx=True, dcb=True, db=True, bias=True, dz=None, seg=False, pre=False,
                 fold=True, special=False, rows=None):
        self.dev, self.N, self.Fin, self.F2, self.nout1 = dev, N, Fin, F2, nout1
        self.c, self.ref = split_case(N, Fin, F2, nout1, seg, pre, bias, special)
        c, Cy = self.c, nout1 + F2
        self.pre, self.seg, self.fold = pre, seg, fold
        self.rows = N if rows is None else rows              # num_rows passed (0: the empty call on a case's buffers)
        la, lx = (1 if a == 'off' else 0), (1 if x == 'off' else 0)
        self.ldgy, self.ldy, self.ldg = _ld(Cy, a), _ld(nout1, a), _ld(nout1, a)
        self.ldx = self.lddx = _ld(max(Fin, 1), 'odd' if dz == 'oddx' else x)
        self.la, self.lx = la, lx
        nrow_gy = (c['nseg'] if seg else N) + PAD
        self.gy = _up(_wide(c['gy'][:nrow_gy], self.ldgy), dev, la)
        self.y = None if pre else _up(_wide(c['y'], self.ldy), dev, la)
        self.gseg = _up(c['seg'], dev) if seg else None
        self.x = _up(_wide(c['x'], self.ldx), dev, lx) if F2 else None
        self.w = [(_up(c[k], dev) if F2 and c[k] is not None else None) for k in ('w11', 'b11', 'w12', 'b12')]
        o = self.out = {}
        if not pre:
            o['G'] = _Out(dev, N, self.ldg, self.ldg, off4=bool(la))
        if F2 and dx and not dz:
            o['dx'] = _Out(dev, N, Fin, self.lddx, off4=bool(lx))
        if dz:
            o['dz'] = _Out(dev, N, 4, 4)
        if fold:
            if dcb:
                o['dcb'] = _Out(dev, 1, nout1, nout1)
            if F2:
                o['dw11'], o['dw12'] = _Out(dev, F2, Fin, Fin), _Out(dev, F2, Fin, Fin)
                if db:
                    o['db11'], o['db12'] = _Out(dev, 1, F2, F2), _Out(dev, 1, F2, F2)
        self.need = int(G.lib().gml_ml3_split_bwd_workspace_bytes(N, Fin if F2 else 0, nout1, F2))
        self.npart = 2 * F2 * Fin + 2 * F2 + nout1           # sb_npart, csrc/gml_ml3_bwd.hip:487
        assert self.need % (4 * self.npart) == 0
        self.grid = self.need // (4 * self.npart)
        assert self.grid == min(-(-N // CAPS['split'][0]), CAPS['split'][1]), 'the size query no longer follows sb_grid'
        self.ws = _flat(dev, self.need // 4)
        self.inst, self.cp = split_inst(Fin, F2, nout1, self.ldgy, self.ldy, self.ldg, self.ldx, self.lddx, not la, not lx, bool(dz),
                                        'dx' in o, pre)
        self.what = 'split N=%d Fin=%d F2=%d nout1=%d a=%s x=%s dz=%s seg=%d pre=%d %s CP=%d' % (N, Fin, F2, nout1, a, x, dz, seg, pre,
                                                                                             self.inst, self.cp)

    def launch(self, ex=None, **over):
        """the call; `over` replaces single arguments (error answers)"""
        o = self.out
        ptr = lambda k: o[k].ptr() if k in o else _p(None)
        A = dict(gy=_p(self.gy, self.la), ldgy=self.ldgy, gy_seg=_p(self.gseg), y=_p(self.y, self.la), ldy=self.ldy, x=_p(self.x, self.lx),
                 ldx=self.ldx if self.F2 else 0, w11=_p(self.w[0]), b11=_p(self.w[1]), w12=_p(self.w[2]), b12=_p(self.w[3]), G=ptr('G'),
                 ldg=self.ldg, dx=ptr('dx'), lddx=self.lddx, dz=ptr('dz'), dcb=ptr('dcb'), dw11=ptr('dw11'), db11=ptr('db11'),
                 dw12=ptr('dw12'), db12=ptr('db12'), num_rows=self.rows, Fin=self.Fin, nout1=self.nout1, F2=self.F2, ws=self.ws.ptr(),
                 ws_bytes=self.need, stream=_st(self.dev))
        use_ex = ex if ex is not None else (self.seg or self.pre or 'dz' in o or 'gy_seg' in over or 'dz' in over)
        A.update(over)
        if not use_ex:
            A.pop('gy_seg'), A.pop('dz')
        fn = G.lib().gml_ml3_split_bwd_ex if use_ex else G.lib().gml_ml3_split_bwd
        return _done(fn(*A.values()))

    def unchanged(self):
        return all(o.unchanged() for o in self.out.values())

    def check(self):
        o, ref, N, nout1, F2, what = self.out, self.ref, self.N, self.nout1, self.F2, self.what
        key = lambda out: ('split', self.inst, out)
        if 'G' in o:
            want = np.zeros((N, self.ldg), np.float32)       # columns [nout1, ldg) are +0.0 by contract
            want[:, :nout1] = ref['G']
            _exact(o['G'], want, what + ' G')
            got = R.split(o['G'].get(), N, self.ldg, self.ldg)[0]
            for r in self.c['where']:                        # (y > 0) at +0.0, -0.0, a denormal, NaN: 0, 0, gy, 0
                k = min(nout1, 4)
                assert _same(got[r, :k], np.array([0, 0, self.c['gy'][r, 2] if k > 2 else 0, 0], np.float32)[:k]), what + ' special y'
        if 'dx' in o:
            _hold(o['dx'], ref['dx'], what + ' dx', key('dx'))
        if 'dz' in o:
            _hold(o['dz'], ref['dz'], what + ' dz', key('dz'), bound=False)
            assert (_bits(R.split(o['dz'].get(), N, 4, 4)[0][:, 2 * F2:]) == 0).all(), what + ': dz beyond 2 F2 is not +0.0'
        for k in ('dcb', 'dw11', 'dw12', 'db11', 'db12'):
            if k in o:
                _hold(o[k], ref[k], what + ' ' + k, key(k))
        _ws_exact(self.ws, self.need // 4, what)
        RAN.add(self.inst)

    def bits(self):
        return {k: _bits(v.get()).copy() for k, v in self.out.items()}


def run_split(dev, N, Fin, F2, nout1, expect=None, **kw):
    s = _Split(dev, N, Fin, F2, nout1, **kw)
    if expect is not None:
        assert s.inst == expect, (s.what, expect)
    assert s.launch() == OK, s.what
    s.check()
    return s


# Fin, F2, nout1 grids of the issue; CP = 32 / 64 / 128 through nout1 + F2
FINS = (1, 15, 16, 17, 32, 33, 48, 49, 64)
F2S = (1, 2, 3, 8, 15, 16, 17, 24)                          # 2 F2 <= 48 is the row-per-lane limit: 24 stands for 32


@pytest.mark.parametrize('Fin', FINS)
def test_split_shapes(dev, Fin):
    """every Fin against every F2 and a rotating nout1 (1, 5, 30, 32, 62, 64, 128 - F2: CP = 32, 64 and 128) at two row counts"""
    cps = set()
    for i, F2 in enumerate(F2S):
        nout1 = (1, 5, 30, 32, 62, 64, 128 - F2)[(i + FINS.index(Fin)) % 7]
        for N in (129, 1000):
            cps.add(run_split(dev, N, Fin, F2, nout1).cp)
        cps.add(run_split(dev, 65, Fin, F2, 128 - F2).cp)
    assert cps == {32, 64, 128}, cps


@pytest.mark.parametrize('nout1', (1, 5, 30, 32, 62, 64))
@pytest.mark.parametrize('F2', (0, 2, 16))
def test_split_conv_widths(dev, nout1, F2):
    for N in (64, 257):
        run_split(dev, N, 33, F2, nout1)
    if F2:
        run_split(dev, 257, 33, F2, 128 - F2)


# one shape per FINP: (Fin, F2, nout1); the conditions run on the whole small row list
PER_FINP = ((15, 3, 30), (32, 8, 5), (33, 15, 62), (64, 17, 32))
CONDS = {'plain': {}, 'a odd': dict(a='odd'), 'a off': dict(a='off'), 'x odd': dict(x='odd'), 'x off': dict(x='off'),
         'both odd': dict(a='odd', x='odd'), 'no dx': dict(dx=False), 'no dcb': dict(dcb=False), 'no db': dict(db=False),
         'no bias': dict(bias=False), 'seg': dict(seg=True), 'seg a odd': dict(seg=True, a='odd'), 'premasked': dict(pre=True),
         'premasked x odd': dict(pre=True, x='odd'), 'special y': dict(special=True), 'special y a odd': dict(special=True, a='odd')}


@pytest.mark.parametrize('cond', sorted(CONDS))
@pytest.mark.parametrize('Fin,F2,nout1', PER_FINP)
def test_split_conditions(dev, Fin, F2, nout1, cond):
    kw = CONDS[cond]
    finp = next(f for f in (16, 32, 48, 64) if Fin <= f)
    va = 1 if kw.get('a') else 4
    vx = 1 if kw.get('x') else 4
    for N in N_SMALL:
        s = run_split(dev, N, Fin, F2, nout1, **kw)
        assert s.inst == (('mm', finp) if F2 >= 16 and finp >= 32 and va == vx == 4 else ('rpl', finp, va, vx)), s.what


@pytest.mark.parametrize('cond', ('plain', 'a odd', 'a off', 'seg', 'premasked', 'special y', 'no dcb'))
def test_split_without_hadamard_branch(dev, cond):
    """F2 = 0: x and w* NULL, the relu mask and the bias sums of a plain SpectConv"""
    kw = CONDS[cond]
    for nout1 in (5, 32, 62, 127 if kw.get('a') == 'odd' else 128):       # (an odd ldg >= 128 is 129: beyond the 128-column tile)
        for N in N_SMALL:
            run_split(dev, N, 0, 0, nout1, expect=('rpl', 0, 1 if kw.get('a') else 4, 4), **kw)


@pytest.mark.parametrize('Fin,F2', ((24, 16), (32, 24), (33, 16), (48, 24), (49, 17), (64, 24)))
@pytest.mark.parametrize('cond', ('plain', 'no dx', 'seg', 'premasked', 'no bias', 'special y'))
def test_split_matrix_core_form(dev, Fin, F2, cond):
    finp = next(f for f in (32, 48, 64) if Fin <= f)
    for N in N_SMALL:
        run_split(dev, N, Fin, F2, 32 if cond != 'seg' else 30, expect=('mm', finp), **CONDS[cond])


def test_split_sixteen_inputs_stay_on_the_row_per_lane_form(dev):
    """FINP = 16 at 16 <= F2: `mm` asks FINP >= 32 -- the compiled <16, 4, 4, false, MM> is never launched"""
    for F2 in (16, 24):
        for N in (1, 129, 1000):
            run_split(dev, N, 16, F2, 32, expect=('rpl', 16, 4, 4))


@pytest.mark.parametrize('F2', (1, 2))
@pytest.mark.parametrize('Fin', (3, 16, 17, 32, 33, 64))
@pytest.mark.parametrize('kind', ('al', 'oddx', 'seg', 'premasked', 'wide', 'a off'))
def test_split_dz_hand_over(dev, F2, Fin, kind):
    """dz [N, 4] instead of dx: aligned rows of <= 32 columns at FINP <= 32 reach the pipelined DZO form (with a segment map and in
    the pre-masked form too), anything else the general kernel with dz set"""
    finp = next(f for f in (16, 32, 48, 64) if Fin <= f)
    kw = dict(al={}, oddx=dict(dz='oddx'), seg=dict(seg=True), premasked=dict(pre=True), wide={}, **{'a off': dict(a='off')})[kind]
    nout1 = 62 if kind == 'wide' else 32 - F2
    dzo = kind in ('al', 'seg', 'premasked') and finp <= 32
    exp = ('dzo', finp) if dzo else ('rpl', finp, 1 if kind == 'a off' else 4, 1 if kind == 'oddx' else 4)
    for N in N_SMALL:
        run_split(dev, N, Fin, F2, nout1, expect=exp, **dict(dict(dz='al'), **kw))


CAP_CLASSES = {'rpl16': ((16, 8, 24), {}, ('rpl', 16, 4, 4)), 'dzo32': ((32, 2, 30), dict(dz='al'), ('dzo', 32)),
               'mm48': ((48, 24, 40), {}, ('mm', 48)), 'finp0': ((0, 0, 32), {}, ('rpl', 0, 4, 4))}


@pytest.mark.parametrize('cls', sorted(CAP_CLASSES))
def test_split_grid_cap_and_the_first_row_past_it(dev, cls):
    """131072 rows fill 1024 workgroups with one tile each; at 131073 workgroup 0 takes a second trip over a ONE-ROW tile -- in the
    DZO form the tile whose rows were prefetched, clamped to that one row, during the first trip's pass B"""
    (Fin, F2, nout1), kw, exp = CAP_CLASSES[cls]
    q = lambda n: int(G.lib().gml_ml3_split_bwd_workspace_bytes(n, Fin, nout1, F2)) // (4 * (2 * F2 * Fin + 2 * F2 + nout1))
    cap = CAP['split']
    assert [q(n) for n in (cap - 128, cap - 127, cap, cap + 1, 4 * cap)] == [1023, 1024, 1024, 1024, 1024]
    for N in (cap, cap + 1):
        s = run_split(dev, N, Fin, F2, nout1, expect=exp, **kw)
        assert s.grid == CAPS['split'][1]
        del s
    TRIPS.add('split ' + cls)
    _large_case.cache_clear()


@pytest.mark.parametrize('Fin,F2,nout1,kw', ((15, 3, 30, {}), (33, 16, 32, {}), (32, 2, 30, dict(dz='al')), (0, 0, 62, {}),
                                              (49, 8, 5, dict(a='odd', x='odd')), (17, 1, 31, dict(seg=True))))
def test_split_no_fold_form_and_repeat(dev, Fin, F2, nout1, kw):
    """every one of dcb, dw*, db* NULL: the partials [dw11 | dw12 | db11 | db12 | dcb] stay in the workspace, and gml_fold_many on
    them gives bit for bit what the folded call gives; two launches of a case agree bit for bit"""
    for N in N_SMALL:
        a = run_split(dev, N, Fin, F2, nout1, **kw)
        b = run_split(dev, N, Fin, F2, nout1, **kw)
        ba, bb = a.bits(), b.bits()
        assert all(np.array_equal(ba[k], bb[k]) for k in ba), a.what + ': two launches differ'
        s = _Split(dev, N, Fin, F2, nout1, fold=False, **kw)
        assert s.inst == a.inst and s.launch(ex=True) == OK
        s.check()
        for k in ('G', 'dx', 'dz'):
            assert k not in ba or np.array_equal(ba[k], s.bits()[k]), s.what + ': %s differs without the fold' % k
        names = ('dw11', 'dw12', 'db11', 'db12', 'dcb')
        sizes = (F2 * Fin, F2 * Fin, F2, F2, nout1)
        outs = {k: _Out(dev, 1, n, max(n, 1)) for k, n in zip(names, sizes)}
        job = G.FoldJob()
        job.partial, job.nparts, job.n = s.ws.ptr().value, s.grid, s.npart
        for i, (k, n) in enumerate(zip(names, sizes)):
            job.dst[i], job.ndst[i] = (outs[k].ptr().value if n else None), n
        assert _done(G.lib().gml_fold_many(ctypes.addressof(job), 1, _st(dev))) == OK
        for k, n in zip(names, sizes):
            if n:
                got = R.split(outs[k].get(), 1, n, n)[0].ravel()
                want = R.split(a.out[k].get(), a.out[k].n, a.out[k].ncols, a.out[k].ldo)[0].ravel()
                assert _same(got, want), s.what + ': %s of gml_fold_many differs from the folded call' % k


def test_split_error_answers(dev):
    N, Fin, F2, nout1 = 130, 17, 2, 30
    mk = lambda **kw: _Split(dev, N, Fin, F2, nout1, **kw)

    def refused(s, want, why, **over):
        assert s.launch(**over) == want, 'split: %s should answer %d' % (why, want)
        assert s.unchanged(), 'split: an output changed under the error answer for ' + why
        assert (s.ws.get().view(np.int32) == R.SENTINEL).all(), 'split: the workspace was written under the error answer for ' + why

    s = mk()
    dz = _Out(dev, N, 4, 4)
    dz4 = _Out(dev, N, 4, 4, off4=True)
    refused(s, BAD, 'dz together with dx', dz=dz.ptr())
    s2 = mk(dx=False)
    refused(s2, BAD, 'dz not 16-byte aligned', dz=dz4.ptr())
    s3 = _Split(dev, N, Fin, 3, nout1, dx=False)
    refused(s3, BAD, 'dz with 2 F2 > 4', dz=dz.ptr())
    assert dz.unchanged() and dz4.unchanged()
    refused(s, BAD, 'ldgy < nout1 + F2', ldgy=nout1 + F2 - 1)
    refused(s, BAD, 'ldy < nout1', ldy=nout1 - 1)
    refused(s, BAD, 'ldg < nout1', ldg=nout1 - 1)
    refused(s, BAD, 'ldx < Fin', ldx=Fin - 1)
    refused(s, BAD, 'lddx < Fin', lddx=Fin - 1)
    refused(s, BAD, 'y without G', G=_p(None))
    refused(s, BAD, 'G without y', y=_p(None))
    refused(s, BAD, 'num_rows < 0', num_rows=-1)
    refused(s, BAD, 'nout1 = 0', nout1=0)
    sp = mk(pre=True)
    seg = _up(np.zeros(N + PAD, np.int32), dev)
    refused(sp, BAD, 'gy_seg in the pre-masked form', gy_seg=_p(seg))
    refused(s, BAD, 'dw11 without dw12', dw12=_p(None))
    refused(s, BAD, 'w11 NULL', w11=_p(None))
    refused(s, BAD, 'x NULL', x=_p(None))
    refused(s, BAD, 'gy NULL', gy=_p(None))
    refused(s, UNS, 'Fin = 65', Fin=65, ldx=68, lddx=68)
    refused(s, UNS, '2 F2 > 48', F2=25, ldgy=nout1 + 25)
    refused(s, UNS, 'ldg > 128', ldg=132)
    assert G.lib().gml_ml3_split_bwd_workspace_bytes(N, 65, nout1, F2) == 0 and G.lib().gml_ml3_split_bwd_workspace_bytes(N, Fin, nout1, 25) == 0
    refused(s, WSP, 'a workspace 4 bytes short', ws_bytes=s.need - 4)
    refused(s, WSP, 'ws NULL', ws=_p(None))
    # nothing above left a trace: the same buffers now take the call
    assert s.launch() == OK
    s.check()
    # num_rows = 0 zeroes dcb, dw*, db* and nothing else
    for kw in ({}, dict(db=False), dict(dcb=False)):
        z = mk(rows=0, **kw)
        assert z.launch(ws=_p(None), ws_bytes=0) == OK
        for k, o in z.out.items():
            if k in ('G', 'dx'):
                assert o.unchanged(), 'split num_rows = 0: %s was written' % k
            else:
                _exact(o, np.zeros((o.n, o.ncols), np.float32), 'split num_rows = 0 ' + k)
    z = _Split(dev, N, 0, 0, nout1, rows=0)
    assert z.launch(ws=_p(None), ws_bytes=0) == OK and z.out['G'].unchanged()
    _exact(z.out['dcb'], np.zeros((1, nout1), np.float32), 'split num_rows = 0, F2 = 0: dcb')


# ------------------------------------------------------------------------------------------------- gml_node_mix_fwd / gml_node_mix_bwd
def mix_inst(Fin, direction):
    """node_mix_finp, csrc/gml_misc.hip:210; the template's second argument is the direction (node_mix_launch :224-239)"""
    return (next(f for f in (16, 32, 48, 64) if Fin <= f), direction)


@functools.lru_cache(maxsize=64)
def _mix_small(N, Fin, F2, bias):
    return _mix_make(N, Fin, F2, bias)


@functools.lru_cache(maxsize=1)
def _mix_large(N, Fin, F2, bias):
    return _mix_make(N, Fin, F2, bias)


def _mix_make(N, Fin, F2, bias):
    c = NR.mix_inputs(N, Fin, F2, PAD)
    if not bias:
        c['b11'] = c['b12'] = None
    fwd = NR.mix_ref(c['x'][:N], c['w11'], c['b11'], c['w12'], c['b12'])
    bwd = NR.node_mix_bwd_ref(c['x'][:N], c['g'][:N], c['w11'], c['b11'], c['w12'], c['b12'])
    acc = NR.node_mix_bwd_ref(c['x'][:N], c['g'][:N], c['w11'], c['b11'], c['w12'], c['b12'], c['dx0'])['dx']
    return c, fwd, bwd, acc


def mix_case(N, Fin, F2, bias=True):
    return (_mix_small if N <= 4096 else _mix_large)(N, Fin, F2, bias)


def run_mix_fwd(dev, N, Fin, F2, ld='al', off=False, bias=True):
    c, (v, t), _, _ = mix_case(N, Fin, F2, bias)
    ldx, ldo = (Fin if ld == 'tight' else _ld(Fin, ld)), (F2 if ld == 'tight' else _ld(F2, ld) + (1 if ld == 'pad' else 0))
    x = _up(_wide(c['x'], ldx), dev, 1 if off else 0)
    w = [(_up(c[k], dev) if c[k] is not None else None) for k in ('w11', 'b11', 'w12', 'b12')]
    out = _Out(dev, N, F2, ldo)
    what = 'node_mix_fwd N=%d Fin=%d F2=%d ld=%s off=%d' % (N, Fin, F2, ld, off)
    rc = _done(G.lib().gml_node_mix_fwd(_p(x, 1 if off else 0), ldx, _p(w[0]), _p(w[1]), _p(w[2]), _p(w[3]), out.ptr(), ldo, N, Fin, F2, _st(dev)))
    assert rc == OK, what
    inst = mix_inst(Fin, 'fwd')
    _hold(out, R.Ref(v, t, Fin + 1.0), what, ('node_mix', inst, 'out'), bound=False)
    RAN.add(inst)


def run_mix_bwd(dev, N, Fin, F2, ld='al', off=False, bias=True, dx='old', db=True):
    """dx: 'old' (accumulates onto old values), 'zero' (onto zeros), None (NULL)"""
    c, _, ref, acc = mix_case(N, Fin, F2, bias)
    tight = ld == 'tight'
    ldx, ldg, lddx = (Fin if tight else _ld(Fin, ld)), (F2 if tight else _ld(F2, ld)), (Fin if tight else _ld(Fin, ld) + (1 if ld == 'pad' else 0))
    x = _up(_wide(c['x'], ldx), dev, 1 if off else 0)
    g = _up(_wide(c['g'], ldg), dev)
    w = [(_up(c[k], dev) if c[k] is not None else None) for k in ('w11', 'b11', 'w12', 'b12')]
    o = {'dw11': _Out(dev, F2, Fin, Fin), 'dw12': _Out(dev, F2, Fin, Fin)}
    if db:
        o['db11'], o['db12'] = _Out(dev, 1, F2, F2), _Out(dev, 1, F2, F2)
    if dx:
        o['dx'] = _Out(dev, N, Fin, lddx, out0=c['dx0'] if dx == 'old' else np.zeros((N, Fin), np.float32))
    need = int(G.lib().gml_node_mix_bwd_workspace_bytes(N, Fin, F2))
    npart = 2 * F2 * Fin + 2 * F2
    assert need == 4 * 4 * npart * min(-(-N // CAPS['mix'][0]), CAPS['mix'][1]), 'the size query no longer follows node_mix_grid'
    ws = _flat(dev, need // 4)
    ptr = lambda k: o[k].ptr() if k in o else _p(None)
    what = 'node_mix_bwd N=%d Fin=%d F2=%d ld=%s off=%d dx=%s db=%d' % (N, Fin, F2, ld, off, dx, db)
    rc = _done(G.lib().gml_node_mix_bwd(_p(x, 1 if off else 0), ldx, _p(w[0]), _p(w[1]), _p(w[2]), _p(w[3]), _p(g), ldg, ptr('dx'), lddx, ptr('dw11'),
                                        ptr('db11'), ptr('dw12'), ptr('db12'), N, Fin, F2, ws.ptr(), need, _st(dev)))
    assert rc == OK, what
    inst = mix_inst(Fin, 'bwd')
    for k in o:
        _hold(o[k], (acc if dx == 'old' else ref['dx']) if k == 'dx' else ref[k], what + ' ' + k, ('node_mix', inst, k))
    _ws_exact(ws, need // 4, what)
    RAN.add(inst)
    return {k: _bits(v.get()).copy() for k, v in o.items()}


@pytest.mark.parametrize('Fin', FINS)
def test_node_mix_shapes(dev, Fin):
    for i, F2 in enumerate(F2S):
        ld = ('tight', 'al', 'pad', 'odd')[(i + Fin) % 4]
        for N in (129, 257, 1000):
            run_mix_fwd(dev, N, Fin, F2, ld)
            run_mix_bwd(dev, N, Fin, F2, ld)


@pytest.mark.parametrize('Fin,F2', ((15, 3), (32, 8), (33, 15), (64, 24)))
@pytest.mark.parametrize('cond', ('tight', 'al', 'pad', 'odd', 'off', 'no bias', 'no dx', 'dx zero', 'no db'))
def test_node_mix_conditions(dev, Fin, F2, cond):
    ld = cond if cond in ('tight', 'al', 'pad', 'odd') else 'al'
    for N in N_SMALL:
        run_mix_fwd(dev, N, Fin, F2, ld, off=cond == 'off', bias=cond != 'no bias')
        a = run_mix_bwd(dev, N, Fin, F2, ld, off=cond == 'off', bias=cond != 'no bias', dx={'no dx': None, 'dx zero': 'zero'}.get(cond, 'old'),
                        db=cond != 'no db')
        if N == 257:
            b = run_mix_bwd(dev, N, Fin, F2, ld, off=cond == 'off', bias=cond != 'no bias', dx={'no dx': None, 'dx zero': 'zero'}.get(cond, 'old'),
                            db=cond != 'no db')
            assert all(np.array_equal(a[k], b[k]) for k in a), 'node_mix_bwd: two launches differ'


@pytest.mark.parametrize('direction', ('fwd', 'bwd'))
def test_node_mix_grid_cap_and_the_first_row_past_it(dev, direction):
    Fin, F2 = 17, 3
    q = lambda n: int(G.lib().gml_node_mix_bwd_workspace_bytes(n, Fin, F2)) // (4 * 4 * (2 * F2 * Fin + 2 * F2))
    cap = CAP['mix']
    assert [q(n) for n in (cap - 256, cap - 255, cap, cap + 1, 4 * cap)] == [511, 512, 512, 512, 512]
    for N in (cap, cap + 1):
        (run_mix_fwd if direction == 'fwd' else run_mix_bwd)(dev, N, Fin, F2)
    TRIPS.add('node_mix ' + direction)
    _mix_large.cache_clear()


def test_node_mix_error_answers(dev):
    N, Fin, F2 = 70, 17, 3
    c = mix_case(N, Fin, F2)[0]
    x, g = _up(_wide(c['x'], 20), dev), _up(_wide(c['g'], 4), dev)
    w = [_up(c[k], dev) for k in ('w11', 'b11', 'w12', 'b12')]
    out = _Out(dev, N, F2, 4)
    o = [_Out(dev, N, Fin, 20), _Out(dev, F2, Fin, Fin), _Out(dev, 1, F2, F2), _Out(dev, F2, Fin, Fin), _Out(dev, 1, F2, F2)]
    need = int(G.lib().gml_node_mix_bwd_workspace_bytes(N, Fin, F2))
    ws = _flat(dev, need // 4)
    L, st = G.lib(), _st(dev)

    def fwd(want, why, x=_p(x), ldx=20, w11=_p(w[0]), outp=None, ldo=4, n=N, fin=Fin, f2=F2):
        rc = _done(L.gml_node_mix_fwd(x, ldx, w11, _p(w[1]), _p(w[2]), _p(w[3]), out.ptr() if outp is None else outp, ldo, n, fin, f2, st))
        assert rc == want and out.unchanged(), 'node_mix_fwd: ' + why

    def bwd(want, why, x=_p(x), ldx=20, ldg=4, lddx=20, dw12=None, n=N, fin=Fin, f2=F2, wsp=None, wsb=need, gp=_p(g)):
        rc = _done(L.gml_node_mix_bwd(x, ldx, _p(w[0]), _p(w[1]), _p(w[2]), _p(w[3]), gp, ldg, o[0].ptr(), lddx, o[1].ptr(), o[2].ptr(),
                                      o[3].ptr() if dw12 is None else dw12, o[4].ptr(), n, fin, f2, ws.ptr() if wsp is None else wsp, wsb, st))
        assert rc == want, 'node_mix_bwd: %s answered %d' % (why, rc)
        assert all(b.unchanged() for b in o) and ws.unchanged(), 'node_mix_bwd: an output changed under the error answer for ' + why

    fwd(BAD, 'ldx < Fin', ldx=Fin - 1)
    fwd(BAD, 'ldo < F2', ldo=F2 - 1)
    fwd(BAD, 'x NULL', x=_p(None))
    fwd(BAD, 'w11 NULL', w11=_p(None))
    fwd(BAD, 'F2 = 0', f2=0)
    fwd(BAD, 'num_rows < 0', n=-1)
    fwd(UNS, 'Fin = 65', fin=65, ldx=68)
    fwd(UNS, '2 F2 > 48', f2=25, ldo=25)
    fwd(OK, 'num_rows = 0 writes nothing', n=0)
    bwd(BAD, 'ldx < Fin', ldx=Fin - 1)
    bwd(BAD, 'ldg < F2', ldg=F2 - 1)
    bwd(BAD, 'lddx < Fin', lddx=Fin - 1)
    bwd(BAD, 'dw12 NULL', dw12=_p(None))
    bwd(BAD, 'x NULL', x=_p(None))
    bwd(BAD, 'gout NULL', gp=_p(None))
    bwd(UNS, 'Fin = 65', fin=65, ldx=68, lddx=68)
    bwd(UNS, '2 F2 > 48', f2=25, ldg=25)
    bwd(WSP, 'a workspace 4 bytes short', wsb=need - 4)
    bwd(WSP, 'ws NULL', wsp=_p(None))
    assert L.gml_node_mix_bwd_workspace_bytes(N, 65, F2) == 0 and L.gml_node_mix_bwd_workspace_bytes(N, Fin, 25) == 0
    rc = _done(L.gml_node_mix_bwd(_p(x), 20, _p(w[0]), _p(w[1]), _p(w[2]), _p(w[3]), _p(g), 4, o[0].ptr(), 20, o[1].ptr(), o[2].ptr(), o[3].ptr(),
                                  o[4].ptr(), 0, Fin, F2, _p(None), 0, st))
    assert rc == OK and o[0].unchanged(), 'node_mix_bwd num_rows = 0 wrote dx'
    for b in o[1:]:
        _exact(b, np.zeros((b.n, b.ncols), np.float32), 'node_mix_bwd num_rows = 0')


# -------------------------------------------------------------------------------------------------------------------- gml_relu_bwd
@pytest.mark.parametrize('F', (1, 3, 4, 30, 32, 33, 128))
@pytest.mark.parametrize('ldk', ('F', 'up4', 'F+5'))
def test_relu_bwd(dev, F, ldk):
    ldg = {'F': F, 'up4': _up4(F), 'F+5': F + 5}[ldk]
    for N in N_SMALL:
        rng = _rng('relu', F, ldk, N)
        gy = _f32(rng.standard_normal((N + PAD, F + 1)))
        y = np.maximum(_f32(rng.standard_normal((N + PAD, F + 2))), np.float32(0))
        vals = np.array([0.0, -0.0, 1e-45, np.nan], np.float32)[:F]
        for r in {0, N - 1}:
            y[r, :vals.size] = vals
        g, gy_d, y_d = _Out(dev, N, ldg, ldg), _up(gy, dev), _up(y, dev)
        rc = _done(G.lib().gml_relu_bwd(_p(gy_d), F + 1, _p(y_d), F + 2, g.ptr(), ldg, N, F, _st(dev)))
        assert rc == OK
        want = np.zeros((N, ldg), np.float32)
        want[:, :F] = NR.relu_bwd_ref(gy[:N, :F], y[:N, :F])
        _exact(g, want, 'relu_bwd N=%d F=%d ldg=%d' % (N, F, ldg))
        k = vals.size
        assert _same(R.split(g.get(), N, ldg, ldg)[0][0, :k], np.array([0, 0, gy[0, 2] if k > 2 else 0, 0], np.float32)[:k])
    for over, want in ((dict(ldgy=F - 1), BAD), (dict(ldy=F - 1), BAD), (dict(ldg=F - 1), BAD), (dict(F=0), BAD), (dict(n=-1), BAD)):
        a = dict(ldgy=F + 1, ldy=F + 2, ldg=ldg, n=N, F=F)
        a.update(over)
        g = _Out(dev, N, ldg, ldg)
        rc = _done(G.lib().gml_relu_bwd(_p(gy_d), a['ldgy'], _p(y_d), a['ldy'], g.ptr(), a['ldg'], a['n'], a['F'], _st(dev)))
        assert rc == want and g.unchanged(), ('relu_bwd', over)


# ------------------------------------------------------------------------------------------------------------------------- gml_xty
XTY_AB = (1, 15, 16, 17, 47, 48, 49, 64)


def _xty_inputs(n, a, b):
    return NR.xty_inputs(n, a, b, PAD)


def run_xty(dev, n, a, b, pad=False):
    A, B = _xty_inputs(n, a, b)
    lda, ldb = (a + 3, b + 1) if pad else (a, b)
    out = _Out(dev, a, b, b)
    need = int(G.lib().gml_xty_workspace_bytes(n, a, b))
    assert need == 4 * a * b * min(-(-n // CAPS['xty'][0]), CAPS['xty'][1]), 'the size query no longer follows xty_grid'
    ws, A_d, B_d = _flat(dev, need // 4), _up(_wide(A, lda), dev), _up(_wide(B, ldb), dev)
    rc = _done(G.lib().gml_xty(_p(A_d), lda, _p(B_d), ldb, out.ptr(), n, a, b, ws.ptr(), need, _st(dev)))
    what = 'xty n=%d a=%d b=%d pad=%d' % (n, a, b, pad)
    assert rc == OK, what
    ldc = lambda v: 16 if v <= 16 else (48 if v <= 48 else 80)                   # xty_ld, csrc/gml_ml3_bwd.hip:618
    _hold(out, NR.xty_ref(A[:n], B[:n]), what, ('xty', (ldc(a), ldc(b)), 'out'))
    _ws_exact(ws, need // 4, what)
    RAN.add(('xty', ldc(a), ldc(b)))
    return _bits(out.get()).copy()


@pytest.mark.parametrize('a', XTY_AB)
def test_xty_shapes(dev, a):
    for b in XTY_AB:
        for n in (N_SMALL if b in (17, 64) else (257,)):
            run_xty(dev, n, a, b, pad=(a + b + n) % 2 == 1)
    assert np.array_equal(run_xty(dev, 1000, a, 33), run_xty(dev, 1000, a, 33)), 'xty: two launches differ'


def test_xty_grid_cap_and_the_first_row_past_it(dev):
    a, b = 17, 33
    q = lambda n: int(G.lib().gml_xty_workspace_bytes(n, a, b)) // (4 * a * b)
    cap = CAP['xty']
    assert [q(n) for n in (cap - 256, cap - 255, cap, cap + 1, 4 * cap)] == [511, 512, 512, 512, 512]
    for n in (cap, cap + 1):
        run_xty(dev, n, a, b)
    TRIPS.add('xty')


def test_xty_error_answers(dev):
    n, a, b = 100, 17, 5
    A, B = _xty_inputs(n, a, b)
    At, Bt = _up(A, dev), _up(B, dev)
    out = _Out(dev, a, b, b)
    need = int(G.lib().gml_xty_workspace_bytes(n, a, b))
    ws = _flat(dev, need // 4)
    L, st = G.lib(), _st(dev)

    def call(want, why, Ap=_p(At), lda=a, ldb=b, o=None, n=n, a=a, b=b, wsp=None, wsb=need):
        rc = _done(L.gml_xty(Ap, lda, _p(Bt), ldb, out.ptr() if o is None else o, n, a, b, ws.ptr() if wsp is None else wsp, wsb, st))
        assert rc == want and out.unchanged() and ws.unchanged(), 'xty: ' + why

    call(BAD, 'lda < a', lda=a - 1)
    call(BAD, 'ldb < b', ldb=b - 1)
    call(BAD, 'out NULL', o=_p(None))
    call(BAD, 'A NULL', Ap=_p(None))
    call(BAD, 'n < 0', n=-1)
    call(UNS, 'a = 65', a=65, lda=65)
    call(UNS, 'b = 65', b=65, ldb=65)
    call(WSP, 'a workspace 4 bytes short', wsb=need - 4)
    call(WSP, 'ws NULL', wsp=_p(None))
    assert L.gml_xty_workspace_bytes(n, 65, b) == 0 and L.gml_xty_workspace_bytes(n, a, 65) == 0
    assert _done(L.gml_xty(_p(At), a, _p(Bt), b, out.ptr(), 0, a, b, _p(None), 0, st)) == OK
    _exact(out, np.zeros((a, b), np.float32), 'xty n = 0')


# --------------------------------------------------------------------------------------------------------------------------- pools
POOL_LISTS = {'empty ends': NR.SEG_SIZES, 'reversed, full last': NR.SEG_SIZES[::-1] + (9,)}


def _pool_x(sizes, F, relu=False):
    ptr = NR.seg_ptr(sizes)
    rows = int(ptr[-1])
    rng = _rng('pool', sizes, F)
    x = _f32(rng.standard_normal((rows + PAD, F)))
    if relu:                                                 # a layer output: exact zeros, and the values (x > 0) has to decide
        x = np.maximum(x, np.float32(0))
        x[::7, 3], x[::5, 31], x[1::9, 0] = np.float32(-0.0), np.float32(1e-45), np.float32(-1e-45)
    return ptr, rows, x


def _i32_out(dev, n, ncols, guard=PAD):
    host = np.full((n + guard) * ncols, R.SENTINEL, np.int32)
    return host, torch.from_numpy(host.copy()).to(dev)


@pytest.mark.parametrize('lst', sorted(POOL_LISTS))
@pytest.mark.parametrize('F', (1, 7, 32, 33, 64))
def test_segment_sum_and_bcast(dev, lst, F):
    sizes = POOL_LISTS[lst]
    ptr, rows, x = _pool_x(sizes, F)
    nseg, L, st = len(sizes), G.lib(), _st(dev)
    ptr_d = _up(ptr, dev)
    g = _f32(_rng('poolg', lst, F).standard_normal((nseg + PAD, F + 3)))
    g_d = _up(g, dev)
    for mean in (0, 1, 2, 3):
        xs = x.copy()
        if mean & 2:
            xs[ptr[-2]:ptr[-1]] = np.nan                     # the padding graph's rows are not read
        for ldx, ldo in ((F, F), (F + 1, F + 2)):
            out, x_d = _Out(dev, nseg, F, ldo), _up(_wide(xs, ldx), dev)
            assert _done(L.gml_segment_sum(_p(x_d), ldx, _p(ptr_d), out.ptr(), ldo, nseg, F, mean, st)) == OK
            s, m = NR.segment_sum_ref(xs[:rows], ptr, mean)
            what = 'segment_sum %s F=%d mean=%d ldx=%d' % (lst, F, mean, ldx)
            if mean & 1:
                got, guards = R.split(out.get(), nseg, F, ldo)
                assert (guards == R.SENTINEL).all(), what
                assert (np.abs(got.astype(np.float64) - m) <= np.spacing(np.abs(m))).all(), what + ': a mean beyond 1 ulp'
                MEANS['cases'] += 1
                MEANS['bit-equal'] += int(_same(got, m))
                if mean & 2:
                    assert (_bits(got[-1]) == 0).all(), what + ': the skipped row is not +0.0'
            else:
                _exact(out, s, what)
    for mean in (0, 1):
        for ldo in (F, F + 1):
            out = _Out(dev, rows, F, ldo)
            assert _done(L.gml_segment_bcast(_p(g_d), F + 3, _p(ptr_d), out.ptr(), ldo, nseg, F, mean, st)) == OK
            want = NR.segment_bcast_ref(g[:nseg, :F], ptr, mean)
            what = 'segment_bcast %s F=%d mean=%d ldo=%d' % (lst, F, mean, ldo)
            if mean:
                got, guards = R.split(out.get(), rows, F, ldo)
                assert (guards == R.SENTINEL).all(), what
                assert (np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want))).all(), what + ': the mean scale beyond 1 ulp'
            else:
                _exact(out, want, what)
    out = _Out(dev, nseg, F, F)
    for a in (dict(ldx=F - 1), dict(ldo=F - 1), dict(F=0), dict(n=-1)):
        k = dict(ldx=F, ldo=F, F=F, n=nseg)
        k.update(a)
        assert _done(L.gml_segment_sum(_p(x_d), k['ldx'], _p(ptr_d), out.ptr(), k['ldo'], k['n'], k['F'], 0, st)) == BAD and out.unchanged()
        assert _done(L.gml_segment_bcast(_p(g_d), F + 3 if 'ldx' not in a else F - 1, _p(ptr_d), out.ptr(), k['ldo'], k['n'], k['F'], 0,
                                         st)) == BAD and out.unchanged()


@pytest.mark.parametrize('lst', sorted(POOL_LISTS))
@pytest.mark.parametrize('mean', (0, 1, 2, 3))
def test_segment_sum_mask_and_bcast_mask(dev, lst, mean):
    """two segments share a wave of gml_k_segment_sum_mask32 and each takes its own half of a ballot cast inside a divergent branch:
    the list pairs segments of different lengths, either one the longer, with an empty one, and across the 32-row step of the loop"""
    sizes = POOL_LISTS[lst]
    ptr, rows, x = _pool_x(sizes, 32, relu=True)
    nseg, L, st = len(sizes), G.lib(), _st(dev)
    live = rows if not (mean & 2) else int(ptr[-2])
    if mean & 2:
        x[ptr[-2]:ptr[-1]] = np.nan
    ptr_d = _up(ptr, dev)
    for ldx, ldo in ((32, 32), (37, 33)):
        x_d = _up(_wide(x, ldx), dev)
        plain, out, mask = _Out(dev, nseg, 32, ldo), _Out(dev, nseg, 32, ldo), _Out(dev, rows, 1, 1)
        assert _done(L.gml_segment_sum(_p(x_d), ldx, _p(ptr_d), plain.ptr(), ldo, nseg, 32, mean, st)) == OK
        assert _done(L.gml_segment_sum_mask(_p(x_d), ldx, _p(ptr_d), out.ptr(), ldo, mask.ptr(), nseg, 32, mean, st)) == OK
        what = 'segment_sum_mask %s mean=%d ldx=%d' % (lst, mean, ldx)
        assert _same(out.get(), plain.get()), what + ': sums differ from gml_segment_sum'
        if not (mean & 1):
            _exact(out, NR.segment_sum_ref(x[:rows], ptr, mean)[0], what)
        words = np.full(rows, R.SENTINEL, np.int32)          # the skipped segment's words are not written
        words[:live] = NR.relu_words_ref(x[:live]).view(np.int32)
        _exact(mask, words.view(np.float32), what + ' mask words')
    # the broadcast that applies the pattern
    words = NR.relu_words_ref(np.nan_to_num(x[:rows], nan=0.0))
    seg = np.concatenate([NR.seg_of(ptr), np.full(PAD, nseg - 1, np.int32)])
    g = _f32(_rng('poolgm', lst).standard_normal((nseg + PAD, 36)))
    g_d, seg_d, w_d = _up(g, dev), _up(seg, dev), _up(np.concatenate([words, np.zeros(PAD, np.uint32)]).view(np.int32), dev)
    for nrelu in (0, 1, 30, 31, 32):
        for ldo in (32, 36):
            out = _Out(dev, rows, 32, ldo)
            assert _done(L.gml_segment_bcast_mask(_p(g_d), 36, _p(seg_d), _p(w_d), out.ptr(), ldo, rows, 32, nrelu, st)) == OK
            _exact(out, NR.segment_bcast_mask_ref(g, seg[:rows], words, nrelu), 'segment_bcast_mask %s nrelu=%d ldo=%d' % (lst, nrelu, ldo))
    if mean == 0:
        out, off = _Out(dev, rows, 32, 36), _Out(dev, rows, 32, 36, off4=True)
        g1 = _up(g, dev, 1)
        call = lambda gp, ldg, o, ldo, F=32, nrelu=30: _done(L.gml_segment_bcast_mask(gp, ldg, _p(seg_d), _p(w_d), o.ptr(), ldo, rows, F, nrelu, st))
        assert call(_p(g1, 1), 36, out, 36) == BAD and call(_p(g_d), 36, off, 36) == BAD, 'segment_bcast_mask: a misaligned base'
        assert call(_p(g_d), 35, out, 36) == BAD and call(_p(g_d), 36, out, 33) == BAD, 'segment_bcast_mask: an odd leading dimension'
        assert call(_p(g_d), 36, out, 36, nrelu=33) == BAD and call(_p(g_d), 36, out, 36, F=16) == UNS
        mask = _Out(dev, rows, 1, 1)
        assert _done(L.gml_segment_sum_mask(_p(x_d), 37, _p(ptr_d), out.ptr(), 36, mask.ptr(), nseg, 16, 0, st)) == UNS
        assert _done(L.gml_segment_sum_mask(_p(x_d), 31, _p(ptr_d), out.ptr(), 36, mask.ptr(), nseg, 32, 0, st)) == BAD
        assert out.unchanged() and off.unchanged() and mask.unchanged()


@pytest.mark.parametrize('lst', sorted(POOL_LISTS))
@pytest.mark.parametrize('F', (1, 7, 32, 33, 64))
def test_segment_max_and_its_backward(dev, lst, F):
    sizes = POOL_LISTS[lst]
    ptr, rows, x = _pool_x(sizes, F)
    nseg, L, st = len(sizes), G.lib(), _st(dev)
    for s in range(nseg):                                    # duplicated maxima: first and last row, first and middle, middle and last
        r0, r1 = int(ptr[s]), int(ptr[s + 1])
        if r1 - r0 >= 3:
            a, b = ((r0, r1 - 1), (r0, (r0 + r1) // 2), ((r0 + r1) // 2, r1 - 1))[s % 3]
            x[a, s % F] = x[b, s % F] = np.float32(9.0)
            x[r0:r1, (s + 1) % F] = np.float32(-3.0)         # a whole column of equal values: the first row
    ptr_d = _up(ptr, dev)
    v, arg = NR.segment_max_ref(x[:rows], ptr)
    g = _f32(_rng('poolgx', lst, F).standard_normal((nseg + PAD, F + 1)))
    g_d = _up(g, dev)
    for ldx, ldo in ((F, F), (F + 3, F + 1)):
        x_d = _up(_wide(x, ldx), dev)
        for with_arg in (True, False):
            out = _Out(dev, nseg, F, ldo)
            ah, a_d = _i32_out(dev, nseg, F)
            rc = _done(L.gml_segment_max(_p(x_d), ldx, _p(ptr_d), out.ptr(), ldo, _p(a_d if with_arg else None), nseg, F, st))
            assert rc == OK
            _exact(out, v, 'segment_max %s F=%d ldx=%d argmax=%d' % (lst, F, ldx, with_arg))
            got = a_d.cpu().numpy()
            if with_arg:
                assert np.array_equal(got[:nseg * F].reshape(nseg, F), arg), 'segment_max: argmax is not the first row that attains the maximum'
                assert (got[nseg * F:] == R.SENTINEL).all()
            else:
                assert np.array_equal(got, ah)
        a_d = _up(np.concatenate([arg.ravel(), np.full(PAD * F, -1, np.int32)]), dev)
        out = _Out(dev, rows, F, ldo)                        # prefilled with the sentinel: every row of every segment is written
        assert _done(L.gml_segment_max_bwd(_p(g_d), F + 1, _p(ptr_d), _p(a_d), out.ptr(), ldo, nseg, F, st)) == OK
        _exact(out, NR.segment_max_bwd_ref(g[:nseg, :F], ptr, arg), 'segment_max_bwd %s F=%d ldo=%d' % (lst, F, ldo))
    out = _Out(dev, nseg, F, F)
    assert _done(L.gml_segment_max(_p(x_d), F - 1, _p(ptr_d), out.ptr(), F, _p(None), nseg, F, st)) == BAD
    assert _done(L.gml_segment_max(_p(x_d), F, _p(ptr_d), out.ptr(), F - 1, _p(None), nseg, F, st)) == BAD
    assert _done(L.gml_segment_max_bwd(_p(x_d), F, _p(ptr_d), _p(None), out.ptr(), F, nseg, F, st)) == BAD and out.unchanged()


# ------------------------------------------------------------------------------------------------------------------------ coverage
def test_every_instantiation_ran_and_worst_figures_report():
    """runs last (file order): all 23 reachable split instantiations of the 24 compiled, the 4 x 2 node-mix ones, and the cap + 1
    case of every kernel class"""
    split_ran = {i for i in RAN if i in SPLIT_ALL}
    mix_ran = {i for i in RAN if i in MIX_ALL}
    print('gml_ml3_split_bwd instantiations run: %d / %d reachable (24 compiled; <16, MM> unreachable)' % (len(split_ran), len(SPLIT_ALL)))
    print('gml_k_node_mix instantiations run: %d / %d' % (len(mix_ran), len(MIX_ALL)))
    print('cap + 1 cases run: %s' % sorted(TRIPS))
    print('means: %d cases, %d bit-equal to float32(sum) / float32(len)' % (MEANS['cases'], MEANS['bit-equal']))
    print('%-10s %-22s %-6s %6s %12s %12s' % ('kernel', 'instantiation', 'output', 'cases', 'max-norm', 'term sum'))
    for (kern, inst, out), (n, a, b) in sorted(WORST.items()):
        print('%-10s %-22s %-6s %6d %12.3e %12.3e' % (kern, inst, out, n, a, b))
    assert split_ran == SPLIT_ALL, 'not run: %s' % sorted(SPLIT_ALL - split_ran)
    assert mix_ran == MIX_ALL, 'not run: %s' % sorted(MIX_ALL - mix_ran)
    assert {('xty', p, q) for p in (16, 48, 80) for q in (16, 48, 80)} <= RAN
    assert TRIPS == {'split ' + c for c in CAP_CLASSES} | {'node_mix fwd', 'node_mix bwd', 'xty'}, TRIPS
