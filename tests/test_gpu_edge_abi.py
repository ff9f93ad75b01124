"""The ML3Layer edge branch at the level of its C ABI (include/gml.h): every entry point -- gml_edge_mlp_fwd / _fwd6 / _fwd_exact, the
stacks _fwd_stack / _fwd_stack6 / _fwd_stack6_sym(_dev), gml_edge_mlp_bwd / _bwd_exact / _bwd_sym(_dev), gml_edge_presplit,
gml_gather_rows_presplit, gml_edge_mlp_wide_fwd / _wide_bwd -- on every kernel family gml_edge_mlp_plan names, against the float64
restatement of tests/_edge_ref.py: one launch and one numpy reference per case, through _lib.lib() directly, so that a case decides
what functional.py never varies: ea_split or not, out_t or not, gin or not, folded or deferred weight gradients, a workspace of the
exact size, the unique-row lists and their device-side count, and the error answers.

Which family a case reaches is asked of gml_edge_mlp_plan (csrc/gml_edge_plan.h), as tests/test_gpu_edge_plan.py does: a request the
plan refuses must come back GML_E_UNSUPPORTED with every output bit-unchanged.  The edge counts walk the kernels' boundaries: 16 (a
tile), 32 (a wave's tile pair: for an odd tile count the second tile of the last pair lies wholly past E), 64 (a backward workgroup
trip, a one-edge-per-lane backward batch, a chain16 forward trip), 128 (a forward workgroup trip), 256 (a one-edge-per-lane forward
block), 512 (the wide kernels' block), and the E at which each persistent grid reaches its cap, and that E + 1, where exactly one
workgroup takes a second trip of its stride loop (CAPS below: read off the launchers; the backward's from its size queries).

Every output sits in a buffer of _conv_ref.alloc(): 8 rows behind out, out[l], out_t, gin, dw1 .. dw4, go, hid and gz and 16 floats
behind the workspace -- which is passed at exactly the size the call needs -- hold a NaN sentinel and must still hold it; after an
error answer every output must be bit-unchanged.  ea, ea_split and gout carry 8 readable rows behind their E rows: the slack slots of
a device-counted list point there (a kernel that walked them would write the guard rows of the outputs), and every index a case
passes stays inside an allocation it owns.  Values are held to TOL = 1e-4 (the bf16-piece chains) resp. 2e-5 (one edge per lane in
fp32: gml_edge_mlp_*_exact at any S, S = 1, the wide kernels) on the max-norm (conftest.rel_err) AND elementwise on each element's own
term sum (tests/_edge_ref.py).  Rows 0, E // 2 and E - 1 of ea are exact zeros wherever E >= 8 -- the padding edges of a static batch
-- and must give an out row of +0.0 and a gin row of 0 on every family.

The worst figures per (family, entry, output) are printed by the last test (pytest -rP) and recorded in DESIGN.md s4.3b."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import _conv_ref as R
import _edge_ref as ER
from gnn_matlang_amd import _lib as G
from test_gpu_conv_fwd_abi import _Out, _done, _f32, _p, _rng, _up

assert os.environ.get('GML_EDGE_VALU', '0') in ('0', ''), 'run without GML_EDGE_VALU: it turns every two-piece answer of the plan into the VALU family'

pytestmark = pytest.mark.gpu

TOL, TOL_F32 = 1e-4, 2e-5
OK, BAD, UNS, WSP = G.GML_OK, G.GML_E_BADARG, G.GML_E_UNSUPPORTED, G.GML_E_WORKSPACE
FWD, BWD = G.GML_EDGE_FWD, G.GML_EDGE_BWD
TWO, THREE, EXACT = G.GML_EDGE_TWO_PIECE, G.GML_EDGE_THREE_PIECE, G.GML_EDGE_EXACT
SPLIT, GIN, DUAL, UNIQ = G.GML_EDGE_HAS_SPLIT, G.GML_EDGE_WANT_GIN, G.GML_EDGE_DUAL, G.GML_EDGE_UNIQUE
NONE, VALU = G.GML_EDGE_FAM_NONE, G.GML_EDGE_FAM_VALU
FAM = {G.GML_EDGE_FAM_VALU: 'valu', G.GML_EDGE_FAM_CHAIN: 'chain', G.GML_EDGE_FAM_CHAIN16: 'chain16', G.GML_EDGE_FAM_CHAIN6: 'chain6',
       G.GML_EDGE_FAM_CHAIN16X6: 'chain16x6', G.GML_EDGE_FAM_SYM6: 'sym6', G.GML_EDGE_FAM_SYM16X6: 'sym16x6',
       G.GML_EDGE_FAM_SYM_CHAIN: 'sym_chain', G.GML_EDGE_FAM_SYM_CHAIN16: 'sym_chain16'}
SS = tuple(range(1, 17))
E_SMALL = (1, 15, 16, 17, 31, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
E_MULTI = 1000                                              # several workgroups of every kernel, no boundary: the conditions' second size
PAD = R.GUARD_ROWS                                          # readable rows behind ea / ea_split / gout
NCU = 256                                                   # GML_NUM_CU (csrc/gml_common.h); asserted against the backward's size query
# forward launch geometry, read off the launchers: family -> (edges per workgroup trip, workgroups at the cap)
CAPS_FWD = {'chain': (128, 6 * NCU),                        # gml_launch_edge_chain_fwd: cdiv(tiles, 8), <= 6 per CU
            'chain stack': (128, 4 * NCU),                  # gml_launch_edge_chain_fwd_stack
            'chain16': (64, 4 * NCU),                       # gml_launch_edge_chain16_fwd: cdiv(tiles, 4)
            'chain6': (128, 4 * NCU), 'sym6': (128, 4 * NCU),           # gml_launch_edge_chain6_fwd, .._fwd_sym
            'chain16x6': (128, 2 * NCU), 'sym16x6': (128, 2 * NCU),     # gml_launch_edge_chain16x6_fwd(_sym)
            'valu': (256, 16 * NCU)}                        # gml_launch_edge_mlp_fwd
# backward: family -> (edges per trip, partial rows at the cap); asserted against gml_edge_mlp_bwd_parts / _bwd_sym_parts
CAPS_BWD = {'chain': (64, 6 * NCU), 'sym_chain': (64, 6 * NCU), 'chain16': (64, 2 * NCU), 'sym_chain16': (64, 2 * NCU), 'valu': (64, 8 * NCU)}
WORST = {}                                                  # (family, entry, output) -> [cases, worst max-norm, worst term-sum figure]
RAN = set()                                                 # (family, direction, S, layers)
TRIPS = set()                                               # (family, direction) whose cap + 1 case ran


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    assert G.lib().gml_version() >= 1
    return torch.device('cuda:0')


def _st(dev):
    from gnn_matlang_amd.graph import _stream
    return _stream(dev)


def _note(fam, entry, out, e):
    w = WORST.setdefault((fam, entry, out), [0, 0.0, 0.0])
    w[0] += 1
    w[1], w[2] = max(w[1], e[0]), max(w[2], e[1])


# ------------------------------------------------------------------------------------------------------------------------- cases
def _inputs(S, E, kind):
    """Host operands of one shape.  ea ~ 0.7 N(0, 1), four weight sets drawn as tests/test_gpu_edge_plan.reference draws them (layer l
    of a stack uses set l; set 0 is the backward's: its ea rows keep a relu margin, oracle.relu_margin.make_safe_edges).  E >= 8: rows
    0, E // 2 and E - 1 (and their mirrors) are exact zeros, with gout left non-zero.  The unique-row list by `kind`:
      mixed     edges [0, P), P = E // 3, have a mirror P + i carrying bitwise the same row; the rest are one-sided; entries shuffled,
                so that mirrors fall in the same tile, in another tile and in another workgroup's tile
      none      no mirrors: every edge its own entry
      all       every entry mirrored, edge i with E / 2 + i (E even)
      adjacent  every entry mirrored with the next row, edge 2i with 2i + 1: always the same tile (E even)
      zeros     every row of ea an exact zero (the dw of such a batch must be exactly zero)"""
    from oracle.relu_margin import make_safe_edges
    g = torch.Generator().manual_seed(1000 * S + E % 997 + 7)
    ws = [[torch.randn(2 * S, S, generator=g) * 0.7 for _ in range(3)] + [torch.randn(S, 4 * S, generator=g) * 0.5] for _ in range(4)]
    ea = make_safe_edges(torch.randn(E + PAD, S, generator=g) * 0.7, *ws[0], scale=0.7, generator=g)
    gout = torch.randn(E + PAD, S, generator=g).numpy()
    ea = ea.numpy()
    P = {'mixed': E // 3, 'none': 0, 'all': E // 2, 'adjacent': E // 2, 'zeros': 0}[kind]
    assert kind not in ('all', 'adjacent') or E % 2 == 0
    rng = _rng('lists', S, E, kind)
    if kind == 'adjacent':
        a, b, rest = np.arange(0, E, 2), np.arange(1, E, 2), np.arange(0)
    else:
        a, b, rest = np.arange(P), np.arange(P, 2 * P), np.arange(2 * P, E)
    zero = []
    if kind == 'zeros':
        ea[:E] = 0.0
        zero = list(range(E))
    elif E >= 8:
        mid = E // 2
        zero = [0, E - 1, mid]
        ea[zero] = 0.0
        for x, y in ((a, b), (b, a)):                        # the mirrors of zero rows are zero rows
            hit = np.isin(x, zero)
            ea[y[hit]] = 0.0
            zero += list(y[hit])
    ea[b] = ea[a]
    order = rng.permutation(a.size + rest.size)
    uid = np.concatenate([a, rest])[order].astype(np.int32)
    mir = np.concatenate([b, np.full(rest.size, -1)])[order].astype(np.int32)
    return dict(S=S, E=E, ea=_f32(ea), gout=_f32(gout), ws=[[_f32(t.numpy()) for t in w] for w in ws], uid=uid, mir=mir,
                tpos=rng.permutation(E).astype(np.int32), zero=sorted(set(zero)))


@functools.lru_cache(maxsize=None)
def _small_inputs(S, E, kind):
    return _inputs(S, E, kind)


@functools.lru_cache(maxsize=2)
def _large_inputs(S, E, kind):
    return _inputs(S, E, kind)


def case(S, E, kind='mixed'):
    return _small_inputs(S, E, kind) if E <= 4096 else _large_inputs(S, E, kind)


def _fwd_ref(S, E, kind, l):
    c = case(S, E, kind)
    return ER.edge_fwd_ref(c['ea'][:E], *c['ws'][l])


def _bwd_ref(S, E, kind, sym):
    c = case(S, E, kind)
    return ER.edge_bwd_ref(c['ea'][:E], *c['ws'][0], c['gout'][:E], uid=c['uid'] if sym else None, mir=c['mir'] if sym else None)


_small_fwd, _large_fwd = functools.lru_cache(maxsize=None)(_fwd_ref), functools.lru_cache(maxsize=4)(_fwd_ref)
_small_bwd, _large_bwd = functools.lru_cache(maxsize=None)(_bwd_ref), functools.lru_cache(maxsize=2)(_bwd_ref)


def fwd_ref(S, E, kind, l):
    """float64 reference of layer l's output, computed once per shape"""
    return (_small_fwd if E <= 4096 else _large_fwd)(S, E, kind, l)


def bwd_ref(S, E, kind, sym=False):
    return (_small_bwd if E <= 4096 else _large_bwd)(S, E, kind, bool(sym))


_DEV = {}


def dcase(dev, S, E, kind='mixed'):
    """the case's operands on the device (made once per shape; no call writes them): ea, gout and the pre-split image with their 8
    readable rows, the weights, tpos, uid / mir"""
    key = (S, E, kind)
    if key not in _DEV:
        if E > 4096:
            for k in [k for k in _DEV if k[1] > 4096]:
                del _DEV[k]
        c = case(S, E, kind)
        d = {k: _up(c[k], dev) for k in ('ea', 'gout', 'uid', 'mir', 'tpos')}
        d['ws'] = [[_up(t, dev) for t in w] for w in c['ws']]
        d['cnt'] = _up(np.array([c['uid'].size], np.int32), dev)
        d['es'] = torch.zeros((E + PAD) * (8 if S <= 8 else 16), dtype=torch.int32, device=dev)
        assert _done(G.lib().gml_edge_presplit(_p(d['ea']), _p(d['es']), E + PAD, S, _st(dev))) == OK
        _DEV[key] = d
    return _DEV[key]


def _arr(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*[p.value for p in ptrs])


def _plan(direction, S, So, L, flags):
    return int(G.lib().gml_edge_mlp_plan(direction, S, So, L, flags))


def _tol(fam):
    return TOL_F32 if fam == VALU else TOL


def _flat(dev, n, tail=16):
    """a workspace of n floats with `tail` sentinel floats behind it"""
    return _Out(dev, 1, n, n + tail, guard_rows=0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------------------------------- forward
def run_fwd(dev, entry, S, E, split=False, dual=False, L=0, kind='mixed', count=None, slack=0):
    """One forward launch and its checks; returns the L output arrays (None after a refusal).  entry: fwd (gml_edge_mlp_fwd), fwd6,
    exact, stack, stack6, sym, sym_dev (count = *count, `slack` extra list slots pointing at the guard rows E + k)."""
    Lb, st = G.lib(), _st(dev)
    c, d = case(S, E, kind), dcase(dev, S, E, kind)
    nl = max(L, 1)
    outs = [_Out(dev, E, S, S) for _ in range(nl)]
    out_t = _Out(dev, E, S, S) if dual else None
    w = d['ws']
    one = (_p(w[0][0]), _p(w[0][1]), _p(w[0][2]), _p(w[0][3]), outs[0].ptr(), _p(d['tpos'] if dual else None),
           out_t.ptr() if dual else _p(None), E, S, S, st)
    wl = [_arr([_p(w[l][i]) for l in range(nl)]) for i in range(4)]
    oa = _arr([o.ptr() for o in outs])
    U = c['uid'].size
    slack = min(slack, E - U)                                # (gml.h: the capacity of a list is at most num_edges)
    written = np.ones(E, bool)
    if entry == 'fwd':
        flags, rc = TWO | (SPLIT if split else 0), Lb.gml_edge_mlp_fwd(_p(d['ea']), _p(d['es'] if split else None), *one)
    elif entry == 'fwd6':
        flags, rc = THREE, Lb.gml_edge_mlp_fwd6(_p(d['ea']), *one)
    elif entry == 'exact':
        flags, rc = EXACT, Lb.gml_edge_mlp_fwd_exact(_p(d['ea']), *one)
    elif entry == 'stack':
        flags, rc = TWO | SPLIT, Lb.gml_edge_mlp_fwd_stack(_p(d['es']), L, *wl, oa, E, S, S, st)
    elif entry == 'stack6':
        flags, rc = THREE, Lb.gml_edge_mlp_fwd_stack6(_p(d['ea']), L, *wl, oa, E, S, S, st)
    elif entry == 'sym':
        flags, rc = THREE | UNIQ, Lb.gml_edge_mlp_fwd_stack6_sym(_p(d['ea']), _p(d['uid']), _p(d['mir']), U, L, *wl, oa, E, S, S, st)
    else:
        assert entry == 'sym_dev'
        rng = _rng('slack', S, E, kind, slack)
        uid = _up(np.concatenate([c['uid'], E + rng.integers(0, PAD, slack)]).astype(np.int32), dev)
        mir = _up(np.concatenate([c['mir'], E + rng.integers(0, PAD, slack)]).astype(np.int32), dev)
        cnt = _up(np.array([U if count is None else count], np.int32), dev)
        flags, rc = THREE | UNIQ, Lb.gml_edge_mlp_fwd_stack6_sym_dev(_p(d['ea']), _p(uid), _p(mir), _p(cnt), U + slack, L, *wl, oa, E, S, S, st)
        if count is not None and count < U:
            written[:] = False
            for a in (c['uid'][:count], c['mir'][:count]):
                written[a[a >= 0]] = True
    rc = _done(rc)
    fam = _plan(FWD, S, S, L, flags | (DUAL if dual else 0))
    what = '%s S=%d E=%d L=%d split=%d dual=%d %s family=%d' % (entry, S, E, L, split, dual, kind, fam)
    if fam == NONE:
        assert rc == UNS, (what, rc)
        assert all(o.unchanged() for o in outs) and (out_t is None or out_t.unchanged()), what + ': an output changed under an error answer'
        return None
    assert rc == OK, (what, rc)
    got = []
    for l, o in enumerate(outs):
        ref = fwd_ref(S, E, kind, l)
        buf = o.get()
        if not written.all():                                # rows no entry names must still hold the sentinel; the others are checked
            rows = buf.reshape(E + R.GUARD_ROWS, S)
            assert (_bits(rows[:E][~written]) == R.SENTINEL).all(), what + ': a row beyond *count was written'
            buf = buf.copy()
            buf.reshape(E + R.GUARD_ROWS, S)[:E][~written] = ref.v[~written]
        _note(FAM[fam], entry, 'out', R.check(buf, ref.v, ref.t, E, S, S, _tol(fam), what + ' out[%d]' % l))
        v = R.split(buf, E, S, S)[0]
        z = [r for r in c['zero'] if written[r]]
        assert not _bits(v[z]).any(), what + ': the out row of a zero support row is not +0.0'
        got.append(v.copy())
    if dual:
        t, guards = R.split(out_t.get(), E, S, S)
        assert (guards == R.SENTINEL).all(), what + ': guard rows behind out_t overwritten'
        assert _same(t[c['tpos']], got[0]), what + ': out_t[tpos] is not bitwise out'
    RAN.add((FAM[fam], 'fwd', S, L))
    return got


@pytest.mark.parametrize('S', SS)
def test_forward_single_layer(dev, S):
    """gml_edge_mlp_fwd (ea_split x out_t), _fwd6 and _fwd_exact (out_t or not) at every boundary size"""
    for E in E_SMALL:
        for split in (0, 1):
            for dual in (0, 1):
                run_fwd(dev, 'fwd', S, E, split=split, dual=dual)
        for dual in (0, 1):
            run_fwd(dev, 'fwd6', S, E, dual=dual)
            run_fwd(dev, 'exact', S, E, dual=dual)


@pytest.mark.parametrize('S', SS)
def test_forward_stacks_and_unique_rows(dev, S):
    """gml_edge_mlp_fwd_stack (2 .. 4 layers), _fwd_stack6 (1 .. 4) and the unique-row forms with the host and the device count
    (capacity U + 5, the slack slots pointing at the guard rows).  Outside S in {4, 8} the plan refuses the stacks (the unique-row
    form serves one layer for 2 <= S <= 16): the answer is GML_E_UNSUPPORTED and nothing is written."""
    for E in E_SMALL:
        for L in (1, 2, 3, 4):
            if S in (4, 8) or E in (17, 129):               # (the refusals do not depend on E: two sizes)
                run_fwd(dev, 'stack', S, E, L=L)
                run_fwd(dev, 'stack6', S, E, L=L)
            if S in (4, 8) or L == 1 or E in (17, 129):
                run_fwd(dev, 'sym', S, E, L=L)
                run_fwd(dev, 'sym_dev', S, E, L=L, slack=5)


# ------------------------------------------------------------------------------------------------------------------------- backward
def _parts(entry, S, E, U, split, gin):
    Lb = G.lib()
    if entry in ('sym', 'sym_dev'):
        return int(Lb.gml_edge_mlp_bwd_sym_parts(U, S))
    if entry == 'exact':                                     # always the one-edge-per-lane family; the query answers for gml_edge_mlp_bwd
        return _valu_parts(S, E)
    return int(Lb.gml_edge_mlp_bwd_parts(E, S, S, int(split), int(gin)))


def _cdiv(a, b):
    return -(-a // b)


def _valu_waves(S):
    """waves per workgroup of the one-edge-per-lane backward (csrc/gml_edge_plan.h, edge_plan_valu_bwd_wg_waves)"""
    return 4 if ((7 * S) | 1) * 64 * 4 * 4 <= 64 * 1024 else 2


def _valu_parts(S, E):
    """partial rows of the one-edge-per-lane backward (gml_edge_mlp_bwd_waves): one per wave, at most 8 per CU, whole workgroups;
    test_workspace_query_covers_every_family holds it to the library's query wherever that answers for this family"""
    w = _valu_waves(S)
    return max(w, _cdiv(min(8 * NCU, _cdiv(E, 64)), w) * w)


def run_bwd(dev, entry, S, E, split=False, gin=False, kind='mixed', fold=True, count=None, slack=0, short=0, expect=None):
    """One backward launch and its checks; returns {'gin', 'dw1' .. 'dw4', 'ws', 'parts'} (None after a refusal).  entry: bwd, exact,
    sym, sym_dev.  fold = False: dw1 .. dw4 = NULL, the partial rows stay in the workspace.  short: ws_bytes that much below the
    call's need."""
    Lb, st = G.lib(), _st(dev)
    c, d = case(S, E, kind), dcase(dev, S, E, kind)
    sym = entry in ('sym', 'sym_dev')
    U = c['uid'].size
    slack = min(slack, E - U)                                # (the capacity of a list is at most num_edges)
    parts = _parts(entry, S, E, U + slack, split, gin)
    NW = 10 * S * S
    assert parts > 0
    ws = _flat(dev, parts * NW)
    shapes = [(2 * S, S)] * 3 + [(S, 4 * S)]
    dws = [_Out(dev, r, k, k) for r, k in shapes]
    g = _Out(dev, E, S, S) if gin else None
    w = [_p(t) for t in d['ws'][0]]
    dwp = [o.ptr() if fold else _p(None) for o in dws]
    tail = (*dwp, E, S, S, ws.ptr(), parts * NW * 4 - short, st)
    live = U
    if entry == 'bwd':
        flags = TWO | (SPLIT if split else 0) | (GIN if gin else 0)
        rc = Lb.gml_edge_mlp_bwd(_p(d['ea']), _p(d['es'] if split else None), *w, _p(d['gout']), g.ptr() if gin else _p(None), *tail)
    elif entry == 'exact':
        flags = EXACT | (GIN if gin else 0)
        rc = Lb.gml_edge_mlp_bwd_exact(_p(d['ea']), *w, _p(d['gout']), g.ptr() if gin else _p(None), *tail)
    elif entry == 'sym':
        flags = TWO | SPLIT | UNIQ
        rc = Lb.gml_edge_mlp_bwd_sym(_p(d['es']), _p(d['uid']), _p(d['mir']), U, *w, _p(d['gout']), *tail)
    else:
        assert entry == 'sym_dev'
        flags = TWO | SPLIT | UNIQ
        rng = _rng('slack', S, E, kind, slack)
        uid = _up(np.concatenate([c['uid'], E + rng.integers(0, PAD, slack)]).astype(np.int32), dev)
        mir = _up(np.concatenate([c['mir'], E + rng.integers(0, PAD, slack)]).astype(np.int32), dev)
        cnt = _up(np.array([U if count is None else count], np.int32), dev)
        live = U if count is None else min(max(count, 0), U + slack)
        rc = Lb.gml_edge_mlp_bwd_sym_dev(_p(d['es']), _p(uid), _p(mir), _p(cnt), U + slack, *w, _p(d['gout']), *tail)
    rc = _done(rc)
    fam = _plan(BWD, S, S, 0, flags)
    what = '%s S=%d E=%d split=%d gin=%d fold=%d %s family=%d' % (entry, S, E, split, gin, fold, kind, fam)
    if fam == NONE or expect not in (None, OK):
        assert rc == (UNS if expect is None else expect), (what, rc)
        assert all(o.unchanged() for o in dws) and (g is None or g.unchanged()) and ws.unchanged(), what + ': an output changed under an error answer'
        return None
    assert rc == OK, (what, rc)
    assert live == U or live == 0, 'a case checks a whole list or an empty one'
    ref = bwd_ref(S, E, kind, sym)
    tol, name = _tol(fam), FAM[fam]
    res = {'parts': parts}
    wbuf = ws.get()
    assert (_bits(wbuf[parts * NW:]) == R.SENTINEL).all(), what + ': the floats behind the workspace were written'
    rows = wbuf[:parts * NW].reshape(parts, NW)
    res['ws'] = rows.copy()
    # every float of the call's partial rows is written
    assert np.isfinite(rows).all(), what + ': %d floats of the %d partial rows were not written' % (int((~np.isfinite(rows)).sum()), parts)
    if live == 0:
        assert not rows.any(), what + ': an empty list leaves zeros in every partial row'
    off = 0
    for i, (o, (r, k)) in enumerate(zip(dws, shapes)):
        key = 'dw%d' % (i + 1)
        rv, rt = (ref[key].v, ref[key].t) if live else (np.zeros((r, k)), np.zeros((r, k)))
        if fold:
            _note(name, entry, key, R.check(o.get(), rv, rt, r, k, k, tol, what + ' ' + key))
            res[key] = R.split(o.get(), r, k, k)[0].copy()
        else:
            assert o.unchanged(), what + ': %s written by a call that was given none' % key
            part = rows[:, off:off + r * k].astype(np.float64).sum(0).reshape(r, k)      # the float64 sum of the partial rows
            e = R.errors(part, rv, rt)
            assert e[0] <= tol and (np.abs(part - rv) <= tol * rt + 1e-30).all(), (what, key, e)
            _note(name, entry + ' nofold', key, e)
        off += r * k
    if gin:
        _note(name, entry, 'gin', R.check(g.get(), ref['gin'].v, ref['gin'].t, E, S, S, tol, what + ' gin'))
        res['gin'] = R.split(g.get(), E, S, S)[0].copy()
        assert not res['gin'][c['zero']].any(), what + ': the gin row of a zero support row is not zero'
    if kind == 'zeros' and fold:
        assert not any(res['dw%d' % i].any() for i in (1, 2, 3, 4)), what + ': dw of a batch of zero rows is not exactly zero'
    RAN.add((name, 'bwd', S, 0))
    return res


@pytest.mark.parametrize('S', SS)
def test_backward(dev, S):
    """gml_edge_mlp_bwd (ea_split x gin), _bwd_exact (gin or not), _bwd_sym and _bwd_sym_dev (capacity U + 5, slack slots at the guard
    rows) at every boundary size"""
    for E in E_SMALL:
        for split in (0, 1):
            for gin in (0, 1):
                run_bwd(dev, 'bwd', S, E, split=split, gin=gin)
        for gin in (0, 1):
            run_bwd(dev, 'exact', S, E, gin=gin)
        run_bwd(dev, 'sym', S, E)
        run_bwd(dev, 'sym_dev', S, E, slack=5)


# ------------------------------------------------------------------------------------------------------------------------- grid caps
def _cap_fwd(fam):
    per, groups = CAPS_FWD[fam]
    return per * groups


@pytest.mark.parametrize('name,entry,S,kw', [
    ('chain', 'fwd', 4, dict(split=1, dual=1)), ('chain', 'fwd', 4, dict(split=0)), ('chain stack', 'stack', 4, dict(L=2)),
    ('chain16', 'fwd', 12, dict(split=1)), ('valu', 'fwd', 1, {}), ('chain6', 'fwd6', 4, {}), ('chain6', 'stack6', 4, dict(L=2)),
    ('chain16x6', 'fwd6', 12, dict(dual=1)), ('sym6', 'sym', 4, dict(L=2, kind='none')), ('sym16x6', 'sym_dev', 12, dict(L=1, kind='none'))],
    ids=lambda v: str(v) if not isinstance(v, dict) else ','.join('%s=%s' % kv for kv in sorted(v.items())) or '-')
def test_forward_at_the_grid_cap(dev, name, entry, S, kw):
    """the E at which the launcher's grid reaches its cap (every workgroup one trip) and that E + 1 (one workgroup a second trip);
    unique rows: a list without mirrors, so that the entries are the edges"""
    cap = _cap_fwd(name)
    for E in (cap, cap + 1):
        assert run_fwd(dev, entry, S, E, **kw) is not None
        fam = name.split()[0]
        assert (fam, 'fwd', S, kw.get('L', 0)) in RAN
    TRIPS.add((name, 'fwd'))


@pytest.mark.parametrize('name,entry,S,kw', [
    ('chain', 'bwd', 4, dict(split=1, gin=1)), ('chain16', 'bwd', 12, dict(split=1)), ('valu', 'bwd', 1, dict(gin=1)),
    ('sym_chain', 'sym', 4, dict(kind='none')), ('sym_chain16', 'sym_dev', 12, dict(kind='none'))],
    ids=lambda v: str(v) if not isinstance(v, dict) else ','.join('%s=%s' % kv for kv in sorted(v.items())))
def test_backward_at_the_grid_cap(dev, name, entry, S, kw):
    """the same for the backward; the cap is the library's own answer: parts(E) reaches CAPS_BWD at exactly this E and stays there
    for E + 1, whose extra trip's worth of edges (64) no longer has a workgroup of its own"""
    per, cap = CAPS_BWD[name]
    E = per * cap
    q = (lambda n: int(G.lib().gml_edge_mlp_bwd_sym_parts(n, S))) if entry.startswith('sym') else \
        (lambda n: int(G.lib().gml_edge_mlp_bwd_parts(n, S, S, kw.get('split', 0), kw.get('gin', 0))))
    step = _valu_waves(S) if name == 'valu' else 1           # (the one-edge-per-lane grid grows by whole workgroups)
    assert q(E) == cap and q(E - per * step) == cap - step, (name, q(E), q(E - per * step), cap)
    assert q(E + 1) == cap and _cdiv(E + 1, per) == cap + 1, 'E + 1 no longer needs a second trip: the launch geometry changed'
    for n in (E, E + 1):
        r = run_bwd(dev, entry, S, n, **kw)
        assert r is not None and r['parts'] == cap
    TRIPS.add((name, 'bwd'))


def test_workspace_query_covers_every_family():
    """gml_edge_mlp_bwd_workspace_bytes is what callers allocate: at least every family's partial rows, at the cap too"""
    Lb = G.lib()
    assert int(Lb.gml_edge_mlp_bwd_parts(64 * 6 * NCU, 4, 4, 1, 0)) == 6 * NCU, 'GML_NUM_CU is no longer %d' % NCU
    for S in SS:
        for E in E_SMALL + (E_MULTI, 64 * 8 * NCU + 1):
            need = max(int(Lb.gml_edge_mlp_bwd_parts(E, S, S, sp, gi)) for sp in (0, 1) for gi in (0, 1))
            need = max(need, int(Lb.gml_edge_mlp_bwd_sym_parts(E, S)), _valu_parts(S, E))
            if S == 1 or S > 8:                              # gin without the image: the one-edge-per-lane family answers
                assert int(Lb.gml_edge_mlp_bwd_parts(E, S, S, 0, 1)) == _valu_parts(S, E), (S, E)
            assert int(Lb.gml_edge_mlp_bwd_workspace_bytes(E, S, S)) >= need * 10 * S * S * 4, (S, E)


# ------------------------------------------------------------------------------------------------------------------------- conditions
# one representative per backward family: (entry, S, keywords)
BWD_FAMS = [('bwd', 1, dict(gin=1)), ('bwd', 4, dict(split=1, gin=1)), ('bwd', 3, dict()), ('bwd', 12, dict(split=1)),
            ('bwd', 12, dict(split=1, gin=1)), ('sym', 4, dict()), ('sym', 12, dict()), ('sym_dev', 6, dict(slack=5)), ('sym_dev', 16, dict(slack=5))]
_ids = lambda v: str(v) if not isinstance(v, dict) else ','.join('%s=%s' % kv for kv in sorted(v.items())) or '-'


def _fold_many(dev, ws_rows, S):
    """gml_fold_many of partial rows [parts, 10 S^2] into fresh guarded dw1 .. dw4; returns the four arrays"""
    parts, NW = ws_rows.shape
    src = _up(ws_rows, dev)
    shapes = [(2 * S, S)] * 3 + [(S, 4 * S)]
    dws = [_Out(dev, r, k, k) for r, k in shapes]
    job = (G.FoldJob * 1)()
    job[0].partial, job[0].nparts, job[0].n = src.data_ptr(), parts, NW
    for k, (o, (r, kk)) in enumerate(zip(dws, shapes)):
        job[0].dst[k], job[0].ndst[k] = o.ptr().value, r * kk
    job[0].dst[4], job[0].ndst[4] = None, 0
    assert _done(G.lib().gml_fold_many(ctypes.addressof(job), 1, _st(dev))) == OK
    out = []
    for o, (r, k) in zip(dws, shapes):
        v, guards = R.split(o.get(), r, k, k)
        assert (guards == R.SENTINEL).all(), 'gml_fold_many wrote behind a destination'
        out.append(v.copy())
    return out


@pytest.mark.parametrize('E', [33, E_MULTI])
@pytest.mark.parametrize('entry,S,kw', BWD_FAMS, ids=_ids)
def test_deferred_fold(dev, entry, S, kw, E):
    """dw1 .. dw4 = NULL: exactly `parts` rows of 10 S^2 floats are written and nothing behind them (run_bwd), their float64 sum meets
    the bars, and gml_fold_many of them is bitwise the dw of the folding call -- which is itself bitwise repeatable"""
    a = run_bwd(dev, entry, S, E, **kw)
    b = run_bwd(dev, entry, S, E, **kw)
    n = run_bwd(dev, entry, S, E, fold=False, **kw)
    assert _same(a['ws'], n['ws']), 'the partial rows depend on whether the call folds them'
    for k in a:
        if k != 'parts':
            assert _same(a[k], b[k]), (entry, S, E, k, 'two launches differ')
    folded = _fold_many(dev, n['ws'], S)
    for i in range(4):
        assert _same(folded[i], a['dw%d' % (i + 1)]), (entry, S, E, 'dw%d' % (i + 1), 'gml_fold_many differs from the folding call')


@pytest.mark.parametrize('E', [33, E_MULTI])
@pytest.mark.parametrize('entry,S,kw', BWD_FAMS + [('exact', 5, dict(gin=1)), ('exact', 16, dict())], ids=_ids)
def test_workspace_one_byte_short(dev, entry, S, kw, E):
    """ws_bytes one byte below `parts` rows: GML_E_WORKSPACE before any launch (every launcher compares ws_bytes with grid * NW floats
    ahead of its hipLaunchKernelGGL: gml_edge_mlp_impl.h, gml_edge_chain_impl.h, gml_edge_chain16_impl.h, gml_edge_chain_sym.hip),
    every output bit-unchanged"""
    assert run_bwd(dev, entry, S, E, short=1, expect=WSP, **kw) is None
    assert run_bwd(dev, entry, S, E, short=1, fold=False, expect=BAD if entry == 'exact' else WSP, **kw) is None


@pytest.mark.parametrize('S', [1, 4, 12])
def test_zero_edges(dev, S):
    """num_edges = 0: GML_OK, no output touched -- except the folding backward's dw, which become zeros"""
    Lb, st = G.lib(), _st(dev)
    d = dcase(dev, S, 17)
    w = [_p(t) for t in d['ws'][0]]
    out, out_t, g, ws = _Out(dev, 4, S, S), _Out(dev, 4, S, S), _Out(dev, 4, S, S), _flat(dev, 10 * S * S)
    one = (*w, out.ptr(), _p(d['tpos']), out_t.ptr(), 0, S, S, st)
    assert _done(Lb.gml_edge_mlp_fwd(_p(d['ea']), _p(d['es']), *one)) == OK
    assert _done(Lb.gml_edge_mlp_fwd_exact(_p(d['ea']), *one)) == OK
    assert _done(Lb.gml_edge_mlp_fwd6(_p(d['ea']), *one)) == (OK if S >= 2 else UNS)
    wl = [_arr([w[i]] * 2) for i in range(4)]
    oa = _arr([out.ptr(), out_t.ptr()])
    if S == 4:
        assert _done(Lb.gml_edge_mlp_fwd_stack(_p(d['es']), 2, *wl, oa, 0, S, S, st)) == OK
        assert _done(Lb.gml_edge_mlp_fwd_stack6(_p(d['ea']), 2, *wl, oa, 0, S, S, st)) == OK
        assert _done(Lb.gml_edge_mlp_fwd_stack6_sym(_p(d['ea']), _p(d['uid']), _p(d['mir']), 0, 2, *wl, oa, 0, S, S, st)) == OK
    assert _done(Lb.gml_edge_presplit(_p(d['ea']), out.ptr(), 0, S, st)) == OK
    assert out.unchanged() and out_t.unchanged()
    shapes = [(2 * S, S)] * 3 + [(S, 4 * S)]
    for entry in ('bwd', 'exact', 'nofold'):
        dws = [_Out(dev, r, k, k) for r, k in shapes]
        dwp = [_p(None)] * 4 if entry == 'nofold' else [o.ptr() for o in dws]
        tail = (*dwp, 0, S, S, ws.ptr(), 10 * S * S * 4, st)
        if entry == 'exact':
            rc = Lb.gml_edge_mlp_bwd_exact(_p(d['ea']), *w, _p(d['gout']), g.ptr(), *tail)
        else:
            rc = Lb.gml_edge_mlp_bwd(_p(d['ea']), _p(d['es']), *w, _p(d['gout']), g.ptr(), *tail)
        assert _done(rc) == OK, entry
        assert g.unchanged() and ws.unchanged(), entry
        for o, (r, k) in zip(dws, shapes):
            if entry == 'nofold':
                assert o.unchanged()
            else:
                z = np.zeros((r, k))
                R.check(o.get(), z, z, r, k, k, TOL, 'num_edges = 0: dw')
    assert int(Lb.gml_edge_mlp_bwd_parts(0, S, S, 1, 0)) == 0


@pytest.mark.parametrize('E', [64, E_MULTI])
@pytest.mark.parametrize('kind', ['none', 'all', 'adjacent', 'mixed', 'zeros'])
@pytest.mark.parametrize('S', [4, 7, 12])
def test_unique_row_lists(dev, S, kind, E):
    """the unique-row forward and backward over lists without mirrors, with every entry mirrored (far apart / in the same tile) and
    mixed; the forward is bitwise gml_edge_mlp_fwd_stack6 resp. gml_edge_mlp_fwd6 on the same rows (the mirrors are bitwise copies);
    the device-counted forms with count = U < capacity are bitwise the host-counted ones; a batch of zero rows gives dw = 0 exactly"""
    L = 2 if S == 4 else 1
    sym = run_fwd(dev, 'sym', S, E, L=L, kind=kind)
    symd = run_fwd(dev, 'sym_dev', S, E, L=L, kind=kind, slack=7)
    plain = run_fwd(dev, 'stack6', S, E, L=L, kind=kind) if S == 4 else run_fwd(dev, 'fwd6', S, E, kind=kind)
    for l in range(L):
        assert _same(sym[l], plain[l]) and _same(symd[l], plain[l]), (S, kind, E, l)
    U = case(S, E, kind)['uid'].size
    q = lambda n: int(G.lib().gml_edge_mlp_bwd_sym_parts(n, S))
    slack = max([k for k in range(0, min(7, E - U) + 1) if q(U + k) == q(U)])      # the same grid: the same partial rows, the same fold
    a, b = run_bwd(dev, 'sym', S, E, kind=kind), run_bwd(dev, 'sym_dev', S, E, kind=kind, slack=slack)
    for k in ('ws', 'dw1', 'dw2', 'dw3', 'dw4'):
        assert _same(a[k], b[k]), (S, kind, E, k)
    if kind == 'zeros':
        run_bwd(dev, 'bwd', S, E, kind=kind, split=1, gin=S <= 8)
        run_bwd(dev, 'exact', S, E, kind=kind, gin=1)


@pytest.mark.parametrize('S,E', [(4, 1), (4, 2), (12, 1), (12, 2), (5, 2)])
def test_unique_row_list_of_one(dev, S, E):
    """U = 1: one edge alone (E = 1), one entry and its mirror (E = 2)"""
    kind = 'all' if E == 2 else 'none'
    assert case(S, E, kind)['uid'].size == 1
    for entry in ('sym', 'sym_dev'):
        assert run_fwd(dev, entry, S, E, L=1, kind=kind, slack=2) is not None
        assert run_bwd(dev, entry, S, E, kind=kind, slack=2) is not None


@pytest.mark.parametrize('S,E', [(4, 33), (4, E_MULTI), (12, 33), (12, E_MULTI)])
def test_device_count_empty_and_clamped(dev, S, E):
    """*count = 0: the forward writes nothing, the backward leaves zeros in all parts(capacity) partial rows and dw = 0;
    *count > capacity is clamped to capacity (capacity = U: no slack slot exists to walk) and is bitwise the host-counted call"""
    L = 2 if S == 4 else 1
    U = case(S, E)['uid'].size
    run_fwd(dev, 'sym_dev', S, E, L=L, count=0, slack=5)
    run_bwd(dev, 'sym_dev', S, E, count=0, slack=5)
    run_bwd(dev, 'sym_dev', S, E, count=0, slack=5, fold=False)
    host = run_fwd(dev, 'sym', S, E, L=L)
    big = run_fwd(dev, 'sym_dev', S, E, L=L, count=U + 3, slack=0)
    assert all(_same(x, y) for x, y in zip(host, big))
    a, b = run_bwd(dev, 'sym', S, E), run_bwd(dev, 'sym_dev', S, E, count=U + 3)
    for k in ('ws', 'dw1', 'dw2', 'dw3', 'dw4'):
        assert _same(a[k], b[k]), (S, E, k)


@pytest.mark.parametrize('S', [4, 12])
def test_device_capacity_beyond_the_lists_grid(dev, S):
    """the 64 entries of 96 edges fill one workgroup; a capacity of 72 launches a second one, which finds no entry: the first partial
    row is bitwise the host-counted call's, the second is zeros (gml.h: "zeros where a workgroup has no entry"), the slack slots are
    not walked"""
    q = lambda n: int(G.lib().gml_edge_mlp_bwd_sym_parts(n, S))
    assert case(S, 96)['uid'].size == 64 and (q(64), q(72)) == (1, 2), 'the launch geometry changed: choose the list length anew'
    a, w = run_bwd(dev, 'sym', S, 96), run_bwd(dev, 'sym_dev', S, 96, slack=8)
    assert (a['parts'], w['parts']) == (1, 2) and _same(w['ws'][:1], a['ws']) and not w['ws'][1:].any()
    n = run_bwd(dev, 'sym_dev', S, 96, slack=8, fold=False)
    assert _same(n['ws'], w['ws'])


@pytest.mark.parametrize('E', [33, E_MULTI])
@pytest.mark.parametrize('S', [4, 8])
def test_stack_equals_single_layer_calls(dev, S, E):
    """gml.h: "same results either way" -- a stack of L layers is bitwise L single-layer calls of the same arithmetic"""
    Lb, st = G.lib(), _st(dev)
    d = dcase(dev, S, E)
    for L in (2, 3, 4):
        two, six = run_fwd(dev, 'stack', S, E, L=L), run_fwd(dev, 'stack6', S, E, L=L)
        for l in range(L):
            w = [_p(t) for t in d['ws'][l]]
            for entry, stack in (('fwd', two), ('fwd6', six)):
                o = _Out(dev, E, S, S)
                tail = (*w, o.ptr(), _p(None), _p(None), E, S, S, st)
                rc = Lb.gml_edge_mlp_fwd(_p(d['ea']), _p(d['es']), *tail) if entry == 'fwd' else Lb.gml_edge_mlp_fwd6(_p(d['ea']), *tail)
                assert _done(rc) == OK
                v, guards = R.split(o.get(), E, S, S)
                assert (guards == R.SENTINEL).all()
                assert _same(v, stack[l]), (entry, S, E, L, l)


@pytest.mark.parametrize('S', [1, 2, 5, 8, 11, 16])
def test_two_launches_are_bitwise_equal(dev, S):
    """no atomics, a fixed fold order: fresh buffers, the same bits, forward and backward (the chains' backward: test_deferred_fold too)"""
    for E in (33, E_MULTI):
        for entry, kw in (('fwd', dict(split=1, dual=1)), ('fwd', dict()), ('fwd6', dict()), ('exact', dict(dual=1))):
            a, b = run_fwd(dev, entry, S, E, **kw), run_fwd(dev, entry, S, E, **kw)
            assert (a is None) == (b is None) and (a is None or _same(a[0], b[0])), (entry, S, E)
        for entry, kw in (('bwd', dict(split=1)), ('bwd', dict(gin=1)), ('exact', dict(gin=1)), ('sym', dict())):
            a, b = run_bwd(dev, entry, S, E, **kw), run_bwd(dev, entry, S, E, **kw)
            assert (a is None) == (b is None), (entry, S, E)
            for k in (a or {}):
                assert k == 'parts' or _same(a[k], b[k]), (entry, S, E, k)


# ------------------------------------------------------------------------------------------------------------------------- presplit
def _special_rows(S, E, seed):
    """rows of normal draws with the values a split can get wrong: +-0, denormals, 1 +- 2^-23, the largest magnitudes whose bf16
    rounding stays finite"""
    rng = _rng('presplit', S, E, seed)
    x = _f32(rng.standard_normal((E, S)) * 0.7)
    sp = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -5.9e-39, 1 + 2.0 ** -23, 1 - 2.0 ** -23, -1 - 2.0 ** -23, 3.0e38, -3.0e38,
                   np.float32(2.0 ** 127), 65280.0, 2.0 ** -126], np.float32)
    flat = x.ravel()
    pos = rng.choice(flat.size, size=min(sp.size, flat.size), replace=False)
    flat[pos] = sp[:pos.size]
    return flat.reshape(E, S)


def _unsplit(img, S):
    """(hi, lo) [E, W] float32 of a pre-split image [E, W words]: word j = bf16 pair (2j, 2j + 1), low half first; hi words, then lo"""
    W = img.shape[1]
    img = img.view(np.uint32)
    halves = []
    for part in (img[:, :W // 2], img[:, W // 2:]):
        v = np.empty((img.shape[0], W), np.uint32)
        v[:, 0::2], v[:, 1::2] = part << np.uint32(16), part & np.uint32(0xffff0000)
        halves.append(v.view(np.float32))
    return halves


def _check_split(img, x, S, what):
    hi, lo = _unsplit(img, S)
    assert not hi[:, S:].view(np.uint32).any() and not lo[:, S:].view(np.uint32).any(), what + ': columns >= S of the image are not zero'
    back = hi[:, :S].astype(np.float64) + lo[:, :S].astype(np.float64)
    assert np.isfinite(back).all(), what
    err = np.abs(back - x.astype(np.float64))
    # hi truncates to 8 significant bits (residual < 2^-7 |x|), lo rounds the residual to 8 more (to 2^-9 of it): 2^-16 |x|.  Below
    # 2^-126 the hardware may flush a denormal piece: an absolute 2^-126 covers it
    assert (err <= 2.0 ** -16 * np.abs(x) + 2.0 ** -126).all(), (what, float((err / np.maximum(np.abs(x), 1e-300)).max()))


@pytest.mark.parametrize('S', SS)
def test_presplit(dev, S):
    """gml_edge_presplit, both row widths: hi + lo reconstructs every value to 2^-16 relative, the columns S .. 7 (S .. 15) are zero,
    the 8 rows behind the image are untouched"""
    W = 8 if S <= 8 else 16
    for E in (1, 255, 256, 257):
        x = _special_rows(S, E, 0)
        img, xd = _Out(dev, E, W, W), _up(x, dev)
        assert _done(G.lib().gml_edge_presplit(_p(xd), img.ptr(), E, S, _st(dev))) == OK
        v, guards = R.split(img.get(), E, W, W)
        assert (guards == R.SENTINEL).all(), 'presplit S=%d E=%d wrote behind its image' % (S, E)
        _check_split(v, x, S, 'presplit S=%d E=%d' % (S, E))


@pytest.mark.parametrize('S', range(1, 9))
def test_gather_rows_presplit_equals_gather_then_presplit(dev, S):
    """gml_gather_rows_presplit is bitwise gml_gather_rows followed by gml_edge_presplit, guards behind both outputs intact"""
    Lb, st = G.lib(), _st(dev)
    for E in (1, 255, 256, 257):
        x = _special_rows(S, E, 1)
        perm = _rng('perm', S, E).integers(0, E, E).astype(np.int32)          # (a gather: rows may repeat)
        xd, pd = _up(x, dev), _up(perm, dev)
        o1, i1, o2, i2 = _Out(dev, E, S, S), _Out(dev, E, 8, 8), _Out(dev, E, S, S), _Out(dev, E, 8, 8)
        assert _done(Lb.gml_gather_rows_presplit(_p(xd), _p(pd), o1.ptr(), i1.ptr(), E, S, st)) == OK
        assert _done(Lb.gml_gather_rows(_p(xd), _p(pd), o2.ptr(), E, S, st)) == OK
        assert _done(Lb.gml_edge_presplit(o2.ptr(), i2.ptr(), E, S, st)) == OK
        assert _same(o1.get(), o2.get()) and _same(i1.get(), i2.get()), (S, E)
        v, guards = R.split(o1.get(), E, S, S)
        assert (guards == R.SENTINEL).all() and _same(v, x[perm])
        assert (R.split(i1.get(), E, 8, 8)[1] == R.SENTINEL).all()
        _check_split(R.split(i1.get(), E, 8, 8)[0], x[perm], S, 'gather_rows_presplit S=%d E=%d' % (S, E))


# ------------------------------------------------------------------------------------------------------------------------- wide
WIDE = [(17, 17), (20, 47), (33, 20), (24, 24), (48, 48)]


@functools.lru_cache(maxsize=None)
def _wide_case(S, So, E):
    from oracle.relu_margin import make_safe_edges
    g = torch.Generator().manual_seed(100 * S + So + E)
    ws = [torch.randn(2 * S, S, generator=g) * 0.7 for _ in range(3)] + [torch.randn(So, 4 * S, generator=g) * 0.5]
    ea = make_safe_edges(torch.randn(E, S, generator=g) * 0.7, *ws, scale=0.7, generator=g).numpy()
    zero = [0, E // 2, E - 1] if E >= 8 else []
    ea[zero] = 0.0
    gout = torch.randn(E, So, generator=g).numpy()
    ws = [_f32(t.numpy()) for t in ws]
    return dict(ea=_f32(ea), ws=ws, gout=_f32(gout), zero=zero, fwd=ER.edge_fwd_ref(ea, *ws), bwd=ER.edge_bwd_ref(ea, *ws, gout, wide=True))


@pytest.mark.parametrize('S,So', WIDE)
def test_wide_forward_and_backward(dev, S, So):
    """gml_edge_mlp_wide_fwd and gml_edge_mlp_wide_bwd (one edge per lane, exact fp32 products: the 2e-5 bar) with rows that are and
    are not multiples of 4 floats, around the 512-edge block.  The backward is given the reference's out (its relu pattern is an
    input).  hid and gz rows pad each block of 2 S to H2R columns: the pad columns come from zero weight rows and must be zero (to
    the tanh's 1e-4 absolute where a tanh product lands there)."""
    Lb, st = G.lib(), _st(dev)
    H2, H2R = 2 * S, int(Lb.gml_edge_mlp_wide_bwd_h2r(S))
    assert H2R == (H2 + 3) // 4 * 4
    for E in E_SMALL + (511, 512, 513):
        c = _wide_case(S, So, E)
        what = 'wide S=%d So=%d E=%d' % (S, So, E)
        ea, gout, wd = _up(c['ea'], dev), _up(c['gout'], dev), [_up(t, dev) for t in c['ws']]
        w = [_p(t) for t in wd]
        out = _Out(dev, E, So, So)
        assert _done(Lb.gml_edge_mlp_wide_fwd(_p(ea), *w, out.ptr(), E, S, So, st)) == OK, what
        f = c['fwd']
        _note('wide', 'wide_fwd', 'out', R.check(out.get(), f.v, f.t, E, So, So, TOL_F32, what + ' out'))
        assert not _bits(R.split(out.get(), E, So, So)[0][c['zero']]).any(), what + ': the out row of a zero support row is not +0.0'
        go, hid, gz = _Out(dev, E, So, So), _Out(dev, E, 2 * H2R, 2 * H2R), _Out(dev, E, 3 * H2R, 3 * H2R)
        oref = _up(_f32(f.v), dev)
        assert _done(Lb.gml_edge_mlp_wide_bwd(_p(ea), *w, _p(oref), _p(gout), go.ptr(), hid.ptr(), gz.ptr(), E, S, So, st)) == OK, what
        b = c['bwd']

        def padded(r, tanh_blocks):
            nb = r.v.shape[1]
            v, t = np.zeros((E, nb, H2R)), np.zeros((E, nb, H2R))
            v[:, :, :H2], t[:, :, :H2] = r.v, r.t
            for k in tanh_blocks:
                t[:, k, H2:] = 1.0
            return v.reshape(E, nb * H2R), t.reshape(E, nb * H2R)
        _note('wide', 'wide_bwd', 'go', R.check(go.get(), b['go'].v, b['go'].t, E, So, So, TOL_F32, what + ' go'))
        _note('wide', 'wide_bwd', 'hid', R.check(hid.get(), *padded(b['hid'], (1,)), E, 2 * H2R, 2 * H2R, TOL_F32, what + ' hid'))
        _note('wide', 'wide_bwd', 'gz', R.check(gz.get(), *padded(b['gz'], ()), E, 3 * H2R, 3 * H2R, TOL_F32, what + ' gz'))
        for o, n in ((go, So), (hid, 2 * H2R), (gz, 3 * H2R)):
            assert not R.split(o.get(), E, n, n)[0][c['zero']].any(), what + ': a zero support row gives a non-zero backward row'
    RAN.add(('wide', 'fwd', S, So))


# ------------------------------------------------------------------------------------------------------------------------- error answers
def _fwd_call(dev, entry, S, So, E=17, **over):
    """a single-layer forward call on guarded outputs with one argument replaced; returns (rc, outputs unchanged)"""
    Lb, st = G.lib(), _st(dev)
    d = dcase(dev, S if 1 <= S <= 16 else 16, 17)
    out, out_t = _Out(dev, 17, So, So), _Out(dev, 17, So, So)
    a = dict(ea=_p(d['ea']), es=_p(d['es']), w1=_p(d['ws'][0][0]), w2=_p(d['ws'][0][1]), w3=_p(d['ws'][0][2]), w4=_p(d['ws'][0][3]),
             out=out.ptr(), tpos=_p(d['tpos']), out_t=out_t.ptr())
    a.update(over)
    tail = (a['w1'], a['w2'], a['w3'], a['w4'], a['out'], a['tpos'], a['out_t'], E, S, So, st)
    rc = {'fwd': lambda: Lb.gml_edge_mlp_fwd(a['ea'], a['es'], *tail), 'fwd6': lambda: Lb.gml_edge_mlp_fwd6(a['ea'], *tail),
          'exact': lambda: Lb.gml_edge_mlp_fwd_exact(a['ea'], *tail)}[entry]()
    return _done(rc), out.unchanged() and out_t.unchanged()


def _off(p, nbytes=4):
    return ctypes.c_void_p(p.value + nbytes)


@pytest.mark.parametrize('entry', ['fwd', 'fwd6', 'exact'])
def test_forward_error_answers(dev, entry):
    """every documented refusal happens on the host, before any launch (csrc/gml_edge_mlp.hip, gml_edge_chain6_a.hip: the checks
    precede the dispatch): the return code, and every output bit-unchanged"""
    NULL = _p(None)
    d = dcase(dev, 4, 17)
    assert _fwd_call(dev, entry, 4, 4) == (OK, False)
    assert _fwd_call(dev, entry, 4, 5) == (UNS, True)                        # S != Sout
    assert _fwd_call(dev, entry, 17, 17) == (UNS, True)                      # S > 16: gml_edge_mlp_wide_fwd's range
    assert _fwd_call(dev, entry, 0, 4) == (BAD, True) and _fwd_call(dev, entry, 4, 4, E=-1) == (BAD, True)
    for k in ('ea', 'w1', 'w2', 'w3', 'w4', 'out'):                          # a NULL among the required pointers
        assert _fwd_call(dev, entry, 4, 4, **{k: NULL}) == (BAD, True), k
    assert _fwd_call(dev, entry, 4, 4, tpos=NULL) == (BAD, True)             # out_t without tpos
    for k in ('ea', 'out', 'out_t') + (('es',) if entry == 'fwd' else ()):   # 4 bytes off where the entry checks & 15
        assert _fwd_call(dev, entry, 4, 4, **{k: _off(_p(d[k]) if k in d else _Out(dev, 18, 4, 4).ptr())}) == (BAD, True), k
    if entry == 'fwd6':
        assert _fwd_call(dev, entry, 1, 1) == (UNS, True)                    # the three-piece chains start at S = 2


def test_stack_error_answers(dev):
    """the stacks: a shape or layer count the plan refuses, NULL arrays and entries, misaligned ea / ea_split / out[l]; the unique-row
    forms: num_unique = 0 or > num_edges, NULL lists, a NULL count"""
    Lb, st = G.lib(), _st(dev)
    S, E, NULL = 4, 17, _p(None)
    d = dcase(dev, S, E)
    w = d['ws']

    def call(entry, L=2, S_=S, So=S, U=None, **over):
        outs = [_Out(dev, E, So, So) for _ in range(max(L, 1))]
        a = dict(ea=_p(d['ea']), es=_p(d['es']), uid=_p(d['uid']), mir=_p(d['mir']), cnt=_p(d['cnt']),
                 wl=[_arr([_p(w[l % 4][i]) for l in range(max(L, 1))]) for i in range(4)], oa=_arr([o.ptr() for o in outs]))
        a.update(over)
        U = d['uid'].numel() if U is None else U
        if entry == 'stack':
            rc = Lb.gml_edge_mlp_fwd_stack(a['es'], L, *a['wl'], a['oa'], E, S_, So, st)
        elif entry == 'stack6':
            rc = Lb.gml_edge_mlp_fwd_stack6(a['ea'], L, *a['wl'], a['oa'], E, S_, So, st)
        elif entry == 'sym':
            rc = Lb.gml_edge_mlp_fwd_stack6_sym(a['ea'], a['uid'], a['mir'], U, L, *a['wl'], a['oa'], E, S_, So, st)
        else:
            rc = Lb.gml_edge_mlp_fwd_stack6_sym_dev(a['ea'], a['uid'], a['mir'], a['cnt'], U, L, *a['wl'], a['oa'], E, S_, So, st)
        return _done(rc), all(o.unchanged() for o in outs)

    for entry in ('stack', 'stack6', 'sym', 'sym_dev'):
        assert call(entry, L=5) == (UNS, True) and call(entry, S_=4, So=5) == (UNS, True) and call(entry, L=0) == (BAD, True), entry
        assert call(entry, S_=6, So=6) == (UNS, True), entry                 # stacks: S in {4, 8}
        assert call(entry, wl=[NULL] * 4) == (BAD, True) and call(entry, oa=NULL) == (BAD, True), entry
        assert call(entry, oa=_arr([_Out(dev, E, S, S).ptr(), NULL])) == (BAD, True), entry
        assert call(entry, oa=_arr([_Out(dev, E, S, S).ptr(), _off(_Out(dev, E + 1, S, S).ptr())])) == (BAD, True), entry
        src = 'es' if entry == 'stack' else 'ea'
        assert call(entry, **{src: NULL}) == (BAD, True) and call(entry, **{src: _off(_p(d[src]))}) == (BAD, True), entry
    assert call('stack', L=1) == (UNS, True)                                 # the two-piece stack starts at two layers
    for entry in ('sym', 'sym_dev'):
        assert call(entry, uid=NULL) == (BAD, True) and call(entry, mir=NULL) == (BAD, True), entry
        assert call(entry, U=E + 1) == (BAD, True), entry
    assert call('sym', U=0) == (BAD, True) and call('sym_dev', U=0) == (BAD, True) and call('sym_dev', cnt=NULL) == (BAD, True)


@pytest.mark.parametrize('entry', ['bwd', 'exact', 'sym', 'sym_dev'])
def test_backward_error_answers(dev, entry):
    """the backward's refusals, all ahead of the dispatch (csrc/gml_edge_mlp.hip, gml_edge_chain_sym.hip): S != Sout, S > 16, a NULL
    among the required pointers, some but not all of dw NULL, pointers 4 bytes off where the entry checks & 15"""
    Lb, st = G.lib(), _st(dev)
    E, NULL = 17, _p(None)

    def call(S=4, So=4, U=None, **over):
        d = dcase(dev, min(S, 16), E)
        shapes = [(2 * S, S)] * 3 + [(So, 4 * S)]
        dws = [_Out(dev, r, k, k) for r, k in shapes]
        g, ws = _Out(dev, E, S, S), _flat(dev, 8 * 10 * S * S)   # (E = 17: at most 4 partial rows on any family)
        a = dict(ea=_p(d['ea']), es=_p(d['es']), uid=_p(d['uid']), mir=_p(d['mir']), cnt=_p(d['cnt']), gout=_p(d['gout']), gin=g.ptr(),
                 ws=ws.ptr(), **{'w%d' % (i + 1): _p(d['ws'][0][i]) for i in range(4)}, **{'dw%d' % (i + 1): dws[i].ptr() for i in range(4)})
        a.update(over)
        U_ = d['uid'].numel() if U is None else U
        wq = [a['w1'], a['w2'], a['w3'], a['w4']]
        tail = (a['dw1'], a['dw2'], a['dw3'], a['dw4'], E, S, So, a['ws'], 8 * 10 * S * S * 4, st)
        if entry == 'bwd':
            rc = Lb.gml_edge_mlp_bwd(a['ea'], a['es'], *wq, a['gout'], a['gin'], *tail)
        elif entry == 'exact':
            rc = Lb.gml_edge_mlp_bwd_exact(a['ea'], *wq, a['gout'], a['gin'], *tail)
        elif entry == 'sym':
            rc = Lb.gml_edge_mlp_bwd_sym(a['es'], a['uid'], a['mir'], U_, *wq, a['gout'], *tail)
        else:
            rc = Lb.gml_edge_mlp_bwd_sym_dev(a['es'], a['uid'], a['mir'], a['cnt'], U_, *wq, a['gout'], *tail)
        return _done(rc), all(o.unchanged() for o in dws) and g.unchanged() and ws.unchanged()

    sym = entry.startswith('sym')
    assert call()[0] == OK
    assert call(So=5) == (UNS, True) and call(S=17, So=17) == (UNS, True)
    required = ('w1', 'w2', 'w3', 'w4', 'gout', 'ws') + (('es', 'uid', 'mir') if sym else ('ea',))
    for k in required:
        assert call(**{k: NULL}) == (BAD, True), k
    for k in ('dw1', 'dw2', 'dw3', 'dw4'):                                   # some but not all of dw NULL
        assert call(**{k: NULL}) == (BAD, True), k
        assert call(**{j: NULL for j in ('dw1', 'dw2', 'dw3', 'dw4') if j != k}) == (BAD, True), k
    if entry == 'exact':                                                     # no deferred fold on the exact entry
        assert call(dw1=NULL, dw2=NULL, dw3=NULL, dw4=NULL) == (BAD, True)
    d = dcase(dev, 4, E)
    for k in (('es', 'gout') if sym else ('ea', 'gout', 'gin') + (('es',) if entry == 'bwd' else ())):
        assert call(**{k: _off(_p(d[k]) if k in d else _Out(dev, E + 1, 4, 4).ptr())}) == (BAD, True), k
    if sym:
        assert call(U=0) == (BAD, True) and call(U=E + 1) == (BAD, True) and call(S=1, So=1) == (UNS, True)
    if entry == 'sym_dev':
        assert call(cnt=NULL) == (BAD, True)


def test_wide_and_presplit_error_answers(dev):
    """gml_edge_mlp_wide_fwd / _bwd: max(S, Sout) <= 16 or > 48, NULL pointers, rows of 4-float multiples off their alignment;
    gml_edge_presplit / gml_gather_rows_presplit: S beyond their widths, NULL, a misaligned image"""
    Lb, st = G.lib(), _st(dev)
    E, NULL = 17, _p(None)
    c = _wide_case(24, 24, E)
    ea, gout, w = _up(c['ea'], dev), _up(c['gout'], dev), [_up(t, dev) for t in c['ws']]
    keep = [ea, gout] + w

    def fwd(S=24, So=24, **over):
        out = _Out(dev, E, 48, 48)
        a = dict(ea=_p(ea), out=out.ptr(), **{'w%d' % (i + 1): _p(w[i]) for i in range(4)})
        a.update(over)
        return _done(Lb.gml_edge_mlp_wide_fwd(a['ea'], a['w1'], a['w2'], a['w3'], a['w4'], a['out'], E, S, So, st)), out.unchanged()

    def bwd(S=24, So=24, **over):
        outs = [_Out(dev, E, 48, 48), _Out(dev, E, 192, 192), _Out(dev, E, 288, 288)]
        a = dict(ea=_p(ea), out=_p(gout), gout=_p(gout), go=outs[0].ptr(), hid=outs[1].ptr(), gz=outs[2].ptr(),
                 **{'w%d' % (i + 1): _p(w[i]) for i in range(4)})
        a.update(over)
        rc = Lb.gml_edge_mlp_wide_bwd(a['ea'], a['w1'], a['w2'], a['w3'], a['w4'], a['out'], a['gout'], a['go'], a['hid'], a['gz'], E, S, So, st)
        return _done(rc), all(o.unchanged() for o in outs)

    assert fwd()[0] == OK and bwd()[0] == OK
    for f in (fwd, bwd):
        assert f(S=16, So=16) == (UNS, True) and f(S=8, So=12) == (UNS, True) and f(S=49, So=49) == (UNS, True) and f(S=20, So=50) == (UNS, True)
        assert f(S=0) == (BAD, True)
        for k in ('ea', 'w1', 'w2', 'w3', 'w4'):
            assert f(**{k: NULL}) == (BAD, True), k
        assert f(ea=_off(_p(ea))) == (BAD, True)
    assert fwd(out=NULL) == (BAD, True) and fwd(out=_off(_Out(dev, E + 1, 48, 48).ptr())) == (BAD, True)
    for k in ('out', 'gout', 'go', 'hid', 'gz'):
        assert bwd(**{k: NULL}) == (BAD, True), k
        assert bwd(**{k: _off(_Out(dev, E + 1, 288, 288).ptr())}) == (BAD, True), k
    d = dcase(dev, 4, E)
    img, rows = _Out(dev, E + 1, 16, 16), _Out(dev, E + 1, 8, 8)
    ps = lambda S, ea_=_p(d['ea']), im=img.ptr(): _done(Lb.gml_edge_presplit(ea_, im, E, S, st))
    assert ps(17) == UNS and ps(0) == BAD and ps(4, ea_=NULL) == BAD and ps(4, im=NULL) == BAD and ps(4, im=_off(img.ptr())) == BAD
    gp = lambda S, in_=_p(d['ea']), pm=_p(d['tpos']), o=rows.ptr(), im=img.ptr(): _done(Lb.gml_gather_rows_presplit(in_, pm, o, im, E, S, st))
    assert gp(9) == UNS and gp(0) == BAD and gp(4, in_=NULL) == BAD and gp(4, pm=NULL) == BAD and gp(4, o=NULL) == BAD and gp(4, im=NULL) == BAD
    assert gp(4, im=_off(img.ptr())) == BAD and gp(8, o=_off(rows.ptr())) == BAD
    assert img.unchanged() and rows.unchanged() and keep


# ------------------------------------------------------------------------------------------------------------------------- report
def test_worst_figures_and_coverage_report():
    """prints what the matrix measured (pytest -rP): per family, entry and output the worst max-norm figure and the worst
    |got - ref| / term sum (each already asserted by its own case), and asserts the coverage: every instantiation the plan can reach
    ran, every family id of gml_edge_mlp_plan was reached, every cap case took its second trip"""
    assert WORST, 'no case ran'
    print('%-12s %-16s %-5s %6s %12s %12s' % ('family', 'entry', 'out', 'cases', 'max-norm', 'term-sum'))
    for (fam, entry, out), (n, e_max, e_ts) in sorted(WORST.items()):
        print('%-12s %-16s %-5s %6d %12.2e %12.2e' % (fam, entry, out, n, e_max, e_ts))
        tol = TOL_F32 if fam in ('valu', 'wide') else TOL
        assert e_max <= tol and e_ts <= tol
    # the compiled instantiations (GML_EMLP_S, GML_ECHAIN_S, GML_ECHAIN16_S, GML_ECHAIN_STACKS, GML_ECHAIN6_S, GML_ECHAIN6_STACKS,
    # GML_ESYM_SINGLES) as the plan can reach them: the two-piece chain is compiled for S = 1 as well, which the plan keeps on the
    # one-edge-per-lane kernels
    want = [('valu', d, S, 0) for d in ('fwd', 'bwd') for S in SS]
    want += [('chain', d, S, 0) for d in ('fwd', 'bwd') for S in range(2, 9)] + [('chain', 'fwd', S, L) for S in (4, 8) for L in (2, 3, 4)]
    want += [('chain16', d, S, 0) for d in ('fwd', 'bwd') for S in range(9, 17)]
    want += [('chain6', 'fwd', S, 0) for S in range(2, 9)] + [('chain6', 'fwd', S, L) for S in (4, 8) for L in (1, 2, 3, 4)]
    want += [('chain16x6', 'fwd', S, 0) for S in range(9, 17)]
    want += [('sym6', 'fwd', S, L) for S in (4, 8) for L in (1, 2, 3, 4)] + [('sym6', 'fwd', S, 1) for S in (2, 3, 5, 6, 7)]
    want += [('sym16x6', 'fwd', S, 1) for S in range(9, 17)]
    want += [('sym_chain', 'bwd', S, 0) for S in range(2, 9)] + [('sym_chain16', 'bwd', S, 0) for S in range(9, 17)]
    want += [('wide', 'fwd') + s for s in WIDE]
    missing = [w for w in want if w not in RAN]
    assert not missing, 'instantiations no case reached: %s' % missing
    assert {f for f, _, _, _ in RAN} >= set(FAM.values()), 'a family id of gml_edge_mlp_plan was not reached'
    caps = {(k, 'fwd') for k in CAPS_FWD} | {(k, 'bwd') for k in CAPS_BWD}
    assert TRIPS == caps, 'cap cases that did not run: %s' % sorted(caps - TRIPS)
