"""Every answer of gml_edge_mlp_plan on the device: where it names a family, the entry point of that request runs and agrees with
oracle.spect_conv_oracle (tolerances of tests/test_gpu_parity.py: TOL, 2e-5 for the one-edge-per-lane fp32 family); where it says
none, the entry point returns GML_E_UNSUPPORTED and leaves its NaN-filled outputs alone.  E = 17: one edge past a 16-edge tile;
E = 200 003: persistent workgroups take a second trip of their stride loop.  Requests no entry point can express (a stacked exact
forward, a unique-row backward without pre-split rows, ...) are not run."""
import ctypes
import functools
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-4
SS = (1, 2, 3, 4, 6, 8, 9, 12, 16)
ES = (17, 200003)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from gnn_matlang_amd import _lib
    assert _lib.lib().gml_version() >= 1
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def reference(S, E):
    """inputs and float64 oracle results, computed once per shape: the first E // 3 edges have a mirror (edge P + i carries the same
    row, as the supports of a symmetric graph do), the rest are one-sided; four weight sets (layer l of a stack uses set l)"""
    from oracle import spect_conv_oracle as O
    from oracle.relu_margin import make_safe_edges
    g = torch.Generator().manual_seed(1000 * S + E % 997)
    ws = [[torch.randn(2 * S, S, generator=g) * 0.7 for _ in range(3)] + [torch.randn(S, 4 * S, generator=g) * 0.5] for _ in range(4)]
    ea = torch.randn(E, S, generator=g)
    ea = make_safe_edges(ea, *ws[0], generator=g)            # set 0 is the backward's: no relu argument within rounding of zero
    P = E // 3
    ea[P:2 * P] = ea[:P]
    order = torch.randperm(E - P, generator=g)
    uid = torch.cat([torch.arange(P), torch.arange(2 * P, E)])[order].int()
    mir = torch.cat([torch.arange(P, 2 * P), torch.full((E - 2 * P,), -1)])[order].int()
    ys = [O.edge_mlp_forward(ea.double(), *[t.double() for t in w]) for w in ws]
    eo = ea.double().requires_grad_(True)
    wo = [t.double().requires_grad_(True) for t in ws[0]]
    gout = torch.randn(E, S, generator=g)
    (O.edge_mlp_forward(eo, *wo) * gout.double()).sum().backward()
    return dict(ea=ea, ws=ws, ys=[y.float() for y in ys], gout=gout, gin=eo.grad.float(), dws=[t.grad.float() for t in wo], uid=uid, mir=mir,
                tpos=torch.randperm(E, generator=g).int())


def close(got, ref, tol, what):
    """conftest.rel_err (max |got - ref| / max |ref|), evaluated on the device"""
    ref = ref.to(got.device)
    assert bool(torch.isfinite(got).all()), what
    e = float((got.double() - ref.double()).abs().max() / ref.abs().max().clamp_min(1e-30))
    assert e <= tol, '%s: rel err %.3e > %.1e' % (what, e, tol)


def untouched(ts, what):
    assert all(bool(torch.isnan(t).all()) for t in ts), what


@pytest.mark.parametrize('S', SS)
def test_every_plan_answer_runs_or_is_refused(dev, S):
    from gnn_matlang_amd import _lib as G, functional as Fn
    L_ = G.lib()
    p, st = Fn._ptr, Fn._stream(dev)
    nan = lambda *shape: torch.full(shape, float('nan'), device=dev)
    for E in ES:
        R = reference(S, E)
        ea, gout, tpos = R['ea'].to(dev), R['gout'].to(dev), R['tpos'].to(dev)
        ws = [[t.to(dev) for t in w] for w in R['ws']]
        ys, dws_ref, gin_ref = [y.to(dev) for y in R['ys']], [t.to(dev) for t in R['dws']], R['gin'].to(dev)
        es = Fn.edge_presplit(ea)
        U = R['uid'].numel()
        pad = torch.zeros(3, dtype=torch.int32)              # the device-count form: capacity U + 3, *count = U
        uid, mir = R['uid'].to(dev), R['mir'].to(dev)
        uid_c, mir_c = torch.cat([R['uid'], pad]).to(dev), torch.cat([R['mir'], pad - 1]).to(dev)
        count = torch.tensor([U], dtype=torch.int32, device=dev)
        # ---- forward
        for L, arith, split, dual, sym in itertools.product(range(6), (G.GML_EDGE_TWO_PIECE, G.GML_EDGE_THREE_PIECE, G.GML_EDGE_EXACT),
                                                            (0, 1), (0, 1), (0, 1)):
            three, exact = arith == G.GML_EDGE_THREE_PIECE, arith == G.GML_EDGE_EXACT
            if (sym and (L == 0 or not three or dual)) or (L > 0 and (exact or dual or (not three and not split))) or (L == 0 and split and arith):
                continue                                     # no entry point takes this request (or: the same call as split = 0)
            flags = arith | (G.GML_EDGE_HAS_SPLIT if split else 0) | (G.GML_EDGE_DUAL if dual else 0) | (G.GML_EDGE_UNIQUE if sym else 0)
            fam = int(L_.gml_edge_mlp_plan(G.GML_EDGE_FWD, S, S, L, flags))
            what = 'fwd S=%d E=%d L=%d flags=%d family=%d' % (S, E, L, flags, fam)
            outs = [nan(E, S) for _ in range(max(L, 1))]
            out_t = nan(E, S) if dual else None
            arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
            wl = [arr([ws[l % 4][i] for l in range(max(L, 1))]) for i in range(4)]
            one = (p(ws[0][0]), p(ws[0][1]), p(ws[0][2]), p(ws[0][3]), p(outs[0]), p(tpos if dual else None), p(out_t), E, S, S, st)
            if L == 0:
                rcs = [L_.gml_edge_mlp_fwd_exact(p(ea), *one) if exact else L_.gml_edge_mlp_fwd6(p(ea), *one) if three
                       else L_.gml_edge_mlp_fwd(p(ea), p(es if split else None), *one)]
            elif sym:
                rcs = [L_.gml_edge_mlp_fwd_stack6_sym(p(ea), p(uid), p(mir), U, L, *wl, arr(outs), E, S, S, st)]
                outs2 = [nan(E, S) for _ in range(L)]
                rcs.append(L_.gml_edge_mlp_fwd_stack6_sym_dev(p(ea), p(uid_c), p(mir_c), p(count), U + 3, L, *wl, arr(outs2), E, S, S, st))
                outs += outs2
            elif three:
                rcs = [L_.gml_edge_mlp_fwd_stack6(p(ea), L, *wl, arr(outs), E, S, S, st)]
            else:
                rcs = [L_.gml_edge_mlp_fwd_stack(p(es), L, *wl, arr(outs), E, S, S, st)]
            if fam == G.GML_EDGE_FAM_NONE:
                assert all(rc == G.GML_E_UNSUPPORTED for rc in rcs), (what, rcs)
                untouched(outs + ([out_t] if dual else []), what)
                continue
            assert all(rc == G.GML_OK for rc in rcs), (what, rcs)
            tol = 2e-5 if fam == G.GML_EDGE_FAM_VALU else TOL
            for i, o in enumerate(outs):
                close(o, ys[i % max(L, 1) % 4], tol, what)
            if dual:
                assert torch.equal(out_t[tpos.long()], outs[0]), what
        # ---- backward
        nbytes = int(L_.gml_edge_mlp_bwd_workspace_bytes(E, S, S))
        wsp = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        w = ws[0]
        for exact, split, gin, sym in itertools.product((0, 1), repeat=4):
            if (sym and (exact or gin or not split)) or (exact and split):
                continue
            flags = (G.GML_EDGE_EXACT if exact else 0) | (G.GML_EDGE_HAS_SPLIT if split else 0) | (G.GML_EDGE_WANT_GIN if gin else 0) | \
                    (G.GML_EDGE_UNIQUE if sym else 0)
            fam = int(L_.gml_edge_mlp_plan(G.GML_EDGE_BWD, S, S, 0, flags))
            what = 'bwd S=%d E=%d flags=%d family=%d' % (S, E, flags, fam)
            runs = []
            for dev_count in ((0, 1) if sym else (0,)):
                dws = [nan(2 * S, S), nan(2 * S, S), nan(2 * S, S), nan(S, 4 * S)]
                g = nan(E, S) if gin else None
                tail = (*[p(t) for t in dws], E, S, S, p(wsp), nbytes, st)
                if sym and dev_count:
                    rc = L_.gml_edge_mlp_bwd_sym_dev(p(es), p(uid_c), p(mir_c), p(count), U + 3, *[p(t) for t in w], p(gout), *tail)
                elif sym:
                    rc = L_.gml_edge_mlp_bwd_sym(p(es), p(uid), p(mir), U, *[p(t) for t in w], p(gout), *tail)
                elif exact:
                    rc = L_.gml_edge_mlp_bwd_exact(p(ea), *[p(t) for t in w], p(gout), p(g), *tail)
                else:
                    rc = L_.gml_edge_mlp_bwd(p(ea), p(es if split else None), *[p(t) for t in w], p(gout), p(g), *tail)
                runs.append((rc, dws, g))
            for rc, dws, g in runs:
                if fam == G.GML_EDGE_FAM_NONE:
                    assert rc == G.GML_E_UNSUPPORTED, (what, rc)
                    untouched(dws + ([g] if gin else []), what)
                    continue
                assert rc == G.GML_OK, (what, rc)
                tol = 2e-5 if fam == G.GML_EDGE_FAM_VALU else TOL
                for i in range(4):
                    close(dws[i], dws_ref[i], tol, what + ' dw%d' % (i + 1))
                if gin:
                    close(g, gin_ref, tol, what + ' gin')
