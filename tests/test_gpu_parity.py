"""GPU parity: the HIP path (through the C ABI of libgml_hip.so) against the oracle and the golden
vectors captured from the reference.  Tolerance: north_star's 1e-4 relative fp32
(max|got-ref| / max|ref| <= 1e-4, conftest.rel_err); integer/index work bit-exact."""
import os

import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4
T = lambda a: torch.tensor(np.asarray(a))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from gnn_matlang_amd import _lib
    assert _lib.lib().gml_version() >= 1          # the .so is loaded: no silent fallback exists
    return torch.device('cuda:0')


@pytest.fixture(params=['default', 'f32', 'default-ring', 'bf16x3'])
def arith(request):
    """arithmetic of the fused kernels.  'default' (round 6): the FORWARD pass fp32-class -- edge branch on three-piece bf16 products
    (gml_edge_mlp_fwd6), conv projection + Hadamard branch on f16 (hi, lo) pieces under power-of-two scales (GML_F16X3) -- and the
    backward kernels on the bf16 hi/lo split (three products per fp32 product, ~2^-17 operand residual); 'f32': the exact f32-input
    MFMA family everywhere (GML_F32_MFMA); 'bf16x3': the bf16 pairs in the forward too (rounds 1-5's default: GML_EDGE_FWD6=0
    GML_FWD_F16=0).  The golden suites run in all of them -- and once more with the fused backward on its LDS-DMA landing-ring kernel
    (bwd4, opt-in: GML_DMA_RING), so that the non-default kernel stays parity-checked."""
    from gnn_matlang_amd import functional as Fn
    old = Fn.F32_MFMA, Fn.BWD_DMA, Fn.EDGE_FWD6, Fn.FWD_F16
    Fn.F32_MFMA = request.param == 'f32'
    Fn.BWD_DMA = request.param.endswith('-ring')
    if request.param == 'bf16x3':
        Fn.EDGE_FWD6 = Fn.FWD_F16 = False
    yield request.param.split('-')[0]
    Fn.F32_MFMA, Fn.BWD_DMA, Fn.EDGE_FWD6, Fn.FWD_F16 = old


def cu(a, dev):
    return T(a).to(dev)


def close(got, ref, tol=TOL, what=''):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    e = rel_err(got, ref)
    assert e <= tol, '%s: rel err %.3e > %.1e' % (what, e, tol)


# ------------------------------------------------------------------------------------------ CSR
def _csr_check(ei, N, dev):
    from gnn_matlang_amd.graph import GraphCSR
    from oracle.csr_oracle import csr_from_coo, transpose_view
    g = GraphCSR.from_edge_index(cu(ei, dev), N)
    rowptr, col, perm = csr_from_coo(ei[0], ei[1], N)
    rp_t, col_t, pos_t = transpose_view(ei[0], ei[1], N, perm)
    for got, ref, name in ((g.rowptr, rowptr, 'rowptr'), (g.col, col, 'col'), (g.perm, perm, 'perm'),
                           (g.rowptr_t, rp_t, 'rowptr_t'), (g.col_t, col_t, 'col_t'), (g.pos_t, pos_t, 'pos_t')):
        assert np.array_equal(got.cpu().numpy(), ref), name          # integer work: bit-exact
    from oracle.csr_oracle import group_records
    for rec, rp, cl, rows, name in ((g.ginfo, rowptr, col, 64, 'ginfo'), (g.ginfo_t, rp_t, col_t, 64, 'ginfo_t'),
                                    (g.ginfo_t128, rp_t, col_t, 128, 'ginfo_t128')):
        info, order = group_records(rp, cl, N, rows)
        got = rec.cpu().numpy()
        assert np.array_equal(got[:, :4], info), name
        if rows == 128:                                               # lane position -> row bytes: a permutation per group
            ob = got[:, 4:].astype(np.int32).view(np.uint8).reshape(got.shape[0], -1)[:, :128]
            assert np.array_equal(ob, order), name + ' order'
            assert all(sorted(r.tolist()) == list(range(128)) for r in ob), name + ' not a permutation'


def test_csr_bit_exact(dev, golden):
    for f in ('model_zinc_gnnml3.npz', 'model_counting_gnnml3.npz', 'model_mutag_gnnml3.npz',
              'model_sr25_gnnml3.npz'):
        g = golden(f)
        _csr_check(g['batch/edge_index2'], g['batch/x'].shape[0], dev)
        _csr_check(g['batch/edge_index'], g['batch/x'].shape[0], dev)
    rng = np.random.default_rng(0)
    # unsorted input with duplicates, empty rows and a long row (stability matters)
    N, E = 5000, 60000
    ei = rng.integers(0, N, size=(2, E))
    ei[1, :3000] = 17
    ei[:, 100:110] = ei[:, 90:100]
    _csr_check(ei, N, dev)
    _csr_check(np.zeros((2, 0), dtype=np.int64), 7, dev)            # no edges
    _csr_check(np.array([[0], [0]], dtype=np.int64), 1, dev)


def test_csr_large_is_stable_sort(dev):
    from gnn_matlang_amd.graph import GraphCSR
    torch.manual_seed(0)
    N, E = 1_500_000, 9_000_000
    src = torch.randint(0, N, (E,), device=dev)
    dst = (src + torch.randint(-20, 21, (E,), device=dev)).clamp_(0, N - 1)
    g = GraphCSR.from_edge_index(torch.stack([src, dst]), N)
    perm = g.perm.long()
    d = dst[perm]
    assert bool((d[1:] >= d[:-1]).all())                                   # sorted by target
    same = d[1:] == d[:-1]
    assert bool((perm[1:][same] > perm[:-1][same]).all())                  # stable inside a row
    assert bool((g.col.long() == src[perm]).all())
    assert int(g.rowptr[-1]) == E
    assert bool((torch.bincount(dst, minlength=N) == (g.rowptr[1:] - g.rowptr[:-1])).all())
    assert bool((perm[g.pos_t.long()] == g.perm_t.long()).all())


# ------------------------------------------------------------------------------------------ SpectConv
def test_spectconv_golden(dev, golden, arith):
    from gnn_matlang_amd import SpectConv
    g = golden('spectconv.npz')
    for k in range(int(g['ncases'])):
        c = g.sub('case%03d/' % k)
        S, fin, fout, selfconn, depthwise, bias = [int(v) for v in c['meta']]
        m = SpectConv(fin, fout, S, selfconn=bool(selfconn), depthwise=bool(depthwise), bias=bool(bias)).to(dev)
        sd = {'weight': T(c['weight'])}
        if bias:
            sd['bias'] = T(c['bias'])
        if depthwise:
            sd['DSweight'] = T(c['DSweight'])
        m.load_state_dict(sd)
        x = cu(c['x'], dev).requires_grad_(True)
        ea = cu(c['edge_attr'], dev).requires_grad_(True)
        y = m(x, cu(c['edge_index'], dev), ea)
        what = 'case %d meta %s' % (k, c['meta'])
        close(y, c['out'], what=what + ' out')
        (y * cu(c['gout'], dev)).sum().backward()
        close(x.grad, c['g_x'], what=what + ' g_x')
        close(ea.grad, c['g_edge_attr'], what=what + ' g_edge_attr')
        close(m.weight.grad, c['g_weight'], what=what + ' g_weight')
        if bias:
            close(m.bias.grad, c['g_bias'], what=what + ' g_bias')
        if depthwise:
            close(m.DSweight.grad, c['g_DSweight'], what=what + ' g_DSweight')


def test_spectconcat_golden(dev, golden, arith):
    from gnn_matlang_amd import SpectConCatConv
    g = golden('spectconv.npz')
    for k in range(int(g['nconcat'])):
        c = g.sub('concat%d/' % k)
        S, fin, fout, selfconn = [int(v) for v in c['meta']]
        m = SpectConCatConv(fin, fout, S, selfconn=bool(selfconn)).to(dev)
        m.load_state_dict({'weight': T(c['weight']), 'bias': T(c['bias'])})
        x = cu(c['x'], dev).requires_grad_(True)
        ea = cu(c['edge_attr'], dev).requires_grad_(True)
        y = m(x, cu(c['edge_index'], dev), ea)
        close(y, c['out'], what='concat out')
        (y * cu(c['gout'], dev)).sum().backward()
        close(x.grad, c['g_x'], what='concat g_x')
        close(ea.grad, c['g_edge_attr'], what='concat g_ea')
        close(m.weight.grad, c['g_weight'], what='concat g_w')
        close(m.bias.grad, c['g_bias'], what='concat g_b')


def _random_graph(rng, N, deg, sort=True):
    src = np.repeat(np.arange(N), deg)
    dst = np.clip(src + rng.integers(-6, 7, size=src.shape), 0, N - 1)
    ei = np.unique(np.vstack((src, dst)), axis=1)      # row-major order like np.where
    return ei.astype(np.int64)


@pytest.mark.parametrize('S,fin,fout', [(1, 1, 1), (2, 3, 17), (5, 25, 30), (7, 32, 33), (9, 20, 16), (10, 48, 8),
                                        (11, 64, 64), (12, 2, 16), (12, 32, 16), (13, 36, 40), (16, 16, 130),
                                        (24, 32, 32), (48, 48, 32), (6, 128, 128), (6, 2, 64), (3, 200, 24)])
def test_fused_forward_and_grads_vs_oracle(dev, S, fin, fout):
    """shape sweep (support splits, odd widths, Fout > 128, wide Fin) against the CPU oracle."""
    from gnn_matlang_amd import SpectConv
    from oracle import spect_conv_oracle as O
    rng = np.random.default_rng(S * 1000 + fin)
    torch.manual_seed(S * 7 + fout)
    N = 203                                            # not a multiple of 16; includes empty rows
    ei = _random_graph(rng, N, 5)
    ei = ei[:, ei[1] != 77]                            # node 77 has no in-edges
    E = ei.shape[1]
    ea = torch.randn(E, S)
    x = torch.randn(N, fin)
    m = SpectConv(fin, fout, S, selfconn=False).to(dev)
    with torch.no_grad():
        m.bias.uniform_(-0.5, 0.5)
    w, b = m.weight.detach().cpu(), m.bias.detach().cpu()
    xo, eo, wo, bo = (t.clone().requires_grad_(True) for t in (x, ea, w, b))
    yo = O.spectconv_forward(xo, T(ei), eo, wo, bo, False)
    gout = torch.randn_like(yo)
    (yo * gout).sum().backward()
    xg, eg = x.to(dev).requires_grad_(True), ea.to(dev).requires_grad_(True)
    y = m(xg, T(ei).to(dev), eg)
    close(y, yo, what='out')
    (y * gout.to(dev)).sum().backward()
    close(xg.grad, xo.grad, what='g_x')
    close(eg.grad, eo.grad, what='g_edge_attr')
    close(m.weight.grad, wo.grad, what='g_weight')
    close(m.bias.grad, bo.grad, what='g_bias')


@pytest.mark.parametrize('S,fin,fout,deg', [(8, 32, 30, 5), (8, 25, 30, 24), (4, 32, 16, 24), (8, 32, 32, 40),
                                             (12, 32, 32, 5), (12, 32, 30, 7), (12, 20, 9, 24), (12, 32, 16, 10), (12, 32, 16, 11)])
def test_eight_wave_forward_staged_and_global_paths(dev, S, fin, fout, deg):
    """the 128-row forward kernel on groups inside its LDS capacities (deg 5) and far outside (deg >= 24: > 1024 edges
    per group -> global-gather path), aligned and unaligned x rows, against the oracle; backward rides along.  S = 12
    (counting.py) stays on the register-staged 8-wave kernel, which stages up to 1,536 edges per group there (deg 10, 11:
    groups between the old bound of 1,024 and the new one); its backward is the 12-support / 16-column instantiation of the
    8-wave backward."""
    from gnn_matlang_amd import SpectConv
    from oracle import spect_conv_oracle as O
    rng = np.random.default_rng(S * 100 + deg)
    torch.manual_seed(deg)
    N = 517
    ei = _random_graph(rng, N, deg)
    ea, x = torch.randn(ei.shape[1], S), torch.randn(N, fin)
    m = SpectConv(fin, fout, S, selfconn=False).to(dev)
    w, b = m.weight.detach().cpu(), m.bias.detach().cpu()
    xo, eo, wo = (t.clone().requires_grad_(True) for t in (x, ea, w))
    yo = O.spectconv_forward(xo, T(ei), eo, wo, b, False)
    gout = torch.randn_like(yo)
    (yo * gout).sum().backward()
    xg, eg = x.to(dev).requires_grad_(True), ea.to(dev).requires_grad_(True)
    y = m(xg, T(ei).to(dev), eg)
    close(y, yo, what='out')
    (y * gout.to(dev)).sum().backward()
    close(xg.grad, xo.grad, what='g_x')
    close(eg.grad, eo.grad, what='g_edge_attr')
    close(m.weight.grad, wo.grad, what='g_weight')


def test_register_staged_forward_through_the_raw_abi(dev, monkeypatch):
    """The register-staged 8-wave kernel (fwd2) at S = 4 / 8, where the ring kernel (fwd3) is the default: reached only through
    the C ABI, (a) by x rows that are not float4-addressable (ldx = Fin = 25; functional always pads them) and (b) in accumulate
    mode (aligned x, out pre-filled: out0 + conv).  128-row records, N = 300: the third group is partial.  Both projections
    (f16 pieces, the default, and bf16 pairs)."""
    from gnn_matlang_amd import _lib, functional as Fn
    from gnn_matlang_amd.graph import GraphCSR
    from oracle import spect_conv_oracle as O
    rng = np.random.default_rng(300)
    torch.manual_seed(300)
    N = 300
    ei = _random_graph(rng, N, 5)
    csr = GraphCSR.from_edge_index(T(ei).to(dev), N)
    for S, fout in ((8, 30), (4, 9)):
        ea = torch.randn(ei.shape[1], S)
        val = csr.sort_values(ea.to(dev))
        for fin, accum in ((25, False), (32, True)):
            x, w, b, out0 = torch.randn(N, fin), torch.randn(S, fin, fout) / fin ** 0.5, torch.rand(fout) - 0.5, torch.randn(N, fout)
            yo = O.spectconv_forward(x, T(ei), ea, w, b, False) + (out0 if accum else 0)
            xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
            for f16 in (True, False):
                monkeypatch.setattr(Fn, 'FWD_F16', f16)
                out = out0.to(dev) if accum else torch.full((N, fout), float('nan'), device=dev)
                Fn._fused_conv(csr.rowptr, csr.col, csr.ginfo128, None, val, xd, fin, wd, (fin * fout, fout, 1), bd, out, fout, N,
                               S, fin, fout, _lib.GML_GROUPS128 | (_lib.GML_ACCUM if accum else 0), 0)
                close(out, yo, what='S=%d fin=%d accum=%s f16=%s' % (S, fin, accum, f16))


@pytest.mark.parametrize('S,fin,fout,selfconn,depthwise', [(4, 1, 4, False, True), (4, 21, 30, False, True), (4, 3, 4, True, True),
                                                           (8, 32, 30, True, True), (8, 7, 16, False, True),
                                                           (4, 20, 30, True, False), (8, 32, 16, False, False)])
def test_ring_kernel_epilogues_vs_oracle(dev, S, fin, fout, selfconn, depthwise):
    """The ring kernel's epilogues (gml_spectconv_fwd_epi) at both of its support counts: depthwise SpectConv
    (libs/spect_conv.py:81-91; depthwise=True) with and without the self term, and SpectConCatConv (:137-158; depthwise=False here)
    -- forward and every gradient against the oracle modules.  (S = 4 depthwise once put its scales on the lo image of W:
    the randomised sweep found it, these cases pin it.)"""
    from gnn_matlang_amd import SpectConv, SpectConCatConv
    from oracle.spect_conv_oracle import OracleSpectConv, OracleSpectConCatConv
    rng = np.random.default_rng(S * 10 + fin)
    torch.manual_seed(S + fout)
    N = 300
    ei = _random_graph(rng, N, 4)
    x, ea = torch.randn(N, fin), torch.randn(ei.shape[1], S)
    if depthwise:
        ref = OracleSpectConv(fin, fout, S, selfconn=selfconn, depthwise=True).double()
        m = SpectConv(fin, fout, S, selfconn=selfconn, depthwise=True).to(dev)
        with torch.no_grad():
            ref.DSweight.normal_(0, 0.5)
    else:
        ref = OracleSpectConCatConv(fin, fout, S, selfconn=selfconn).double()
        m = SpectConCatConv(fin, fout, S, selfconn=selfconn).to(dev)
    with torch.no_grad():
        ref.bias.uniform_(-0.5, 0.5)
    m.load_state_dict({n: p.detach().float() for n, p in ref.state_dict().items()})
    xr, er = x.double().requires_grad_(True), ea.double().requires_grad_(True)
    yr = ref(xr, T(ei), er)
    go = torch.randn_like(yr)
    (yr * go).sum().backward()
    xg, eg = x.to(dev).requires_grad_(True), ea.to(dev).requires_grad_(True)
    y = m(xg, T(ei).to(dev), eg)
    close(y, yr, what='out')
    (y * go.float().to(dev)).sum().backward()
    close(xg.grad, xr.grad, what='g_x')
    close(eg.grad, er.grad, what='g_edge_attr')
    gp = dict(m.named_parameters())
    for n, p in ref.named_parameters():
        close(gp[n].grad, p.grad, what=n)


def test_exact_fp32_mode_is_closer_to_the_oracle(dev):
    """GML_F32_MFMA (f32-input MFMA: exact fp32 products) must agree with the oracle at fp32-roundoff level, an
    order of magnitude tighter than the default bf16 hi/lo split is asked to."""
    from gnn_matlang_amd import SpectConv, functional as Fn
    from oracle import spect_conv_oracle as O
    rng = np.random.default_rng(77)
    torch.manual_seed(77)
    N, S, fin, fout = 300, 8, 32, 30
    ei = _random_graph(rng, N, 6)
    ea, x = torch.randn(ei.shape[1], S), torch.randn(N, fin)
    m = SpectConv(fin, fout, S, selfconn=False).to(dev)
    w, b = m.weight.detach().cpu(), m.bias.detach().cpu()
    xo, eo, wo = (t.clone().requires_grad_(True) for t in (x, ea, w))
    yo = O.spectconv_forward(xo, T(ei), eo, wo, b, False)
    gout = torch.randn_like(yo)
    (yo * gout).sum().backward()
    errs = {}
    old = Fn.F32_MFMA
    try:
        for mode in (False, True):
            Fn.F32_MFMA = mode
            m.zero_grad()
            xg, eg = x.to(dev).requires_grad_(True), ea.to(dev).requires_grad_(True)
            y = m(xg, T(ei).to(dev), eg)
            (y * gout.to(dev)).sum().backward()
            errs[mode] = max(rel_err(y.detach().cpu().numpy(), yo.detach().numpy()),
                             rel_err(xg.grad.cpu().numpy(), xo.grad.numpy()),
                             rel_err(eg.grad.cpu().numpy(), eo.grad.numpy()),
                             rel_err(m.weight.grad.cpu().numpy(), wo.grad.numpy()))
    finally:
        Fn.F32_MFMA = old
    assert errs[True] <= 2e-6, errs
    assert errs[False] <= TOL, errs


def test_edge_branch_valu_kernels_via_environment(dev):
    """GML_EDGE_VALU=1 (read once per process) routes S <= 8 to the one-edge-per-lane fp32 kernels: same results."""
    import subprocess
    import sys
    code = (
        "import sys, torch, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "from gnn_matlang_amd import functional as Fn\n"
        "from oracle import spect_conv_oracle as O\n"
        "torch.manual_seed(3)\n"
        "S, E = 8, 3000\n"
        "ea = torch.randn(E, S)\n"
        "ws = [torch.randn(2 * S, S) * 0.7 for _ in range(3)] + [torch.randn(S, 4 * S) * 0.5]\n"
        "eo = ea.clone().requires_grad_(True); wo = [w.clone().requires_grad_(True) for w in ws]\n"
        "yo = O.edge_mlp_forward(eo, *wo); g = torch.randn_like(yo); (yo * g).sum().backward()\n"
        "d = torch.device('cuda:0'); wd = [w.to(d) for w in ws]\n"
        "y, _ = Fn.edge_mlp_fwd(ea.to(d), *wd)\n"
        "r = Fn.edge_mlp_bwd(ea.to(d), *wd, g.to(d), True)\n"
        "def rel(a, b): return float((a.cpu() - b).abs().max() / b.abs().max())\n"
        "e = max([rel(y, yo.detach()), rel(r[0], eo.grad)] + [rel(r[i + 1], wo[i].grad) for i in range(4)])\n"
        "print('MAXERR', e)\n" % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    env = dict(os.environ, GML_EDGE_VALU='1')
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    err = float(out.stdout.strip().split('MAXERR')[-1])
    assert err <= 2e-5, out.stdout


def test_empty_and_tiny_inputs(dev):
    from gnn_matlang_amd import SpectConv, ML3Layer
    m = SpectConv(4, 3, 2, selfconn=False).to(dev)
    x = torch.randn(5, 4, device=dev)
    ei = torch.zeros(2, 0, dtype=torch.int64, device=dev)
    y = m(x, ei, torch.zeros(0, 2, device=dev))                     # no edges: out = bias
    assert torch.equal(y, m.bias.detach().expand(5, 3))
    l = ML3Layer(True, 2, 2, 4, 3, 2).to(dev)
    xg = x.clone().requires_grad_(True)
    out = l(xg, ei, torch.zeros(0, 2, device=dev))
    out.sum().backward()
    assert out.shape == (5, 5) and torch.isfinite(xg.grad).all()
    assert float(l.fc1_1.weight.grad.abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------ C ABI pieces
def test_spmm_sddmm_edge_mlp_node_mix_vs_oracle(dev):
    from gnn_matlang_amd import functional as Fn
    from gnn_matlang_amd.graph import GraphCSR
    from oracle import spect_conv_oracle as O
    from oracle.relu_margin import make_safe_edges
    rng = np.random.default_rng(5)
    torch.manual_seed(5)
    N = 333
    ei = _random_graph(rng, N, 6)
    E = ei.shape[1]
    csr = GraphCSR.from_edge_index(T(ei).to(dev), N)
    for S, fin in ((8, 32), (3, 7), (12, 70), (1, 130), (4, 32), (4, 21), (8, 17)):
        ea, x = torch.randn(E, S), torch.randn(N, fin)
        val = csr.sort_values(ea.to(dev), cache=False)
        h = Fn.spmm(csr, val, x.to(dev), S, fin).view(N, S, fin)
        href = torch.stack([O.propagate_add(x, T(ei), ea[:, s]) for s in range(S)], 1)
        close(h, href, what='spmm S=%d' % S)
        gw = torch.randn(N, S, fin)
        dval = csr.unsort_values(Fn.sddmm(csr, x.to(dev), gw.to(dev).view(N, S * fin), S, fin))
        ref = torch.einsum('ef,esf->es', x[ei[0]], gw[ei[1]])
        close(dval, ref, what='sddmm S=%d' % S)
    # one partly filled 128-row group, staged (E <= 1024): waves without rows finish first (LDS tile vs staging areas)
    for N2, S, fin in ((7, 4, 32), (20, 4, 32), (20, 8, 32), (20, 4, 13), (100, 4, 32)):
        dst = np.repeat(np.arange(N2), rng.integers(5, 1000 // N2, N2))
        ei2 = np.stack([rng.integers(0, N2, dst.size), dst]).astype(np.int64)
        csr2 = GraphCSR.from_edge_index(T(ei2).to(dev), N2)
        ea, x = torch.randn(ei2.shape[1], S), torch.randn(N2, fin)
        h = Fn.spmm(csr2, csr2.sort_values(ea.to(dev), cache=False), x.to(dev), S, fin).view(N2, S, fin)
        href = torch.stack([O.propagate_add(x, T(ei2), ea[:, s]) for s in range(S)], 1)
        close(h, href, what='spmm small N=%d S=%d' % (N2, S))
    # (the last cases: fewer edges than one 16-edge tile, and exactly one tile)
    for S, E2 in [(S, 1000 + S) for S in range(1, 17)] + [(12, 7), (9, 1), (8, 1), (16, 16), (6, 15)]:
        ea = torch.randn(E2, S)
        ws = [torch.randn(2 * S, S) * 0.7 for _ in range(3)] + [torch.randn(S, 4 * S) * 0.5]
        ea = make_safe_edges(ea, *ws)                      # no relu argument within rounding of zero
        eo = ea.clone().requires_grad_(True)
        wo = [w.clone().requires_grad_(True) for w in ws]
        yo = O.edge_mlp_forward(eo, *wo)
        gout = torch.randn_like(yo)
        (yo * gout).sum().backward()
        wd = [w.to(dev) for w in ws]
        y, _ = Fn.edge_mlp_fwd(ea.to(dev), *wd)
        tp = torch.randperm(E2, device=dev).int()
        y2, yt = Fn.edge_mlp_fwd(ea.to(dev), *wd, tpos=tp)
        assert torch.equal(y2, y) and torch.equal(yt[tp.long()], y)          # second order: same rows, permuted
        close(y, yo, what='edge mlp fwd S=%d' % S)
        gin, d1, d2, d3, d4 = Fn.edge_mlp_bwd(ea.to(dev), *wd, gout.to(dev), True)
        close(gin, eo.grad, what='edge mlp gin S=%d' % S)
        for got, w, n in ((d1, wo[0], 'dw1'), (d2, wo[1], 'dw2'), (d3, wo[2], 'dw3'), (d4, wo[3], 'dw4')):
            close(got, w.grad, what='edge mlp %s S=%d' % (n, S))
        if S <= 8:                                         # ready-made bf16 hi | lo operand: the same bits
            es = Fn.edge_presplit(ea.to(dev))
            y3, yt3 = Fn.edge_mlp_fwd(ea.to(dev), *wd, tpos=tp, ea_split=es)
            assert torch.equal(y3, y) and torch.equal(yt3, yt)
            r3 = Fn.edge_mlp_bwd(ea.to(dev), *wd, gout.to(dev), True, ea_split=es)
            assert torch.equal(r3[0], gin) and torch.equal(r3[4], d4)     # no support value enters these: same bits
            # dW1..3 contract the SUPPORT rows: with the pre-split stream they are hi + lo of it (the fp32 rows are not
            # read at all, r02), i.e. the supports to 2^-17 instead of exactly -- held to the oracle like the plain path
            for got, w, n in ((r3[1], wo[0], 'dw1'), (r3[2], wo[1], 'dw2'), (r3[3], wo[2], 'dw3')):
                close(got, w.grad, what='edge mlp (pre-split) %s S=%d' % (n, S))
            r4 = Fn.edge_mlp_bwd(ea.to(dev), *wd, gout.to(dev), False, ea_split=es)
            assert r4[0] is None and all(torch.equal(a_, b_) for a_, b_ in zip(r4[1:], r3[1:]))
        else:                                              # 8 < S <= 16: K = 16-slot matrix-core chain on the 64-byte pre-split rows
            es = Fn.edge_presplit(ea.to(dev))
            assert es.shape == (E2, 16)
            y3, yt3 = Fn.edge_mlp_fwd(ea.to(dev), *wd, tpos=tp, ea_split=es)
            close(y3, yo, what='edge chain16 fwd S=%d' % S)
            assert torch.equal(yt3[tp.long()], y3)
            r5 = Fn.edge_mlp_bwd(ea.to(dev), *wd, gout.to(dev), False, ea_split=es)
            assert r5[0] is None
            for got, w, n in ((r5[1], wo[0], 'dw1'), (r5[2], wo[1], 'dw2'), (r5[3], wo[2], 'dw3'), (r5[4], wo[3], 'dw4')):
                close(got, w.grad, what='edge chain16 %s S=%d' % (n, S))
            r6 = Fn.edge_mlp_bwd(ea.to(dev), *wd, gout.to(dev), True, ea_split=es)     # supports' gradient wanted: VALU kernels
            close(r6[0], eo.grad, what='edge mlp gin (S > 8, pre-split given) S=%d' % S)


@pytest.mark.gpu
def test_ml3_output_stage_backward_vs_autograd(dev):
    """gml_ml3_split_bwd (relu mask + conv bias sums + Hadamard-branch backward in one pass) and
    gml_segment_bcast against torch autograd of the same expressions on the CPU (fp32)."""
    from gnn_matlang_amd import functional as Fn
    torch.manual_seed(11)
    for N, Fin, nout1, F2 in ((1000, 25, 30, 2), (257, 32, 30, 2), (513, 2, 16, 16), (300, 48, 32, 16),
                              (777, 48, 24, 24), (1, 7, 5, 3), (900, 0, 64, 0), (333, 0, 128, 0)):
        C = nout1 + F2
        y = torch.randn(N, C)
        gy = torch.randn(N, C)
        G_ref = gy[:, :nout1] * (y[:, :nout1] > 0)
        if F2:
            x = torch.randn(N, Fin, requires_grad=True)
            lin = [torch.nn.Linear(Fin, F2) for _ in range(2)]
            h = torch.tanh(lin[0](x)) * torch.tanh(lin[1](x))
            (h * gy[:, nout1:]).sum().backward()
            args = (x.detach().to(dev), lin[0].weight.detach().to(dev), lin[0].bias.detach().to(dev),
                    lin[1].weight.detach().to(dev), lin[1].bias.detach().to(dev))
            r = Fn.ml3_split_bwd(gy.to(dev), y.to(dev), nout1, *args, need_dx=True, need_dcb=True)
        else:
            r = Fn.ml3_split_bwd(gy.to(dev), y.to(dev), nout1, need_dcb=True)
        assert r is not None, (N, Fin, nout1, F2)
        G, dx, dcb, dw11, db11, dw12, db12 = r
        what = 'N=%d Fin=%d nout1=%d F2=%d ' % (N, Fin, nout1, F2)
        assert torch.equal(G.cpu(), G_ref), what + 'G'                      # a select: bit-exact
        if G._base is not None and G._base.size(1) > nout1:
            assert float(G._base[:, nout1:].abs().sum()) == 0., what + "padding"
        close(dcb, G_ref.sum(0), what=what + 'dcb')
        if F2:
            close(dx, x.grad, what=what + 'dx')
            close(dw11, lin[0].weight.grad, what=what + 'dw11')
            close(db11, lin[0].bias.grad, what=what + 'db11')
            close(dw12, lin[1].weight.grad, what=what + 'dw12')
            close(db12, lin[1].bias.grad, what=what + 'db12')
    # weight gradient of a small dense layer over many rows
    for n, pa, q in ((1000, 32, 32), (257, 1, 32), (5000, 10, 48), (3, 64, 64), (70000, 32, 32)):
        a, b = torch.randn(n, pa), torch.randn(n, q)
        close(Fn.xty(a.to(dev), b.to(dev)), a.double().t().mm(b.double()).float(), what='xty %d %d %d' % (n, pa, q))
    # pooling gradient
    sizes = torch.tensor([3, 1, 0, 7, 64, 2, 129])
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)]).int()
    g = torch.randn(len(sizes), 32)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), sizes)
    for mean in (False, True):
        ref = g[batch] / (sizes[batch].clamp(min=1).float().unsqueeze(-1) if mean else 1.)
        got = Fn.segment_bcast(g.to(dev), ptr.to(dev), int(sizes.sum()), mean)
        close(got, ref, tol=1e-6, what='segment_bcast mean=%s' % mean)


def test_spectral_design_on_device(dev, golden):
    """gml_spectral_count / gml_spectral_design (batched Jacobi eigh in LDS) against the reference's own vectors
    (every golden SpectralDesign case that fits the 80-node kernel) and, batched, against the host implementation:
    mask and its row-major order bit-exact, support values to 5e-6 absolute (float64 solver roundoff, float32 output;
    laplacien=False cases: the reference solves A in float32, 5e-5)."""
    import ast
    from gnn_matlang_amd import SpectralDesign, synthetic
    g = golden('spectral_design.npz')
    ran = 0
    for k in range(int(g['ncases'])):
        c = g.sub('case%02d/' % k)
        kw = ast.literal_eval(str(c['kw']))
        n = c['in_x'].shape[0]
        if n > SpectralDesign.MAX_DEVICE_NODES:
            continue
        sd = SpectralDesign(**kw)
        d = sd.design_device(T(c['in_x']).to(dev), T(c['in_edge_index']).long().to(dev),
                             torch.tensor([0, n], dtype=torch.int32, device=dev))
        assert np.array_equal(d['edge_index2'].cpu().numpy(), c['edge_index2']), str(c['name'])
        assert np.array_equal(d['x'].cpu().numpy(), c['x']), str(c['name'])
        tol = 5e-6 if kw.get('laplacien', True) else 5e-5
        np.testing.assert_allclose(d['edge_attr2'].cpu().numpy(), c['edge_attr2'], rtol=0, atol=tol, err_msg=str(c['name']))
        np.testing.assert_allclose(d['lmax'].cpu().numpy()[0], c['lmax'], rtol=2e-6)
        ran += 1
    assert ran >= 40, ran
    # a collated batch of mixed sizes (incl. an edgeless graph) against the host path
    raw = synthetic.make_graphs('zinc', 60, seed=11) + synthetic.make_graphs('counting', 20, seed=12)
    raw.append((np.ones((3, raw[0][0].shape[1]), np.float32), np.zeros((2, 0), np.int64), 0.0))
    raw = [(np.asarray(x, np.float32)[:, :1], ei, y) for x, ei, y in raw]       # one feature column for all
    sd = SpectralDesign(recfield=2, dv=2, nfreq=7, adddegree=True)
    host = sd.design_many(raw)
    sizes = np.array([x.shape[0] for x, _, _ in raw])
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    X = np.concatenate([x for x, _, _ in raw])
    EI = np.concatenate([np.asarray(ei, np.int64) + ptr[i] for i, (_, ei, _) in enumerate(raw)], 1)
    d = sd.design_device(T(X).to(dev), T(EI).to(dev), torch.tensor(ptr, dtype=torch.int32, device=dev))
    ei2 = np.concatenate([h['edge_index2'] + ptr[i] for i, h in enumerate(host)], 1)
    ea2 = np.concatenate([h['edge_attr2'] for h in host])
    assert np.array_equal(d['edge_index2'].cpu().numpy(), ei2)
    np.testing.assert_allclose(d['edge_attr2'].cpu().numpy(), ea2, rtol=0, atol=5e-6)
    np.testing.assert_allclose(d['lmax'].cpu().numpy(), np.array([h['lmax'] for h in host]), rtol=2e-6, atol=1e-6)
    assert np.array_equal(d['x'].cpu().numpy(), np.concatenate([h['x'] for h in host]))


@pytest.mark.parametrize('kw', [dict(recfield=2, dv=2, nfreq=7, adddegree=True), dict(recfield=1, dv=5, nfreq=5, addadj=True),
                                dict(recfield=1, dv=3, nfreq=4, laplacien=False, vmax=2.5)])
def test_spectral_design_on_device_large_graphs(dev, kw):
    """Graphs beyond the LDS-resident eigen-solver (more than 80 nodes: proteins has up to 620, libs/utils.py:546-610 is
    size-agnostic): design_device sends those through the device's dense libraries (float64 eigh + GEMMs), the small ones of the
    same batch through the kernels, and merges in graph order -- same mask, same order, same supports as the host path."""
    from gnn_matlang_amd import SpectralDesign
    rng = np.random.default_rng(5)
    raw = []
    for n, deg in ((12, 3), (130, 4), (7, 2), (97, 3), (81, 5), (40, 4), (200, 3), (3, 0)):
        src = np.repeat(np.arange(n), deg)
        dst = rng.integers(0, n, src.size)
        keep = src != dst
        ei = np.unique(np.concatenate([np.stack([src[keep], dst[keep]]), np.stack([dst[keep], src[keep]])], 1), axis=1).astype(np.int64)
        raw.append((np.ones((n, 1), np.float32), ei.reshape(2, -1), 0.0))
    sd = SpectralDesign(**kw)
    host = sd.design_many(raw)
    sizes = np.array([x.shape[0] for x, _, _ in raw])
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    X = np.concatenate([x for x, _, _ in raw])
    EI = np.concatenate([ei + ptr[i] for i, (_, ei, _) in enumerate(raw)], 1)
    d = sd.design_device(T(X).to(dev), T(EI).to(dev), torch.tensor(ptr, dtype=torch.int32, device=dev))
    ei2 = np.concatenate([h['edge_index2'] + ptr[i] for i, h in enumerate(host)], 1)
    ea2 = np.concatenate([h['edge_attr2'] for h in host])
    assert np.array_equal(d['edge_index2'].cpu().numpy(), ei2)
    np.testing.assert_allclose(d['edge_attr2'].cpu().numpy(), ea2, rtol=0, atol=1e-5)
    np.testing.assert_allclose(d['lmax'].cpu().numpy(), np.array([h['lmax'] for h in host]), rtol=2e-6, atol=1e-6)
    assert np.array_equal(d['x'].cpu().numpy(), np.concatenate([h['x'] for h in host]))


# ------------------------------------------------------------------------------------------ ML3Layer
def test_ml3layer_golden(dev, golden, arith):
    from gnn_matlang_amd import ML3Layer
    g = golden('ml3layer.npz')
    for k in range(int(g['ncases'])):
        c = g.sub('case%03d/' % k)
        learnedge, ne, neo, ninp, nout1, nout2 = [int(v) for v in c['meta']]
        m = ML3Layer(bool(learnedge), ne, neo, ninp, nout1, nout2).to(dev)
        m.load_state_dict({n[len('param/'):]: T(v) for n, v in c.items() if n.startswith('param/')})
        x = cu(c['x'], dev).requires_grad_(True)
        ea = cu(c['edge_attr'], dev).requires_grad_(True)
        y = m(x, cu(c['edge_index'], dev), ea)
        what = 'ml3 case %d %s' % (k, c['meta'])
        close(y, c['out'], what=what + ' out')
        (y * cu(c['gout'], dev)).sum().backward()
        close(x.grad, c['g_x'], what=what + ' g_x')
        close(ea.grad, c['g_edge_attr'], what=what + ' g_edge_attr')
        for n, p in m.named_parameters():
            close(p.grad, c['grad/' + n], what=what + ' ' + n)


@pytest.mark.parametrize('ne,neo,Fin,n1,n2', [(5, 3, 9, 24, 6), (3, 8, 9, 24, 6), (4, 12, 9, 24, 6),
                                              (4, 4, 80, 64, 16), (3, 3, 21, 16, 40),
                                              (12, 12, 32, 30, 2), (12, 12, 32, 29, 3), (12, 12, 28, 12, 4), (12, 12, 32, 16, 16),
                                              (24, 24, 20, 16, 2), (48, 48, 20, 16, 2), (17, 17, 12, 16, 0), (30, 22, 12, 16, 2),
                                              (20, 41, 12, 16, 2)])  # (> 16 supports: gml_edge_mlp_wide_fwd, csrc/gml_edge_wide.hip)
def test_ml3layer_wide_shapes(dev, ne, neo, Fin, n1, n2):
    """Shapes off the fused kernels' main road, against the oracle in fp64: nedgeoutput != nedgeinput (allowed by
    spect_conv.py:66-71, unused by the scripts), ninp = 80 (ptc.py:331-338) and a wide Hadamard branch; the last three
    are counting.py's 12 supports on the 8-wave kernel with its fused Hadamard columns."""
    from gnn_matlang_amd import ML3Layer
    from oracle.spect_conv_oracle import OracleML3Layer
    from oracle.relu_margin import make_safe
    torch.manual_seed(ne * 17 + neo)
    N = 333
    rng = np.random.default_rng(neo)
    dst = np.repeat(np.arange(N), rng.integers(0, 6, N))
    src = rng.integers(0, N, dst.size)
    o = np.lexsort((dst, src))
    ei = torch.from_numpy(np.stack([src[o], dst[o]]).astype(np.int64))
    ref = OracleML3Layer(True, ne, neo, Fin, n1, n2).double()
    m = ML3Layer(True, ne, neo, Fin, n1, n2).to(dev)
    m.load_state_dict({n: p.detach().float() for n, p in ref.state_dict().items()})
    x, ea, go = torch.randn(N, Fin), torch.randn(ei.size(1), ne) * 0.5, torch.randn(N, n1 + n2)
    ea, mask = make_safe(x, ei, ea, ref.state_dict(), True)       # no relu argument within rounding of zero
    go[:, :n1] *= mask.float()
    xr, er = x.double().requires_grad_(True), ea.double().requires_grad_(True)
    yr = ref(xr, ei, er)
    (yr * go.double()).sum().backward()
    xg, eg = x.to(dev).requires_grad_(True), ea.to(dev).requires_grad_(True)
    y = m(xg, ei.to(dev), eg)
    (y * go.to(dev)).sum().backward()
    close(y, yr, what='out')
    close(xg.grad, xr.grad, what='g_x')
    close(eg.grad, er.grad, what='g_edge_attr')
    gp = dict(m.named_parameters())
    for n, p in ref.named_parameters():
        close(gp[n].grad, p.grad, what=n)


@pytest.mark.parametrize('S,So,E', [(24, 24, 5000), (48, 48, 3001), (17, 17, 777), (33, 20, 1000), (20, 47, 64), (48, 48, 1)])
def test_edge_branch_beyond_16_supports_vs_fp64(dev, S, So, E):
    """gml_edge_mlp_wide_fwd (the edge branch for 16 < S <= 48, libs/spect_conv.py:190-194, 205-207) against the
    oracle's expression in float64 -- exact fp32 products, so far inside 1e-4 -- and the same values as the library road it replaces;
    gradients THROUGH THE HIP BACKWARD (round 6: gml_edge_mlp_wide_bwd + gml_xty_wide) against float64 autograd,
    the supports' own gradient included."""
    from gnn_matlang_amd import functional as Fn
    torch.manual_seed(S * 100 + So)
    ea = torch.randn(E, S) * 0.7
    w1, w2, w3 = [torch.randn(2 * S, S) / S ** 0.5 for _ in range(3)]
    w4 = torch.randn(So, 4 * S) / (4 * S) ** 0.5
    D = lambda t: t.double().requires_grad_(True)
    er, r1, r2, r3, r4 = D(ea), D(w1), D(w2), D(w3), D(w4)
    ref = torch.relu(torch.cat([torch.relu(er @ r1.t()), torch.tanh(er @ r2.t()) * torch.tanh(er @ r3.t())], 1) @ r4.t())
    go = torch.randn(E, So)
    (ref * go.double()).sum().backward()
    C = lambda t: t.to(dev).requires_grad_(True)
    ed, d1, d2, d3, d4 = C(ea), C(w1), C(w2), C(w3), C(w4)
    out = Fn.EdgeBranchWide.apply(ed, d1, d2, d3, d4)
    close(out, ref, tol=1e-5, what='wide edge branch S=%d So=%d' % (S, So))
    close(out, Fn._edge_branch_torch(ed, d1, d2, d3, d4), tol=1e-5, what='vs the library road')
    (out * go.to(dev)).sum().backward()
    for got, want, n in ((ed, er, 'ea'), (d1, r1, 'w1'), (d2, r2, 'w2'), (d3, r3, 'w3'), (d4, r4, 'w4')):
        close(got.grad, want.grad, what='grad ' + n)


# ------------------------------------------------------------------------------------------ models (H1-H5)
def _batch_from(g, dev):
    from gnn_matlang_amd.graph import Batch
    b = g.sub('batch/')
    ptr = np.concatenate([[0], np.cumsum(np.bincount(b['batch']))]).astype(np.int32)
    return Batch(x=T(b['x']), edge_index=T(b['edge_index']), edge_index2=T(b['edge_index2']),
                 edge_attr2=T(b['edge_attr2']), batch=T(b['batch']), ptr=T(ptr), y=T(b['y'])).to(dev)


@pytest.mark.parametrize('fname,ctor,loss', [
    ('model_zinc_gnnml3.npz', 'zinc_gnnml3', 'zinc_loss'),
    ('model_counting_gnnml3.npz', 'counting_gnnml3', 'counting_loss'),
    ('model_mutag_gnnml3.npz', 'mutag_gnnml3', 'mutag_loss'),
    pytest.param('model_mutag_gnnml1.npz', 'mutag_gnnml1', 'mutag_loss', id='model_mutag_gnnml1.npz-GNNML1Mutag-mutag_loss'),   # (the id it has always had)
])
def test_model_step_golden(dev, golden, fname, ctor, loss, arith):
    """logits, loss, every parameter gradient and the 5-step Adam loss trajectory against the reference's own outputs.
    Bar: 1e-4 of the tensor's scale in BOTH arithmetics, no exception: the first layer of a BatchNorm model (mutag GNNML3; its
    weight / bias gradients were 1.6e-4 / 1.3e-4 off in rounds 2-3, three BatchNorm backwards amplifying the split products'
    ~1e-5) runs on the exact-product kernels (models.GNNML3.forward, functional.exact_products)."""
    from gnn_matlang_amd import models
    g = golden(fname)
    data = _batch_from(g, dev)
    m = getattr(models, ctor)()
    m.load_state_dict({k: T(v) for k, v in g.sub('param/').items()})      # reference state_dict keys
    m = m.to(dev).train()
    loss_fn = getattr(models, loss)
    pre = m(data)
    l = loss_fn(pre, data.y)
    l.backward()
    close(pre, g['logits'], what='logits')
    assert abs(l.item() - float(g['loss'])) <= TOL * abs(float(g['loss']))
    for n, p in m.named_parameters():
        close(p.grad, g['grad/' + n], what='grad ' + n)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    traj = []
    for _ in range(5):
        opt.zero_grad()
        l = loss_fn(m(data), data.y)
        l.backward()
        opt.step()
        traj.append(l.item())
    np.testing.assert_allclose(traj, g['loss_traj'], rtol=TOL)


def test_sr25_isomorphism_golden(dev, golden, arith):
    """sr25.py:282-300 -- forward only, untrained nets, pairs never separated across seeds."""
    from gnn_matlang_amd import models
    g = golden('model_sr25_gnnml3.npz')
    data = _batch_from(g, dev)
    Mcnt = 0
    for seed in range(3):
        m = models.sr25_gnnml3()
        m.load_state_dict({k: T(v) for k, v in g.sub('seed%d/param/' % seed).items()})
        m = m.to(dev).eval()
        with torch.no_grad():
            E = m(data).cpu().numpy()
        close(E, g['seed%d/emb' % seed], what='sr25 embeddings seed %d' % seed)
        Mcnt = Mcnt + 1 * (np.abs(E[:, None] - E[None]).sum(2) > 0.001)
        assert int(((Mcnt == 0).sum() - 15) / 2) == int(g['seed%d/similar' % seed])


def test_sr25_gnnml1_sum_variant_golden(dev, golden):
    """sr25.py:192-246 with model = GNNML1() (sum form): embeddings and the `similar` count against the reference's"""
    from gnn_matlang_amd import models
    g = golden('model_sr25_gnnml1.npz')
    data = _batch_from(g, dev)
    Mcnt = 0
    for seed in range(3):
        m = models.sr25_gnnml1(2)
        m.load_state_dict({k: T(v) for k, v in g.sub('seed%d/param/' % seed).items()})
        m = m.to(dev).eval()
        with torch.no_grad():
            E = m(data).cpu().numpy()
        close(E, g['seed%d/emb' % seed], what='GNNML1 embeddings seed %d' % seed)
        Mcnt = Mcnt + 1 * (np.abs(E[:, None] - E[None]).sum(2) > 0.001)
        assert int(((Mcnt == 0).sum() - 15) / 2) == int(g['seed%d/similar' % seed])
    # the other assembly of the class (mnist75.py:262-326: relu, mean-pool, bn1, 32 -> 10) runs and trains
    m2 = models.mnist75_gnnml1(2).to(dev).train()
    out = m2(data)
    assert out.shape == (15, 10) and torch.isfinite(out).all()
    out[:, 0].sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m2.parameters())


def test_global_max_pool(dev):
    """gml_segment_max / _bwd (global_max_pool, enzymes.py:384) against torch: values, arg-max gradient routing, empty segment"""
    from gnn_matlang_amd import models
    from gnn_matlang_amd.graph import Batch
    rng = np.random.default_rng(11)
    sizes = [5, 1, 0, 17, 64, 3]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    x = torch.tensor(rng.standard_normal((ptr[-1], 13)).astype(np.float32), device=dev, requires_grad=True)
    data = Batch(x=x, ptr=T(ptr).to(dev), batch=T(np.repeat(np.arange(len(sizes)), sizes)).to(dev))
    out = models.global_max_pool(x, data)
    gout = torch.randn_like(out)
    (out * gout).sum().backward()
    xr = x.detach().clone().requires_grad_(True)
    ref = torch.stack([xr[ptr[i]:ptr[i + 1]].max(0)[0] if sizes[i] else torch.zeros(13, device=dev) for i in range(len(sizes))])
    (ref * gout).sum().backward()
    assert torch.equal(out, ref) and torch.equal(x.grad, xr.grad)


def test_mnist75_gnnml3_vs_oracle(dev, arith):
    """config 4 (TF DSGCNN: S=6 near-dense supports of 75-node graphs, widths 2->64->128->128, mean readout + BN):
    the TF reference cannot run here, so this config is checked against the CPU oracle only (parity unpinned by
    reference outputs); it exercises the wide-feature paths (multi-chunk forward, unfused backward)."""
    from gnn_matlang_amd import SpectralDesign, collate, models, synthetic
    from oracle import models_oracle as MO
    raw = synthetic.make_graphs('mnist75', 6, seed=9)
    host = collate(SpectralDesign(recfield=3, dv=10, nfreq=5).design_many(raw))      # prepareMnist_gnnml3_tf.py:14-17
    assert host.edge_attr2.shape[1] == 6
    data = host.to(dev)
    torch.manual_seed(3)
    ref = MO.mnist_gnnml3().train()
    m = models.mnist_gnnml3()
    m.load_state_dict(ref.state_dict())
    m = m.to(dev).train()
    pre_ref = ref(host.x, host.edge_index2, host.edge_attr2, host.batch, host.num_graphs)
    l_ref = MO.mnist_loss(pre_ref, host.y)
    l_ref.backward()
    pre = m(data)
    l = models.mnist_loss(pre, data.y)
    l.backward()
    close(pre, pre_ref, what='mnist logits')
    assert abs(l.item() - l_ref.item()) <= TOL * abs(l_ref.item())
    rp = dict(ref.named_parameters())
    for n, p in m.named_parameters():
        close(p.grad, rp[n].grad, tol=TOL, what='mnist grad ' + n)
    # dense-block evaluation (batched library GEMMs over [B, S*75, 75] support blocks): same parameters, same values
    md = models.mnist_gnnml3(dense_n=75)
    md.load_state_dict(ref.state_dict())
    md = md.to(dev).train()
    pre_d = md(data)
    ld = models.mnist_loss(pre_d, data.y)
    ld.backward()
    close(pre_d, pre_ref, what='mnist logits (dense blocks)')
    for n, p in md.named_parameters():
        close(p.grad, rp[n].grad, tol=TOL, what='mnist dense grad ' + n)


def test_mnist75_gnnml3_tf_golden(dev, golden, arith):
    """Config 4 against the fixture that restates the TensorFlow graph (libs/models_tf.py:223-268) in its dense-batched
    form (oracle/make_golden.py:gen_mnist_tf): logits, loss, every gradient; sparse kernels and the dense-block path."""
    from gnn_matlang_amd import models
    from gnn_matlang_amd.optim import TFAdam
    g = golden('model_mnist_gnnml3_tf.npz')
    data = _batch_from(g, dev)
    data.y = data.y.long()
    for dense_n in (0, 75):
        m = models.mnist_gnnml3(dense_n=dense_n)
        m.load_state_dict({k: T(v) for k, v in g.sub('param/').items()}, strict=False)
        m = m.to(dev).train()
        pre = m(data)
        l = models.mnist_loss(pre, data.y)
        l.backward()
        close(pre, g['logits'], what='logits dense_n=%d' % dense_n)
        assert abs(l.item() - float(g['loss'])) <= TOL * abs(float(g['loss']))
        for n, p in m.named_parameters():
            close(p.grad, g['grad/' + n], what='grad %s dense_n=%d' % (n, dense_n))
        opt = TFAdam(m.parameters(), lr=0.01)
        traj = []
        for _ in range(2):                                            # (later steps: see tests/test_oracle_golden.py)
            opt.zero_grad()
            l = models.mnist_loss(m(data), data.y)
            l.backward()
            opt.step()
            traj.append(l.item())
        # (lr = 0.01 Adam turns the round-off-level gradients of dead first-layer units into +-lr steps: the loss after ONE
        #  update already differs by ~1e-4 between any two float32 summation orders; tests/test_oracle_golden.py)
        np.testing.assert_allclose(traj[:1], g['loss_traj'][:1], rtol=TOL)       # before any update: the 1e-4 bar
        np.testing.assert_allclose(traj[1:], g['loss_traj'][1:2], rtol=5e-4)     # after ONE lr = 0.01 step (the oracle itself: 1.4e-4)


# ------------------------------------------------------------------------------------------ full size
def _big_zinc_batch(dev, ngraph_pool=512, reps=64):
    from gnn_matlang_amd import synthetic, SpectralDesign
    from gnn_matlang_amd.graph import collate
    raw = synthetic.make_graphs('zinc', ngraph_pool, seed=3)
    ds = SpectralDesign(recfield=2, dv=2, nfreq=7).design_many(raw)
    return collate(ds * reps).to(dev)


def test_full_size_properties(dev):
    """BASELINE-size ZINC-like batch (32768 graphs, ~0.75M nodes, ~4.9M support edges): properties that
    need no oracle -- bitwise run-to-run determinism (no atomics on the value path), linearity in x,
    fused forward == unfused SpMM + GEMM, the adjoint identity <A^T g, v> == <g, A v> between the backward's d/dx and the
    forward (SpectConv is linear in x: exact up to round-off, no finite-difference truncation), and agreement with the
    oracle on a slice of whole graphs."""
    from gnn_matlang_amd import ML3Layer, SpectConv, functional as Fn
    from oracle import spect_conv_oracle as O
    torch.manual_seed(0)
    data = _big_zinc_batch(dev)
    N = data.x.size(0)
    csr = data.csr()
    conv = SpectConv(25, 30, 8, selfconn=False).to(dev)
    y1 = conv(data.x, csr, data.edge_attr2)
    y2 = conv(data.x, csr, data.edge_attr2)
    assert torch.equal(y1, y2)                                             # deterministic
    x2 = torch.randn_like(data.x)
    ya = conv(data.x + 2 * x2, csr, data.edge_attr2) - conv.bias
    yb = (y1 - conv.bias) + 2 * (conv(x2, csr, data.edge_attr2) - conv.bias)
    close(ya, yb, what='linearity')
    val = csr.sort_values(data.edge_attr2)
    h = Fn.spmm(csr, val, data.x, 8, 25)
    yu = torch.addmm(conv.bias, h, conv.weight.view(8 * 25, 30))
    close(y1, yu, what='fused vs unfused')
    # adjoint identity: x.grad of sum(y * g) is A^T g; against a random direction v it must equal <g, A v>
    xg = data.x.clone().requires_grad_(True)
    gout, v = torch.randn_like(y1), torch.randn_like(data.x)
    (conv(xg, csr, data.edge_attr2) * gout).sum().backward()
    av = (conv(v, csr, data.edge_attr2) - conv.bias).double()
    lhs, rhs = (xg.grad.double() * v.double()).sum().detach(), (gout.double() * av).sum().detach()
    assert abs(float(lhs - rhs)) <= TOL * float((gout.double().norm() * av.norm()).detach()), ('adjoint identity', float(lhs), float(rhs))
    # oracle on the first 40 graphs (whole graphs: block-diagonal => independent of the rest)
    ng = 40
    n0 = int(data.ptr[ng])
    e_mask = (data.edge_index2[1] < n0)
    ei = data.edge_index2[:, e_mask].cpu()
    ea = data.edge_attr2[e_mask].cpu()
    layer = ML3Layer(True, 8, 8, 25, 30, 2).to(dev)
    out = layer(data.x, csr, data.edge_attr2)
    p = {n: v.detach().cpu() for n, v in layer.named_parameters()}
    ref = O.ml3layer_forward(data.x[:n0].cpu(), ei, ea, p, True, 2)
    close(out[:n0], ref, what='ML3Layer vs oracle on a slice')
    # gradients at full size: sharded evaluation must give the same parameter gradients
    out.square().sum().backward()
    gfull = {n: v.grad.clone() for n, v in layer.named_parameters()}
    layer.zero_grad()
    from gnn_matlang_amd.graph import GraphCSR
    half = int(data.ptr[data.num_graphs // 2])
    acc = None
    for lo, hi in ((0, half), (half, N)):
        m = (data.edge_index2[1] >= lo) & (data.edge_index2[1] < hi)
        ei_s = (data.edge_index2[:, m] - lo).contiguous()
        o = layer(data.x[lo:hi].contiguous(), GraphCSR.from_edge_index(ei_s, hi - lo), data.edge_attr2[m].contiguous())
        o.square().sum().backward()
    for n, v in layer.named_parameters():
        close(v.grad, gfull[n], tol=TOL, what='sharded grad ' + n)


def test_bench_size_train_step_vs_fp64_oracle(dev):
    """The HEADLINE arithmetic at the HEADLINE size -- bench.py's own batch, 131,072 ZINC-like graphs = 2,048 distinct graphs x 64 copies
    with a target each -- one train step, logits and EVERY parameter gradient against the oracle in float64 under the term-sum
    criterion (oracle/parity_at_size.py: the copies make one float64 pass over the pool the exact reference for the whole batch;
    T = the layer-local sums of |x| |val| |g| |w| products over all copies).  At the initial parameters AND after 100 Adam steps on
    the batch (weights grown, sums cancelling harder, nearly dead relu units: the state bench.py's own parity block is in after its
    timed steps).  sign(pre - y) and the head's relu mask are the device's own (see PS.reference).

    Round 6: the trained state is held to 1e-4 ON EVERY GRADIENT in the default arithmetic -- the carve-out
    of round 5 is gone.  What it took (tools/precision_diag.py, profiles/r06_precision_diag.jsonl): the FORWARD pass fp32-class
    (edge branch: three bf16 pieces + relative-accurate tanh; conv projection / Hadamard branch: f16 pieces under power-of-two
    scales); the backward kernels' bf16 pairs were measured not to matter.  The old all-bf16x3 arithmetic runs through the same
    check: held at the initial state and on the logits, its trained-state gradients (8.5e-3 of their term sums here) are printed."""
    import bench
    from gnn_matlang_amd import functional as Fn, models
    from oracle import parity_at_size as PS
    full, base = bench.build_batch(131072, 2048, 1000, dev)
    torch.manual_seed(0)
    m = models.zinc_gnnml3().to(dev)
    host = base.to(torch.device('cpu'))
    torch.cuda.synchronize()
    worst = {}
    for state in ('init', 'trained'):
        if state == 'trained':
            opt = torch.optim.Adam(m.parameters(), lr=1e-3)
            for _ in range(100):
                opt.zero_grad(set_to_none=True)
                models.zinc_loss(m(full), full.y).backward()
                opt.step()
        T = None
        for mode in ('default', 'bf16x3', 'f32'):
            m.zero_grad()
            keep = Fn.EDGE_FWD6, Fn.FWD_F16
            if mode == 'bf16x3':
                Fn.EDGE_FWD6 = Fn.FWD_F16 = False
            try:
                with Fn.exact_products(mode == 'f32'):
                    cap = {}
                    pre = m(full, _capture=cap)
                    models.zinc_loss(pre, full.y).backward()
            finally:
                Fn.EDGE_FWD6, Fn.FWD_F16 = keep
            ref = PS.reference(host, m.state_dict(), full.y, pre_dev=pre[:, 0], T=T, head_pre_dev=cap['head_pre'])
            T = ref['T']
            rep = PS.compare(ref, pre[:, 0].detach().cpu().numpy(), {n: p.grad.detach().cpu().numpy() for n, p in m.named_parameters()}, tol=TOL)
            worst[state, mode] = (rep['logits_rel_err'], rep['worst_termsum'], rep['worst_maxnorm'], ref['head_units_flipped'])
            bad = {n: v for n, v in rep['tensors'].items() if v['termsum'] > TOL}
            assert rep['logits_rel_err'] <= TOL, (state, mode, rep['logits_rel_err'])
            # every tensor, both states, in the default and the exact arithmetic; the all-bf16x3 arithmetic at the initial state only
            assert not (state == 'init' or mode != 'bf16x3') or not bad, (state, mode, bad)
    print('bench-size parity (logits, worst term-sum, worst max-norm, head units taken from the device):', worst)
    # the default arithmetic's trained-state gradients are fp32-class, not merely inside the bar
    assert worst['trained', 'default'][1] <= 3e-5, worst


# ------------------------------------------------------------------------------------------ randomised sweeps (short)
@pytest.mark.parametrize('sweep', ['ml3', 'conv', 'spectral'])
def test_randomised_sweep_short(dev, sweep):
    """A short run of tools/fuzz_parity.py (the long runs are in profiles/r01_i_fuzz_parity.jsonl): random shapes and
    graphs through every kernel family against the oracle in fp64."""
    import argparse
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tools'))
    import fuzz_parity
    a = argparse.Namespace(cases=24, seed=2026, only=-1, verbose=False, sweep=sweep)
    fails = {'ml3': lambda: fuzz_parity.ml3_sweep(a), 'conv': lambda: fuzz_parity.conv_sweep(a, dev),
             'spectral': lambda: fuzz_parity.spectral_sweep(a, dev)}[sweep]()
    assert fails == 0


# ------------------------------------------------------------------------------------------ drop-in behaviour (round 2)
def test_bad_node_ids_raise_like_the_reference(dev):
    """an edge_index entry outside [0, num_nodes) is an error (the reference's scatter raises an index error)"""
    from gnn_matlang_amd.graph import GraphCSR
    ei = torch.tensor([[0, 1, 2], [1, 2, 7]], device=dev)
    with pytest.raises(IndexError):
        GraphCSR.from_edge_index(ei, 4)
    GraphCSR.from_edge_index(torch.tensor([[0, 1, 2], [1, 2, 3]], device=dev), 4)


def test_wider_edge_attr_and_int64_ptr(dev):
    """the reference reads edge_attr[:, i] for i < K only (libs/spect_conv.py:77): wider inputs are legal and their
    gradient keeps the input's shape; PyG-style int64 segment pointers pool correctly"""
    from gnn_matlang_amd import SpectConv, ML3Layer
    from gnn_matlang_amd.functional import segment_sum
    from oracle import spect_conv_oracle as O
    rng = np.random.default_rng(5)
    N, E, K = 40, 160, 3
    ei = cu(rng.integers(0, N, size=(2, E)), dev)
    x = cu(rng.standard_normal((N, 6)).astype(np.float32), dev)
    ea = cu(rng.standard_normal((E, K + 2)).astype(np.float32), dev).requires_grad_(True)
    conv = SpectConv(6, 5, K, selfconn=False).to(dev)
    out = conv(x, ei, ea)
    out.square().sum().backward()
    assert ea.grad.shape == ea.shape and float(ea.grad[:, K:].abs().max()) == 0.0
    ref = O.OracleSpectConv(6, 5, K, selfconn=False)
    ref.load_state_dict({k: v.detach().cpu() for k, v in conv.state_dict().items()})
    ea_c = ea.detach().cpu().requires_grad_(True)
    out_r = ref(x.cpu(), ei.cpu(), ea_c)
    out_r.square().sum().backward()
    close(out, out_r, what='out')
    close(ea.grad, ea_c.grad, what='d edge_attr')
    lay = ML3Layer(False, K, K, 6, 8, 4).to(dev)                       # learnedge=False: conv1 reads the first K columns
    assert lay(x, ei, ea.detach()).shape == (N, 12)
    ptr64 = torch.tensor([0, 10, 25, 40], dtype=torch.int64, device=dev)
    pooled = segment_sum(x.contiguous(), ptr64)
    close(pooled, torch.stack([x[0:10].sum(0), x[10:25].sum(0), x[25:40].sum(0)]).cpu(), what='int64 ptr pooling')


def test_padded_static_batch_equals_plain_batch(dev):
    """dataset.DeviceDataset.batch_padded (static shapes, index build without a host read: what the captured epoch of
    bench.py replays) gives the same loss and parameter gradients as the plain batch of the same graphs."""
    from gnn_matlang_amd import SpectralDesign, models, synthetic
    from gnn_matlang_amd.dataset import DeviceDataset
    raw = synthetic.make_graphs('zinc', 40, seed=8)
    dsd = DeviceDataset.from_graphs(SpectralDesign(recfield=2, dv=2, nfreq=7).design_many(raw), dev)
    bd = dsd.bounds(8)
    ids = torch.tensor([5, 33, 0, 17, 21, 40, 40, 40], device=dev)              # 5 graphs + 3 absent slots
    torch.manual_seed(1)
    m = models.zinc_gnnml3().to(dev)
    bp = dsd.batch_padded(ids, bd)
    pre = m(bp)
    lp = ((pre[:8, 0] - bp.y[:8]).abs() * bp.graph_valid).sum()
    lp.backward()
    gp = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad()
    b = dsd.batch(ids[:5])
    l = models.zinc_loss(m(b), b.y)
    l.backward()
    assert abs(lp.item() - l.item()) <= 1e-5 * abs(l.item())
    for n, p in m.named_parameters():
        close(gp[n], p.grad, tol=2e-5, what='padded vs plain grad ' + n)


@pytest.mark.parametrize('padded', [False, True])
def test_fused_head_and_l1_loss_equals_the_plain_path(dev, padded):
    """models.zinc_step_loss (head + L1-sum loss as one launch each way, csrc/gml_head.hip; Zinc12k.py:343-345, :365) against
    zinc_loss(model(data)) through library calls: loss and every parameter gradient, on a plain batch and on a padded static batch
    (absent slots masked by graph_valid, padding graph ignored)."""
    from gnn_matlang_amd import SpectralDesign, models, synthetic
    from gnn_matlang_amd.dataset import DeviceDataset
    raw = synthetic.make_graphs('zinc', 40, seed=8)
    dsd = DeviceDataset.from_graphs(SpectralDesign(recfield=2, dv=2, nfreq=7).design_many(raw), dev)
    ids = torch.tensor([5, 33, 0, 17, 21, 40, 40, 40], device=dev)
    torch.manual_seed(1)
    m = models.zinc_gnnml3().to(dev)
    if padded:
        dsd.y = dsd.y.float()
        b = dsd.batch_padded(ids, dsd.bounds(8))
        pre = m(b)
        lp = ((pre[:8, 0] - b.y[:8]).abs() * b.graph_valid).sum()
    else:
        b = dsd.batch(ids[:5])
        lp = models.zinc_loss(m(b), b.y.float())
    lp.backward()
    gp = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad()
    lf = models.zinc_step_loss(m, b)
    assert lf.grad_fn is not None and 'HeadL1' in type(lf.grad_fn).__name__, 'the fused head did not run'
    lf.backward()
    assert abs(lp.item() - lf.item()) <= 1e-5 * abs(lp.item())
    for n, p in m.named_parameters():
        close(p.grad, gp[n], tol=2e-5, what='fused head vs plain path grad ' + n)
    # an upstream scale reaches every gradient through the kernel
    m.zero_grad()
    (0.25 * models.zinc_step_loss(m, b)).backward()
    for n, p in m.named_parameters():
        close(p.grad, 0.25 * gp[n], tol=2e-5, what='scaled ' + n)


@pytest.mark.parametrize('rows', [1, 255, 257, 1000, 70001])
def test_head_and_l1_loss_for_any_batch_size_vs_fp64(dev, rows):
    """functional.HeadL1BigFunction (csrc/gml_head_big.hip; Zinc12k.py:343-345, :365): loss and every gradient against the same
    head evaluated in fp64 by torch -- row counts around the 256-row tiles and beyond one tile per workgroup, rows that do not enter
    the loss (zero gradient), a validity mask, an upstream scale, the running loss sum, the deferred-fold road (bit-identical), and a
    bitwise repeat."""
    from gnn_matlang_amd import functional as Fn
    g = torch.Generator().manual_seed(rows)
    R, Rl = rows, max(rows - 3, 1) if rows > 1 else 1
    p = torch.randn(R, 32, generator=g).to(dev).requires_grad_(True)
    y = torch.randn(Rl, generator=g).to(dev)
    valid = (torch.rand(Rl, generator=g) > 0.2).float().to(dev)
    w1 = (torch.randn(32, 32, generator=g) * 0.3).to(dev).requires_grad_(True)
    b1 = (torch.randn(32, generator=g) * 0.3).to(dev).requires_grad_(True)
    w2 = (torch.randn(1, 32, generator=g) * 0.3).to(dev).requires_grad_(True)
    b2 = (torch.randn(1, generator=g) * 0.3).to(dev).requires_grad_(True)
    prm = [p, w1, b1, w2, b2]
    assert Fn.head_l1_big_supported(p, w1, w2)

    def ref():
        pd, w1d, b1d, w2d, b2d = [t.detach().double().requires_grad_(True) for t in prm]
        pre = torch.relu(pd @ w1d.t() + b1d) @ w2d.t() + b2d
        l = ((pre[:Rl, 0] - y.double()).abs() * valid.double()).sum()
        (0.5 * l).backward()
        return l, [pd.grad, w1d.grad, b1d.grad, w2d.grad, b2d.grad]

    def run(defer):
        for t in prm:
            t.grad = None
        acc = torch.full((1,), 2.0, device=dev)
        l = Fn.HeadL1BigFunction.apply(p, y, valid, w1, b1, w2, b2, acc)
        if defer:
            with Fn.deferred_folds(prm):
                (0.5 * l).backward()
        else:
            (0.5 * l).backward()
        assert abs(float(acc) - 2.0 - float(l.detach())) <= 1e-5 * max(abs(float(l.detach())), 1.0)
        return l.detach().clone(), [t.grad.clone() for t in prm]

    lr, gr = ref()
    l0, g0 = run(False)
    assert abs(float(l0) - float(lr)) <= 2e-6 * max(abs(float(lr)), 1.0), (float(l0), float(lr))
    for a, b, n in zip(g0, gr, ['p', 'w1', 'b1', 'w2', 'b2']):
        close(a, b, tol=2e-6, what='big head grad ' + n)
    assert not g0[0][Rl:].any()                                                   # rows outside the loss: zero gradient
    l1, g1 = run(True)
    assert torch.equal(l0, l1)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)


@pytest.mark.parametrize('model', ['zinc', 'counting'])
def test_deferred_folds_are_bit_identical(dev, model):
    """functional.deferred_folds (include/gml.h "Deferred folds": the partial-sum folds of a backward pass as ONE gml_fold_many launch)
    gives bitwise the gradients of the per-kernel folds -- conv weights (gml_k_reduce_rows), the output stage's sums
    (gml_k_split_fold) and the edge branch's four matrices (gml_k_reduce_partials; counting.py's 12 supports: the chain16 family)."""
    from gnn_matlang_amd import SpectralDesign, collate, functional as Fn, models, synthetic
    if model == 'zinc':
        raw = synthetic.make_graphs('zinc', 48, seed=3)
        b = collate(SpectralDesign(recfield=2, dv=2, nfreq=7).design_many(raw)).to(dev)
        torch.manual_seed(2)
        m, loss = models.zinc_gnnml3().to(dev), models.zinc_loss
    else:
        raw = synthetic.make_graphs('counting', 40, seed=3)
        b = collate(SpectralDesign(recfield=1, dv=1, nfreq=10, adddegree=True, laplacien=False, addadj=True).design_many(raw)).to(dev)
        torch.manual_seed(2)
        m, loss = models.counting_gnnml3().to(dev), models.counting_loss
    y = b.y.float() if b.y.dim() == 1 else b.y[:, 0].float()
    loss(m(b), y).backward()
    ref = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad()
    l = loss(m(b), y)
    seen = []
    flush = Fn.flush_folds
    Fn.flush_folds = lambda jobs: (seen.append(len(jobs)), flush(jobs))
    try:
        with Fn.deferred_folds(m.parameters()):
            l.backward()
    finally:
        Fn.flush_folds = flush
    assert seen and seen[0] >= 3 * m.nlayers - 1, ('the folds were not deferred', seen)     # conv + output stage + edge branch per layer
    for n, p in m.named_parameters():
        assert torch.equal(p.grad, ref[n]), 'deferred fold differs: ' + n


@pytest.mark.parametrize('fused_pool', [True, False])
def test_padded_batch_loss_that_touches_the_padding_row(dev, monkeypatch, fused_pool):
    """the padding graph's pooled row is WRITTEN as zeros (GML_POOL_SKIP_LAST), so it does not depend on x -- a loss that
    gives that row a gradient (here: every pooled row, the padding graph's included) must not send anything back to the padding
    nodes, whose features are relu(bias) != 0 after the first layer.  Both backward roads: the pool fused into the last layer
    (un-expanded gradient) and the stand-alone _SegmentPool."""
    from gnn_matlang_amd import SpectralDesign, models, synthetic
    from gnn_matlang_amd.dataset import DeviceDataset
    if not fused_pool:
        monkeypatch.setenv('GML_NO_POOL_FUSE', '1')
    raw = synthetic.make_graphs('zinc', 40, seed=8)
    dsd = DeviceDataset.from_graphs(SpectralDesign(recfield=2, dv=2, nfreq=7).design_many(raw), dev)
    bd = dsd.bounds(8)
    ids = torch.tensor([5, 33, 0, 17, 21, 40, 40, 40], device=dev)
    torch.manual_seed(1)
    m = models.zinc_gnnml3().to(dev)
    with torch.no_grad():
        for i in range(1, 5):
            getattr(m, 'conv%d' % i).conv1.bias.fill_(0.3)          # padding nodes carry relu(bias) > 0 from layer 1 on
    bp = dsd.batch_padded(ids, bd)
    pre = m(bp)                                                   # [8 + 1, 1]: the last row belongs to the padding graph
    assert pre.size(0) == 9
    lp = (pre[:8, 0] * bp.graph_valid).sum() + 7.0 * pre[8, 0]    # the padding row enters the loss with a non-zero gradient
    lp.backward()
    gp = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad()
    b = dsd.batch(ids[:5])
    l = m(b)[:, 0].sum()
    l.backward()
    for n, p in m.named_parameters():
        if n.startswith('fc'):
            continue                                              # the head does see the (constant) padding row
        close(gp[n], p.grad, tol=2e-5, what='padded (loss touches the padding row) vs plain grad ' + n)


@pytest.mark.parametrize('ids', [[5, 33, 0, 17, 21, 40, 40, 40], [39, 38, 37, 36, 35, 34, 33, 32], [40] * 8, [7, 40, 7, 7, 40, 3, 3, 7]])
def test_assembled_batch_is_bit_identical_to_the_padded_batch_and_its_index(dev, ids):
    """dataset.DeviceDataset.batch_assembled (csrc/gml_csr.hip gml_batch_assemble: one launch from the per-graph structure
    computed once per data set) against batch_padded + GraphCSR.from_edge_index on the same graph ids: every tensor of the
    batch and every array of both CSR views bit-identical, the index arrays also against oracle/csr_oracle.py; then the same
    loss and gradients through the model.  Absent slots, repeated graphs and the all-absent batch included."""
    from gnn_matlang_amd import SpectralDesign, models, synthetic
    from gnn_matlang_amd.dataset import DeviceDataset
    from oracle import csr_oracle
    raw = synthetic.make_graphs('zinc', 40, seed=8)
    dsd = DeviceDataset.from_graphs(SpectralDesign(recfield=2, dv=2, nfreq=7).design_many(raw), dev)
    dsd.y = dsd.y.float()
    bd = dsd.bounds(8)
    ids = torch.tensor(ids, device=dev)
    bp, ba = dsd.batch_padded(ids, bd), dsd.batch_assembled(ids, bd)
    for name in ('x', 'edge_attr2', 'y', 'graph_valid'):
        assert torch.equal(getattr(bp, name).float(), getattr(ba, name)), name
    assert torch.equal(bp.ptr.int(), ba.ptr) and torch.equal(bp.batch.int(), ba.batch)
    cp, ca = bp.csr('edge_index2'), ba.csr('edge_index2')
    for name in ('rowptr', 'col', 'perm', 'rowptr_t', 'col_t', 'perm_t', 'pos_t', 'tpos', 'ginfo128', 'ginfo_t128'):
        assert torch.equal(getattr(cp, name), getattr(ca, name)), name
    assert ca.gmax128 == cp.gmax128 and ca.gmax_t128 == cp.gmax_t128 and ca.src_sorted and cp.src_sorted and (ca.N, ca.E) == (cp.N, cp.E)
    ei = bp.edge_index2.cpu().numpy()
    rp, col, perm = csr_oracle.csr_from_coo(ei[0], ei[1], bd['n_pad'])
    assert np.array_equal(rp, ca.rowptr.cpu().numpy()) and np.array_equal(col, ca.col.cpu().numpy()) and np.array_equal(perm, ca.perm.cpu().numpy())
    rpt, colt, post = csr_oracle.transpose_view(ei[0], ei[1], bd['n_pad'], perm)
    assert np.array_equal(rpt, ca.rowptr_t.cpu().numpy()) and np.array_equal(colt, ca.col_t.cpu().numpy()) and np.array_equal(post, ca.pos_t.cpu().numpy())
    # the pre-split supports that travel with the assembled batch = the split of its supports
    from gnn_matlang_amd import functional as Fn
    assert torch.equal(ca.presplit(ba.edge_attr2), Fn.edge_presplit(bp.edge_attr2.contiguous()))
    torch.manual_seed(1)
    m = models.zinc_gnnml3().to(dev)
    out = []
    for b in (bp, ba):
        m.zero_grad()
        pre = m(b)
        l = ((pre[:8, 0] - b.y[:8]).abs() * b.graph_valid).sum()
        l.backward()
        out.append((l.item(), {n: p.grad.clone() for n, p in m.named_parameters()}))
    assert out[0][0] == out[1][0]
    for n in out[0][1]:
        assert torch.equal(out[0][1][n], out[1][1][n]), n


def test_static_epoch_covers_every_graph_once(dev):
    """DeviceDataset.epoch_static: every graph of the data set appears in exactly one batch slot, the rest are absent slots, every
    batch has the same padded shape, and the summed L1 loss over the epoch equals the plain epoch's (same model, no update)."""
    from gnn_matlang_amd import SpectralDesign, models, synthetic
    from gnn_matlang_amd.dataset import DeviceDataset
    raw = synthetic.make_graphs('zinc', 50, seed=18)
    dsd = DeviceDataset.from_graphs(SpectralDesign(recfield=2, dv=2, nfreq=7).design_many(raw), dev)
    dsd.y = dsd.y.float()
    torch.manual_seed(2)
    m = models.zinc_gnnml3().to(dev)
    tot_s, shapes, valid = 0.0, set(), 0
    with torch.no_grad():
        for b in dsd.epoch_static(16, generator=torch.Generator().manual_seed(4)):
            pre = m(b)
            tot_s += float(((pre[:16, 0] - b.y[:16]).abs() * b.graph_valid).sum())
            shapes.add((tuple(b.x.shape), tuple(b.edge_attr2.shape)))
            valid += int(b.graph_valid.sum())
        tot_p = sum(float(models.zinc_loss(m(b), b.y)) for b in dsd.epoch(16, generator=torch.Generator().manual_seed(4)))
    assert valid == 50 and len(shapes) == 1
    assert abs(tot_s - tot_p) <= 1e-5 * abs(tot_p)


# ------------------------------------------------------------------------------------------ dense-block support product
@pytest.mark.parametrize('n,S,F', [(75, 6, 2), (75, 6, 64), (75, 6, 128), (16, 1, 30), (33, 3, 7), (96, 2, 20), (5, 4, 48)])
def test_dense_support_mm_vs_fp64(dev, n, S, F):
    """gml_dense_support_mm (csrc/gml_dense.hip; libs/layers_tf.py:231 `matmul(support[:, i], x)` for every support of
    every graph) and its adjoint against fp64 einsum: ragged n (not a multiple of 16 / 32), F off the 4-alignment."""
    from gnn_matlang_amd import dense_block as DB
    g = torch.Generator().manual_seed(100 * n + F)
    B = 5
    blocks = (torch.randn(B, S, n, n, generator=g) * (torch.rand(B, S, n, n, generator=g) < 0.8)).to(dev)
    x = torch.randn(B * n, F, generator=g).to(dev).requires_grad_(True)
    sup = DB.DenseSupports(blocks, keep_blocks=False)
    h = DB._SupportProduct.apply(x, sup)
    ref = torch.einsum('bsji,bif->bjsf', blocks.double(), x.detach().double().view(B, n, F)).reshape(B * n, S * F)
    close(h, ref.float(), what='Hcat n=%d S=%d F=%d' % (n, S, F))
    gh = torch.randn(B * n, S * F, generator=g).to(dev)
    h.backward(gh)
    gref = torch.einsum('bsji,bjsf->bif', blocks.double(), gh.double().view(B, n, S, F)).reshape(B * n, F)
    close(x.grad, gref.float(), what='dX n=%d S=%d F=%d' % (n, S, F))
    # the packed images: hi + lo reproduces the block to 2^-16 relative, padding columns are zero
    img = sup.fwd.view(torch.bfloat16).float()
    rec = img[:, :, 0] + img[:, :, 1]
    assert float((rec[..., :n] - blocks).abs().max()) <= 2.0 ** -16 * float(blocks.abs().max())
    assert float(rec[..., n:].abs().max() if sup.KP > n else 0.0) == 0.0
    assert torch.equal(sup.bwd.view(torch.bfloat16)[..., :n], sup.fwd.view(torch.bfloat16)[..., :n].transpose(-1, -2))


def test_ml3_hadamard_dx_handover_matches_accumulate(dev, monkeypatch):
    """2 nout2 <= 4 (Zinc12k.py's 30+2 layers): the Hadamard branch's share of dx reaches the conv backward as dz [N, 4]
    (gml_ml3_split_bwd_ex + gml_spectconv_bwd_mix) instead of a written dx the conv kernel accumulates into: same gradients."""
    from gnn_matlang_amd import ML3Layer, functional as Fn
    rng = np.random.default_rng(21)
    torch.manual_seed(21)
    N, S = 700, 8
    ei = _random_graph(rng, N, 6)
    order = np.lexsort((ei[1], ei[0]))
    ei = ei[:, order]                                        # source-sorted, as SpectralDesign emits
    layer = ML3Layer(True, S, S, 32, 30, 2).to(dev)
    x0, ea = torch.randn(N, 32, device=dev), torch.randn(ei.shape[1], S, device=dev)
    gout = torch.randn(N, 32, device=dev)
    res = {}
    for mode in ('dz', 'accumulate'):
        if mode == 'accumulate':
            monkeypatch.setenv('GML_NO_DZ', '1')
        layer.zero_grad()
        x = x0.clone().requires_grad_(True)
        Fn.PATHS.clear()
        (layer(x, T(ei).to(dev), ea) * gout).sum().backward()
        res[mode] = [x.grad.clone()] + [p.grad.clone() for p in layer.parameters()]
    monkeypatch.delenv('GML_NO_DZ')
    from gnn_matlang_amd.graph import csr_for
    assert Fn.conv_bwd_takes_dz(csr_for(T(ei).to(dev), N), S, 32, 30, 4)          # the hand-over form did run
    for a, b in zip(res['dz'], res['accumulate']):
        close(a, b, tol=2e-5, what='dz hand-over vs accumulate')


def test_stacked_ml3_relu_handover_matches_unchained(dev, monkeypatch):
    """Two / three stacked ML3Layers declared with chain_after (Zinc12k.py:338-341): the upper layer's conv backward writes dx
    already multiplied by the lower layer's relu mask (gml_spectconv_bwd_mix_relu), the lower layer's output stage runs
    pre-masked (no saved-output read, no G array).  Same gradients as the unchained stack -- every tensor, including the
    lower layers' conv bias (column sums of the masked gradient) -- and the hand-over is dropped, not mis-applied, when the
    intermediate tensor is not the declared one (a clone in between)."""
    from gnn_matlang_amd import ML3Layer, functional as Fn
    rng = np.random.default_rng(41)
    torch.manual_seed(41)
    N, S = 900, 8
    ei = _random_graph(rng, N, 6)
    ei = ei[:, np.lexsort((ei[1], ei[0]))]                   # source-sorted, as SpectralDesign emits
    eit = T(ei).to(dev)
    layers = [ML3Layer(True, S, S, 25, 30, 2).to(dev), ML3Layer(True, S, S, 32, 30, 2).to(dev), ML3Layer(True, S, S, 32, 30, 2).to(dev)]
    x0, ea = torch.randn(N, 25, device=dev), torch.randn(ei.shape[1], S, device=dev)
    gout = torch.randn(N, 32, device=dev)

    def run(chained, clone_between=False):
        for i, l in enumerate(layers):
            l.zero_grad()
            l.chain_after(layers[i - 1] if (chained and i > 0) else None)
        x = x0.clone().requires_grad_(True)
        h = x
        Fn.PATHS.clear()
        for i, l in enumerate(layers):
            h = l(h, eit, ea)
            if clone_between and i == 0:
                h = h.clone()                                # a different tensor object: the declaration does not apply to it
        (h * gout).sum().backward()
        return [x.grad.clone()] + [p.grad.clone() for l in layers for p in l.parameters()]

    calls = []
    real = Fn.ml3_split_bwd
    monkeypatch.setattr(Fn, 'ml3_split_bwd', lambda *a, **k: (calls.append(bool(k.get('premasked'))), real(*a, **k))[1])
    monkeypatch.setattr(Fn, 'BWD_HAD', False)                # the two-launch form first: output stage, then conv backward
    ref = run(False)
    assert calls == [False, False, False]
    del calls[:]
    got = run(True)
    assert calls == [False, True, True], calls               # (backward order: top layer first; the two below ran pre-masked)
    for a, b in zip(got, ref):
        close(a, b, tol=1e-6, what='relu hand-over vs unchained')
    del calls[:]
    got = run(True, clone_between=True)
    assert calls == [False, True, False], calls
    for a, b in zip(got, ref):
        close(a, b, tol=1e-6, what='relu hand-over with a foreign tensor in between')
    # the pre-masked layers' output stage inside their conv backward (gml_spectconv_bwd_had; the default): they make no output-stage
    # launch at all; fc11 / fc12 weight gradients move to bf16x3 products, so the comparison is at 2e-5 of each tensor's scale
    monkeypatch.setattr(Fn, 'BWD_HAD', True)
    del calls[:]
    got = run(True)
    assert calls == [False, True], calls                     # (top layer; the first layer's input WANTS a gradient in this test and its 25
                                                             #  features are not a multiple of 4 -- no dz form: it keeps the one-pass kernel)
    for a, b in zip(got, ref):
        close(a, b, tol=2e-5, what='relu hand-over, output stage inside the conv backward, vs unchained')
    del calls[:]
    got = run(True, clone_between=True)
    assert calls == [False, False], calls                    # (top layer, and the first layer whose hand-over was dropped)
    for a, b in zip(got, ref):
        close(a, b, tol=2e-5, what='output stage inside the conv backward with a foreign tensor in between')


def test_relu_handover_below_a_layer_without_hadamard_branch(dev, monkeypatch):
    """The lower layer of a declared pair has no Hadamard branch (nout2 = 0: its output is all relu(conv) columns, 32 of them):
    its output stage then runs the mask-and-bias-sums kernel in its pre-masked form.  Same gradients as undeclared."""
    from gnn_matlang_amd import ML3Layer, functional as Fn
    rng = np.random.default_rng(47)
    torch.manual_seed(47)
    N, S = 500, 8
    ei = _random_graph(rng, N, 5)
    ei = ei[:, np.lexsort((ei[1], ei[0]))]
    eit = T(ei).to(dev)
    lower, upper = ML3Layer(True, S, S, 20, 32, 0).to(dev), ML3Layer(True, S, S, 32, 30, 2).to(dev)
    x0, ea = torch.randn(N, 20, device=dev), torch.randn(ei.shape[1], S, device=dev)
    gout = torch.randn(N, 32, device=dev)
    calls = []
    real = Fn.ml3_split_bwd
    monkeypatch.setattr(Fn, 'ml3_split_bwd', lambda *a, **k: (calls.append(bool(k.get('premasked'))), real(*a, **k))[1])

    def run(chained):
        upper.chain_after(lower if chained else None)
        for l in (lower, upper):
            l.zero_grad()
        x = x0.clone().requires_grad_(True)
        (upper(lower(x, eit, ea), eit, ea) * gout).sum().backward()
        return [x.grad.clone()] + [p.grad.clone() for l in (lower, upper) for p in l.parameters()]

    ref = run(False)
    del calls[:]
    got = run(True)
    assert calls == [False, True], calls
    for a, b in zip(got, ref):
        close(a, b, tol=1e-6, what='relu hand-over below a plain relu(conv) layer')


@pytest.mark.parametrize('S,nl', [(8, 4), (8, 2), (4, 3)])
def test_stacked_edge_branches_in_one_pass(dev, monkeypatch, S, nl):
    """Layers declared with chain_after read the same raw supports (Zinc12k.py:338-341): the first layer's forward computes the
    edge branches of the whole stack in one pass (gml_edge_mlp_fwd_stack) and the others pick theirs up.  Outputs and every
    gradient are bit-identical to the per-layer launches (same arithmetic, same order); a weight update between two forwards
    invalidates what was stashed (version check)."""
    from gnn_matlang_amd import ML3Layer, functional as Fn
    rng = np.random.default_rng(43)
    torch.manual_seed(43)
    N = 700
    ei = _random_graph(rng, N, 5)
    ei = ei[:, np.lexsort((ei[1], ei[0]))]                   # source-sorted, as SpectralDesign emits
    eit = T(ei).to(dev)
    layers = [ML3Layer(True, S, S, 32, 30, 2).to(dev) for _ in range(nl)]
    for i in range(1, nl):
        layers[i].chain_after(layers[i - 1])
    x0, ea = torch.randn(N, 32, device=dev), torch.randn(ei.shape[1], S, device=dev)
    gout = torch.randn(N, 32, device=dev)

    monkeypatch.setattr(Fn, 'VERBOSE', True)                 # (Fn.PATHS is filled)

    def run(stack):
        monkeypatch.setattr(Fn, 'EDGE_STACK', stack)
        for l in layers:
            l.zero_grad()
        x = x0.clone().requires_grad_(True)
        Fn.PATHS.clear()
        h = x
        for l in layers:
            h = l(h, eit, ea)
        (h * gout).sum().backward()
        return [h.detach().clone(), x.grad.clone()] + [p.grad.clone() for l in layers for p in l.parameters()], dict(Fn.PATHS)

    ref, paths0 = run(False)
    got, paths1 = run(True)
    assert not any('stack of' in k for k in paths0)
    assert any('stack of %d layers' % nl in k for k in paths1), paths1
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    # stale stash: forward the first layer only (stashes for the others), change a weight of layer 2, then run the stack
    monkeypatch.setattr(Fn, 'EDGE_STACK', True)
    layers[0](x0.clone().requires_grad_(True), eit, ea)
    with torch.no_grad():
        layers[1].fc1_4.weight.mul_(1.25)
    got2, _ = run(True)
    ref2, _ = run(False)
    for a, b in zip(got2, ref2):
        assert torch.equal(a, b)


@pytest.mark.parametrize('mean', [False, True])
def test_ml3_forward_pooled_matches_layer_then_pool(dev, mean):
    """ML3Layer.forward_pooled (the layer and the global add / mean pool that follows it as one autograd node: the pool's
    gradient is consumed un-expanded by gml_ml3_split_bwd_ex) against the layer followed by the pooling op."""
    from gnn_matlang_amd import ML3Layer, models
    from gnn_matlang_amd.graph import Batch
    rng = np.random.default_rng(31)
    torch.manual_seed(31)
    sizes = torch.tensor([5, 1, 17, 0, 64, 3, 130, 2])              # (one empty graph)
    N = int(sizes.sum())
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)]).int().to(dev)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), sizes).to(dev)
    ei = _random_graph(rng, N, 5)
    ei = ei[:, np.lexsort((ei[1], ei[0]))]
    layer = ML3Layer(True, 8, 8, 32, 30, 2).to(dev)
    x0, ea = torch.randn(N, 32, device=dev), torch.randn(ei.shape[1], 8, device=dev)
    gp = torch.randn(len(sizes), 32, device=dev)
    data = Batch(x=x0, edge_index=T(ei).to(dev), edge_index2=T(ei).to(dev), edge_attr2=ea, batch=batch, ptr=ptr, y=torch.zeros(len(sizes), device=dev))
    res = []
    for fused in (True, False):
        layer.zero_grad()
        x = x0.clone().requires_grad_(True)
        if fused:
            out = layer.forward_pooled(x, T(ei).to(dev), ea, ptr, batch.int(), mean)
        else:
            out = (models.global_mean_pool if mean else models.global_add_pool)(layer(x, T(ei).to(dev), ea), data)
        (out * gp).sum().backward()
        res.append([out.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in layer.parameters()])
    assert torch.equal(res[0][0], res[1][0])                             # same kernels forward: same bits
    for a, b in zip(res[0][1:], res[1][1:]):
        close(a, b, tol=2e-5, what='pooled layer vs layer + pool (mean=%s)' % mean)


# ------------------------------------------------------------------------------------------ term-sum criterion
def _termsum_close(got, ref, tsum, what):
    """|got - ref| <= 1e-4 * T elementwise, T = the sum of the ABSOLUTE values of the terms the element is a sum of (fp64).
    n u T bounds the round-off of ANY fp32 evaluation order of that sum -- the reference's own included -- so this bar stays
    meaningful for elements whose terms cancel, which the max-norm metric of ``close`` averages away."""
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref, t = np.asarray(ref, np.float64), np.asarray(tsum, np.float64)
    bad = np.abs(got - ref) > TOL * t + 1e-30
    assert not bad.any(), '%s: %d elements beyond 1e-4 of their term sum, worst %.3e' % (
        what, int(bad.sum()), float((np.abs(got - ref) / np.maximum(t, 1e-300)).max()))


def test_spectconv_golden_termsum(dev, golden, arith):
    """forward output and d/dx of every default-branch SpectConv golden case against the reference's vectors under the
    term-sum criterion: T_out = sum_s sum_e |val| |x[src]| |W_s| (+ |x| |W_self| + |b|), T_gx = sum_s sum_e |val| (|gout[dst]| |W_s|^T)"""
    from gnn_matlang_amd import SpectConv
    from oracle.spect_conv_oracle import spectconv_forward
    g = golden('spectconv.npz')
    for k in range(int(g['ncases'])):
        c = g.sub('case%03d/' % k)
        S, fin, fout, selfconn, depthwise, bias = [int(v) for v in c['meta']]
        if depthwise:
            continue                                      # (mapped onto the default branch through a weight transform)
        m = SpectConv(fin, fout, S, selfconn=bool(selfconn), bias=bool(bias)).to(dev)
        sd = {'weight': T(c['weight'])}
        if bias:
            sd['bias'] = T(c['bias'])
        m.load_state_dict(sd)
        x = cu(c['x'], dev).requires_grad_(True)
        y = m(x, cu(c['edge_index'], dev), cu(c['edge_attr'], dev))
        (y * cu(c['gout'], dev)).sum().backward()
        xa, va, wa = T(c['x']).double().abs(), T(c['edge_attr']).double().abs(), T(c['weight']).double().abs()
        ei = T(c['edge_index'])
        t_out = spectconv_forward(xa, ei, va, wa, T(c['bias']).double().abs() if bias else None, selfconn=bool(selfconn))
        ga = T(c['gout']).double().abs()
        t_gx = torch.zeros_like(xa)
        ns = wa.size(0) - (1 if selfconn else 0)
        for s in range(ns):
            t_gx.index_add_(0, ei[0], va[:, s:s + 1] * (ga @ wa[s].t())[ei[1]])
        if selfconn:
            t_gx += ga @ wa[-1].t()
        what = 'case %d meta %s' % (k, c['meta'])
        _termsum_close(y, c['out'], t_out.numpy(), what + ' out')
        _termsum_close(x.grad, c['g_x'], t_gx.numpy(), what + ' g_x')


def _ml3_termsums(c):
    """oracle/termsums.py on a golden case (dict view of the fixture)."""
    from oracle.termsums import ml3_termsums
    D = lambda a: T(a).double()
    P = {n[len('param/'):]: D(v) for n, v in c.items() if n.startswith('param/')}
    return ml3_termsums(c['meta'], D(c['x']), D(c['edge_attr']), T(c['edge_index']), D(c['gout']), P)


def test_ml3layer_golden_termsum(dev, golden, arith):
    """every ML3Layer golden case (libs/spect_conv.py:162-212 run by the reference itself): output, d/dx, d/d edge_attr and EVERY
    parameter gradient -- the edge branch's four weight matrices and the Hadamard branch's included -- elementwise within 1e-4 of
    the element's own term sum (the max-norm `close` of test_ml3layer_golden averages cancelling elements away)."""
    from gnn_matlang_amd import ML3Layer
    g = golden('ml3layer.npz')
    for k in range(int(g['ncases'])):
        c = g.sub('case%03d/' % k)
        learnedge, ne, neo, ninp, nout1, nout2 = [int(v) for v in c['meta']]
        m = ML3Layer(bool(learnedge), ne, neo, ninp, nout1, nout2).to(dev)
        m.load_state_dict({n[len('param/'):]: T(v) for n, v in c.items() if n.startswith('param/')})
        x = cu(c['x'], dev).requires_grad_(True)
        ea = cu(c['edge_attr'], dev).requires_grad_(True)
        y = m(x, cu(c['edge_index'], dev), ea)
        (y * cu(c['gout'], dev)).sum().backward()
        ts = _ml3_termsums(c)
        what = 'ml3 case %d %s ' % (k, c['meta'])
        _termsum_close(y, c['out'], ts['out'], what + 'out')
        _termsum_close(x.grad, c['g_x'], ts['g_x'], what + 'g_x')
        _termsum_close(ea.grad, c['g_edge_attr'], ts['g_edge_attr'], what + 'g_edge_attr')
        for n, p in m.named_parameters():
            _termsum_close(p.grad, c['grad/' + n], ts[n], what + n)


def test_tanh_approximation_bound(dev):
    """gml_tanh (csrc/gml_common.h: 1 - 2 / (exp2(2 log2(e) x) + 1) on v_exp_f32 / v_rcp_f32) against tanh in fp64 through the
    Hadamard-branch kernel (out = tanh(x w11 + b11) * tanh(x w12 + b12) with w11 = 1, w12 = 0, b12 = large: the second
    factor is 1 to the last bit): absolute error <= 4e-7 over [-12, 12] -- a few ulp of 1.0, the bound DESIGN s6 states."""
    from gnn_matlang_amd import functional as Fn, _lib
    from gnn_matlang_amd.graph import _ptr, _stream
    n = 1 << 16
    xs = torch.linspace(-12, 12, n, dtype=torch.float64)
    xs = torch.cat([xs, torch.tensor([0.0, 1e-4, -1e-4, 1e-8, 30.0, -30.0], dtype=torch.float64)])
    x = xs.float().view(-1, 1).contiguous().to(dev)
    w11 = torch.ones(1, 1, device=dev)
    b11 = torch.zeros(1, device=dev)
    w12 = torch.zeros(1, 1, device=dev)
    b12 = torch.full((1,), 40.0, device=dev)
    out = torch.empty(x.size(0), 1, device=dev)
    _lib.call('gml_node_mix_fwd', _ptr(x), 1, _ptr(w11), _ptr(b11), _ptr(w12), _ptr(b12), _ptr(out), 1, x.size(0), 1, 1, _stream(dev))
    ref = torch.tanh(x.cpu().double().view(-1))
    err = (out.cpu().double().view(-1) - ref).abs().max().item()
    assert err <= 4e-7, 'tanh approximation: max abs error %.3e' % err


@pytest.mark.parametrize('deg', [3, 13, 40])
def test_spmm_ring_kernel_any_support_count(dev, deg):
    """gml_spmm_fwd on the LDS-DMA ring kernel (csrc/gml_spmm3_impl.h): any S (value rows of 4 .. 192 bytes, every alignment
    class), any Fin % 4 == 0 (feature chunks of 32), row degrees from sparse to beyond the staging capacity (deg = 40: blocks
    that gather from global memory), partly filled last groups -- against the oracle's propagate (libs/spect_conv.py:77)."""
    from gnn_matlang_amd import functional as Fn
    from gnn_matlang_amd.graph import GraphCSR
    from oracle import spect_conv_oracle as O
    rng = np.random.default_rng(deg)
    torch.manual_seed(deg)
    for N in (333, 1000):
        dst = np.repeat(np.arange(N), rng.integers(max(deg - 3, 0), deg + 4, N))
        lo = np.maximum(dst - 30, 0)
        src = lo + rng.integers(0, 61, dst.size) % np.minimum(61, N - lo)          # banded like a block-diagonal batch
        o = np.lexsort((dst, src))
        ei = np.stack([src[o], dst[o]]).astype(np.int64)
        csr = GraphCSR.from_edge_index(T(ei).to(dev), N)
        for S, fin in ((6, 32), (12, 48), (24, 32), (48, 32), (48, 48), (1, 4), (2, 20), (3, 32), (5, 64), (7, 8), (16, 12)):
            ea, x = torch.randn(ei.shape[1], S), torch.randn(N, fin)
            val = csr.sort_values(ea.to(dev), cache=False)
            h = Fn.spmm(csr, val, x.to(dev), S, fin).view(N, S, fin)
            href = torch.stack([O.propagate_add(x.double(), T(ei), ea[:, s].double()) for s in range(S)], 1)
            close(h, href, what='spmm ring N=%d deg=%d S=%d Fin=%d' % (N, deg, S, fin))


@pytest.mark.parametrize('n,S,Fin,Fout', [(75, 6, 2, 64), (75, 6, 64, 128), (75, 6, 128, 128), (40, 3, 20, 24), (96, 2, 33, 70)])
def test_dense_weight_gradient_kernel_vs_fp64(dev, monkeypatch, n, S, Fin, Fout):
    """gml_dense_conv_bwd_w (csrc/gml_dense.hip: dW without Hcat and without a library GEMM -- VERDICT r04 item 7; opt-in through
    GML_DENSE_DW_HIP, see dense_block.py for the measured reason) against fp64 einsum, MNIST-75's three layer shapes + ragged ones."""
    from gnn_matlang_amd import dense_block as DB
    monkeypatch.setattr(DB, 'DW_LIBRARY', False)
    g = torch.Generator().manual_seed(n + Fin + 3 * Fout)
    B = 70                                                   # (more graphs than slices: several graphs per workgroup, a ragged last slice)
    blocks = (torch.randn(B, S, n, n, generator=g) * (torch.rand(B, S, n, n, generator=g) < 0.8)).to(dev)
    x = torch.randn(B * n, Fin, generator=g).to(dev)
    w = (torch.randn(S, Fin, Fout, generator=g) * 0.3).to(dev).requires_grad_(True)
    sup = DB.DenseSupports(blocks, keep_blocks=False)
    out = DB._DenseConv.apply(x, w, None, sup)
    go = torch.randn(B * n, Fout, generator=g).to(dev)
    out.backward(go)
    h = torch.einsum('bsji,bif->bjsf', blocks.double(), x.double().view(B, n, Fin))
    close(w.grad, torch.einsum('bjsf,bjo->sfo', h, go.double().view(B, n, Fout)).float(), what='dW without Hcat n=%d S=%d %d->%d' % (n, S, Fin, Fout))


@pytest.mark.parametrize('n,S,Fin,Fout', [(75, 6, 2, 64), (75, 6, 64, 128), (75, 6, 128, 128), (5, 4, 48, 10), (33, 3, 7, 30), (64, 2, 20, 64),
                                           (96, 2, 33, 100), (20, 1, 16, 16)])
def test_dense_conv_chained_vs_fp64(dev, n, S, Fin, Fout):
    """gml_dense_conv_fwd (csrc/gml_dense.hip: support product and projection in one launch, libs/layers_tf.py:231-236) through
    dense_block._DenseConv: output, Hcat-based weight gradient and dX against fp64 einsum; ragged n, odd widths, mixed n in one
    process (the big-LDS attribute of the kernels latches per device)."""
    from gnn_matlang_amd import dense_block as DB
    g = torch.Generator().manual_seed(7 * n + Fin + Fout)
    B = 4
    blocks = (torch.randn(B, S, n, n, generator=g) * (torch.rand(B, S, n, n, generator=g) < 0.8)).to(dev)
    x = torch.randn(B * n, Fin, generator=g).to(dev).requires_grad_(True)
    w = (torch.randn(S, Fin, Fout, generator=g) * 0.3).to(dev).requires_grad_(True)
    b = torch.randn(Fout, generator=g).to(dev).requires_grad_(True)
    sup = DB.DenseSupports(blocks, keep_blocks=False)
    out = DB._DenseConv.apply(x, w, b, sup)
    h = torch.einsum('bsji,bif->bjsf', blocks.double(), x.detach().double().view(B, n, Fin))
    ref = torch.einsum('bjsf,sfo->bjo', h, w.detach().double()).reshape(B * n, Fout) + b.detach().double()
    close(out, ref.float(), what='chained out n=%d S=%d %d->%d' % (n, S, Fin, Fout))
    go = torch.randn(B * n, Fout, generator=g).to(dev)
    out.backward(go)
    gd = go.double().view(B, n, Fout)
    close(w.grad, torch.einsum('bjsf,bjo->sfo', h, gd).float(), what='chained dW')
    close(b.grad, gd.sum((0, 1)).float(), what='chained db')
    dh = torch.einsum('bjo,sfo->bjsf', gd, w.detach().double())
    close(x.grad, torch.einsum('bsji,bjsf->bif', blocks.double(), dh).reshape(B * n, Fin).float(), what='chained dX')


def test_static_caps_csr_deferred_check(dev):
    """GraphCSR built with static_caps reads nothing back (capturable); check() reports what the index kernels flagged"""
    from gnn_matlang_amd.graph import GraphCSR
    ei = torch.tensor([[0, 0, 1, 2, 2], [0, 1, 1, 0, 2]], device=dev)
    GraphCSR.from_edge_index(ei, 3, static_caps=(8, 8)).check()                       # sorted, in range: fine
    bad = GraphCSR.from_edge_index(torch.tensor([[1, 0, 2], [0, 1, 2]], device=dev), 3, static_caps=(8, 8))
    with pytest.raises(ValueError):
        bad.check()
    oob = GraphCSR.from_edge_index(torch.tensor([[0, 1, 2], [0, 7, 2]], device=dev), 3, static_caps=(8, 8))
    with pytest.raises(IndexError):
        oob.check()


def test_captured_layer_with_unpadded_rows_reads_fresh_data_on_replay(dev):
    """functional.rows4 keeps a zero-padded copy of a first-layer input whose rows are not float4-addressable
    (Zinc12k.py's 25 features).  Under HIP-graph capture the copy must be RECORDED in the graph, not served from that cache:
    capture a layer on a static x, copy new data into it, replay, compare with eager on the new data."""
    from gnn_matlang_amd import ML3Layer
    rng = np.random.default_rng(5)
    torch.manual_seed(5)
    N = 300
    ei = _random_graph(rng, N, 5)
    eit = T(ei).to(dev)
    layer = ML3Layer(True, 8, 8, 25, 30, 2).to(dev)
    ea = torch.randn(ei.shape[1], 8, device=dev)
    static_x = torch.randn(N, 25, device=dev)
    with torch.no_grad():
        for _ in range(2):
            layer(static_x, eit, ea)                          # warm-up: fills the cache for this tensor object
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = layer(static_x, eit, ea)
        new = torch.randn(N, 25, device=dev)
        static_x.copy_(new)
        g.replay()
        torch.cuda.synchronize()
        ref = layer(new.clone(), eit, ea)
    assert torch.equal(out, ref)


def test_stacked_edge_branch_not_served_after_inplace_edit_of_the_supports(dev, monkeypatch):
    """the edge-branch outputs the head of a stack computes for the layers stacked on it are keyed by the
    supports' buffer AND version: an in-place edit of edge_attr between two layers of a declared stack must not be answered with
    the branch output of the old supports."""
    from gnn_matlang_amd import ML3Layer, functional as Fn
    rng = np.random.default_rng(44)
    torch.manual_seed(44)
    N = 400
    ei = _random_graph(rng, N, 5)
    ei = ei[:, np.lexsort((ei[1], ei[0]))]
    eit = T(ei).to(dev)
    l1, l2 = ML3Layer(True, 8, 8, 32, 30, 2).to(dev), ML3Layer(True, 8, 8, 32, 30, 2).to(dev)
    l2.chain_after(l1)
    monkeypatch.setattr(Fn, 'EDGE_STACK', True)
    x0 = torch.randn(N, 32, device=dev)
    ea = torch.randn(ei.shape[1], 8, device=dev)
    h = l1(x0.clone().requires_grad_(True), eit, ea)          # stashes l2's branch output for THESE supports
    with torch.no_grad():
        ea.mul_(0.5)                                          # same buffer, new contents
    got = l2(h, eit, ea)
    monkeypatch.setattr(Fn, 'EDGE_STACK', False)
    ref = l2(h.detach().clone().requires_grad_(True), eit, ea.clone())
    assert torch.equal(got.detach(), ref.detach())


def _banded_graph(rng, N, deg, spread):
    """every node draws `deg` neighbours within +-spread (duplicates removed): up to min(deg, 2 spread + 1) entries per row and
    a column window of 128 + 2 spread rows per 128-row group; source-sorted like SpectralDesign's output"""
    src = np.repeat(np.arange(N), deg)
    dst = np.clip(src + rng.integers(-spread, spread + 1, size=src.shape), 0, N - 1)
    return np.unique(np.vstack((src, dst)), axis=1).astype(np.int64)


@pytest.mark.parametrize('S,fin,fout,deg,spread', [
    (6, 48, 32, 13, 12),     # sr25.py:252-262 hidden layers: 6 supports, 48 features, 13 entries per row -> 3 edge chunks per group
    (6, 2, 32, 13, 12),      # sr25's first layer (2 features, rows padded to float4)
    (6, 32, 32, 40, 30),     # ~ 30 entries per row: 5-6 chunks, window 188 rows
    (6, 48, 24, 40, 30),
    (4, 48, 24, 5, 6),       # mutag.py:272-288 hidden layers: 4 supports, 48 features
    (4, 40, 24, 40, 30),
    (8, 32, 30, 40, 30),     # a ZINC-shaped layer on high-degree groups: the caller's hint routes it to the chunked kernel
    (4, 32, 16, 40, 30),
    (6, 48, 32, 40, 100),    # window of 328 rows: beyond what the chunked ring stages -> functional.fwd_groups keeps the 64-row family
    (8, 20, 30, 30, 100),
])
def test_chunked_ring_forward_any_degree(dev, monkeypatch, S, fin, fout, deg, spread):
    """gml_k_spectconv_fwd4 (the chunked road is opt-in, functional.FWD_CHUNKS -- switched on here): groups with more edges than one LDS edge buffer are walked in chunks with the
    accumulators kept across them; 6 supports (24-byte value rows) and 48 input features (third 16-wide feature block); against
    the oracle, forward and every gradient (the backward rides along on whatever kernel serves the shape)."""
    from gnn_matlang_amd import SpectConv, functional as Fn
    from oracle import spect_conv_oracle as O
    monkeypatch.setattr(Fn, 'FWD_CHUNKS', True)
    rng = np.random.default_rng(S * 100 + deg + fin)
    torch.manual_seed(deg + fin)
    N = 700                                               # 5.5 groups: the ring runs over several items per workgroup
    ei = _banded_graph(rng, N, deg, spread)
    ei = ei[:, ei[1] != 130]                              # an empty target row inside the second group
    ea, x = torch.randn(ei.shape[1], S), torch.randn(N, fin)
    m = SpectConv(fin, fout, S, selfconn=False).to(dev)
    with torch.no_grad():
        m.bias.uniform_(-0.5, 0.5)
    w, b = m.weight.detach().cpu(), m.bias.detach().cpu()
    xo, eo, wo = (t.clone().requires_grad_(True) for t in (x, ea, w))
    yo = O.spectconv_forward(xo, T(ei), eo, wo, b, False)
    gout = torch.randn_like(yo)
    (yo * gout).sum().backward()
    old = Fn.VERBOSE
    Fn.VERBOSE = True
    Fn.PATHS.clear()
    try:
        xg, eg = x.to(dev).requires_grad_(True), ea.to(dev).requires_grad_(True)
        y = m(xg, T(ei).to(dev), eg)
        paths = dict(Fn.PATHS)
    finally:
        Fn.VERBOSE = old
    if spread <= 30:
        assert any('8-wave' in k for k in paths), paths    # (not the 4-wave / 64-row family)
    else:                                                 # a window the ring cannot stage: the caller keeps the batch on the 64-row family
        assert not any('8-wave' in k for k in paths) or S == 8 and fin <= 32, paths
    close(y, yo, what='out')
    (y * gout.to(dev)).sum().backward()
    close(xg.grad, xo.grad, what='g_x')
    close(eg.grad, eo.grad, what='g_edge_attr')
    close(m.weight.grad, wo.grad, what='g_weight')


@pytest.mark.parametrize('chunks', [False, True])
@pytest.mark.parametrize('ne,Fin,n1,n2,deg', [(6, 48, 32, 16, 13), (6, 2, 32, 16, 13), (6, 48, 32, 16, 3), (4, 48, 24, 24, 4), (6, 48, 32, 16, 40)])
def test_ml3layer_sr25_shapes_with_learned_supports(dev, monkeypatch, ne, Fin, n1, n2, deg, chunks):
    """ML3Layer at sr25.py:252-262's shapes (6 supports, 2 -> 48 -> 48, 32 + 16) and mutag.py's (24 + 24), training with the edge
    branch: the branch runs in source order and the chunked ring forward gathers its 24-byte value rows through the position
    map (two overlapping 16-byte lanes per row); against the oracle in fp64.  deg 40: five chunks per group forward (one X window),
    a backward beyond the 8-wave kernel's 16 staged edges per row (the 64-row family)."""
    from gnn_matlang_amd import ML3Layer, functional as Fn
    from oracle.spect_conv_oracle import OracleML3Layer
    from oracle.relu_margin import make_safe
    monkeypatch.setattr(Fn, 'FWD_CHUNKS', chunks)          # (13 entries per row: edge chunks on the ring kernel, or the 64-row family)
    torch.manual_seed(ne * 19 + Fin)
    N = 400
    rng = np.random.default_rng(Fin + deg)
    ei = torch.from_numpy(_banded_graph(rng, N, deg, 12))
    ref = OracleML3Layer(True, ne, ne, Fin, n1, n2).double()
    m = ML3Layer(True, ne, ne, Fin, n1, n2).to(dev)
    m.load_state_dict({n: p.detach().float() for n, p in ref.state_dict().items()})
    x, ea, go = torch.randn(N, Fin), torch.randn(ei.size(1), ne) * 0.5, torch.randn(N, n1 + n2)
    ea, mask = make_safe(x, ei, ea, ref.state_dict(), True)
    go[:, :n1] *= mask.float()
    xr, er = x.double().requires_grad_(True), ea.double().requires_grad_(True)
    yr = ref(xr, ei, er)
    (yr * go.double()).sum().backward()
    for raw in (False, True):                              # supports with / without their own gradient (raw: the source-order fast road)
        m.zero_grad()
        xg = x.to(dev).requires_grad_(True)
        eg = ea.to(dev).requires_grad_(not raw)
        y = m(xg, ei.to(dev), eg)
        (y * go.to(dev)).sum().backward()
        close(y, yr, what='out')
        close(xg.grad, xr.grad, what='g_x')
        if not raw:
            close(eg.grad, er.grad, what='g_edge_attr')
        gp = dict(m.named_parameters())
        for n, p in ref.named_parameters():
            close(gp[n].grad, p.grad, what=n)


@pytest.mark.parametrize('S,fin,deg', [(6, 48, 5), (6, 48, 13), (6, 32, 13), (6, 32, 5), (4, 48, 5), (4, 48, 13), (8, 32, 13), (8, 32, 5), (6, 2, 5)])
def test_repeated_launches_are_bit_identical(dev, S, fin, deg):
    """Stress check behind DESIGN s4.1c: the same fused forward launched 16 times, with a cache-thrashing kernel in between,
    must give the same bits every time (and the oracle's values).  Round 4 found a gfx950 trap this way: one operand form of
    v_pk_fma_f32 (op_sel:[0,1,0]) lost a low product about once in 10^7 issues -- a row's last edge missing from one aggregate on
    SOME waves of SOME launches (mostly the first ones of a process: tests/stress/ runs this in fresh processes), invisible to a
    single parity run.  deg 13: groups walked in edge chunks; deg 5: one item per workgroup."""
    from gnn_matlang_amd import SpectConv
    from oracle import spect_conv_oracle as O
    rng = np.random.default_rng(1)
    torch.manual_seed(0)
    N = 1500
    ei = _banded_graph(rng, N, deg, 12)
    ea, x = torch.randn(ei.shape[1], S), torch.randn(N, fin)
    m = SpectConv(fin, 32, S, selfconn=False).to(dev)
    yo = O.spectconv_forward(x, T(ei), ea, m.weight.detach().cpu(), m.bias.detach().cpu(), False)
    xd, ed, eid = x.to(dev), ea.to(dev), T(ei).to(dev)
    junk = torch.randn(32, 1024, 1024, device=dev)
    first = None
    with torch.no_grad():
        for rep in range(16):
            if rep % 2:
                junk.mul_(1.0001)
            y = m(xd, eid, ed)
            if first is None:
                first = y.clone()
                close(first, yo, what='out')
            else:
                assert torch.equal(y, first), 'launch %d differs from launch 0 in %d rows' % (rep, int((y != first).any(1).sum()))


@pytest.mark.parametrize('ne,Fin,n1,n2,deg', [(6, 48, 32, 16, 13), (8, 32, 30, 2, 6), (4, 48, 24, 24, 4), (12, 32, 16, 16, 7)])
def test_repeated_training_steps_are_bit_identical(dev, ne, Fin, n1, n2, deg):
    """The same ML3Layer forward + backward repeated 8 times (edge branch, fused forward with gathered values, fused backward,
    output stage): every gradient bit-identical across the repeats (all kernels are atomics-free and order their loads by
    hand around the matrix pipe)."""
    from gnn_matlang_amd import ML3Layer
    torch.manual_seed(ne + Fin)
    rng = np.random.default_rng(ne)
    N = 1200
    ei = torch.from_numpy(_banded_graph(rng, N, deg, 12)).to(dev)
    m = ML3Layer(True, ne, ne, Fin, n1, n2).to(dev)
    x, ea, go = torch.randn(N, Fin, device=dev), torch.randn(ei.size(1), ne, device=dev) * 0.5, torch.randn(N, n1 + n2, device=dev)
    junk = torch.randn(32, 1024, 1024, device=dev)
    first = None
    for rep in range(8):
        if rep % 2:
            junk.mul_(1.0001)
        m.zero_grad()
        xg = x.clone().requires_grad_(True)
        y = m(xg, ei, ea)
        (y * go).sum().backward()
        got = [y.detach().clone(), xg.grad.clone()] + [p.grad.clone() for p in m.parameters()]
        if first is None:
            first = got
        else:
            for i, (a, b) in enumerate(zip(got, first)):
                assert torch.equal(a, b), 'repeat %d: tensor %d differs' % (rep, i)


@pytest.mark.parametrize('N,C,affine', [(1000, 48, True), (4097, 32, True), (70000, 48, True), (333, 64, False), (5, 4, True)])
def test_batchnorm_kernels_vs_torch(dev, N, C, affine):
    """models.BatchNorm1d (csrc/gml_bn.hip: statistics, normalise, and the backward as four launches) against torch.nn.BatchNorm1d in
    training mode on the same input: output, running statistics after two steps, d/dx, d/d weight, d/d bias (mutag.py:272-288)."""
    from gnn_matlang_amd import models
    torch.manual_seed(N + C)
    x0 = (torch.randn(N, C) * 1.5 + 0.7).relu()                          # post-relu activations, like a layer output
    go = torch.randn(N, C)
    ref = torch.nn.BatchNorm1d(C, affine=affine).double()
    m = models.BatchNorm1d(C, affine=affine).to(dev)
    if affine:
        with torch.no_grad():
            ref.weight.uniform_(0.5, 1.5); ref.bias.uniform_(-0.5, 0.5)
            m.weight.copy_(ref.weight.float()); m.bias.copy_(ref.bias.float())
    for step in range(2):
        xr = x0.double().requires_grad_(True)
        xg = x0.to(dev).requires_grad_(True)
        yr = ref(xr)
        yg = m(xg)
        (yr * go.double()).sum().backward()
        (yg * go.to(dev)).sum().backward()
        close(yg, yr, tol=2e-5, what='y')
        close(xg.grad, xr.grad, tol=2e-5, what='dx')
    close(m.running_mean, ref.running_mean, tol=2e-5, what='running_mean')
    close(m.running_var, ref.running_var, tol=2e-5, what='running_var')
    assert int(m.num_batches_tracked) == 2
    if affine:
        close(m.weight.grad, ref.weight.grad, tol=2e-5, what='d weight')
        close(m.bias.grad, ref.bias.grad, tol=2e-5, what='d bias')
    m.eval()
    close(m(x0.to(dev)), ref.eval()(x0.double()), tol=2e-5, what='eval')


# ------------------------------------------------------------------------------------------ fused GNNML1 block (round 5)
@pytest.mark.parametrize('mode,act', [(0, 0), (0, 1), (1, 0), (1, 1), (2, 1), (2, 0)])
@pytest.mark.parametrize('N,Fin,n1,n2,n3,unit', [(1000, 64, 64, 64, 64, True), (777, 2, 64, 64, 64, True), (333, 8, 16, 32, 16, True),
                                                 (500, 64, 16, 32, 16, False), (130, 25, 10, 20, 7, False), (1, 3, 64, 64, 64, True),
                                                 (65, 33, 48, 48, 48, False)])
def test_gnnml1_block_vs_fp64(dev, mode, act, N, Fin, n1, n2, n3, unit):
    """csrc/gml_gnnml1.hip: one GNNML1 block (sr25.py:231-240 sum / concat forms, mutag.py:253-262 factor form) forward and backward --
    output, dx and all eight parameter gradients -- against the same formulas in float64 (a directed random graph: the backward's
    transposed view is a different matrix; per-edge values or the scripts' ones).  Exact fp32 products: 2e-5 of the tensor's scale."""
    from gnn_matlang_amd import functional as Fn
    from gnn_matlang_amd.graph import GraphCSR
    if mode == 0:
        n2 = n3 = n1
    rng = np.random.default_rng(N + Fin)
    torch.manual_seed(N)
    deg = 5
    src = rng.integers(0, N, size=N * deg)
    dst = np.clip(src + rng.integers(-20, 21, size=src.shape), 0, N - 1)
    ei = torch.from_numpy(np.unique(np.vstack((src, dst)), axis=1).astype(np.int64))
    E = ei.size(1)
    val = None if unit else torch.randn(E)
    x = torch.randn(N, Fin)
    W = dict(w1=torch.randn(n1, Fin) * 0.3, b1=torch.randn(n1) * 0.1, wc=torch.randn(1, Fin, n2) * 0.2, bc=torch.randn(n2) * 0.1,
             w2=torch.randn(n3, Fin) * 0.3, b2=torch.randn(n3) * 0.1, w3=torch.randn(n3, Fin) * 0.3, b3=torch.randn(n3) * 0.1)
    C = n1 if mode == 0 else n1 + n2 + n3
    gout = torch.randn(N, C)

    def ref(x, W, val):
        A = torch.tanh if act == 0 else torch.relu
        v = torch.ones(E, dtype=x.dtype) if val is None else val
        h = torch.zeros_like(x).index_add_(0, ei[1], v.unsqueeze(1) * x[ei[0]])          # libs/spect_conv.py:98-99: aggregate at the target
        a, c = x @ W['w1'].t() + W['b1'], h @ W['wc'][0] + W['bc']
        f2, f3 = x @ W['w2'].t() + W['b2'], x @ W['w3'].t() + W['b3']
        if mode == 0:
            return A(a + c + f2 * f3)
        return torch.cat([A(a), A(c), A(f2 * f3) if mode == 1 else A(f2) * A(f3)], 1)

    x64 = x.double().requires_grad_(True)
    W64 = {k: v.double().requires_grad_(True) for k, v in W.items()}
    y64 = ref(x64, W64, None if val is None else val.double())
    (y64 * gout.double()).sum().backward()

    csr = GraphCSR.from_edge_index(ei.to(dev), N)
    xd = x.to(dev).requires_grad_(True)
    Wd = {k: v.to(dev).requires_grad_(True) for k, v in W.items()}
    vs = None if val is None else csr.sort_values(val.to(dev).view(-1, 1)).view(-1)
    assert Fn.gnnml1_block_supported(xd, Fin, n1, n2, n3, mode)
    y = Fn.GNNML1BlockFunction.apply(xd, csr, vs, Wd['w1'], Wd['b1'], Wd['wc'], Wd['bc'], Wd['w2'], Wd['b2'], Wd['w3'], Wd['b3'], mode, act)
    (y * gout.to(dev)).sum().backward()
    tol = 2e-5
    close(y, y64.float(), tol=tol, what='out')
    close(xd.grad, x64.grad.float(), tol=tol, what='dx')
    for k in W:
        close(Wd[k].grad, W64[k].grad.float(), tol=tol, what=k)


def test_one_launch_adam_follows_torch_adam(dev):
    """optim.OneLaunchAdam (gml_adam_many: every parameter tensor of the model in one launch, step count on the device) against
    torch.optim.Adam over 8 steps with fresh random gradients: parameters equal to 1e-6 of their scale; 70 tensors (two chunks of the
    job table), sizes 1 .. 5000, a non-contiguous gradient; then captured in a HIP graph and replayed -- the count keeps advancing."""
    from gnn_matlang_amd.optim import OneLaunchAdam
    torch.manual_seed(0)
    sizes = [1, 3, 4, 5, 1023, 1024, 1025, 5000, 4096, 4097, 150000] + [int(v) for v in torch.randint(1, 2000, (59,))]     # chunk 1: one workgroup; chunk 0: the multi-workgroup form
    pa = [torch.randn(n, device=dev).requires_grad_(True) for n in sizes]
    pb = [p.detach().clone().requires_grad_(True) for p in pa]
    oa, ob = OneLaunchAdam(pa, lr=1e-2), torch.optim.Adam(pb, lr=1e-2)
    for it in range(8):
        for a, b in zip(pa, pb):
            g = torch.randn_like(a) * (10.0 ** (it % 3 - 1))
            a.grad = g.clone() if a.numel() != 1024 else g.repeat_interleave(2)[::2]       # (a strided view: made contiguous by the optimizer)
            b.grad = g.clone()
        oa.step()
        ob.step()
    for a, b in zip(pa, pb):
        close(a, b, tol=1e-6, what='adam n=%d' % a.numel())
    # capture: static gradients, replays advance the device step count
    for a, b in zip(pa, pb):
        a.grad = torch.randn_like(a)
        b.grad = a.grad.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        oa.step()
    torch.cuda.current_stream().wait_stream(side)
    ob.step()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                  # (recorded, not run)
        oa.step()
    for _ in range(3):
        g.replay()
        ob.step()
    torch.cuda.synchronize()
    for a, b in zip(pa, pb):
        close(a, b, tol=2e-6, what='adam replay n=%d' % a.numel())


@pytest.mark.parametrize('S,fin,fout,deg,N', [(6, 33, 17, 5, 517), (6, 37, 32, 13, 300), (6, 48, 30, 16, 1000), (6, 44, 24, 3, 129),
                                               (4, 47, 31, 5, 517), (4, 48, 24, 8, 2049), (4, 36, 32, 2, 1), (6, 40, 32, 13, 128)])
def test_one_launch_48_feature_backward_odd_shapes(dev, S, fin, fout, deg, N):
    """bwd3 with a third 16-feature block (NFB = 3, round 5): 33 .. 48 input features in ONE launch for S = 4 and 6 -- widths that are
    not multiples of 4 (scalar x rows), of 16 (partial third block), ragged row counts, one node, sr25's 13 entries per row (the
    S = 6 class reads its value rows inside the edge loop and stores dval from it; lane kq = 3 of the padded fold stores nothing).
    Output, dx, d edge_attr, dW, db against the oracle; GML_VERBOSE confirms the one-launch road."""
    from gnn_matlang_amd import SpectConv, functional as Fn
    from oracle import spect_conv_oracle as O
    rng = np.random.default_rng(S * 100 + fin)
    torch.manual_seed(fin)
    ei = _banded_graph(rng, N, deg, 12) if N > 1 else np.zeros((2, 1), dtype=np.int64)
    ea, x = torch.randn(ei.shape[1], S), torch.randn(N, fin)
    m = SpectConv(fin, fout, S, selfconn=False).to(dev)
    w, b = m.weight.detach().cpu(), m.bias.detach().cpu()
    xo, eo, wo, bo = (t.clone().requires_grad_(True) for t in (x, ea, w, b))
    yo = O.spectconv_forward(xo, T(ei), eo, wo, bo, False)
    gout = torch.randn_like(yo)
    (yo * gout).sum().backward()
    xg, eg = x.to(dev).requires_grad_(True), ea.to(dev).requires_grad_(True)
    old = Fn.VERBOSE
    Fn.VERBOSE = True
    Fn.PATHS.clear()
    try:
        y = m(xg, T(ei).to(dev), eg)
        (y * gout.to(dev)).sum().backward()
        paths = dict(Fn.PATHS)
    finally:
        Fn.VERBOSE = old
    assert any('conv_bwd: fused (group kind 128)' in k and 'two launches' not in k for k in paths), paths
    close(y, yo, what='out')
    close(xg.grad, xo.grad, what='g_x')
    close(eg.grad, eo.grad, what='g_edge_attr')
    close(m.weight.grad, wo.grad, what='g_weight')
    close(m.bias.grad, bo.grad, what='g_bias')


@pytest.mark.parametrize('n,a,b', [(1000, 768, 128), (129, 384, 64), (5, 12, 64), (70000, 768, 128), (4097, 130, 10), (128, 128, 128), (1, 33, 1)])
def test_xty_wide_vs_fp64(dev, n, a, b):
    """gml_xty_wide (csrc/gml_xty_wide.hip): Hcat^T g of the dense-block layer -- a wide tall matrix against a <= 128-column one on the
    bf16 matrix cores (bf16x3) -- against float64; row counts and widths off every tile size, strided row views."""
    from gnn_matlang_amd import functional as Fn
    torch.manual_seed(n + a)
    A = torch.randn(n, a + 3, device=dev)[:, :a]
    B = torch.randn(n, b + 5, device=dev)[:, 1:b + 1]
    out = Fn.xty_wide(A, B)
    assert out is not None
    ref = A.double().t() @ B.double()
    close(out, ref.float(), tol=2e-5, what='xty_wide')


def test_deferred_folds_with_existing_grads_accumulate_correctly(dev):
    """a deferred-fold scope hands autograd tensors that are filled only at scope exit -- correct only when every .grad is
    None.  With gradients already present (zero_grad(set_to_none=False), micro-batch accumulation) the scope must be inert: two
    backward passes inside scopes accumulate exactly what two plain backward passes accumulate."""
    from gnn_matlang_amd import SpectralDesign, collate, functional as Fn, models, synthetic
    raw = synthetic.make_graphs('zinc', 32, seed=5)
    b = collate(SpectralDesign(recfield=2, dv=2, nfreq=7).design_many(raw)).to(dev)
    torch.manual_seed(4)
    m = models.zinc_gnnml3().to(dev)
    for _ in range(2):
        models.zinc_loss(m(b), b.y).backward()
    ref = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    for k in range(2):
        l = models.zinc_loss(m(b), b.y)
        scope = Fn.deferred_folds(m.parameters())
        assert scope.active == (k == 0)
        with scope:
            l.backward()
    for n, p in m.named_parameters():
        assert torch.equal(p.grad, ref[n]), 'accumulated gradient differs: ' + n
    m.zero_grad(set_to_none=False)                                   # zeroed buffers kept: the scope must stand aside
    l = models.zinc_loss(m(b), b.y)
    with Fn.deferred_folds(m.parameters()) as scope:
        assert not scope.active
        l.backward()
    for n, p in m.named_parameters():
        assert torch.allclose(p.grad * 2, ref[n], rtol=0, atol=0) or torch.equal(p.grad + p.grad, ref[n]), n


def test_gnnml1_block_bias_gradients_do_not_share_memory(dev):
    """in the sum form (mode 0) fc_i1.bias and conv_i1.bias receive the same column sums; the two gradients autograd
    adopts must not be one buffer (clip_grad_norm_ / accumulation would hit both).  Plus: two backward passes accumulate to twice one,
    and an in-place scale of every gradient scales each bias gradient ONCE."""
    from gnn_matlang_amd import SpectralDesign, collate, models, synthetic
    raw = synthetic.make_graphs('counting', 12, seed=9)
    b = collate(SpectralDesign(recfield=1, dv=1, nfreq=10, adddegree=True, laplacien=False, addadj=True).design_many(raw)).to(dev)
    torch.manual_seed(1)
    m = models.GNNML1Blocks(int(b.x.size(1)), (16, 16, 16), 3, form='sum', act='tanh', head='lin10', nclass=10).to(dev)
    m(b).square().sum().backward()
    spans = {}
    for n, p in m.named_parameters():
        if p.grad is None:
            continue
        lo, hi = p.grad.data_ptr(), p.grad.data_ptr() + p.grad.numel() * 4
        for n2, (lo2, hi2) in spans.items():
            assert hi <= lo2 or hi2 <= lo, 'gradients of %s and %s overlap in memory' % (n, n2)
        spans[n] = (lo, hi)
    assert 'fc11.bias' in spans and 'conv11.bias' in spans
    one = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    assert torch.equal(one['fc11.bias'], one['conv11.bias'])
    for n, p in m.named_parameters():
        if p.grad is not None:
            p.grad.mul_(0.5)
    for n, p in m.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, one[n] * 0.5), n
            p.grad.mul_(2.0)
    m(b).square().sum().backward()
    for n, p in m.named_parameters():
        if p.grad is not None:
            assert torch.allclose(p.grad, 2 * one[n], rtol=1e-5, atol=1e-6 * float(one[n].abs().max())), n


def test_one_launch_adam_checkpoint_resume_and_first_steps(dev):
    """(1) OneLaunchAdam's state_dict carries the step count and the moments, and a fresh optimizer that loads it BEFORE
    its first step continues exactly where the first one stopped (bias corrections included); loading into a running optimizer works
    too.  (2) the bias corrections at t = 1 .. 3 are formed without cancellation: one step from zero moments moves every parameter by
    lr * sign(g) to 2e-7 relative (|g| >> eps), which 1 - __powf(0.999, t) missed by 3e-5."""
    from gnn_matlang_amd.optim import OneLaunchAdam
    torch.manual_seed(3)
    sizes = [7, 1024, 5000]
    grads = [[torch.randn(n, device=dev) for n in sizes] for _ in range(6)]

    def run(opt, ps, its):
        for it in its:
            for p, g in zip(ps, grads[it]):
                p.grad = g.clone()
            opt.step()
    p0 = [torch.randn(n, device=dev) for n in sizes]
    pa = [p.clone().requires_grad_(True) for p in p0]
    oa = OneLaunchAdam(pa, lr=1e-2)
    run(oa, pa, range(6))                                         # six uninterrupted steps
    pb = [p.clone().requires_grad_(True) for p in p0]
    ob = OneLaunchAdam(pb, lr=1e-2)
    run(ob, pb, range(3))
    sd = ob.state_dict()
    assert all(float(torch.as_tensor(s['step']).reshape(-1)[0]) == 3.0 and 'exp_avg' in s and 'exp_avg_sq' in s for s in sd['state'].values())
    import copy
    sd = copy.deepcopy(sd)
    pc = [p.detach().clone().requires_grad_(True) for p in pb]
    oc = OneLaunchAdam(pc, lr=1e-2)
    oc.load_state_dict(sd)                                        # before the first step
    run(oc, pc, range(3, 6))
    for a, c in zip(pa, pc):
        assert torch.equal(a, c), 'resumed run differs from the uninterrupted one'
    ob.load_state_dict(copy.deepcopy(sd))                         # into a running optimizer
    run(ob, pb, range(3, 6))
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
    # (2) first step: p - lr * g / (|g| + eps) exactly as torch computes it in double
    for t in range(1, 4):
        q = [torch.zeros(n, device=dev).requires_grad_(True) for n in sizes]
        r = [torch.zeros(n, device=dev).requires_grad_(True) for n in sizes]
        oq, orr = OneLaunchAdam(q, lr=1e-2), torch.optim.Adam(r, lr=1e-2)
        for it in range(t):
            for a, b, g in zip(q, r, grads[it]):
                a.grad, b.grad = g.clone(), g.clone()
            oq.step()
            orr.step()
        for a, b in zip(q, r):
            err = float((a.detach() - b.detach()).abs().max() / b.detach().abs().max())
            assert err <= 3e-7, ('bias correction', t, err)


@pytest.mark.parametrize('cx,cw', [(0, 0), (40, 20), (-40, -20), (60, -50), (-90, 30)])
def test_f16_forward_is_scale_invariant(dev, cx, cw):
    """GML_F16X3 (the forward projection on f16 pieces): the per-tile / per-column power-of-two scales make the arithmetic
    independent of the operands' magnitude -- x * 2^cx and W * 2^cw give EXACTLY 2^(cx + cw) times the unscaled output (no overflow
    to inf at 2^60, no flush at 2^-90, bit for bit), for the conv columns and, with the Hadamard branch's weights scaled too, for
    its pre-activations (checked through the conv columns only: tanh is not homogeneous).  And the result sits at fp32 level
    against float64: 3e-6 of the term sum where the bf16 pairs sit at 1e-5."""
    from gnn_matlang_amd import ML3Layer, SpectralDesign, collate, synthetic, functional as Fn
    raw = synthetic.make_graphs('zinc', 64, seed=11)
    b = collate(SpectralDesign(recfield=2, dv=2, nfreq=7).design_many(raw)).to(dev)
    torch.manual_seed(5)
    layer = ML3Layer(False, 8, 8, 32, 30, 2).to(dev)
    x = torch.randn(b.x.size(0), 32, device=dev)
    csr = b.csr('edge_index2')
    old = Fn.FWD_F16
    Fn.FWD_F16 = True
    try:
        with torch.no_grad():
            y0 = layer(x, csr, b.edge_attr2)
            layer.conv1.bias.zero_()
            y1 = layer(x, csr, b.edge_attr2)[:, :30]
            layer.conv1.weight.mul_(2.0 ** cw)
            y2 = layer(x * 2.0 ** cx, csr, b.edge_attr2)[:, :30]
    finally:
        Fn.FWD_F16 = old
    assert torch.isfinite(y2).all()
    assert torch.equal(y2, y1 * 2.0 ** (cx + cw)), float((y2 / 2.0 ** (cx + cw) - y1).abs().max())
    if cx == 0 and cw == 0:
        # against float64 under the term-sum criterion (relu = the device's own mask where the two disagree near zero)
        xd, vd, wd = x.double().cpu(), b.edge_attr2.double().cpu(), layer.conv1.weight.double().cpu()
        ei = b.edge_index2.cpu()
        ref = torch.zeros(x.size(0), 30, dtype=torch.float64)
        tsum = torch.zeros_like(ref)
        for s_ in range(8):
            h = torch.zeros(x.size(0), 32, dtype=torch.float64).index_add_(0, ei[1], vd[:, s_:s_ + 1] * xd[ei[0]])
            ha = torch.zeros(x.size(0), 32, dtype=torch.float64).index_add_(0, ei[1], vd[:, s_:s_ + 1].abs() * xd[ei[0]].abs())
            ref += h @ wd[s_]
            tsum += ha @ wd[s_].abs()
        got = y1.double().cpu()
        err = ((got - ref.clamp(min=0)).abs() / tsum.clamp(min=1e-300))
        err[(ref.abs() < 1e-5 * tsum)] = 0                      # units at the kink
        assert float(err.max()) <= 3e-6, float(err.max())


# ------------------------------------------------------------------------------------------ the edge branch over unique support rows (round 6)
def _sym_batch(dev, ngraphs=96, perturb=0.0, seed=21):
    from gnn_matlang_amd import SpectralDesign, collate, synthetic
    raw = synthetic.make_graphs('zinc', ngraphs, seed=seed)
    b = collate(SpectralDesign(recfield=2, dv=2, nfreq=7).design_many(raw)).to(dev)
    if perturb > 0:                                        # break the symmetry of a share of the rows by one ulp of one channel
        g = torch.Generator().manual_seed(seed)
        pick = (torch.rand(b.edge_attr2.size(0), generator=g) < perturb).to(dev)
        ch = torch.randint(0, 8, (b.edge_attr2.size(0),), generator=g).to(dev)
        bits = b.edge_attr2.view(torch.int32).clone()
        bits[pick, ch[pick]] ^= 1
        b.edge_attr2 = bits.view(torch.float32)
    return b


@pytest.mark.parametrize('perturb', [0.0, 0.3])
def test_edge_sym_flags_match_a_numpy_pairing(dev, perturb):
    """gml_edge_sym_flags: flag 2 = the edge (src < dst) whose mirror carries bitwise the same row, 0 = that mirror, 1 = alone; every
    edge is covered exactly once by the compacted (uid, mir) list; rows that differ in ONE BIT are not paired."""
    b = _sym_batch(dev, perturb=perturb)
    csr = b.csr('edge_index2')
    vals = csr.to_source_order(csr.sort_values(b.edge_attr2))
    sym = csr.sym_index(vals)
    rp, col = csr.rowptr_t.cpu().numpy().astype(np.int64), csr.col_t.cpu().numpy().astype(np.int64)
    v = vals.cpu().numpy().view(np.uint32)
    E, N = col.size, rp.size - 1
    src = np.repeat(np.arange(N), np.diff(rp))
    key = src * N + col
    pos = np.searchsorted(key, col * N + src)
    has = (pos < E) & (key[np.minimum(pos, E - 1)] == col * N + src)
    same = has & (v == v[np.minimum(pos, E - 1)]).all(axis=1) & (src != col)
    flag = np.where(same & (src < col), 2, np.where(same, 0, 1))
    assert sym is not None
    uid, mir = sym[0].cpu().numpy(), sym[1].cpu().numpy()
    np.testing.assert_array_equal(uid, np.nonzero(flag)[0])
    np.testing.assert_array_equal(mir, np.where(flag[uid] == 2, pos[uid], -1))
    covered = np.zeros(E, dtype=np.int64)
    np.add.at(covered, uid, 1)
    np.add.at(covered, mir[mir >= 0], 1)
    assert (covered == 1).all()
    share = uid.size / E
    assert (share < 0.66) if perturb == 0 else (0.66 < share < 0.9), share


@pytest.mark.parametrize('perturb,layers', [(0.0, 4), (0.3, 4), (0.0, 1), (0.0, 2)])
def test_edge_branch_over_unique_rows_equals_the_plain_kernels(dev, perturb, layers):
    """the edge branch over the batch's unique support rows (gml_edge_mlp_fwd_stack6_sym / gml_edge_mlp_bwd_sym): the forward is BITWISE
    the plain forward (an edge and its mirror get the same row either way), the weight gradients equal the plain backward's to
    summation order (1e-5 of the tensor's scale, and 1e-4 of the term sums against float64)."""
    from gnn_matlang_amd import functional as Fn
    b = _sym_batch(dev, perturb=perturb)
    csr = b.csr('edge_index2')
    vals = csr.to_source_order(csr.sort_values(b.edge_attr2), cache=True)
    sym = csr.sym_index(vals)
    assert sym is not None
    torch.manual_seed(3)
    ws = [tuple(torch.randn(*shp, device=dev) * 0.4 for shp in ((16, 8), (16, 8), (16, 8), (8, 32))) for _ in range(layers)]
    plain = Fn.edge_mlp_fwd_stack(vals, csr.presplit(vals), ws, None) if layers > 1 else [Fn.edge_mlp_fwd(vals, *ws[0], None, csr.presplit(vals))[0]]
    shared = Fn.edge_mlp_fwd_stack(vals, csr.presplit(vals), ws, sym)
    assert shared is not None and len(shared) == layers
    for l in range(layers):
        assert torch.equal(plain[l], shared[l]), 'layer %d: forward over unique rows differs' % l
    gout = torch.randn_like(vals)
    w1, w2, w3, w4 = ws[0]
    ref = Fn.edge_mlp_bwd(vals, w1, w2, w3, w4, gout, False, csr.presplit(vals), None)
    got = Fn.edge_mlp_bwd(vals, w1, w2, w3, w4, gout, False, csr.presplit(vals), sym)
    assert got[0] is None
    for name, a, r in zip(('dw1', 'dw2', 'dw3', 'dw4'), got[1:], ref[1:]):
        close(a, r, tol=1e-5, what='unique-row backward ' + name)
    # against float64 autograd
    e64 = vals.double().cpu()
    p64 = [t.double().cpu().requires_grad_(True) for t in (w1, w2, w3, w4)]
    h = torch.cat([torch.relu(e64 @ p64[0].t()), torch.tanh(e64 @ p64[1].t()) * torch.tanh(e64 @ p64[2].t())], 1)
    out = torch.relu(h @ p64[3].t())
    close(shared[0], out.float(), tol=2e-6, what='forward over unique rows vs float64')
    out.backward(gout.double().cpu())
    for name, a, p in zip(('dw1', 'dw2', 'dw3', 'dw4'), got[1:], p64):
        close(a, p.grad.float(), what='unique-row backward vs float64 ' + name)


def test_model_step_with_and_without_unique_row_sharing(dev):
    """the ZINC GNNML3 step with GML_EDGE_SYM on / off: logits bitwise equal, every parameter gradient within 1e-5 of its scale; static
    (captured-epoch) batches never take the shared road (their tensors are refilled in place: a cached pairing would go stale)."""
    from gnn_matlang_amd import functional as Fn, models
    b = _sym_batch(dev, ngraphs=128)
    torch.manual_seed(0)
    m = models.zinc_gnnml3().to(dev)
    res = {}
    for on in (True, False):
        old = Fn.EDGE_SYM
        Fn.EDGE_SYM = on
        try:
            m.zero_grad()
            pre = m(b)
            models.zinc_loss(pre, b.y).backward()
            res[on] = (pre.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()})
        finally:
            Fn.EDGE_SYM = old
    assert torch.equal(res[True][0], res[False][0])
    for n in res[True][1]:
        close(res[True][1][n], res[False][1][n], tol=1e-5, what='shared vs plain ' + n)
    from gnn_matlang_amd.dataset import DeviceDataset
    from gnn_matlang_amd import SpectralDesign, synthetic
    raw = synthetic.make_graphs('zinc', 64, seed=4)
    dsd = DeviceDataset.from_graphs(SpectralDesign(recfield=2, dv=2, nfreq=7).design_many(raw), dev)
    dsd.prepare()
    sb = dsd.batch_assembled(torch.arange(16, device=dev), dsd.bounds(16))
    c = sb.csr('edge_index2')
    assert c.sym_index(c.to_source_order(c.sort_values(sb.edge_attr2))) is None


def test_pool_with_relu_pattern_and_its_masked_gradient(dev):
    """gml_segment_sum_mask = gml_segment_sum bit for bit + bit c of mask[row] = (x[row][c] > 0); gml_segment_bcast_mask = the pool's
    gradient per row times that pattern below nrelu; add and mean flag, ragged segments incl. empty ones and one beyond 32 rows, the
    padding-graph flag of a static batch."""
    from gnn_matlang_amd import functional as Fn, _lib
    g = torch.Generator().manual_seed(3)
    sizes = torch.tensor([5, 0, 23, 1, 40, 0, 17, 33, 2, 64, 9], dtype=torch.int64)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).to(torch.int32).to(dev)
    N = int(sizes.sum())
    x = torch.randn(N, 32, generator=g).to(dev)
    x[torch.rand(N, 32, generator=g).to(dev) < 0.3] = 0.0                         # exact zeros: not positive
    seg = torch.repeat_interleave(torch.arange(len(sizes)), sizes).to(torch.int32).to(dev)
    bits = ((x > 0).to(torch.int64) << torch.arange(32, device=dev)).sum(1)
    for flag in (0, 1, _lib.GML_POOL_SKIP_LAST):
        ref = Fn.segment_sum(x, ptr, flag)
        got, mask = Fn.segment_sum_mask(x, ptr, flag)
        assert torch.equal(ref, got)
        live = N - (int(sizes[-1]) if flag & _lib.GML_POOL_SKIP_LAST else 0)      # (the padding graph's rows are not read)
        assert torch.equal(mask[:live].to(torch.int64) & 0xffffffff, bits[:live])
    _, mask = Fn.segment_sum_mask(x, ptr, 0)
    gp = torch.randn(len(sizes), 32, generator=g).to(dev)
    for nrelu in (30, 32, 0):
        out = Fn.segment_bcast_mask(gp, seg, mask, nrelu)
        keep = (x > 0) | (torch.arange(32, device=dev) >= nrelu)
        assert torch.equal(out, gp[seg.long()] * keep)


def test_model_step_with_the_output_stage_inside_the_conv_backward(dev):
    """the ZINC GNNML3 step with GML_BWD_HAD on / off (gml_spectconv_bwd_had: relu mask hand-over, Hadamard branch, bias sums and the
    dz . w start of dx inside the conv backward of the layers whose gradient arrives pre-masked) -- the forward is the same code, every
    parameter gradient within 2e-5 of its scale (dw11 / dw12 move from exact fp32 products to bf16x3 ones, the pre-activations are
    summed in another order); the fused road is really taken (launch count of the split kernel) and repeats itself bit for bit;
    a tail group (N not a multiple of 128) and the deferred-fold scope are covered by the two batch sizes / the second loop."""
    from gnn_matlang_amd import functional as Fn, models
    for ngraphs, defer in ((128, False), (37, True)):
        b = _sym_batch(dev, ngraphs=ngraphs)
        torch.manual_seed(1)
        m = models.zinc_gnnml3().to(dev)
        res = {}
        for on in (True, False, True):
            old = Fn.BWD_HAD
            Fn.BWD_HAD = on
            Fn.PROFILE = {}
            try:
                m.zero_grad()
                pre = m(b)
                loss = models.zinc_loss(pre, b.y)
                if defer:
                    with Fn.deferred_folds(list(m.parameters())):
                        loss.backward()
                else:
                    loss.backward()
                torch.cuda.synchronize()
                cur = (pre.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()}, Fn.profile_summary(Fn.PROFILE))
                if on and True in res:
                    for n in cur[1]:
                        assert torch.equal(cur[1][n], res[True][1][n]), 'fused output stage does not repeat itself: ' + n
                res[on] = cur
            finally:
                Fn.BWD_HAD = old
                Fn.PROFILE = None
        assert torch.equal(res[True][0], res[False][0])
        ns_on = res[True][2].get('ml3_split_bwd', {}).get('launches', 0)
        ns_off = res[False][2].get('ml3_split_bwd', {}).get('launches', 0)
        assert ns_off == 4 and ns_on == 0, (ns_on, ns_off)           # no output-stage launch is left (the top layer's gradient is expanded
                                                                     # from the pool with the relu pattern the pool kernel recorded)
        for n in res[True][1]:
            close(res[True][1][n], res[False][1][n], tol=2e-5, what='fused vs split output stage ' + n)


def test_ml3_backward_runs_the_road_its_record_names(dev, monkeypatch):
    """Four chained ZINC layers (8 supports, 32 -> 30 + 2), the top one pooled, one training step: the road records of the four
    backward calls (functional._ml3_bwd_road, under VERBOSE one `ml3_bwd` key each) name the output stage inside the conv backward for
    all four -- masked pool gradient on the top layer, no dx on the bottom one -- and with GML_BWD_HAD off four one-pass stages, three of
    them pre-masked; the launches that ran are the ones the records name, and every gradient of the two settings agrees within 2e-5 of
    its scale (the bar of test_model_step_with_the_output_stage_inside_the_conv_backward)."""
    from gnn_matlang_amd import ML3Layer, functional as Fn
    rng = np.random.default_rng(61)
    torch.manual_seed(61)
    N, S, B = 300, 8, 12
    ei = _random_graph(rng, N, 6)
    ei = ei[:, np.lexsort((ei[1], ei[0]))]                   # source-sorted, as SpectralDesign emits
    eit = T(ei).to(dev)
    layers = [ML3Layer(True, S, S, 32, 30, 2).to(dev) for _ in range(4)]
    for lo, up in zip(layers, layers[1:]):
        up.chain_after(lo)
    x0, ea = torch.randn(N, 32, device=dev), torch.randn(ei.shape[1], S, device=dev)
    ptr = torch.arange(0, N + 1, N // B, dtype=torch.int32, device=dev)
    batch = torch.arange(N, device=dev, dtype=torch.int32) // (N // B)
    gout = torch.randn(B, 32, device=dev)
    ran = []
    spy = lambda name, what: monkeypatch.setattr(Fn, name, (lambda real: lambda *a, **k: (ran.append(what(a, k)), real(*a, **k))[1])(getattr(Fn, name)))
    spy('ml3_split_bwd', lambda a, k: ('stage', bool(k['premasked']), bool(k['dz_out']), k['gy_seg'] is not None))
    spy('fused_conv_bwd', lambda a, k: ('conv', a[1].rows, a[6], a[10] is not None, a[11], a[12] is not None))   # rows, need_x, mix, relu_cols, had
    spy('segment_bcast_mask', lambda a, k: ('masked pool',))
    monkeypatch.setattr(Fn, 'VERBOSE', True)
    res = {}
    for on in (True, False):
        monkeypatch.setattr(Fn, 'BWD_HAD', on)
        for l in layers:
            l.zero_grad()
        Fn.PATHS.clear()
        del ran[:]
        h = x0
        for l in layers[:-1]:
            h = l(h, eit, ea)
        (layers[-1].forward_pooled(h, eit, ea, ptr, batch) * gout).sum().backward()
        torch.cuda.synchronize()
        keys = sorted((k, n) for k, n in Fn.PATHS.items() if k.startswith('ml3_bwd:'))
        res[on] = ([p.grad.clone() for l in layers for p in l.parameters()], keys, list(ran))
    field = lambda keys, text: sum(n for k, n in keys if text + ' ' in k)
    _, keys, launches = res[True]
    assert sum(n for _, n in keys) == 4 and field(keys, 'stage=had') == 4 and field(keys, 'parts=3') == 4, keys
    assert [(n, 'want_dx=1' in k, 'relu_cols=30' in k) for k, n in keys if 'pool_grad=masked ' in k] == [(1, True, True)], keys
    assert [(n, 'relu_cols=0 ' in k, 'pool_grad=None' in k) for k, n in keys if 'want_dx=0 ' in k] == [(1, True, True)], keys
    assert field(keys, 'conv=one128') == 4 and field(keys, 'use_dz=0') == 4
    assert launches == [('masked pool',), ('conv', 128, True, False, 30, True), ('conv', 128, True, False, 30, True),
                        ('conv', 128, True, False, 30, True), ('conv', 128, False, False, 0, True)], launches
    _, keys, launches = res[False]
    assert sum(n for _, n in keys) == 4 and field(keys, 'stage=one_pass') == 4 and field(keys, 'premasked=1') == 3, keys
    assert [(n, 'premasked=0 ' in k, 'dz_out=1 ' in k) for k, n in keys if 'pool_grad=per_segment ' in k] == [(1, True, True)], keys
    assert field(keys, 'relu_cols=30') == 3 and field(keys, 'use_dz=1') == 3 and field(keys, 'conv_accum=0') == 4
    assert launches == [('stage', False, True, True), ('conv', 128, True, True, 30, False), ('stage', True, True, False), ('conv', 128, True, True, 30, False),
                        ('stage', True, True, False), ('conv', 128, True, True, 30, False), ('stage', True, False, False), ('conv', 128, False, False, 0, False)], launches
    for i, (a, b) in enumerate(zip(res[True][0], res[False][0])):
        close(a, b, tol=2e-5, what='output stage inside the conv backward vs one-pass stage, parameter %d' % i)


def test_edge_sym_pairing_with_repeated_and_one_sided_edges(dev):
    """multigraph input (an edge repeated, on one side or on both) and one-sided edges (no mirror at all): such edges are evaluated
    alone; every row of the output is still written exactly once and equals the plain kernels' bit for bit."""
    from gnn_matlang_amd import functional as Fn
    from gnn_matlang_amd.graph import GraphCSR
    g = torch.Generator().manual_seed(5)
    N = 300
    a = torch.randint(0, N, (2, 1500), generator=g)
    und = torch.cat([a, a.flip(0)], 1)                              # symmetric structure
    und = torch.unique(und, dim=1)
    extra = torch.cat([und[:, :200], und[:, :200], und[:, 300:350].flip(0)[:, :0]], 1)      # 200 edges repeated twice more (one side only)
    both = torch.cat([und[:, 400:450], und[:, 400:450].flip(0)], 1)                         # 50 pairs repeated on both sides
    oneside = torch.stack([torch.randint(0, N, (120,), generator=g), torch.randint(0, N, (120,), generator=g)])
    ei = torch.cat([und, extra, both, oneside, torch.arange(N).repeat(2, 1)], 1)
    order = torch.argsort(ei[0] * N + ei[1], stable=True)
    ei = ei[:, order].to(dev)
    # symmetric values: a function of the unordered pair, so mirrors are bitwise equal
    lo, hi = torch.minimum(ei[0], ei[1]), torch.maximum(ei[0], ei[1])
    base = torch.randn(N * N // 64 + 8, 8, generator=g).to(dev)
    vals = base[(lo * 7 + hi * 13) % base.size(0)].contiguous()
    csr = GraphCSR.from_edge_index(ei, N)
    vs = csr.to_source_order(csr.sort_values(vals))
    sym = csr.sym_index(vs)
    assert sym is not None
    uid, mir = sym[0].cpu().numpy(), sym[1].cpu().numpy()
    covered = np.zeros(csr.E, dtype=np.int64)
    np.add.at(covered, uid, 1)
    np.add.at(covered, mir[mir >= 0], 1)
    assert (covered == 1).all(), 'rows written %s times' % np.unique(covered)
    torch.manual_seed(1)
    ws = [tuple(torch.randn(*shp, device=dev) * 0.4 for shp in ((16, 8), (16, 8), (16, 8), (8, 32))) for _ in range(2)]
    plain = Fn.edge_mlp_fwd_stack(vs, csr.presplit(vs), ws, None)
    shared = Fn.edge_mlp_fwd_stack(vs, csr.presplit(vs), ws, sym)
    for l in range(2):
        assert torch.equal(plain[l], shared[l])
    gout = torch.randn_like(vs)
    ref = Fn.edge_mlp_bwd(vs, *ws[0], gout, False, csr.presplit(vs), None)
    got = Fn.edge_mlp_bwd(vs, *ws[0], gout, False, csr.presplit(vs), sym)
    for a_, r_ in zip(got[1:], ref[1:]):
        close(a_, r_, tol=1e-5, what='unique-row backward on a multigraph')


@pytest.mark.parametrize('view', ['source', 'target'])
def test_edge_branch_over_unique_rows_six_supports(dev, view):
    """sr25.py's six supports (rows of 24 bytes: 8-byte vector accesses, scalar stores) on the unique-row kernels, in the training
    order (source view) and the inference order (target view): forward bitwise the plain forward, backward to summation order."""
    from gnn_matlang_amd import SpectralDesign, collate, synthetic, functional as Fn
    raw = synthetic.make_graphs('zinc', 80, seed=8)
    b = collate(SpectralDesign(recfield=1, dv=2, nfreq=5, adddegree=True).design_many(raw)).to(dev)
    assert b.edge_attr2.size(1) == 6
    csr = b.csr('edge_index2')
    vals = csr.sort_values(b.edge_attr2)
    if view == 'source':
        vals = csr.to_source_order(vals, cache=True)
    sym = csr.sym_index(vals, view)
    assert sym is not None and sym[0].numel() < 0.8 * csr.E
    torch.manual_seed(6)
    w = tuple(torch.randn(*shp, device=dev) * 0.4 for shp in ((12, 6), (12, 6), (12, 6), (6, 24)))
    plain = Fn.edge_mlp_fwd(vals, *w, None, csr.presplit(vals))[0]
    shared = Fn.edge_mlp_fwd_stack(vals, None, [w], sym)
    assert shared is not None and torch.equal(plain, shared[0])
    if view == 'source':
        gout = torch.randn_like(vals)
        ref = Fn.edge_mlp_bwd(vals, *w, gout, False, csr.presplit(vals), None)
        got = Fn.edge_mlp_bwd(vals, *w, gout, False, csr.presplit(vals), sym)
        for a_, r_ in zip(got[1:], ref[1:]):
            close(a_, r_, tol=1e-5, what='unique-row backward, six supports')


def test_edge_branch_over_unique_rows_twelve_supports(dev):
    """counting.py's twelve supports (the 9 .. 16-support kernel family) on the unique-row road: forward bitwise the plain three-piece
    forward, weight gradients equal to the plain backward's to summation order, and the counting model's step with the road on / off."""
    from gnn_matlang_amd import SpectralDesign, collate, synthetic, functional as Fn, models
    raw = synthetic.make_graphs('counting', 96, seed=12)
    b = collate(SpectralDesign(recfield=1, dv=1, nfreq=10, adddegree=True, laplacien=False, addadj=True).design_many(raw)).to(dev)
    assert b.edge_attr2.size(1) == 12
    # counting.py's design (laplacien=False) computes its supports in a way that leaves mirrored rows one fp32 ulp apart (14 % of the
    # pairs are bitwise equal): the pairing pass then finds nothing to share and the plain kernels run -- checked first.  The rest of
    # the test runs on the same supports made bitwise symmetric (every edge takes the row of its src < dst orientation).
    csr = b.csr('edge_index2')
    assert csr.sym_index(csr.to_source_order(csr.sort_values(b.edge_attr2))) is None
    ei = b.edge_index2.cpu().numpy()
    N = int(b.x.size(0))
    key, rkey = ei[0].astype(np.int64) * N + ei[1], ei[1].astype(np.int64) * N + ei[0]
    order = np.argsort(key)
    rev = order[np.searchsorted(key[order], rkey)]
    ea = b.edge_attr2.cpu().numpy()
    b.edge_attr2 = torch.from_numpy(np.where((ei[0] <= ei[1])[:, None], ea, ea[rev])).to(dev)
    vals = csr.to_source_order(csr.sort_values(b.edge_attr2), cache=True)
    sym = csr.sym_index(vals)
    assert sym is not None and sym[0].numel() < 0.75 * csr.E
    torch.manual_seed(7)
    w = tuple(torch.randn(*shp, device=dev) * 0.3 for shp in ((24, 12), (24, 12), (24, 12), (12, 48)))
    plain = Fn.edge_mlp_fwd(vals, *w, None, csr.presplit(vals))[0]
    shared = Fn.edge_mlp_fwd_stack(vals, None, [w], sym)
    assert shared is not None and torch.equal(plain, shared[0])
    gout = torch.randn_like(vals)
    ref = Fn.edge_mlp_bwd(vals, *w, gout, False, csr.presplit(vals), None)
    got = Fn.edge_mlp_bwd(vals, *w, gout, False, csr.presplit(vals), sym)
    for a_, r_ in zip(got[1:], ref[1:]):
        close(a_, r_, tol=3e-5, what='unique-row backward, twelve supports')      # (both are bf16x3 sums, split at different points: 1e-5 class)
    torch.manual_seed(0)
    m = models.counting_gnnml3().to(dev)
    y = b.y.float() if b.y.dim() == 1 else b.y[:, 0].float()
    res = {}
    for on in (True, False):
        old = Fn.EDGE_SYM
        Fn.EDGE_SYM = on
        try:
            m.zero_grad()
            pre = m(b)
            models.counting_loss(pre, y).backward()
            res[on] = (pre.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()})
        finally:
            Fn.EDGE_SYM = old
    assert torch.equal(res[True][0], res[False][0])
    for n in res[True][1]:
        close(res[True][1][n], res[False][1][n], tol=3e-5, what='counting, shared vs plain ' + n)


# road kind: (layers in the chain, supports, symmetric supports, supports carry a gradient, grad enabled, rows of the CPU table
# (tests/test_ml3_fwd_road_cpu.py) the forward calls must record, 'edge' path of the branch)
_FWD_ROAD_KINDS = {
    'source + stack + pairs': (4, 8, True, False, True, ['zinc bottom layer, three stackable successors'] + ['the same on a stash hit'] * 3,
                               'stack of 4 layers in one pass, matrix-core chain, three-piece, unique rows'),
    'source single': (1, 8, False, False, True, ['EDGE_STACK off'], 'matrix-core chain, three-piece'),
    'target + pairs under no_grad': (1, 8, True, False, False, ['grad disabled'], 'matrix-core chain, three-piece, unique rows'),
    'supports with gradient': (1, 8, False, True, True, ['supports that carry a gradient'], 'matrix-core chain, three-piece'),
    '20 supports (wide)': (1, 20, False, True, True, ['17 supports'], 'one-launch kernel for 17..48 supports'),
    '50 supports (library)': (1, 50, False, True, True, ['49 supports'], 'library GEMMs (more than 48 supports)'),
}


@pytest.mark.parametrize('kind', sorted(_FWD_ROAD_KINDS))
def test_ml3_forward_runs_the_road_its_record_names(dev, monkeypatch, kind):
    """One forward and one backward per road kind of functional._ml3_fwd_road that can run for real, on two graphs of 20 nodes with 6
    neighbours each, 32 -> 30 + 2: the `ml3_fwd` record of every layer call is the row of the CPU table (written out here from the
    table's tuples, not by the code's formatter), the edge branch took the family that row names, and the output and every gradient
    agree with the float64 oracle within TOL = 1e-4, the bar test_ml3layer_golden (the default roads) and test_ml3layer_wide_shapes
    (trained supports, 17 .. 48 supports, the library GEMMs) hold these roads to.  Under no_grad there is no backward: outputs only."""
    from gnn_matlang_amd import ML3Layer, functional as Fn
    from oracle.spect_conv_oracle import OracleML3Layer
    from oracle.relu_margin import make_safe, make_safe_edges
    from test_ml3_fwd_road_cpu import TABLE
    nl, S, symmetric, sup_grad, grad_on, rows, edge_path = _FWD_ROAD_KINDS[kind]
    torch.manual_seed(71)
    n, N = 20, 40
    src = np.repeat(np.arange(N), 6)
    dst = np.concatenate([(i // n) * n + (i % n + np.array([1, 2, 5, n - 1, n - 2, n - 5])) % n for i in range(N)])
    o = np.lexsort((dst, src))                                 # source-sorted, columns ascending: as SpectralDesign emits
    src, dst = src[o], dst[o]
    ei = torch.from_numpy(np.stack([src, dst]).astype(np.int64))
    refs = [OracleML3Layer(True, S, S, 32, 30, 2).double() for _ in range(nl)]
    ms = [ML3Layer(True, S, S, 32, 30, 2).to(dev) for _ in range(nl)]
    for m, r, lo in zip(ms, refs, [None] + ms):
        m.load_state_dict({k: p.detach().float() for k, p in r.state_dict().items()})
        if lo is not None:
            m.chain_after(lo)
    x, ea, go = torch.randn(N, 32), torch.randn(ei.size(1), S) * 0.5, torch.randn(N, 32)
    if symmetric:                                              # an edge and its mirror carry bitwise the same row
        for _ in range(20):                                    # (rows whose edge-branch relus keep their margin in EVERY layer)
            before = ea.clone()
            for r in refs:
                ea = make_safe_edges(ea, *(getattr(r, 'fc1_%d' % i).weight.detach() for i in (1, 2, 3, 4)), scale=0.5)
            if torch.equal(before, ea):
                break
        low = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(src, dst))}
        ea = torch.stack([ea[low[(min(a, b), max(a, b))]] for a, b in zip(src.tolist(), dst.tolist())])
    elif nl == 1:
        ea, mask = make_safe(x, ei, ea, refs[0].state_dict(), True)       # no relu argument within rounding of zero
        go[:, :30] *= mask.float()
    xr, er = x.double().requires_grad_(True), ea.double().requires_grad_(sup_grad)
    yr = xr
    for r in refs:
        yr = r(yr, ei, er)
    (yr * go.double()).sum().backward()
    monkeypatch.setattr(Fn, 'VERBOSE', True)
    Fn.PATHS.clear()
    xg, eg, eid = x.to(dev).requires_grad_(True), ea.to(dev).requires_grad_(sup_grad), ei.to(dev)
    with torch.set_grad_enabled(grad_on):
        y = xg
        for m in ms:
            y = m(y, eid, eg)
    paths = dict(Fn.PATHS)
    want = {}
    for name in rows:
        rec, conv = TABLE[name][1], TABLE[name][2]
        vals = [int(v) if isinstance(v, bool) else v for v in rec] + [conv[2]]
        key = 'ml3_fwd: %s (S=%d Fin=32 Fout=30)' % (' '.join('%s=%s' % kv for kv in zip(Fn.ML3FwdRoad._fields, vals)), S)
        want[key] = want.get(key, 0) + 1
    assert {k: c for k, c in paths.items() if k.startswith('ml3_fwd:')} == want, paths
    assert [k for k in paths if k.startswith('edge:')] == ['edge: %s (S=%d Fin=- Fout=%d)' % (edge_path, S, S)], paths
    close(y, yr, what=kind + ' out')
    if grad_on:
        (y * go.to(dev)).sum().backward()
        close(xg.grad, xr.grad, what=kind + ' g_x')
        if sup_grad:
            close(eg.grad, er.grad, what=kind + ' g_edge_attr')
        for m, r in zip(ms, refs):
            gp = dict(m.named_parameters())
            for k, p in r.named_parameters():
                close(gp[k].grad, p.grad, what='%s %s' % (kind, k))
