"""The large-graph dense support product (csrc/gml_dense_big.hip) against float64: random NON-symmetric blocks at 40 % fill (grid
supports are symmetric and would hide a missing transpose), both directions with their sa / so offsets, activation rows beyond n
that are NaN, a wider output whose other columns must survive, bitwise repeatability, and the range limits."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4
SENTINEL = -777.25
SS = (1, 3, 11)
FS = (1, 20, 48, 64)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _blocks(n, dev):
    """[11, n, n] float32: 40 % of the entries nonzero, values of mixed sign and magnitude, no symmetry"""
    g = torch.Generator(device='cpu').manual_seed(1000 + n)
    keep = torch.rand(11, n, n, generator=g) < 0.4
    val = torch.randn(11, n, n, generator=g) * (0.05 + torch.rand(11, 1, 1, generator=g))
    b = (val * keep).to(dev)
    assert not torch.equal(b[0], b[0].t())
    return b


def _pack(blocks, transpose):
    from gnn_matlang_amd import _lib
    S, n, _ = blocks.shape
    KP = (n + 31) // 32 * 32
    img = torch.full((S, 2, n, KP), 0x7fc0, dtype=torch.int16, device=blocks.device)      # (bf16 NaN: every element must be written)
    _lib.call('gml_dense_big_pack', _p(blocks), _p(img), S, n, KP, transpose, None)
    return img, KP


def _mm(img, act, lda, sa, out, ldo, so, sum_s, S, n, KP, F):
    from gnn_matlang_amd import _lib
    nws = int(_lib.lib().gml_dense_big_workspace_bytes(S, n, F, sum_s))
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=act.device)
    return _lib.lib().gml_dense_big_support_mm(_p(img), _p(act), lda, sa, _p(out), ldo, so, sum_s, S, n, KP, F, _p(ws), nws, None)


def test_pack_images_are_the_split_blocks(dev):
    """hi + lo reproduces the block to 2^-16 relative, the K padding is zero, transpose = 1 holds the transposed block"""
    b = _blocks(110, dev)[:2]
    for tr in (0, 1):
        img, KP = _pack(b, tr)
        f = (img.view(torch.bfloat16).float()).sum(1)         # hi + lo [S, n, KP]
        want = b.transpose(1, 2) if tr else b
        assert torch.equal(f[:, :, 110:], torch.zeros_like(f[:, :, 110:]))
        assert float((f[:, :, :110] - want).abs().max()) <= 2.0 ** -16 * float(want.abs().max())


@pytest.mark.parametrize('n', [97, 110, 169, 900, 1024])
def test_product_both_directions(dev, n):
    from gnn_matlang_amd import _lib
    blocks = _blocks(n, dev)
    fwd, KP = _pack(blocks, 0)
    bwd, _ = _pack(blocks, 1)
    b64 = blocks.double()
    g = torch.Generator(device='cpu').manual_seed(77 + n)
    worst = 0.0
    for S in SS:
        for F in FS:
            # ---- forward: act = X (sa = 0) as the first n rows of a buffer whose other rows (and pad columns) are NaN
            lda = F + 4
            xbuf = torch.full((n + 9, lda), float('nan'), device=dev)
            x = torch.randn(n, F, generator=g).to(dev)
            xbuf[:n, :F] = x
            pad = 8 if F % 4 == 0 and S != 3 else 5            # (float4-addressable output rows, and rows that are not)
            ldo = S * F + pad
            out = torch.full((n, ldo), SENTINEL, device=dev)
            assert _mm(fwd[:S], xbuf, lda, 0, out, ldo, F, 0, S, n, KP, F) == 0
            ref = torch.matmul(b64[:S], x.double()).permute(1, 0, 2).reshape(n, S * F)      # Hcat[r, s F + f]
            e = rel_err(out[:, :S * F].cpu().numpy(), ref.cpu().numpy())
            assert e <= TOL, ('forward', n, S, F, e)
            assert bool((out[:, S * F:] == SENTINEL).all()), ('forward wrote outside its columns', n, S, F)
            out2 = torch.full((n, ldo), SENTINEL, device=dev)
            assert _mm(fwd[:S], xbuf, lda, 0, out2, ldo, F, 0, S, n, KP, F) == 0
            assert torch.equal(out, out2), ('forward differs between two runs', n, S, F)
            worst = max(worst, e)
            # ---- adjoint: transposed images, act = d Hcat (sa = F), summed over s
            lda = S * F + (4 if F % 4 == 0 else 3)
            gbuf = torch.full((n + 3, lda), float('nan'), device=dev)
            gh = torch.randn(n, S * F, generator=g).to(dev)
            gbuf[:n, :S * F] = gh
            ldo = F + pad
            dx = torch.full((n, ldo), SENTINEL, device=dev)
            assert _mm(bwd[:S], gbuf, lda, F, dx, ldo, 0, 1, S, n, KP, F) == 0
            ref = torch.matmul(b64[:S].transpose(1, 2), gh.double().view(n, S, F).permute(1, 0, 2)).sum(0)   # sum_s D_s^T G_s
            e = rel_err(dx[:, :F].cpu().numpy(), ref.cpu().numpy())
            assert e <= TOL, ('adjoint', n, S, F, e)
            assert bool((dx[:, F:] == SENTINEL).all()), ('adjoint wrote outside its columns', n, S, F)
            dx2 = torch.full((n, ldo), SENTINEL, device=dev)
            assert _mm(bwd[:S], gbuf, lda, F, dx2, ldo, 0, 1, S, n, KP, F) == 0
            assert torch.equal(dx, dx2), ('adjoint differs between two runs', n, S, F)
            worst = max(worst, e)
    print('n=%d worst rel err %.2e' % (n, worst))
    torch.cuda.synchronize()
    assert _lib.GML_OK == 0


def test_python_layer_matches_the_library_product(dev):
    """dense_supports -> _SupportProduct on one 169-node graph: forward and gradient against the fp32 library road"""
    from gnn_matlang_amd import dense_block as DB, functional as Fn
    n, S, F = 169, 3, 20
    blocks = _blocks(n, dev)[:S]
    mask = (blocks != 0).any(0)                               # the union mask lists every (j, i) once
    jj, ii = torch.nonzero(mask, as_tuple=True)
    ei2 = torch.stack([ii, jj])                                # row 0 = source i, row 1 = target j
    ea2 = blocks[:, jj, ii].t().contiguous()
    ptr = torch.tensor([0, n], dtype=torch.int32)
    sup = DB.dense_supports(ei2, ea2, ptr, n)
    assert sup.blocks is None and sup.fwd is not None and tuple(sup.fwd.shape) == (1, S, 2, n, 192)
    x = torch.randn(n, F, device=dev, requires_grad=True)
    h = DB._SupportProduct.apply(x, sup)
    gh = torch.randn_like(h)
    h.backward(gh)
    x64 = x.detach().double()
    ref = torch.matmul(blocks.double(), x64).permute(1, 0, 2).reshape(n, S * F)
    gref = torch.matmul(blocks.double().transpose(1, 2), gh.double().view(n, S, F).permute(1, 0, 2)).sum(0)
    assert rel_err(h.detach().cpu().numpy(), ref.cpu().numpy()) <= TOL
    assert rel_err(x.grad.cpu().numpy(), gref.cpu().numpy()) <= TOL
    with Fn.exact_products():                                 # the library road serves under exact products
        sup2 = DB.dense_supports(ei2, ea2, ptr, n)
    assert sup2.blocks is not None and sup2.fwd is None


def test_outside_the_range(dev):
    """n = 1025 or F = 65: GML_E_UNSUPPORTED from the C entries; the Python layer stays on the sparse road without an exception"""
    from gnn_matlang_amd import _lib, dense_block as DB, models, functional as Fn
    from gnn_matlang_amd.graph import Batch
    L = _lib.lib()
    buf = torch.zeros(1 << 16, device=dev)
    img = torch.zeros(1 << 16, dtype=torch.int16, device=dev)
    assert L.gml_dense_big_support_mm(_p(img), _p(buf), 64, 0, _p(buf), 64, 0, 0, 1, 1025, 1056, 48, None, 0, None) == _lib.GML_E_UNSUPPORTED
    assert L.gml_dense_big_support_mm(_p(img), _p(buf), 80, 0, _p(buf), 80, 0, 0, 1, 900, 928, 65, None, 0, None) == _lib.GML_E_UNSUPPORTED
    assert L.gml_dense_big_support_mm(_p(img), _p(buf), 64, 0, _p(buf), 64, 0, 0, 1, 96, 96, 48, None, 0, None) == _lib.GML_E_UNSUPPORTED
    assert L.gml_dense_big_pack(_p(buf), _p(img), 1, 1025, 1056, 0, None) == _lib.GML_E_UNSUPPORTED
    assert L.gml_dense_big_pack(_p(buf), _p(img), 1, 96, 96, 0, None) == _lib.GML_E_UNSUPPORTED
    assert int(L.gml_dense_big_workspace_bytes(11, 1025, 48, 1)) == 0
    assert not DB.big_applies(1, 1025, 48) and not DB.big_applies(1, 900, 65) and not DB.big_applies(2, 900, 48)
    assert DB.big_applies(1, 1024, 64) and DB.big_applies(1, 97, 1) and not DB.big_applies(1, 96, 1)
    # a node-level model on one graph of 1025 nodes the sparse road, no exception
    n, S = 1025, 11
    g = torch.Generator(device='cpu').manual_seed(3)
    keep = torch.rand(n, n, generator=g) < 0.06
    keep = keep | keep.t()
    ii, jj = torch.nonzero(keep, as_tuple=True)              # sorted by source
    data = Batch(x=torch.randn(n, 1, generator=g), edge_index=torch.stack([ii, jj]), edge_index2=torch.stack([ii, jj]),
                 edge_attr2=torch.randn(ii.numel(), S, generator=g) * 0.02, batch=torch.zeros(n, dtype=torch.int64),
                 ptr=torch.tensor([0, n], dtype=torch.int32), y=torch.randn(n, 3, generator=g),
                 mask=(torch.rand(n, 1, generator=g) < 0.7).float()).to(dev)
    torch.manual_seed(0)
    m = models.filtering_gnnml3(1, S).to(dev)
    assert m._road_of(data).kind != 'big'
    old, Fn.VERBOSE = Fn.VERBOSE, True
    Fn.PATHS.clear()
    try:
        loss = models.filtering_step_loss(m, data)
        loss.backward()
    finally:
        Fn.VERBOSE = old
    assert torch.isfinite(loss) and all(torch.isfinite(p.grad).all() for p in m.parameters())
    assert not any(k.startswith('dense') for k in Fn.PATHS), Fn.PATHS
    Fn.PATHS.clear()
