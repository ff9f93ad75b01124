"""The batched-blocks dense support product (csrc/gml_dense_mid.hip: B equal-size graphs of 97 .. 256 nodes, F <= 128, bank slots)
against float64: random NON-symmetric blocks at 10 % fill, different for every graph and support (a wrong slot or a missing
transpose shows), both directions with their sa / so offsets, activation rows and pad columns that are NaN, a taller and wider output
whose other elements must survive, float4-addressable rows and rows that are not, bitwise repeatability, the range limits, and the
Python layer (EqualSupports, _SupportProduct with bank slots, the library road, dense_supports)."""
import ctypes

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4
SENTINEL = -777.25
G = 5
SS = (1, 6)
FS = (1, 64, 66, 128)
# (bank slots or None, graphs the bank is packed with)
SLOTS = (([4, 0, 4], G), (None, 2), ([2], G), (None, 1))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _blocks(n, dev, graphs=G, S=6):
    """[graphs, S, n, n] float32: 10 % of the entries nonzero, values of mixed sign and magnitude, no symmetry, no two alike"""
    g = torch.Generator(device='cpu').manual_seed(2000 + n)
    keep = torch.rand(graphs, S, n, n, generator=g) < 0.1
    val = torch.randn(graphs, S, n, n, generator=g) * (0.05 + torch.rand(graphs, S, 1, 1, generator=g))
    b = (val * keep).to(dev)
    assert not torch.equal(b[0, 0], b[0, 0].t()) and not torch.equal(b[0, 0], b[-1, -1])
    return b


def _pack(blocks, transpose):
    """bank [G, S, 2, n, KP] of the blocks [G, S, n, n] through the existing pack kernel"""
    from gnn_matlang_amd import _lib
    Gb, S, n, _ = blocks.shape
    KP = (n + 31) // 32 * 32
    img = torch.full((Gb, S, 2, n, KP), 0x7fc0, dtype=torch.int16, device=blocks.device)   # (bf16 NaN: every element must be written)
    _lib.call('gml_dense_big_pack', _p(blocks.contiguous()), _p(img), Gb * S, n, KP, transpose, None)
    return img, KP


def _mm(img, gid, act, lda, sa, out, ldo, so, sum_s, B, Gb, S, n, KP, F):
    from gnn_matlang_amd import _lib
    return _lib.lib().gml_dense_mid_support_mm(_p(img), _p(gid), _p(act), lda, sa, _p(out), ldo, so, sum_s, B, Gb, S, n, KP, F, None)


@pytest.mark.parametrize('n', [97, 128, 129, 200, 256])
def test_product_both_directions(dev, n):
    blocks = _blocks(n, dev)
    b64 = blocks.double()
    g = torch.Generator(device='cpu').manual_seed(91 + n)
    worst = 0.0
    for S in SS:
        bs = blocks[:, :S].contiguous()
        fwd, KP = _pack(bs, 0)
        bwd, _ = _pack(bs, 1)
        for F in FS:
            for cfg, (slots, Gb) in enumerate(SLOTS):
                B = len(slots) if slots is not None else Gb
                gid = torch.tensor(slots, dtype=torch.int32, device=dev) if slots is not None else None
                D = b64[slots if slots is not None else list(range(B)), :S]              # [B, S, n, n]
                tall = B * n + 7
                # ---- forward: act = X (sa = 0): the first B n rows of a taller buffer whose other rows and pad columns are NaN
                lda = F + 4
                xbuf = torch.full((B * n + 9, lda), float('nan'), device=dev)
                x = torch.randn(B * n, F, generator=g).to(dev)
                xbuf[:B * n, :F] = x
                pad = (8, 5)[cfg % 2]                             # (float4-addressable output rows, and rows that are not)
                ldo = S * F + pad
                out = torch.full((tall, ldo), SENTINEL, device=dev)
                assert _mm(fwd, gid, xbuf, lda, 0, out, ldo, F, 0, B, Gb, S, n, KP, F) == 0
                ref = torch.matmul(D, x.double().view(B, 1, n, F)).permute(0, 2, 1, 3).reshape(B * n, S * F)   # Hcat[b n + r, s F + f]
                e = rel_err(out[:B * n, :S * F].cpu().numpy(), ref.cpu().numpy())
                assert e <= TOL, ('forward', n, S, F, slots, e)
                assert bool((out[:, S * F:] == SENTINEL).all()) and bool((out[B * n:] == SENTINEL).all()), ('forward wrote outside', n, S, F, slots)
                out2 = torch.full((tall, ldo), SENTINEL, device=dev)
                assert _mm(fwd, gid, xbuf, lda, 0, out2, ldo, F, 0, B, Gb, S, n, KP, F) == 0
                assert torch.equal(out, out2), ('forward differs between two runs', n, S, F, slots)
                worst = max(worst, e)
                # ---- adjoint: transposed bank, act = d Hcat (sa = F), summed over s
                lda = S * F + (4 if F % 4 == 0 else 3)
                gbuf = torch.full((B * n + 3, lda), float('nan'), device=dev)
                gh = torch.randn(B * n, S * F, generator=g).to(dev)
                gbuf[:B * n, :S * F] = gh
                pad = (5, 8)[cfg % 2]
                ldo = F + pad
                dx = torch.full((tall, ldo), SENTINEL, device=dev)
                assert _mm(bwd, gid, gbuf, lda, F, dx, ldo, 0, 1, B, Gb, S, n, KP, F) == 0
                ref = torch.matmul(D.transpose(2, 3), gh.double().view(B, n, S, F).permute(0, 2, 1, 3)).sum(1).reshape(B * n, F)
                e = rel_err(dx[:B * n, :F].cpu().numpy(), ref.cpu().numpy())
                assert e <= TOL, ('adjoint', n, S, F, slots, e)
                assert bool((dx[:, F:] == SENTINEL).all()) and bool((dx[B * n:] == SENTINEL).all()), ('adjoint wrote outside', n, S, F, slots)
                dx2 = torch.full((tall, ldo), SENTINEL, device=dev)
                assert _mm(bwd, gid, gbuf, lda, F, dx2, ldo, 0, 1, B, Gb, S, n, KP, F) == 0
                assert torch.equal(dx, dx2), ('adjoint differs between two runs', n, S, F, slots)
                worst = max(worst, e)
    print('n=%d worst rel err %.2e' % (n, worst))
    torch.cuda.synchronize()


def test_outside_the_range(dev):
    """GML_E_UNSUPPORTED for n = 96 / 257, F = 0 / 129 and a KP that is not 32 ceil(n / 32); GML_E_BADARG for NULL pointers, images off
    16 bytes and short lda / ldo; nothing is launched (the output keeps its sentinel); the predicate's truth table"""
    from gnn_matlang_amd import _lib, dense_block as DB
    L = _lib.lib()
    buf = torch.zeros(1 << 18, device=dev)
    out = torch.full((1 << 18,), SENTINEL, device=dev)
    img = torch.zeros(1 << 20, dtype=torch.int16, device=dev)

    def mm(n, KP, F, lda=None, ldo=None, im=img, a=buf, o=out, S=2, sum_s=0):
        lda = (S * F if sum_s else F) if lda is None else lda
        ldo = (F if sum_s else S * F) if ldo is None else ldo
        return L.gml_dense_mid_support_mm(_p(im), None, _p(a), lda, F if sum_s else 0, _p(o), ldo, 0 if sum_s else F, sum_s, 2, 2, S, n, KP, F, None)
    U, A = _lib.GML_E_UNSUPPORTED, _lib.GML_E_BADARG
    assert mm(200, 224, 66) == 0 and mm(200, 224, 66, sum_s=1) == 0
    out.fill_(SENTINEL)
    assert mm(96, 96, 48) == U and mm(257, 288, 48) == U
    assert mm(200, 224, 0) == U and mm(200, 224, 129) == U
    assert mm(200, 256, 48) == U and mm(200, 200, 48) == U and mm(97, 97, 48) == U
    assert mm(200, 224, 48, S=0) == U
    assert mm(200, 224, 48, im=None) == A and mm(200, 224, 48, a=None) == A and mm(200, 224, 48, o=None) == A
    assert mm(200, 224, 48, im=img[1:]) == A                          # images 2 bytes off a 16-byte boundary
    assert mm(200, 224, 48, lda=47) == A and mm(200, 224, 48, ldo=95) == A
    assert mm(200, 224, 48, lda=95, sum_s=1) == A and mm(200, 224, 48, ldo=47, sum_s=1) == A
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    t = DB.mid_applies
    assert t(2, 97, 1) and t(64, 200, 66) and t(2, 256, 128) and t(1, 200, 66, bank=True)
    assert not t(1, 200, 66) and not t(2, 96, 66) and not t(2, 257, 66) and not t(2, 200, 129) and not t(2, 200, 0)
    assert not t(0, 200, 66, bank=True)


def _coo(blocks):
    """collated COO supports (global node ids, the union mask lists every (i, j) once) of blocks [G, S, n, n]"""
    Gb, S, n, _ = blocks.shape
    bb, jj, ii = torch.nonzero((blocks != 0).any(1), as_tuple=True)
    ei2 = torch.stack([bb * n + ii, bb * n + jj])                  # row 0 = source i, row 1 = target j
    ea2 = blocks[bb, :, jj, ii].contiguous()
    ptr = torch.arange(Gb + 1, dtype=torch.int32, device=blocks.device) * n
    return ei2, ea2, ptr


def test_equal_supports_and_the_python_layer(dev):
    from gnn_matlang_amd import dense_block as DB, functional as Fn
    n, S, F = 110, 3, 20
    blocks = _blocks(n, dev, graphs=3, S=S)
    ei2, ea2, ptr = _coo(blocks)
    bank = DB.EqualSupports(ei2, ea2, ptr)
    assert (bank.G, bank.S, bank.n, bank.KP) == (3, S, n, 128) and bank._blocks is None
    assert tuple(bank.fwd.shape) == (3, S, 2, n, 128) and bank.fwd.dtype == torch.int16 and tuple(bank.bwd.shape) == tuple(bank.fwd.shape)
    for img, want in ((bank.fwd, blocks), (bank.bwd, blocks.transpose(2, 3))):
        f = img.view(torch.bfloat16).float().sum(2)             # hi + lo [G, S, n, KP]
        assert torch.equal(f[..., n:], torch.zeros_like(f[..., n:]))
        assert float((f[..., :n] - want).abs().max()) <= 2.0 ** -16 * float(want.abs().max())
    # slabs: a bank packed graph by graph holds the same bits
    old, DB.EqualSupports.SLAB_BYTES = DB.EqualSupports.SLAB_BYTES, 4 * S * n * n
    try:
        bank1 = DB.EqualSupports(ei2, ea2, ptr)
    finally:
        DB.EqualSupports.SLAB_BYTES = old
    assert torch.equal(bank1.fwd, bank.fwd) and torch.equal(bank1.bwd, bank.bwd)
    # _SupportProduct with permuted slots: forward and x.grad against float64, the paths recorded
    gid = torch.tensor([2, 0, 1, 2], dtype=torch.int32, device=dev)
    B = int(gid.numel())
    x = torch.randn(B * n, F, device=dev, requires_grad=True)
    old, Fn.VERBOSE = Fn.VERBOSE, True
    Fn.PATHS.clear()
    try:
        h = DB._SupportProduct.apply(x, bank, gid)
        gh = torch.randn_like(h)
        h.backward(gh)
        paths = dict(Fn.PATHS)
    finally:
        Fn.VERBOSE = old
        Fn.PATHS.clear()
    assert any('support product fwd (bf16x3 HIP, batched blocks)' in k for k in paths), paths
    assert any('support product bwd (bf16x3 HIP, batched blocks)' in k for k in paths), paths
    D = blocks.double()[gid.long()]
    ref = torch.matmul(D, x.detach().double().view(B, 1, n, F)).permute(0, 2, 1, 3).reshape(B * n, S * F)
    gref = torch.matmul(D.transpose(2, 3), gh.double().view(B, n, S, F).permute(0, 2, 1, 3)).sum(1).reshape(B * n, F)
    assert rel_err(h.detach().cpu().numpy(), ref.cpu().numpy()) <= TOL
    assert rel_err(x.grad.cpu().numpy(), gref.cpu().numpy()) <= TOL
    # the layer on the kernel and on the library road (exact products): the same values to the tolerance, blocks built on first use
    w = torch.randn(S, F, 7, device=dev) * 0.2
    bias = torch.randn(7, device=dev)
    y = DB.spectconv_dense(x.detach(), bank, w, bias, n, relu=True, gid=gid)
    assert bank._blocks is None
    with Fn.exact_products():
        Fn.VERBOSE = True
        try:
            yl = DB.spectconv_dense(x.detach(), bank, w, bias, n, relu=True, gid=gid)
            assert any('torch.bmm fp32' in k for k in Fn.PATHS), Fn.PATHS
        finally:
            Fn.VERBOSE = old
            Fn.PATHS.clear()
    assert bank._blocks is not None and torch.equal(bank.blocks, blocks)
    yref = torch.relu(ref @ w.double().reshape(S * F, 7) + bias.double())
    assert rel_err(y.cpu().numpy(), yref.cpu().numpy()) <= TOL and rel_err(yl.cpu().numpy(), yref.cpu().numpy()) <= TOL
    with pytest.raises(ValueError):
        DB.spectconv_dense(torch.randn(B * n, 129, device=dev), bank, torch.randn(S, 129, 7, device=dev), None, n, gid=gid)


def test_dense_supports_takes_batches_of_mid_size_graphs(dev):
    """2 graphs of 110 nodes no longer raise and run on the batched-blocks kernel; ONE graph of 169 nodes keeps the large-graph road"""
    from gnn_matlang_amd import dense_block as DB, functional as Fn

    def run(graphs, n):
        blocks = _blocks(n, dev, graphs=graphs, S=2)
        ei2, ea2, ptr = _coo(blocks)
        sup = DB.dense_supports(ei2, ea2, ptr, n)
        assert sup.blocks is None and tuple(sup.fwd.shape) == (graphs, 2, 2, n, (n + 31) // 32 * 32)
        x = torch.randn(graphs * n, 5, device=dev, requires_grad=True)
        old, Fn.VERBOSE = Fn.VERBOSE, True
        Fn.PATHS.clear()
        try:
            h = DB._SupportProduct.apply(x, sup)
            h.sum().backward()
            paths = dict(Fn.PATHS)
        finally:
            Fn.VERBOSE = old
            Fn.PATHS.clear()
        ref = torch.matmul(blocks.double(), x.detach().double().view(graphs, 1, n, 5)).permute(0, 2, 1, 3).reshape(graphs * n, 10)
        assert rel_err(h.detach().cpu().numpy(), ref.cpu().numpy()) <= TOL
        gref = blocks.double().sum(2).sum(1).reshape(graphs * n, 1).expand(-1, 5)          # d/dx of the sum: column sums of every block
        assert rel_err(x.grad.cpu().numpy(), gref.cpu().numpy()) <= TOL
        return paths
    paths = run(2, 110)
    assert any('fwd (bf16x3 HIP, batched blocks)' in k for k in paths) and any('bwd (bf16x3 HIP, batched blocks)' in k for k in paths), paths
    paths = run(1, 169)
    assert any('fwd (bf16x3 HIP, large graph)' in k for k in paths) and any('bwd (bf16x3 HIP, large graph)' in k for k in paths), paths
    with pytest.raises(ValueError):                             # three graphs of 300 nodes: no dense kernel
        ei2, ea2, ptr = _coo(_blocks(300, dev, graphs=3, S=1))
        DB.dense_supports(ei2, ea2, ptr, 300)


# ------------------------------------------------------------------ the mode of the call decides the road, not the supports'
def _coo_by_source(blocks):
    """_coo with a symmetric union mask and the edges sorted by source, as SpectralDesign emits them (both roads read these)"""
    Gb, S, n, _ = blocks.shape
    mask = (blocks != 0).any(1)
    bb, ii, jj = torch.nonzero((mask | mask.transpose(1, 2)).transpose(1, 2), as_tuple=True)
    ptr = torch.arange(Gb + 1, dtype=torch.int32, device=blocks.device) * n
    return torch.stack([bb * n + ii, bb * n + jj]), blocks[bb, :, jj, ii].contiguous(), ptr


def test_supports_built_in_the_other_mode_raise(dev):
    """spectconv_dense takes the road from the library mode of THE CALL; supports that hold the other side raise before any launch"""
    from gnn_matlang_amd import dense_block as DB, functional as Fn
    n, F = 4, 3
    g = torch.Generator(device='cpu').manual_seed(4)
    blocks = torch.randn(1, 1, n, n, generator=g).to(dev)
    ei2, ea2, ptr = _coo(blocks)
    x, w = torch.randn(n, F, generator=g).to(dev), torch.randn(1, F, 2, generator=g).to(dev)
    ref = (blocks[0, 0].double() @ x.double()) @ w[0].double()
    outside = DB.dense_supports(ei2, ea2, ptr, n)
    assert outside.blocks is None and outside.fwd is not None
    with Fn.exact_products():
        inside = DB.dense_supports(ei2, ea2, ptr, n)
        assert inside.blocks is not None and inside.fwd is None
        with pytest.raises(ValueError, match='rebuild'):
            DB.spectconv_dense(x, outside, w, None, n)
        y_in = DB.spectconv_dense(x, inside, w, None, n)
    with pytest.raises(ValueError, match='rebuild'):
        DB.spectconv_dense(x, inside, w, None, n)
    y_out = DB.spectconv_dense(x, outside, w, None, n)
    assert rel_err(y_in.cpu().numpy(), ref.cpu().numpy()) <= TOL and rel_err(y_out.cpu().numpy(), ref.cpu().numpy()) <= TOL
    # the cache on a batch follows the mode
    data = type('B', (), {})()
    data.edge_index2, data.edge_attr2, data.ptr = ei2, ea2, ptr
    a = DB.batch_supports(data, n)
    assert a.fwd is not None and DB.batch_supports(data, n) is a
    with Fn.exact_products():
        b = DB.batch_supports(data, n)
        assert b is not a and b.blocks is not None and DB.batch_supports(data, n) is b
    assert DB.batch_supports(data, n).fwd is not None


_ROADS = {}


def _road_case(kind, dev):
    """(model, batch, _road, the dense_road arguments (graphs, n, bank)) of one forward of each kind; the 97-node data built once"""
    from gnn_matlang_amd import dense_block as DB, models
    from gnn_matlang_amd.graph import Batch
    if not _ROADS:
        torch.manual_seed(5)
        g = torch.Generator(device='cpu').manual_seed(6)
        n, S = 97, 2
        blocks = _blocks(n, dev, graphs=2, S=S)
        ei2, ea2, ptr = _coo_by_source(blocks)
        one = ei2[0] < n
        x = torch.randn(2 * n, 1, generator=g).to(dev)
        node = models.GNNML3(1, S, 8, 4, 2, learnedge=False, pool=None, head='node').to(dev)
        single = Batch(x=x[:n].contiguous(), edge_index2=ei2[:, one].contiguous(), edge_attr2=ea2[one].contiguous(),
                       batch=torch.zeros(n, dtype=torch.int64, device=dev), ptr=ptr[:2].contiguous())
        banked = DB.attach_bank(Batch(x=x, batch=torch.arange(2, device=dev).repeat_interleave(n), ptr=ptr), DB.EqualSupports(ei2, ea2, ptr))
        n5 = 5
        b5 = (torch.randn(2, S, n5, n5, generator=g) * 0.3).to(dev)
        ei5, ea5, ptr5 = _coo_by_source(b5)
        small = Batch(x=torch.randn(2 * n5, 3, generator=g).to(dev), edge_index2=ei5, edge_attr2=ea5,
                      batch=torch.arange(2, device=dev).repeat_interleave(n5), ptr=ptr5)
        pooled = models.GNNML3(3, S, 8, 0, 2, learnedge=False, pool='add', head='mlp32', dense_n=n5).to(dev)
        _ROADS.update(dense_n=(pooled, small, None, (2, n5, False)), big=(node, single, None, (1, n, False)),
                      mid=(node, banked, None, (2, n, True)), sparse=(node, single, 'sparse', None))
    return _ROADS[kind]


@pytest.mark.parametrize('kind', ['dense_n', 'big', 'mid', 'sparse'])
def test_one_forward_and_backward_per_road(dev, kind):
    """the paths one GNNML3 step records are exactly those its two road records name"""
    from gnn_matlang_amd import dense_block as DB, functional as Fn
    m, data, _road, shape = _road_case(kind, dev)
    assert m._road_of(data, _road) == (kind, kind == 'sparse')
    old, Fn.VERBOSE = Fn.VERBOSE, True
    Fn.PATHS.clear()
    try:
        m.zero_grad(set_to_none=True)
        out = m(data, _road=_road)
        out.sum().backward()
        paths = set(Fn.PATHS)
    finally:
        Fn.VERBOSE = old
        Fn.PATHS.clear()
    assert torch.isfinite(out).all() and all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    dense = {k for k in paths if k.startswith('dense: ')}
    csr = {k for k in paths if k.startswith('conv_fwd') or k.startswith('conv_bwd')}
    if kind == 'sparse':
        assert csr and not dense, paths
        return
    want = set()
    for i in range(m.nlayers):
        layer = getattr(m, 'conv%d' % (i + 1))
        S, Fin, Fout = layer.conv1.weight.shape
        r = DB.dense_road(shape[0], shape[1], Fin, Fout, shape[2], False)
        assert r.product == {'dense_n': 'small', 'big': 'big', 'mid': 'mid'}[kind] and r.chained == (kind == 'dense_n')
        if r.chained:
            names, widths = ('support product + projection chained (bf16x3 HIP)', 'projection + support product chained, backward (bf16x3 HIP)'), (Fin, Fout)
        else:
            names, widths = ('support product fwd (bf16x3 HIP%s)' % r.label, 'support product bwd (bf16x3 HIP%s)' % r.label), (Fin, Fin)
        for name in names[:2 if i else 1]:                           # (the first layer's input needs no gradient)
            want.add('dense: %s (S=%s Fin=%s Fout=%s)' % ((name, S) + widths))
        if layer.nout2:
            want.add('dense: Hadamard half (library GEMMs + tanh) (S=- Fin=%s Fout=%s)' % (Fin, layer.nout2))
    assert dense == want and not csr, (sorted(dense), sorted(want), sorted(csr))
