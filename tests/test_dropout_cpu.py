"""CPU side of device dropout and the TU GNNML3 models: the Philox4x32-10 restatement against its known answers, the keep rule,
load_tu on the PTC and ENZYMES fixtures, the state_dict key sets of the three TU factories and the NLL loss."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import _philox


def test_philox_known_answers():
    """The two known-answer vectors of Philox4x32-10: counter 0 / key 0, and every counter and key word 0xffffffff."""
    got = [int(v) for v in _philox.philox4x32_10(0, 0, 0, 0, 0, 0)]
    assert got == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8], ['%08x' % v for v in got]
    f = 0xffffffff
    got = [int(v) for v in _philox.philox4x32_10(f, f, f, f, f, f)]
    assert got == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd], ['%08x' % v for v in got]


def test_draws_follow_the_counter_layout():
    """element e draws word e & 3 of the block of counter (e >> 2 lo, e >> 2 hi, site, counter lo) keyed by (seed lo, seed hi)"""
    seed, ctr, site = 0x123456789abcdef0, 7, 3
    d = _philox.draws(4 * 5 + 3, seed, ctr, site)
    for e in (0, 1, 2, 3, 4, 17, 22):
        blk = _philox.philox4x32_10(e >> 2, 0, site, ctr, seed & 0xffffffff, seed >> 32)
        assert int(d[e]) == int(blk[e & 3])


def test_keep_rule_edge_cases():
    from gnn_matlang_amd.functional import dropout_threshold
    assert dropout_threshold(0.0) == (0, 1.0)                        # u >= 0: everything kept
    t, s = dropout_threshold(1.0)
    assert t == 1 << 32 and s == 0.0                                  # no uint32 draw reaches 2^32: nothing kept
    assert dropout_threshold(0.1)[0] == 429496729
    assert dropout_threshold(0.2)[0] == 858993459
    assert dropout_threshold(0.5)[0] == 1 << 31
    for p in (0.1, 0.2, 0.5):
        assert dropout_threshold(p)[0] == _philox.threshold(p)
        assert np.float32(dropout_threshold(p)[1]) == _philox.scale(p)
    assert _philox.keep_mask(3, 5, 0.0, 1, 2, 3).all()
    assert not _philox.keep_mask(3, 5, 1.0, 1, 2, 3).any()
    for p in (-0.1, 1.5, float('nan')):
        with pytest.raises(ValueError):
            dropout_threshold(p)


def test_dropout_argument_checks_without_a_device():
    """eval / p = 0: the input object itself, nothing launched (so no device needed); p outside [0, 1] raises in eval too"""
    from gnn_matlang_amd import functional as Fn
    x = torch.randn(4, 3)
    assert Fn.dropout(x, 0.3, False, None) is x
    assert Fn.dropout(x, 0.0, True, None) is x
    with pytest.raises(ValueError):
        Fn.dropout(x, 1.2, False, None)
    st = Fn.dropout_state(-1, 'cpu')
    assert st.dtype == torch.int64 and st.tolist() == [-1, 0]
    assert Fn.dropout_state(2 ** 64 - 1, 'cpu').tolist() == [-1, 0]


def test_pack_layout():
    keep = np.zeros(70, dtype=bool)
    keep[[0, 31, 32, 69]] = True
    w = _philox.pack(keep)
    assert w.tolist() == [0x80000001, 0x1, 0x20]


@pytest.mark.parametrize('name,count,nmin,nmax,width,labels', [
    ('ptc', 344, 2, 109, 19, {0, 1}),
    ('enzymes', 600, 2, 126, 3, {0, 1, 2, 3, 4, 5}),
])
def test_load_tu_fixtures(name, count, nmin, nmax, width, labels):
    from gnn_matlang_amd import readers
    g = readers.load_tu(os.path.join(GOLDEN, 'raw', '%s.mat' % name), name)
    assert len(g) == count
    ns = [x.shape[0] for x, _, _ in g]
    assert (min(ns), max(ns)) == (nmin, nmax)
    assert {x.shape[1] for x, _, _ in g} == {width}
    assert {int(y) for _, _, y in g} == labels
    for x, ei, y in g[:20]:
        assert x.dtype == np.float32 and ei.dtype == np.int64 and ei.shape[0] == 2
        assert ei.size == 0 or (ei.min() >= 0 and ei.max() < x.shape[0])
        assert np.all(np.diff(ei[0]) >= 0)                            # row-major np.where order
    with pytest.raises(ValueError):
        readers.load_tu(os.path.join(GOLDEN, 'raw', 'ptc.mat'), 'mutag')


def test_tu_design_widths_match_the_factory_defaults():
    """SpectralDesign with ptc.py:16 / enzymes.py:27 settings: x / edge_attr2 widths 20 / 11 and 4 / 5 (the factories' defaults)"""
    from gnn_matlang_amd import SpectralDesign, readers
    for name, kw, want in (('ptc', dict(nmax=109, adddegree=True, recfield=1, dv=10, nfreq=10), (20, 11)),
                           ('enzymes', dict(nmax=126, adddegree=True, recfield=1, dv=2, nfreq=4), (4, 5))):
        g = readers.load_tu(os.path.join(GOLDEN, 'raw', '%s.mat' % name), name)[:4]
        d = SpectralDesign(**kw).design_many(g)
        assert (d[0]['x'].shape[1], d[0]['edge_attr2'].shape[1]) == want


def _layer_keys(prefix, **kw):
    from gnn_matlang_amd import ML3Layer
    return {prefix + k for k in ML3Layer(**kw).state_dict()}


@pytest.mark.parametrize('ctor', ['ptc_gnnml3', 'enzymes_gnnml3', 'proteins_gnnml3'])
def test_tu_factories_have_the_reference_state_dict_keys(ctor):
    """ptc.py:323-363, enzymes.py:345-386, proteins.py:259-289: the key set, the shapes of the head, and a strict load of a
    state_dict without the (non-persistent) RNG state"""
    from gnn_matlang_amd import models
    ninp, ne, nl, le, n1, n2, top = dict(
        ptc_gnnml3=(20, 11, 4, True, 64, 16, {'fc1.weight': (100, 160), 'fc1.bias': (100,), 'fc2.weight': (2, 100), 'fc2.bias': (2,)}),
        enzymes_gnnml3=(4, 5, 4, False, 64, 0, {'bn4.weight': (128,), 'bn4.bias': (128,), 'bn4.running_mean': (128,),
                                                 'bn4.running_var': (128,), 'bn4.num_batches_tracked': (),
                                                 'fc2.weight': (6, 128), 'fc2.bias': (6,)}),
        proteins_gnnml3=(4, 4, 2, False, 64, 0, {'fc2.weight': (2, 128), 'fc2.bias': (2,)}))[ctor]
    want = set(top)
    fin = ninp
    for i in range(nl):
        want |= _layer_keys('conv%d.' % (i + 1), learnedge=le, nedgeinput=ne, nedgeoutput=ne, ninp=fin, nout1=n1, nout2=n2)
        fin = n1 + n2
    m = getattr(models, ctor)()
    sd = m.state_dict()
    assert set(sd) == want
    for k, shape in top.items():
        assert tuple(sd[k].shape) == shape, k
    assert m.dropout == {'ptc_gnnml3': 0.2, 'enzymes_gnnml3': 0.1, 'proteins_gnnml3': 0.1}[ctor]
    assert 'dropout_state' in dict(m.named_buffers())
    m2 = getattr(models, ctor)()
    m2.load_state_dict(sd, strict=True)


def test_dropout_seed_comes_from_torch_and_leaves_parameter_init_alone():
    from gnn_matlang_amd import models
    torch.manual_seed(3)
    a = models.ptc_gnnml3()
    torch.manual_seed(3)
    b = models.ptc_gnnml3()
    torch.manual_seed(3)
    c = models.ptc_gnnml3(dropout=0.0)
    torch.manual_seed(4)
    d = models.ptc_gnnml3()
    assert torch.equal(a.dropout_state, b.dropout_state) and int(a.dropout_state[1]) == 0
    assert not torch.equal(a.dropout_state, d.dropout_state)
    assert 'dropout_state' not in dict(c.named_buffers())
    for k, v in a.state_dict().items():
        assert torch.equal(v, c.state_dict()[k]), k
    assert models.mnist75_gnnml1().dropout == 0.0 and models.zinc_gnnml3().dropout == 0.0
    assert models.mnist75_gnnml1(dropout=0.1).dropout == 0.1
    with pytest.raises(ValueError):
        models.proteins_gnnml3(dropout=1.5)


def test_tu_loss_is_nll_sum_with_padding_masked():
    import torch.nn.functional as F
    from gnn_matlang_amd import models
    torch.manual_seed(0)
    pre = F.log_softmax(torch.randn(5, 3, dtype=torch.float64), 1)
    y = torch.tensor([2., 0., 1., 1., 7.], dtype=torch.float64)        # row 4: a padding graph's row
    assert torch.equal(models.tu_loss(pre[:4], y[:4]), F.nll_loss(pre[:4], y[:4].long(), reduction='sum'))
    valid = torch.tensor([1., 0., 1., 1.], dtype=torch.float64)
    want = F.nll_loss(pre[[0, 2, 3]], y[[0, 2, 3]].long(), reduction='sum')
    assert torch.allclose(models.tu_loss(pre, y, valid), want, rtol=0, atol=1e-15)
