"""The GNNML1 factories of models.py, all on the one class GNNML1Blocks (Zinc12k.py, counting.py, freqclass.py, ptc.py, enzymes.py,
proteins.py, mutag.py, sr25.py, graph8c.py, mnist75.py, exp_classify.py): their state_dict keys and shapes equal the reference
class's -- written out here from the scripts, modules that are declared and never called included -- so that the reference's
checkpoints load with strict=True; the seeded initialisation; the constructor's errors.  No GPU."""
import pytest
import torch


def _blocks(nblocks, ninp, n1, n2, n3, nin=None):
    """conv_i1 = SpectConv(fin, n2, K = 1, selfconn=False): weight [1, fin, n2], bias [n2]; fc_i1: fin -> n1; fc_i2, fc_i3: fin -> n3.
    nin: what every block after the first reads -- the concatenation n1 + n2 + n3 unless given (the sum form: nout)"""
    out, fin = {}, ninp
    for i in range(1, nblocks + 1):
        out['conv%d1.weight' % i] = (1, fin, n2)
        out['conv%d1.bias' % i] = (n2,)
        for j, n in ((1, n1), (2, n3), (3, n3)):
            out['fc%d%d.weight' % (i, j)] = (n, fin)
            out['fc%d%d.bias' % (i, j)] = (n,)
        fin = n1 + n2 + n3 if nin is None else nin
    return out


def _bns(count, width):
    out = {}
    for i in range(1, count + 1):
        out.update({'bn%d.weight' % i: (width,), 'bn%d.bias' % i: (width,), 'bn%d.running_mean' % i: (width,),
                    'bn%d.running_var' % i: (width,), 'bn%d.num_batches_tracked' % i: ()})
    return out


def _lin(name, nin, nout):
    return {name + '.weight': (nout, nin), name + '.bias': (nout,)}


def _merge(*ds):
    out = {}
    for d in ds:
        assert not set(out) & set(d)
        out.update(d)
    return out


EXPECTED = dict(
    zinc=_merge(_blocks(4, 25, 16, 16, 16), _lin('fc1', 48, 32), _lin('fc2', 32, 1)),                          # Zinc12k.py:261-284
    counting=_merge(_blocks(5, 2, 32, 32, 32), _lin('fc1', 96, 32), _lin('fc2', 32, 1)),                       # counting.py:281-308
    freqclass=_merge(_blocks(3, 1, 32, 32, 32), _lin('fc1', 96, 32), _lin('fc2', 32, 1)),                      # freqclass.py:248-267
    ptc=_merge(_blocks(2, 20, 32, 64, 2), _bns(4, 98), _lin('fc1', 196, 100), _lin('fc2', 100, 2)),            # ptc.py:283-301 (bn2 .. bn4 never called)
    enzymes=_merge(_blocks(4, 4, 16, 16, 16), _bns(4, 48), _lin('fc2', 96, 6)),                                # enzymes.py:289-316 (no fc1)
    proteins=_merge(_blocks(2, 4, 64, 64, 16), _bns(2, 144), _lin('fc2', 288, 2)),                             # proteins.py:218-238 (bn1, bn2 never called)
    mutag=_merge(_blocks(3, 8, 16, 32, 16), _bns(3, 64), _lin('fc1', 64, 32), _lin('fc2', 32, 1)),             # mutag.py:214-246
    sr25=_merge(_blocks(3, 2, 64, 64, 64, nin=64), _lin('fc1', 64, 10)),                                       # sr25.py:192-227 (sum form, no fc2)
    graph8c=_merge(_blocks(3, 2, 64, 64, 64, nin=64), _lin('fc1', 64, 10)),                                    # graph8c.py:205-238
    mnist75=_merge(_blocks(3, 3, 64, 64, 64, nin=64), _bns(1, 64), _lin('fc1', 64, 32), _lin('fc2', 32, 10)),  # mnist75.py:262-289 (bn1: the pooled rows)
    exp_classify=_merge(_blocks(3, 2, 64, 64, 64, nin=64), _lin('fc1', 64, 10), _lin('fc2', 10, 1)))           # exp_classify.py:209-241


def _factory(name):
    from gnn_matlang_amd import models
    return getattr(models, name + '_gnnml1')()


@pytest.mark.parametrize('name', sorted(EXPECTED))
def test_state_dict_keys_and_shapes_are_the_reference_classes(name):
    sd = _factory(name).state_dict()
    exp = EXPECTED[name]
    assert set(sd) == set(exp), (sorted(set(sd) - set(exp)), sorted(set(exp) - set(sd)))
    for k, shape in exp.items():
        assert tuple(sd[k].shape) == shape, (k, tuple(sd[k].shape), shape)


@pytest.mark.parametrize('name', sorted(EXPECTED))
def test_a_reference_checkpoint_loads_strictly(name):
    """a dict of random tensors under the reference's names and shapes loads with strict=True and is what the model then holds"""
    torch.manual_seed(0)
    ck = {k: (torch.tensor(7) if k.endswith('num_batches_tracked') else torch.randn(shape)) for k, shape in EXPECTED[name].items()}
    m = _factory(name)
    res = m.load_state_dict(ck, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    sd = m.state_dict()
    for k, v in ck.items():
        assert torch.equal(sd[k], v), k


@pytest.mark.parametrize('name', sorted(EXPECTED))
def test_parameter_counts(name):
    buffers = ('running_mean', 'running_var', 'num_batches_tracked')
    want = sum(int(torch.Size(shape).numel()) for k, shape in EXPECTED[name].items() if not k.endswith(buffers))
    assert sum(p.numel() for p in _factory(name).parameters()) == want


def test_exp_head_recognises_the_freqclass_head():
    from gnn_matlang_amd import models
    m = models.freqclass_gnnml1()
    assert models._exp_head(m) == (m.fc1, m.fc2, 1)                  # relu(fc1: 96 -> 32), fc2: 32 -> 1
    c = models.counting_gnnml1()
    assert models._exp_head(c) == (c.fc1, c.fc2, 0)                  # fc2(fc1 x), no activation
    assert models._exp_head(models.enzymes_gnnml1()) is None
    e = models.exp_classify_gnnml1()
    assert models._exp_head(e) == (e.fc1, e.fc2, 0)                  # exp_classify.py:240-241: fc2(fc1 x), fc1: 64 -> 10
    assert models._exp_head(models.sr25_gnnml1()) is None            # lin10: no fc2
    assert models._exp_head(models.mnist75_gnnml1()) is None         # bn_mlp: a BatchNorm and a log_softmax around the two linears


# (ninp, blocks, (n1, n2, n3), what later blocks read, the head's modules in creation order, factory arguments)
SEEDED = dict(
    mutag=(8, 3, (16, 32, 16), 64, (('fc1', 64, 32), ('fc2', 32, 1)), {}),
    sr25=(2, 3, (64, 64, 64), 64, (('fc1', 64, 10),), {}),
    mnist75=(3, 3, (64, 64, 64), 64, (('fc1', 64, 32), ('fc2', 32, 10)), dict(dropout=0.1)),
    exp_classify=(2, 3, (64, 64, 64), 64, (('fc1', 64, 10), ('fc2', 10, 1)), {}),
    zinc=(25, 4, (16, 16, 16), 48, (('fc1', 48, 32), ('fc2', 32, 1)), {}))


@pytest.mark.parametrize('name', sorted(SEEDED))
def test_seeded_initialisation_is_the_creation_order_of_the_scripts(name):
    """under one seed the factory holds what the same modules hold when created by hand in the order per block conv_i1, fc_i1, fc_i2,
    fc_i3, then the head (BatchNorms draw nothing; the dropout seed is drawn last): every parameter equal under its name"""
    from gnn_matlang_amd import models
    from gnn_matlang_amd.spect_conv import SpectConv
    ninp, nblocks, (n1, n2, n3), nin, head, kw = SEEDED[name]
    torch.manual_seed(0)
    hand, fin = torch.nn.Module(), ninp
    for i in range(1, nblocks + 1):
        setattr(hand, 'conv%d1' % i, SpectConv(fin, n2, 1, selfconn=False))
        setattr(hand, 'fc%d1' % i, torch.nn.Linear(fin, n1))
        setattr(hand, 'fc%d2' % i, torch.nn.Linear(fin, n3))
        setattr(hand, 'fc%d3' % i, torch.nn.Linear(fin, n3))
        fin = nin
    for n, a, b in head:
        setattr(hand, n, torch.nn.Linear(a, b))
    want = dict(hand.named_parameters())
    torch.manual_seed(0)
    m = getattr(models, name + '_gnnml1')(**kw)
    got = {k: v for k, v in m.named_parameters() if not k.startswith('bn')}
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    for k, v in m.named_parameters():
        if k.startswith('bn'):
            assert torch.equal(v, torch.ones_like(v) if k.endswith('weight') else torch.zeros_like(v)), k


def test_constructor_errors_and_modes():
    from gnn_matlang_amd.models import GNNML1Blocks
    assert GNNML1Blocks._MODES == dict(sum=0, product=1, factors=2, tanh_factors=3, sum_factors=4)
    for widths in ((16, 16, 8), (16, 8, 16), (8, 16, 16)):
        with pytest.raises(ValueError):
            GNNML1Blocks(4, widths, 2, form='sum')
    assert GNNML1Blocks(4, (16, 16, 16), 2, form='sum', head='lin10', nclass=10).fc21.in_features == 16
    with pytest.raises(ValueError):
        GNNML1Blocks(4, (16, 16, 16), 2, form='sum', head='bn_mlp', nbn=1)
    assert type(GNNML1Blocks(4, (16, 16, 16), 2, form='sum', head='bn_mlp', nclass=10).bn1) is torch.nn.BatchNorm1d   # (not models.BatchNorm1d)
    with pytest.raises(ValueError):
        GNNML1Blocks(4, (16, 16, 16), 2, form='concat')
    with pytest.raises(ValueError):
        GNNML1Blocks(4, (16, 16, 16), 2, head='tanh10')
    with pytest.raises(ValueError):
        GNNML1Blocks(4, (16, 16, 16), 2, head='lin2')
