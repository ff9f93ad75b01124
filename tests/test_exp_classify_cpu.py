"""The EXP classification experiment (exp_classify.py), host side: the data split, the two models' state_dict layout against a
plain-torch restatement of the reference classes, the torch-op loss, the accuracy helper and the loud refusal of CPU tensors."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

RAW = os.path.join(GOLDEN, 'raw')


@pytest.fixture(scope='module')
def exp_raw():
    from gnn_matlang_amd import readers
    return readers.load_exp(os.path.join(RAW, 'exp.npz'))


def test_splits_follow_the_reference(exp_raw):
    """exp_classify.py:19-21: val = [0, 200), test = [200, 400), train = [400, 1200), file order kept, every split balanced, the
    two graphs of a pair carry different labels"""
    from gnn_matlang_amd import readers
    val, test, train = readers.exp_classify_splits(exp_raw)
    assert (len(val), len(test), len(train)) == (200, 200, 800)
    for part, lo in ((val, 0), (test, 200), (train, 400)):
        for k in (0, 1, len(part) // 2, len(part) - 1):
            assert part[k] is exp_raw[lo + k]
        y = np.array([int(g[2]) for g in part])
        assert set(y.tolist()) == {0, 1}
        assert int((y == 1).sum()) == len(part) // 2 and int((y == 0).sum()) == len(part) // 2
    y = np.array([int(g[2]) for g in exp_raw])
    assert (y[0::2] != y[1::2]).all()
    with pytest.raises(ValueError):
        readers.exp_classify_splits(exp_raw[:100])


class _RefGNNML3(torch.nn.Module):
    """exp_classify.py:264-281 with the oracle's layers (same attribute names, same shapes)"""

    def __init__(self, ninp=2, ne=6):
        super().__init__()
        from oracle.spect_conv_oracle import OracleML3Layer
        self.conv1 = OracleML3Layer(True, ne, ne, ninp, 32, 16)
        self.conv2 = OracleML3Layer(True, ne, ne, 48, 32, 16)
        self.conv3 = OracleML3Layer(True, ne, ne, 48, 32, 16)
        self.fc1 = torch.nn.Linear(48, 10)
        self.fc2 = torch.nn.Linear(10, 1)


class _RefGNNML1(torch.nn.Module):
    """exp_classify.py:209-241 (concat=False) with the oracle's SpectConv"""

    def __init__(self, ninp=2, nout=64):
        super().__init__()
        from oracle.spect_conv_oracle import OracleSpectConv
        for i, fin in ((1, ninp), (2, nout), (3, nout)):
            setattr(self, 'conv%d1' % i, OracleSpectConv(fin, nout, selfconn=False))
            for j in (1, 2, 3):
                setattr(self, 'fc%d%d' % (i, j), torch.nn.Linear(fin, nout))
        self.fc1 = torch.nn.Linear(nout, 10)
        self.fc2 = torch.nn.Linear(10, 1)


@pytest.mark.parametrize('factory,ref,nin', [('exp_classify_gnnml3', _RefGNNML3, 48), ('exp_classify_gnnml1', _RefGNNML1, 64)])
def test_state_dict_is_the_reference_layout(factory, ref, nin):
    from gnn_matlang_amd import models
    torch.manual_seed(0)
    m, r = getattr(models, factory)(), ref()
    sm, sr = m.state_dict(), r.state_dict()
    assert {k: tuple(v.shape) for k, v in sm.items()} == {k: tuple(v.shape) for k, v in sr.items()}
    assert tuple(sm['fc1.weight'].shape) == (10, nin) and tuple(sm['fc2.weight'].shape) == (1, 10)
    m.load_state_dict(sr, strict=True)
    assert all(torch.equal(m.state_dict()[k], sr[k]) for k in sr)
    r.load_state_dict({k: v + 1 for k, v in sm.items()}, strict=True)


def _ml3_keys(nlayers, learnedge, nout2, head):
    ks = []
    for i in range(1, nlayers + 1):
        ks += ['conv%d.conv1.weight' % i, 'conv%d.conv1.bias' % i]
        if learnedge:
            ks += ['conv%d.fc1_%d.weight' % (i, j) for j in (1, 2, 3, 4)]
        if nout2:
            ks += ['conv%d.%s.%s' % (i, f, w) for f in ('fc11', 'fc12') for w in ('weight', 'bias')]
    return set(ks + ['%s.%s' % (f, w) for f in head for w in ('weight', 'bias')])


def test_existing_constructors_keep_their_keys():
    from gnn_matlang_amd import models
    assert set(models.zinc_gnnml3().state_dict()) == _ml3_keys(4, True, 2, ('fc1', 'fc2'))
    assert set(models.sr25_gnnml3().state_dict()) == _ml3_keys(3, True, 16, ('fc1',))
    assert set(models.exp_gnnml3().state_dict()) == _ml3_keys(3, True, 16, ('fc1',))
    assert set(models.filtering_gnnml3().state_dict()) == _ml3_keys(3, False, 16, ('fc2',))
    ml1 = {'%s.%s' % (n, w) for i in (1, 2, 3) for n in ('conv%d1' % i, 'fc%d1' % i, 'fc%d2' % i, 'fc%d3' % i) for w in ('weight', 'bias')}
    assert set(models.sr25_gnnml1().state_dict()) == ml1 | {'fc1.weight', 'fc1.bias'}
    assert set(models.graph8c_gnnml1().state_dict()) == ml1 | {'fc1.weight', 'fc1.bias'}
    assert tuple(models.sr25_gnnml1().fc1.weight.shape) == (10, 64) and tuple(models.zinc_gnnml3().fc1.weight.shape) == (32, 32)
    with pytest.raises(ValueError):
        models.GNNML3(2, 6, 32, 16, 3, head='mlp')            # hidden > 0 is required


def test_loss_is_the_reference_formula():
    """exp_classify.py:328-329 on random logits in [-10, 10]; the valid form is the sum over the valid rows"""
    from gnn_matlang_amd import models
    g = torch.Generator().manual_seed(3)
    pre = (torch.rand(57, 1, generator=g) * 20 - 10).requires_grad_(True)
    y = (torch.rand(57, generator=g) < 0.5).long()
    ref = F.binary_cross_entropy(torch.sigmoid(pre), y.float().unsqueeze(-1), reduction='sum')
    got = models.exp_classify_loss(pre, y)
    assert torch.equal(got, ref)
    got.backward()
    assert torch.isfinite(pre.grad).all()
    valid = (torch.rand(50, generator=g) < 0.7).float()
    sel = valid.bool()
    part = F.binary_cross_entropy(torch.sigmoid(pre[:50][sel]), y[:50][sel].float().unsqueeze(-1), reduction='sum')
    gotv = models.exp_classify_loss(pre, y, valid)
    # (two float32 sums of <= 50 terms in different orders: <= 50 x 2^-24 = 3e-6 of the sum apart)
    assert abs(float(gotv.detach()) - float(part.detach())) <= 1e-5 * abs(float(part.detach()))


def test_accuracy_from_stats_on_list_array_and_tensor():
    from gnn_matlang_amd import models
    assert models.accuracy_from_stats([12.5, 30.0, 40.0]) == 0.75
    assert models.accuracy_from_stats(np.array([12.5, 30.0, 40.0])) == 0.75
    a = models.accuracy_from_stats(torch.tensor([12.5, 30.0, 40.0]))
    assert isinstance(a, torch.Tensor) and float(a) == 0.75


def test_cpu_tensors_are_refused():
    from gnn_matlang_amd import SpectralDesign, collate, functional as Fn, models, readers
    p, y = torch.randn(4, 48), torch.tensor([0., 1., 1., 0.])
    fc1, fc2 = torch.nn.Linear(48, 10), torch.nn.Linear(10, 1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        Fn.HeadBCEFunction.apply(p, y, None, fc1.weight, fc1.bias, fc2.weight, fc2.bias, 1, None)
    assert not Fn.head_bce_supported(p, fc1.weight, fc2.weight)
    gs = readers.load_exp(os.path.join(RAW, 'exp.npz'))[400:404]
    data = collate(SpectralDesign(nmax=64, recfield=1, dv=2, nfreq=5, adddegree=True).design_many(gs))
    assert data.x.size(1) == 2 and data.edge_attr2.size(1) == 6
    for m in (models.exp_classify_gnnml3(), models.exp_classify_gnnml1()):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            models.exp_classify_step_loss(m, data)
