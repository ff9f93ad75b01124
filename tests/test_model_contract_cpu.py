"""The parameter contract of every model factory: the ORDERED (state_dict key, shape) list and the ORDERED named_parameters list of
tests/golden/model_contract.json.  Order and not sets: the reference's checkpoints load by key, optimiser state and flat gradient
buffers follow the parameter order, and torch.manual_seed(s) gives the reference's weights only in its creation order."""
import inspect
import json
import os

import pytest

from gnn_matlang_amd import models

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'model_contract.json')) as f:
    CONTRACT = json.load(f)


def test_the_fixture_names_every_factory():
    names = sorted(n for n, f in vars(models).items()
                   if inspect.isfunction(f) and f.__module__ == models.__name__ and n.rsplit('_', 1)[-1] in ('gnnml1', 'gnnml3', 'gat', 'ppgn'))
    assert names == sorted(CONTRACT)


@pytest.mark.parametrize('name', sorted(CONTRACT))
def test_state_dict_and_parameter_order(name):
    m = getattr(models, name)()
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == CONTRACT[name]['state']
    assert [k for k, _ in m.named_parameters()] == CONTRACT[name]['params']
