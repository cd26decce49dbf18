"""The replay form of the frozen LogReg policy, host side: which agents offer one (ope_policy), the ctypes mirror of
struct rg_ope_logreg against the header, and the host loop against the reference's own numbers
(tests/golden/ope_logreg_philox_p10.npz, tests/make_golden_ope_logreg.py).  No device needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import golden_util as gu
from make_golden_ope import log_frame
from recogym_amd import _abi
from recogym_amd import evaluate_agent as ev
from recogym_amd.agents import LogregMulticlassIpsAgent
from recogym_amd.agents.logreg_frozen import LogregFrozenAgent
from recogym_amd.envs.configuration import Configuration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def frozen(P, n_classes=None, classes=None, seed=0, **cfg):
    rng = np.random.RandomState(seed)
    classes = np.arange(P if n_classes is None else n_classes) if classes is None else np.asarray(classes)
    return LogregFrozenAgent(Configuration({'num_products': P, 'random_seed': 3, **cfg}), rng.randn(len(classes), P),
                             rng.randn(len(classes)), classes)


def test_ope_policy_is_a_dict_with_ps_all():
    for sr in (False, True):
        ag = frozen(12, with_ps_all=True, select_randomly=sr)
        pol = ag.ope_policy()
        assert pol['kind'] == _abi.RG_POLICY_LOGREG_FROZEN and pol['num_products'] == 12 and pol['policy_seed'] == 0
        lr = pol['logreg']
        assert lr['coef_t'] is ag.coef_t and lr['intercept'] is ag.intercept and lr['classes'] is ag.classes
        assert lr['select_randomly'] is sr
        assert ev.ope_policy_of(ag)['logreg']['coef_t'] is ag.coef_t
    # a strict subset of the products as classes: the argmax form replays (the other actions get 0)
    assert frozen(12, classes=[1, 4, 7], with_ps_all=True).ope_policy()['logreg']['classes'].tolist() == [1, 4, 7]


def test_ope_policy_is_none_where_only_the_host_loop_is_exact():
    assert frozen(12).ope_policy() is None                                          # no `ps-a` at all
    assert frozen(12, with_ps_all=False, select_randomly=True).ope_policy() is None
    assert frozen(12, with_ps_all=True, weight_history_function=gu.WEIGHT_FUNCS['inverse']).ope_policy() is None
    assert frozen(12, classes=[1, 4, 7], with_ps_all=True, select_randomly=True).ope_policy() is None
    assert frozen(12, classes=np.arange(12)[::-1], with_ps_all=True, select_randomly=True).ope_policy() is None
    assert frozen(1025, n_classes=1025, with_ps_all=True, select_randomly=True).ope_policy() is None
    assert frozen(1025, n_classes=1025, with_ps_all=True).ope_policy() is not None


def test_trained_agent_delegates_to_its_frozen_model():
    _, cols = gu.load('philox_p10')
    ag = LogregMulticlassIpsAgent(Configuration({'num_products': 10, 'random_seed': 7, 'select_randomly': False, 'max_iter': 200,
                                                 'solver': 'lbfgs', 'with_ps_all': True}))
    ag.train_from_log(log_frame(cols))
    pol = ev.ope_policy_of(ag)                       # builds the model
    assert ag.frozen is not None and pol is not None
    want = ag.frozen.ope_policy()
    assert pol['kind'] == want['kind'] == _abi.RG_POLICY_LOGREG_FROZEN and pol['num_products'] == 10
    for k in ('coef_t', 'intercept', 'classes'):
        assert pol['logreg'][k] is want['logreg'][k]
    assert pol['logreg']['select_randomly'] is False


def test_struct_layout_matches_header():
    header = open(os.path.join(ROOT, 'include', 'recogym_hip.h')).read()
    struct = header[header.index('typedef struct rg_ope_logreg {'):header.index('} rg_ope_logreg;')]
    fields = re.findall(r'^\s*(const\s+\w+\s*\*|uint32_t|float)\s*([a-zA-Z_0-9]+);', struct, flags=re.M)
    assert [n for _, n in fields] == [n for n, _ in _abi.RgOpeLogreg._fields_], fields
    size = {'uint32_t': 4, 'float': 4}
    want_sizes = [size.get(t, 8) for t, _ in fields]                               # (every other field is a pointer)
    assert [C.sizeof(t) for _, t in _abi.RgOpeLogreg._fields_] == want_sizes
    offs, at = [], 0
    for s in want_sizes:
        at = (at + s - 1) // s * s
        offs.append(at)
        at += s
    assert [getattr(_abi.RgOpeLogreg, n).offset for n, _ in _abi.RgOpeLogreg._fields_] == offs
    assert C.sizeof(_abi.RgOpeLogreg) == (at + 7) // 8 * 8 == 72
    for name in ('rg_ope_logreg_workspace_bytes', 'rg_ope_replay_logreg'):
        assert name in _abi.SYMBOLS and re.search(r'\b' + name + r'\s*\(', header)
    assert len(_abi.SYMBOLS['rg_ope_replay_logreg'][1]) == len(_abi.SYMBOLS['rg_ope_replay'][1]) == 14
    assert _abi.RG_ABI_VERSION == int(re.search(r'#define RG_ABI_VERSION (\d+)', header).group(1)) >= 10


@pytest.mark.parametrize('form', ['argmax', 'softmax'])
def test_host_loop_equals_reference_numbers(form):
    want = np.load(f'{gu.GOLDEN}/ope_logreg_philox_p10.npz')
    _, cols = gu.load('philox_p10')
    ag = LogregFrozenAgent(Configuration({'num_products': 10, 'random_seed': 7, 'with_ps_all': True,
                                          'select_randomly': form == 'softmax'}),
                           want['logreg_coef'], want['logreg_intercept'], want['logreg_classes'])
    rewards, ratio = ev._host_snips(ag, log_frame(cols))
    got = np.asarray(ratio, dtype=np.float64)
    assert got.shape == want[f'{form}__ratio'].shape and np.count_nonzero(got) > 0
    if form == 'argmax':
        assert np.array_equal(got.view(np.uint64), want[f'{form}__ratio'].view(np.uint64))
    else:       # sklearn's softmax sums in an order of its own: (C + 4) 2^-52 relative
        assert np.all(np.abs(got - want[f'{form}__ratio']) <= 1e-12 * np.abs(want[f'{form}__ratio']))
    assert np.array_equal(np.asarray(rewards, dtype=np.float64), want[f'{form}__c'])
