"""Off-policy evaluation on the host loop (recogym_amd.evaluate_agent): equal, bit for bit, to the reference's own
evaluate_SNIPS / evaluate_IPS / evaluate_recall_at_k (tests/golden/ope_*.npz, tests/make_golden_ope.py), and the reference's
quirks: the highest user is not evaluated, rows are taken in frame order, an agent without `ps-a` gives an empty IPS list and
fails SNIPS.  No device needed."""
import json
import sys

import numpy as np
import pandas as pd
import pytest

import golden_util as gu
from make_golden_ope import LOGS, OUC_VARIANTS, log_frame
from recogym_amd import evaluate_agent as ev
from recogym_amd.agents import LastViewTableAgent, OrganicUserEventCounterAgent, RandomAgent
from recogym_amd.envs.configuration import Configuration


def ours(key, P, cols):
    if key == 'random':
        return RandomAgent(Configuration({'num_products': P, 'random_seed': 5, 'with_ps_all': True}))
    if key == 'random_nopsall':
        return RandomAgent(Configuration({'num_products': P, 'random_seed': 5, 'with_ps_all': False}))
    if key == 'bmf':
        return LastViewTableAgent.from_bandit_mf(Configuration({'num_products': P, 'with_ps_all': True}),
                                                 cols['bmf_product_embedding'], cols['bmf_user_embedding'])
    v = OUC_VARIANTS[int(key[3:])]
    return OrganicUserEventCounterAgent(Configuration({'num_products': P, 'random_seed': 11, 'weight_history_function': None,
                                                      'with_ps_all': True, **v}))


def cases():
    out = []
    for name in LOGS:
        z = np.load(f'{gu.GOLDEN}/ope_{name}.npz')
        meta = json.loads(str(z['meta']))
        out += [(name, k) for k in meta['agents']]
    return out


@pytest.mark.parametrize('name,key', cases())
def test_host_loop_equals_reference_fixture(name, key):
    meta, cols = gu.load(name)
    P = meta['env_args']['num_products']
    want = np.load(f'{gu.GOLDEN}/ope_{name}.npz')
    df = log_frame(cols)
    rewards, ratio = ev._host_snips(ours(key, P, cols), df)
    got = np.asarray(ratio, dtype=np.float64)
    assert got.shape == want[f'{key}__ratio'].shape
    assert np.array_equal(got.view(np.uint64), want[f'{key}__ratio'].view(np.uint64)), key
    assert np.array_equal(np.asarray(rewards, dtype=np.float64), want[f'{key}__c'])
    ips = np.asarray(ev._host_ips(ours(key, P, cols), df), dtype=np.float64)
    assert np.array_equal(ips.view(np.uint64), (want[f'{key}__c'] * want[f'{key}__ratio']).view(np.uint64))
    hits = ev.evaluate_recall_at_k(ours(key, P, cols), df, k=5)
    assert np.array_equal(np.asarray(hits, dtype=np.int8), want[f'{key}__recall'])


@pytest.mark.parametrize('name', LOGS)
def test_agent_without_ps_all_gives_empty_ips_and_fails_snips(name):
    meta, cols = gu.load(name)
    P = meta['env_args']['num_products']
    df = log_frame(cols)
    want = np.load(f'{gu.GOLDEN}/ope_{name}.npz')['random_nopsall__ips']
    assert want.size == 0
    assert ev.evaluate_IPS(ours('random_nopsall', P, cols), df) == []
    with pytest.raises(IndexError):
        ev.evaluate_SNIPS(ours('random_nopsall', P, cols), df)


def _tiny():
    # user 0: o(1) b(a=1, c=1) o(2) b(a=2);  user 1: o(3) b(a=3, c=1);  user 2 (the highest id): o(0) b(a=0, c=1)
    rows = [(0, 0, 'organic', 1, None, np.nan), (0, 1, 'bandit', None, 1, 1.0), (1, 0, 'organic', 3, None, np.nan),
            (0, 2, 'organic', 2, None, np.nan), (1, 1, 'bandit', None, 3, 1.0), (0, 3, 'bandit', None, 2, 0.0),
            (2, 0, 'organic', 0, None, np.nan), (2, 1, 'bandit', None, 0, 1.0)]
    return pd.DataFrame({'t': np.array([r[1] for r in rows], dtype=np.float32), 'u': [r[0] for r in rows],
                         'z': [r[2] for r in rows], 'v': pd.array([r[3] for r in rows], dtype=pd.UInt16Dtype()),
                         'a': pd.array([r[4] for r in rows], dtype=pd.UInt16Dtype()),
                         'c': np.array([r[5] for r in rows], dtype=np.float32),
                         'ps': np.where([r[2] == 'bandit' for r in rows], 0.25, np.nan)})


def test_highest_user_excluded_and_frame_order_kept():
    df = _tiny()
    ag = OrganicUserEventCounterAgent(Configuration({'num_products': 4, 'random_seed': 1, 'select_randomly': True,
                                                    'epsilon': 0.0, 'exploit_explore': True, 'reverse_pop': False,
                                                    'weight_history_function': None, 'with_ps_all': True}))
    rewards, ratio = ev._host_snips(ag, df)
    # user 0 (rows interleaved with user 1's: taken in frame order), then user 1; user 2 is not evaluated
    assert [float(x) for x in rewards] == [1.0, 0.0, 1.0]
    assert ratio == [4.0, 2.0, 4.0]          # counts {1}, {1, 2}, {3}: pi = 1, 1/2, 1 over ps = 1/4


def test_verify_agents_ips_resolves():
    import recogym_amd
    assert recogym_amd.verify_agents_IPS is ev.verify_agents_IPS
    for name in ('evaluate_IPS', 'evaluate_SNIPS', 'verify_agents_SNIPS', 'evaluate_recall_at_k', 'verify_agents_recall_at_k'):
        assert getattr(recogym_amd, name) is getattr(ev, name)


def test_verify_agents_ips_formula():
    df = _tiny()
    ag = RandomAgent(Configuration({'num_products': 4, 'random_seed': 1, 'with_ps_all': True}))
    ee = np.asarray(ev._host_ips(ag, df))
    res = ev.verify_agents_IPS(df, {'r': ag})
    se = np.std(ee) / np.sqrt(len(ee))
    assert list(res.columns) == ['Agent', '0.025', '0.500', '0.975']
    assert res['0.500'][0] == np.mean(ee)
    assert res['0.025'][0] == np.mean(ee) - 2 * se and res['0.975'][0] == np.mean(ee) + 2 * se


_REF_ROOTS = ('gym', 'numba', 'recogym')


@pytest.fixture
def reference(monkeypatch):
    """The reference package imported against tests/ref_shims, isolated from the rest of the session: a `gym` another test
    left in sys.modules (a stand-in without `spaces`) must not shadow the shims, and the modules imported here are dropped
    again afterwards (monkeypatch then restores sys.path and whatever was cached before)."""
    import ref_harness as rh
    if not rh.reference_available():
        pytest.skip('reference package not present')
    for k in [k for k in sys.modules if k.split('.')[0] in _REF_ROOTS]:
        monkeypatch.delitem(sys.modules, k)
    monkeypatch.syspath_prepend(rh.SHIMS)
    try:
        yield rh.import_reference()
    finally:
        for k in [k for k in sys.modules if k.split('.')[0] in _REF_ROOTS]:
            sys.modules.pop(k, None)


def test_live_reference_with_mt_agents(reference):
    """Where the reference package is present: its evaluate_SNIPS with its own (MT19937) agents on a fixture log equals this
    package's host loop given the same reference agent objects (the loop calls their act in the reference's order)."""
    import importlib
    ref_ev = importlib.import_module('recogym.evaluate_agent')
    from recogym import Configuration as RConf
    from recogym.agents import OrganicUserEventCounterAgent as ROuc, organic_user_count_args
    meta, cols = gu.load('philox_ouc_eps')
    df = log_frame(cols)
    args = {**organic_user_count_args, 'num_products': meta['env_args']['num_products'], 'random_seed': 3,
            'epsilon': 0.1, 'with_ps_all': True}
    want = ref_ev.evaluate_SNIPS(ROuc(RConf(args)), df)
    got = ev._host_snips(ROuc(RConf(args)), df)
    assert np.array_equal(np.asarray(got[1]).view(np.uint64), np.asarray(want[1], dtype=np.float64).view(np.uint64))
    assert np.array_equal(np.asarray(got[0]), np.asarray(want[0]))
