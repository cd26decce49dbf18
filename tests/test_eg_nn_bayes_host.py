"""EpsilonGreedy round NnIpsAgent (argmax form) and BayesianAgentVB, on the host: every act of every fixture of the reference's own
wrapper round its own agents (tests/golden/nn_eg_*.npz, bayes_eg_*.npz, tests/make_golden_eg_nn_bayes.py) — action, `greedy`, `h0`,
the float64 `ps` bits —, where the wrapper offers its device forms (the opt-in keys `device_models` on the wrapper, `device_replay`
on the inner agent), the host loop of the estimators against the reference's ratios, and the additive entry point of the ABI.
No device needed."""
import os
import re

import numpy as np
import pytest

import eg_nn_bayes_util as xu
import eg_util as eu
import golden_util as gu
from make_golden_ope import log_frame
from recogym_amd import _abi
from recogym_amd import evaluate_agent as ev
from recogym_amd.envs.reco_env_v1 import device_policy_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND = {'nn': _abi.RG_POLICY_NN_IPS, 'bayes': _abi.RG_POLICY_BAYES_VB}
MODEL = {'nn': 'nn_ips', 'bayes': 'bayes_vb'}


def test_fixture_set_covers_the_cases():
    metas = {n: xu.load(n)[0] for n in xu.LOG_FIXTURES}
    nn = [m for m in metas.values() if m['inner'] == 'nn']
    bayes = [m for m in metas.values() if m['inner'] == 'bayes']
    assert len(nn) == 4 and len(bayes) == 3
    for group in (nn, bayes):
        assert {m['eg_args']['epsilon_pure_new'] for m in group} == {True, False}
        assert all(m['census']['explored'] > 0 and m['census']['greedy'] > 0 for m in group)
        assert all(10 * m['census']['unresolved'] <= m['census']['acts'] and 40 <= m['n_users'] <= 150 for m in group)
        assert any(m['longest_user'] > 64 and m['env_args']['prob_leave_bandit'] == 0.01 for m in group)
    assert any(m['env_args']['sigma_omega'] == 0.0 for m in nn) and any(m['env_args']['num_products'] == 40 for m in nn)
    assert all(2 * m['census']['distinct_greedy_actions'] >= m['env_args']['num_products'] for m in nn)
    assert any(m['census']['unresolved'] > 0 for m in nn)             # the confirm protocol runs on a reference log
    assert {m['env_args']['num_products'] for m in bayes} == {4, 10}
    assert xu.model_of(*xu.load('bayes_eg_p10_s120')[:2]).shape == (120, 100)
    # bandit rows that share one act cross a 64-row chunk of the replay: rows 63 and 64 of a user are both bandit rows
    for name in ('nn_eg_p10', 'bayes_eg_p4'):
        u, z = (xu.load(name)[1][k] for k in ('u', 'z'))
        start = np.flatnonzero(np.r_[True, u[1:] != u[:-1]])
        assert any(s + 64 < len(u) and u[s + 64] == u[s] and z[s + 63] == 1 and z[s + 64] == 1 for s in start), name


# ---- the routes --------------------------------------------------------------------------------------------------------------
def hooks(agent):
    return agent.device_policy(), agent.ope_policy(), agent.ope_policy_checked()


@pytest.mark.parametrize('name', ['nn_eg_p10', 'bayes_eg_p4', 'bayes_eg_p10_s120_not_pure_new'])
def test_routes(name):
    meta, cols, P = xu.load(name)
    kind = meta['inner']
    overlay = dict(epsilon=0.3, seed=7, pure_new=meta['eg_args']['epsilon_pure_new'])
    for all_ in (False, True):
        # without the key: the host, as before
        assert hooks(xu.wrapper(meta, cols, P, all_, device_models=None)) == (None, None, None)
        assert hooks(xu.wrapper(meta, cols, P, all_, device_models=False)) == (None, None, None)
    # the step loop: the inner dict plus epsilon_greedy=
    logger = xu.wrapper(meta, cols, P)
    pol, ope, checked = hooks(logger)
    inner_pol = xu.inner_agent(meta, cols, P).device_policy()
    assert ope is None and checked is None
    assert pol['policy'] == KIND[kind] == inner_pol['policy']
    assert pol['epsilon_greedy'] == overlay and set(pol) == set(inner_pol) | {'epsilon_greedy'}
    if kind == 'nn':
        assert all(np.array_equal(pol['nn_ips']['state'][k], inner_pol['nn_ips']['state'][k]) for k in inner_pol['nn_ips']['state'])
    else:
        assert np.array_equal(pol['bayes_vb']['lam'], inner_pol['bayes_vb']['lam'])
    assert device_policy_of(logger) is not None
    # the replay: with_ps_all on the wrapper and the inner agent, and the inner agent's own key `device_replay`
    target = xu.wrapper(meta, cols, P, with_ps_all=True)
    pol, ope, checked = hooks(target)
    inner_checked = xu.inner_agent(meta, cols, P, True).ope_policy_checked()
    assert pol is None and ope is None
    assert checked['kind'] == KIND[kind] and checked['epsilon_greedy'] == overlay and set(checked) == set(inner_checked) | {'epsilon_greedy'}
    assert checked['num_products'] == P and MODEL[kind] in checked
    assert ev.ope_policy_of(target) is None and ev.ope_checked_policy_of(target)['epsilon_greedy'] == overlay
    assert ev._replay_policy_of(target)['epsilon_greedy'] == overlay
    # ... without `device_replay` on the inner agent its own hook is None, and so is the wrapper's
    no_replay = xu.inner_agent(meta, cols, P, True, device_replay=False)
    assert no_replay.ope_policy_checked() is None
    assert hooks(xu.wrap(no_replay, P, meta['eg_args'], with_ps_all=True)) == (None, None, None)
    # with_ps_all on one of the two only: no form at all
    assert hooks(xu.wrap(xu.inner_agent(meta, cols, P, False), P, meta['eg_args'], with_ps_all=True)) == (None, None, None)
    assert hooks(xu.wrap(xu.inner_agent(meta, cols, P, True), P, meta['eg_args'], with_ps_all=False)) == (None, None, None)
    # the listed refusals
    for all_ in (False, True):
        assert hooks(xu.wrapper(meta, cols, P, all_, epsilon_select_worse=True)) == (None, None, None)
        nested = xu.wrap(xu.wrapper(meta, cols, P, all_), P, meta['eg_args'], all_)
        assert hooks(nested) == (None, None, None)
        weighted = xu.inner_agent(meta, cols, P, all_, weight_history_function=lambda t: np.exp(-0.1 * t))
        assert (weighted.device_policy(), weighted.ope_policy_checked()) == (None, None)
        assert hooks(xu.wrap(weighted, P, meta['eg_args'], all_)) == (None, None, None)


def test_routes_refuse_a_sampling_net_one_product_with_pure_new_and_models_beyond_the_caps():
    from recogym_amd.agents.bayesian_poly_vb import MODEL_BYTES_CAP, BayesianVBFrozenAgent
    from recogym_amd.agents.nn_ips import HIDDEN_CAP, NnIpsFrozenAgent
    from recogym_amd.envs.configuration import Configuration
    from ope_models_util import nn_state
    EG = dict(epsilon=0.3, random_seed=7)
    for all_ in (False, True):
        extra = {'with_ps_all': all_, 'device_replay': True}
        # select_randomly: the act is sampled and its `ps-a` is torch's fp32 softmax — out of scope, host path
        sampling = NnIpsFrozenAgent(Configuration({'num_products': 6, 'select_randomly': True, 'random_seed': 3, **extra}), nn_state(6, 5, 1))
        assert hooks(xu.wrap(sampling, 6, EG, all_)) == (None, None, None)
        # one product: nothing to explore with pure_new
        one_nn = NnIpsFrozenAgent(Configuration({'num_products': 1, **extra}), nn_state(1, 5, 1))
        one_bayes = BayesianVBFrozenAgent(Configuration({'num_products': 1, **extra}), np.zeros((3, 1)))
        for one in (one_nn, one_bayes):
            assert hooks(xu.wrap(one, 1, EG, all_)) == (None, None, None)
            assert any(h is not None for h in hooks(xu.wrap(one, 1, dict(EG, epsilon_pure_new=False), all_)))
        # beyond the kernels' caps, and a model that is not finite: the inner hooks are None
        wide = NnIpsFrozenAgent(Configuration({'num_products': 4, **extra}), nn_state(4, HIDDEN_CAP + 1, 1))
        state = nn_state(4, 5, 1)
        state['w2'][0, 0] = np.inf
        bad = NnIpsFrozenAgent(Configuration({'num_products': 4, **extra}), state)
        big = BayesianVBFrozenAgent(Configuration({'num_products': 16, **extra}), np.zeros((MODEL_BYTES_CAP // (8 * 256) + 1, 256)))
        nan = BayesianVBFrozenAgent(Configuration({'num_products': 2, **extra}), np.full((3, 4), np.nan))
        for inner in (wide, bad, big, nan):
            assert (inner.device_policy(), inner.ope_policy_checked()) == (None, None)
            assert hooks(xu.wrap(inner, int(inner.config.num_products), EG, all_)) == (None, None, None)


def test_a_reference_agent_object_inside_stays_on_the_host_loop():
    """ope_policy_checked looks at the inner object's package: an agent of another package is never replayed on the device."""
    meta, cols, P = xu.load('bayes_eg_p4')
    inner = xu.inner_agent(meta, cols, P, True)
    foreign = type('BayesianVBFrozenAgent', (type(inner),), {'__module__': 'recogym.agents.bayesian_poly_vb'})
    other = foreign(inner.config, xu.model_of(meta, cols))
    assert other.ope_policy_checked() is not None
    assert xu.wrap(other, P, meta['eg_args'], with_ps_all=True).ope_policy_checked() is None
    assert xu.wrap(inner, P, meta['eg_args'], with_ps_all=True).ope_policy_checked() is not None


# ---- the host act ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('device_models', [None, True])
@pytest.mark.parametrize('name', xu.LOG_FIXTURES)
def test_act_equals_the_reference_on_every_fixture_row(name, device_models):
    meta, cols, P = xu.load(name)
    acts = eu.host_acts(xu.wrapper(meta, cols, P, device_models=device_models), cols)
    is_b = cols['z'] == 1
    assert len(acts) == int(is_b.sum())
    assert np.array_equal(np.array([int(x['a']) for x in acts]), cols['a'][is_b])
    assert np.array_equal(np.array([x['greedy'] for x in acts], dtype=np.int8), cols['greedy'][is_b])
    assert np.array_equal(np.array([x.get('h0', -1) for x in acts]), cols['h0'][is_b])
    got, want, greedy = np.array([x['ps'] for x in acts]), cols['ps'][is_b], cols['greedy'][is_b] == 1
    # explored rows: epsilon * (1 / n), bit for bit; greedy rows: (1 - epsilon) * the inner ps — 1.0 for BayesianAgentVB, and for
    # NnIpsAgent torch's fp32 prob[a] on the host, the same forward the reference ran: the same bits too
    assert np.array_equal(eu.bits(got[~greedy]), eu.bits(want[~greedy])), 'ps bits on explored rows'
    assert np.array_equal(eu.bits(got[greedy]), eu.bits(want[greedy])), 'ps bits on greedy rows'
    if meta['inner'] == 'bayes':
        assert bool((want[greedy] == (1.0 - meta['eg_args']['epsilon']) * 1.0).all())
    for x in acts:
        assert ('h0' in x) == (not x['greedy']) and x['ps-a'] == ()


# ---- the run forms of the device file mean something (shown without a device) ------------------------------------------------
def test_the_repacked_cases_relabel_and_the_shards_are_ragged():
    """In every repacked case of the device file a user has stopped, and a user with a higher id still acts, when the state is
    repacked: from then on slot != user index, which is what the overlay's lr_ps load must not confuse.  The second shards start
    at id 37: user index != user id."""
    import test_agent_run_forms as rf
    import test_eg_nn_bayes_device as td
    for name, forms in td.FORMS.items():
        for form in forms:
            if form.startswith('repack'):
                print(name, form, rf.assert_repack_relabels(name, int(rf.FORM_ENV[form]['RECOGYM_REPACK'])))
    assert any(xu.load(n)[0]['inner'] == 'nn' and any(f.startswith('repack') for f in forms) for n, forms in td.FORMS.items())
    for name, form in td.SHARDS:
        meta, cols, P = xu.load(name)
        n = meta['n_users']
        assert 0 < rf.SPLIT < n and rf.SPLIT % 64 and (n - rf.SPLIT) % 64, (name, n)
        assert (cols['u'] < rf.SPLIT).any() and (cols['z'][cols['u'] >= rf.SPLIT] == 1).any()
        print(name, 'second shard', form, rf.assert_repack_relabels(name, int(rf.FORM_ENV[form]['RECOGYM_REPACK']), rf.SPLIT))


def test_the_two_product_models_act_on_the_view_count():
    import test_eg_nn_bayes_device as td
    nn, bayes = td.two_product_models()
    for prods, cnts in (([0], [1]), ([1], [2]), ([0, 1], [1, 1])):
        assert nn.act_on(prods, cnts)[0] == 0
    for prods, cnts in (([0], [3]), ([1], [7]), ([0, 1], [2, 1]), ([0, 1], [30, 30])):
        assert nn.act_on(prods, cnts)[0] == 1
    for prods, cnts in (([0], [1]), ([1], [4]), ([0, 1], [2, 2])):
        assert bayes.act_on(prods, cnts) == 1
    for prods, cnts in (([0], [5]), ([1], [9]), ([0, 1], [3, 2]), ([0, 1], [40, 40])):
        assert bayes.act_on(prods, cnts) == 0


# ---- the host estimators -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def frame():
    df = log_frame(gu.load('philox_p10')[1])
    return df[df['u'] <= 60]


@pytest.mark.parametrize('name', xu.OPE_FIXTURES)
def test_host_estimators_equal_the_reference(name, frame, monkeypatch):
    meta, want, P = xu.load(name)
    assert meta['log'] == 'philox_p10'
    monkeypatch.setattr(ev, '_device_present', lambda: False)
    target = xu.wrapper(meta, want, P, with_ps_all=True)
    c, ratio = ev.evaluate_SNIPS(target, frame)
    m = len(ratio)
    assert m > 1000 and np.array_equal(eu.bits(ratio), eu.bits(want['ratio'][:m]))
    assert np.array_equal(np.asarray(c, dtype=np.float64), want['c'][:m])
    assert np.array_equal(eu.bits(ev.evaluate_IPS(target, frame)), eu.bits(want['c'][:m] * want['ratio'][:m]))
    assert len(set(np.asarray(ratio).tolist())) > 2                 # explored and greedy rows, hits and misses


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
def declared_args(header, name):
    m = re.search(r'\b(?:int|size_t)\s+' + name + r'\s*\(([^;]*?)\)\s*;', header, flags=re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(',')]


def test_abi_declares_the_entry_point_and_the_version():
    header = open(os.path.join(ROOT, 'include', 'recogym_hip.h')).read()
    S = _abi.SYMBOLS
    assert int(re.search(r'#define RG_ABI_VERSION (\d+)', header).group(1)) == 15 == _abi.RG_ABI_VERSION
    new = 'rg_sim_set_epsilon_greedy_model_ps'
    assert new in S and S[new] == S['rg_sim_set_epsilon_greedy'] == S['rg_sim_set_epsilon_greedy_model']
    assert declared_args(header, new) == declared_args(header, 'rg_sim_set_epsilon_greedy')
    assert re.search(r'v14, additive since: ' + new, header)
