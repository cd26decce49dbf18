"""EpsilonGreedy on the host against the reference's own class (tests/golden/eg_*.npz, written by tests/make_golden_eg.py from the
unmodified reference with the counter RNG injected): every act of every fixture — action, float64 `ps` bits, `greedy`, `h0` —
the delegation to the inner agent, where the wrapper has a device / replay form, and the host loop of evaluate_IPS against the
reference's ratios.  No device needed."""
import numpy as np
import pytest

import eg_util as eu
from make_golden_ope import log_frame
from recogym_amd import _abi
from recogym_amd import evaluate_agent as ev
from recogym_amd.agents import (BanditCount, EpsilonGreedy, LogregFrozenAgent, OrganicCount, OrganicUserEventCounterAgent, RandomAgent,
                                bandit_count_args, epsilon_greedy_args, organic_count_args, organic_user_count_args)
from recogym_amd.envs.configuration import Configuration
from recogym_amd.envs.context import DefaultContext
from recogym_amd.envs.observation import Observation
from recogym_amd.envs.session import OrganicSessions


def test_fixture_set_covers_the_cases():
    metas = {n: eu.load(n)[0] for n in eu.LOG_FIXTURES}
    eps = {m['eg_args']['epsilon'] for m in metas.values()}
    assert {0.0, 0.3, 1.0} <= eps
    assert {m['inner'] for m in metas.values()} == {'table', 'random', 'ouc'}
    assert {m['env_args']['num_products'] for m in metas.values()} == {2, 10, 1000}
    assert {m['eg_args']['epsilon_pure_new'] for m in metas.values()} == {True, False}
    assert {m['env_args']['sigma_omega'] == 0.0 for m in metas.values()} == {True, False}
    assert any(m['inner'] == 'random' and m['inner_args']['random_seed'] == m['eg_args']['random_seed'] for m in metas.values())
    assert any(m['inner'] == 'random' and m['inner_args']['random_seed'] != m['eg_args']['random_seed'] for m in metas.values())
    assert any(m['inner_args'].get('select_randomly') is False for m in metas.values())
    assert len(eu.OPE_FIXTURES) == 2


def test_argument_table_is_the_references():
    assert set(epsilon_greedy_args) == {'epsilon', 'random_seed', 'epsilon_pure_new', 'epsilon_select_worse', 'with_ps_all'}
    assert {k: v for k, v in epsilon_greedy_args.items() if k != 'random_seed'} == dict(
        epsilon=0.01, epsilon_pure_new=True, epsilon_select_worse=False, with_ps_all=False)
    import recogym_amd.agents as ag
    assert ag.EpsilonGreedy is EpsilonGreedy and ag.epsilon_greedy_args is epsilon_greedy_args


@pytest.mark.parametrize('name', eu.LOG_FIXTURES)
def test_act_equals_the_reference_on_every_fixture_row(name):
    meta, cols, P = eu.load(name)
    acts = eu.host_acts(eu.wrapper(meta, cols, P), cols)
    is_b = cols['z'] == 1
    assert len(acts) == int(is_b.sum())
    assert np.array_equal(np.array([int(x['a']) for x in acts]), cols['a'][is_b])
    assert np.array_equal(eu.bits([x['ps'] for x in acts]), eu.bits(cols['ps'][is_b])), 'ps bits'
    assert np.array_equal(np.array([x['greedy'] for x in acts], dtype=np.int8), cols['greedy'][is_b])
    assert np.array_equal(np.array([x.get('h0', -1) for x in acts]), cols['h0'][is_b])
    for x in acts:
        assert ('h0' in x) == (not x['greedy']) and x['ps-a'] == ()
        assert set(x) - {'h0'} == {'t', 'u', 'a', 'ps', 'ps-a', 'greedy'}
    assert np.array_equal(np.array([x['t'] for x in acts]), cols['t'][is_b])
    assert np.array_equal(np.array([x['u'] for x in acts]), cols['u'][is_b])


def _obs(t, u, views):
    s = OrganicSessions()
    for i, v in enumerate(views):
        s.next(DefaultContext(t - len(views) + i, u), v)
    return Observation(DefaultContext(t, u), s)


def test_ps_all_and_select_worse_follow_numpy():
    """with_ps_all: `ps-a` is eps * product_probas on an explored act and (1 - eps) * the inner vector on a greedy one;
    epsilon_select_worse explores proportionally to 1 - the inner `ps-a` (host path only)."""
    P = 7
    inner = OrganicUserEventCounterAgent(Configuration({**organic_user_count_args, 'num_products': P, 'random_seed': 3, 'with_ps_all': True}))
    for worse in (False, True):
        eg = EpsilonGreedy(Configuration({**epsilon_greedy_args, 'epsilon': 0.5, 'random_seed': 11, 'num_products': P,
                                          'with_ps_all': True, 'epsilon_select_worse': worse}), inner)
        seen = set()
        for t in range(1, 60):
            eg.reset()
            out = eg.act(_obs(t, 4, [1, 1, 5]), 0, False)
            inner.reset()
            g = inner.act(_obs(t, 4, [1, 1, 5]), 0, False)
            seen.add(out['greedy'])
            if out['greedy']:
                assert out['a'] == g['a'] and out['ps'] == 0.5 * g['ps'] and np.array_equal(out['ps-a'], 0.5 * g['ps-a'])
            else:
                p = (1.0 - g['ps-a']) if worse else np.ones(P)
                p[g['a']] = 0.0
                p = p / np.sum(p)
                assert out['h0'] == g['a'] and out['a'] != g['a']
                assert np.array_equal(out['ps-a'], 0.5 * p) and out['ps'] == 0.5 * p[out['a']]
        assert seen == {True, False}
        assert eg.device_policy() is None and (eg.ope_policy() is None)      # OUC inner has no replay form; select_worse none at all


class _Spy:
    def __init__(self):
        self.config = Configuration({'num_products': 4})
        self.calls = []
        self.needs_training = True
        self.accepts_device_log = True

    def act(self, observation, reward, done):
        return {'t': 0, 'u': 0, 'a': 1, 'ps': 1.0, 'ps-a': ()}

    def train(self, observation, action, reward, done=False):
        self.calls.append(('train', observation, action, reward, done))

    def reset(self):
        self.calls.append(('reset',))

    def train_from_log(self, log, num_organic_users=0):
        self.calls.append(('train_from_log', log, num_organic_users))


def test_delegation():
    from copy import deepcopy
    spy = _Spy()
    eg = EpsilonGreedy(Configuration({**epsilon_greedy_args, 'num_products': 4}), spy)
    eg.train('o', 'a', 1, True)
    eg.reset()
    eg.train_from_log('log', 3)
    assert spy.calls == [('train', 'o', 'a', 1, True), ('reset',), ('train_from_log', 'log', 3)]
    assert eg.needs_training is True and eg.accepts_device_log is True
    plain = EpsilonGreedy(Configuration({**epsilon_greedy_args, 'num_products': 4, 'random_seed': 1}),
                          RandomAgent(Configuration({'num_products': 4, 'random_seed': 2})))
    assert not hasattr(plain, 'train_from_log') and not getattr(plain, 'needs_training', False)
    assert plain.batch_safe is True
    plain.agent.batch_safe = False
    assert plain.batch_safe is False
    twin = deepcopy(eg)
    assert twin.agent is not spy and twin.config is eg.config
    oc = EpsilonGreedy(Configuration({**epsilon_greedy_args, 'num_products': 4}), OrganicCount(Configuration({**organic_count_args, 'num_products': 4})))
    assert hasattr(oc, 'train_from_log') and oc.accepts_device_log and oc.needs_training


def _eg(inner, **over):
    return EpsilonGreedy(Configuration({**epsilon_greedy_args, 'epsilon': 0.1, 'random_seed': 5,
                                        'num_products': inner.config.num_products, **over}), inner)


def test_device_and_replay_forms_exist_in_exactly_the_listed_cases():
    P = 6
    def rnd(**k): return RandomAgent(Configuration({'num_products': P, 'random_seed': 2, **k}))
    def ouc(**k): return OrganicUserEventCounterAgent(Configuration({**organic_user_count_args, 'num_products': P, 'random_seed': 2, **k}))
    def cnt(cls, args, **k): return cls(Configuration({**args, 'num_products': P, **k}))
    lr = LogregFrozenAgent(Configuration({'num_products': P}), np.zeros((P, P)), np.zeros(P), np.arange(P))
    # the device form: the three inner kinds, select_worse and with_ps_all off
    for inner, kind in ((rnd(), _abi.RG_POLICY_RANDOM_AGENT), (ouc(), _abi.RG_POLICY_ORGANIC_USER_COUNT),
                        (cnt(OrganicCount, organic_count_args), _abi.RG_POLICY_LAST_VIEW_TABLE),
                        (cnt(BanditCount, bandit_count_args), _abi.RG_POLICY_LAST_VIEW_TABLE)):
        pol = _eg(inner).device_policy()
        assert pol['policy'] == kind and pol['epsilon_greedy'] == dict(epsilon=0.1, seed=5, pure_new=True)
        assert {k: v for k, v in pol.items() if k != 'epsilon_greedy'}.keys() == inner.device_policy().keys() - {'ps_all'}
        assert _eg(inner, epsilon_pure_new=False).device_policy()['epsilon_greedy']['pure_new'] is False
        assert _eg(inner, epsilon_select_worse=True).device_policy() is None
        assert _eg(inner, with_ps_all=True).device_policy() is None
        assert _eg(inner).ope_policy() is None
    assert _eg(lr).device_policy() is None                                    # LogReg inside: the host loop
    assert _eg(_eg(rnd())).device_policy() is None                             # a wrapper inside a wrapper
    assert _eg(rnd(with_ps_all=True)).device_policy() is None                  # the inner agent has no device form
    assert _eg(ouc(weight_history_function=lambda dt: 1.0)).device_policy() is None
    assert _eg(_Spy()).device_policy() is None
    # the replay form: with_ps_all on both, RandomAgent or a last-view table inside
    pol = _eg(rnd(with_ps_all=True), with_ps_all=True).ope_policy()
    assert pol['kind'] == _abi.RG_POLICY_RANDOM_AGENT and pol['policy_seed'] == 2 and pol['epsilon_greedy']['seed'] == 5
    pol = _eg(cnt(OrganicCount, organic_count_args, with_ps_all=True), with_ps_all=True).ope_policy()
    assert pol['kind'] == _abi.RG_POLICY_LAST_VIEW_TABLE and pol['table'].shape == (P,) and pol['epsilon_greedy']['epsilon'] == 0.1
    assert _eg(rnd(with_ps_all=True), with_ps_all=True, epsilon_select_worse=True).ope_policy() is None
    assert _eg(rnd(with_ps_all=True)).ope_policy() is None                     # the wrapper's own with_ps_all is off
    assert _eg(rnd(), with_ps_all=True).ope_policy() is None                   # the inner agent returns no `ps-a`
    assert _eg(ouc(with_ps_all=True), with_ps_all=True).ope_policy() is None   # OUC inside: h0 is its sampled action
    lr_all = LogregFrozenAgent(Configuration({'num_products': P, 'with_ps_all': True}), np.zeros((P, P)), np.zeros(P), np.arange(P))
    assert lr_all.ope_policy() is not None and _eg(lr_all, with_ps_all=True).ope_policy() is None
    assert ev.ope_policy_of(_eg(ouc(with_ps_all=True), with_ps_all=True)) is None
    assert ev._draws(_eg(rnd(with_ps_all=True), with_ps_all=True, epsilon=0.0).ope_policy())     # an EpsilonGreedy target always draws


def test_a_reference_style_epsilon_greedy_object_stays_on_the_host_loop():
    class EpsilonGreedy:                        # duck-typed by name, like the reference's class: no ope_policy of its own
        def __init__(self):
            self.config = Configuration({'num_products': 4, 'with_ps_all': True, 'epsilon': 0.1})
            self.agent = RandomAgent(Configuration({'num_products': 4, 'random_seed': 1, 'with_ps_all': True}))
    assert ev.ope_policy_of(EpsilonGreedy()) is None


@pytest.mark.parametrize('name', eu.OPE_FIXTURES)
def test_host_loop_of_evaluate_ips_equals_the_reference(name):
    meta, want, P = eu.load(name)
    _, cols = eu.gu.load(meta['log'])
    df = log_frame(cols)
    rewards, ratio = ev._host_snips(eu.wrapper(meta, want, P, with_ps_all=True), df)
    assert np.array_equal(eu.bits(ratio), eu.bits(want['ratio'])) and np.array_equal(np.asarray(rewards, dtype=np.float64), want['c'])
    ips = ev._host_ips(eu.wrapper(meta, want, P, with_ps_all=True), df)
    assert np.array_equal(eu.bits(ips), eu.bits(want['c'] * want['ratio']))
    assert (want['ratio'] == 0.0).any() == meta['eg_args']['epsilon_pure_new'] or meta['inner'] == 'table'
