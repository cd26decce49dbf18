"""The exploration study on the host (no GPU): the NumPy forms of the filtered training and of the step statistics, and the masks
the Python layer builds, against the fixtures tests/make_golden_evolution.py recorded from the reference's own evaluate_agent;
the constants and the small helpers of the reference's surface.  Exact throughout."""
import numpy as np
import pytest

import golden_util as gu
import recogym_amd as recogym
from recogym_amd import constants
from recogym_amd import evaluate_agent as ev
from recogym_amd.agents import BanditCount, OrganicCount, bandit_count_args, organic_count_args
from recogym_amd.constants import TrainingApproach
from recogym_amd.envs.configuration import Configuration

FIXTURES = gu.fixtures('evo_')
_CACHE = {}


def load(name):
    if name not in _CACHE:
        _CACHE[name] = gu.load(name)
    return _CACHE[name]


def new_agent(meta):
    P = meta['env_args']['num_products']
    if meta['agent'] == 'oc':
        return OrganicCount(Configuration({**organic_count_args, 'num_products': P}))
    return BanditCount(Configuration({**bandit_count_args, 'num_products': P}))


def phase_log(cols, phase):
    """The rows of one phase as the column dict Simulator.log_columns() returns."""
    k = cols['phase'] == phase
    is_b = cols['z'][k] == 1
    return dict(t=cols['t'][k].astype(np.float32), u=cols['u'][k].astype(np.int32), is_bandit=is_b,
                v=np.where(is_b, 0, cols['v'][k]).astype(np.int32), a=np.where(is_b, cols['a'][k], 0).astype(np.int32),
                c=np.where(is_b, cols['c'][k], np.nan).astype(np.float32), ps=np.full(int(k.sum()), np.nan)), k


def recorded_tables(meta, cols, phase):
    P = meta['env_args']['num_products']
    out = {}
    for tab in ('co_counts', 'pulls_a', 'clicks_a'):
        if tab in cols:
            out[tab] = cols[tab][phase]
        elif tab + '_coo' in cols:
            coo = cols[tab + '_coo']
            coo = coo[coo[:, 0] == phase]
            out[tab] = np.zeros((P, P), dtype=np.int64)
            out[tab][coo[:, 1], coo[:, 2]] = coo[:, 3]
    return out


def test_the_fixtures_are_there():
    assert len(FIXTURES) >= 14
    approaches = {load(n)[0]['approach'] for n in FIXTURES}
    assert approaches == {'ALL_DATA', 'ALL_EXPLORATION_DATA', 'SLIDING_WINDOW_ALL_DATA', 'SLIDING_WINDOW_EXPLORATION_DATA', 'LAST_STEP'}
    for n in FIXTURES:              # no initial user ended in its first organic session
        meta, cols = load(n)
        for u in range(meta['n_init']):
            assert (cols['z'][cols['u'] == u] == 1).any()


@pytest.mark.parametrize('name', FIXTURES)
def test_masked_training_reproduces_the_tables_after_every_phase(name):
    meta, cols = load(name)
    agent = new_agent(meta)
    for phase in range(meta['num_steps'] + 1):
        if meta['approach'] == 'LAST_STEP' and phase >= 2:
            agent = new_agent(meta)              # the training agent of step s >= 2 is a copy of the agent as it was passed in
        log, k = phase_log(cols, phase)
        agent.train_online_from_log(log, cols['trained'][k] == 1)
        want = recorded_tables(meta, cols, phase)
        for tab, value in want.items():
            assert np.array_equal(getattr(agent, tab), value.astype(np.float64)), (phase, tab)
        lpv = agent.last_product_viewed
        assert (-1 if lpv is None else lpv) == cols['lpv'][phase], phase


def test_several_rows_meet_none_in_the_fixture_without_initial_users():
    from recogym_amd.agents import count_tables as ct
    meta, cols = load('evo_bc_noinit_explore')
    log, k = phase_log(cols, 1)
    u, is_b, v, a, click, phantom = ct.online_arrays(log)
    ix, _, _, _ = ct.online_bandit_updates(u, is_b, v, a, click, 10, ct.counted_rows(is_b, phantom, cols['trained'][k] == 1), None)
    assert meta['n_init'] == 0 and (ix < 0).sum() >= 2


@pytest.mark.parametrize('name', FIXTURES)
def test_statistics_reproduce_the_rewards(name):
    meta, cols = load(name)
    P = meta['env_args']['num_products']
    for step in range(1, meta['num_steps'] + 1):
        k = cols['phase'] == step
        is_b = cols['z'][k] == 1
        args = (cols['u'][k], cols['t'][k], is_b, np.where(is_b, cols['a'][k], 0), cols['c'][k] == 1, P)
        counts, clicks, explored = ev.evolution_stats(*args, greedy=cols['greedy'][k])
        want = [cols[c][step - 1] for c in ('success', 'failure', 'success_greedy', 'failure_greedy')]
        assert counts.tolist() == want
        assert np.array_equal(clicks, cols['actions'][:, step - 1])
        eg = meta['eg_args']
        # the explore flip recomputed from the addressed draw is the reference's own `greedy`
        counts2, clicks2, explored2 = ev.evolution_stats(*args, epsilon_greedy=None if eg is None else dict(epsilon=eg['epsilon'],
                                                                                                            seed=eg['random_seed']))
        assert counts2.tolist() == want and np.array_equal(clicks2, clicks)
        if eg is not None:
            assert np.array_equal(explored2, is_b & (cols['greedy'][k] == 0)) and np.array_equal(explored, explored2)
        else:
            assert not explored2.any() and want[2] == want[3] == 0
    assert (cols['actions'][:, -1] == 0).all()


@pytest.mark.parametrize('name', FIXTURES)
def test_training_masks_equal_the_recorded_trained_column(name):
    meta, cols = load(name)
    approach = TrainingApproach[meta['approach']]
    samples = 0
    for step in range(1, meta['num_steps'] + 1):
        k = cols['phase'] == step
        is_act = cols['z'][k] == 1
        explored = None if meta['eg_args'] is None else is_act & (cols['greedy'][k] == 0)
        before = samples
        mask, samples = ev.training_mask(approach, is_act, explored, samples, meta['window'])
        assert samples == before + is_act.sum()
        assert np.array_equal(is_act if mask is None else mask, cols['trained'][k] == 1)
    k = cols['phase'] == 0
    assert np.array_equal(cols['z'][k] == 1, cols['trained'][k] == 1)          # the initial phase trains at every act


def test_constants_have_the_reference_names_and_values():
    recorded = load(FIXTURES[0])[0]['constants']
    assert set(recorded) == {'AgentStats', 'AgentInit', 'TrainingApproach', 'EvolutionCase', 'RoiMetrics'}
    for name, members in recorded.items():
        enum = getattr(constants, name)
        assert {m.name: m.value for m in enum} == members
        assert getattr(recogym, name) is enum


def test_most_valuable_and_missing_greedy_raise():
    is_act = np.array([False, True, True])
    with pytest.raises(AssertionError):
        ev.training_mask(TrainingApproach.MOST_VALUABLE, is_act, is_act, 0, 10)
    with pytest.raises(AssertionError):
        ev.training_mask(TrainingApproach.MOST_VALUABLE, np.zeros(3, dtype=bool), None, 0, 10)          # a step without an act too
    with pytest.raises(KeyError, match='greedy'):
        ev.training_mask(TrainingApproach.ALL_EXPLORATION_DATA, is_act, None, 0, 10)
    with pytest.raises(KeyError, match='greedy'):
        ev.training_mask(TrainingApproach.SLIDING_WINDOW_EXPLORATION_DATA, is_act, None, 0, 10)


def test_sliding_window_counts_acts_across_steps():
    is_act = np.array([True, False, True, True, False, True])
    mask, samples = ev.training_mask(TrainingApproach.SLIDING_WINDOW_ALL_DATA, is_act, None, 1, 3)      # acts are samples 2, 3, 4, 5
    assert mask.tolist() == [False, False, True, False, False, False] and samples == 5
    explored = np.array([True, False, False, True, False, True])
    mask, samples = ev.training_mask(TrainingApproach.SLIDING_WINDOW_EXPLORATION_DATA, is_act, explored, 4, 2)     # 5, 6, 7, 8
    assert mask.tolist() == [False, False, False, False, False, True] and samples == 8


def test_build_agents_format_epsilon_generate_epsilons():
    assert ev.generate_epsilons() == [0.00, 0.01, 0.02, 0.03, 0.05, 0.08] == list(ev.EvolutionEpsilons)
    assert [ev.format_epsilon(e) for e in (0, 0.05, 0.078, 0.3)] == ['0.00', '0.05', '0.08', '0.30']
    init = {**ev.build_agent_init('Organic', OrganicCount, {**organic_count_args}),
            **ev.build_agent_init('Bandit', BanditCount, {**bandit_count_args, 'with_ps_all': True})}
    assert init['Organic'] == {constants.AgentInit.CTOR: OrganicCount, constants.AgentInit.DEF_ARGS: organic_count_args}
    agents = ev.build_agents(init, {'num_products': 7, 'random_seed': 3})
    assert list(agents) == ['Organic', 'Bandit']
    assert isinstance(agents['Organic'], OrganicCount) and isinstance(agents['Bandit'], BanditCount)
    assert agents['Organic'].config.num_products == 7 and agents['Bandit'].config.with_ps_all and agents['Bandit'].config.random_seed == 3


def test_the_surface_is_exported_from_the_package():
    for name in ('build_agent_init', 'build_agents', 'gather_agent_stats', 'generate_epsilons', 'format_epsilon', 'gather_exploration_stats'):
        assert getattr(recogym, name) is getattr(ev, name)
    assert recogym.evaluate_agent is ev and callable(recogym.evaluate_agent)          # the module, called, is the function
    assert recogym.evaluate_agent.evaluate_agent.__defaults__ == (100, 1000, 10, TrainingApproach.ALL_DATA, 10000)
    from recogym_amd.agents.epsilon_greedy import EpsilonGreedy, epsilon_greedy_args
    eg = EpsilonGreedy(Configuration({**epsilon_greedy_args, 'num_products': 10}), OrganicCount())
    assert eg.train_online_from_log.__self__ is eg.agent
    from recogym_amd.agents import RandomAgent, random_args
    assert not hasattr(EpsilonGreedy(Configuration({**epsilon_greedy_args, 'num_products': 10}), RandomAgent(Configuration(random_args))),
                       'train_online_from_log')
