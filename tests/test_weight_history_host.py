"""The time-weighted view history as a table and a rule (agents/views_history.py: weight_table, weighted_list) — the contract the
device form of the likelihood agent's weighted act is held to.  Everything is compared bit for bit with the scipy calls of the
reference (`weighted_views`) or with fixtures of the unmodified reference.  No GPU."""
import numpy as np
import pytest

import golden_util as gu
from recogym_amd.agents import LogregPolyFrozenAgent
from recogym_amd.agents.views_history import WEIGHT_TABLE_LEN, weight_table, weighted_list, weighted_views
from recogym_amd.envs.configuration import Configuration


def exp_t(t):
    return np.exp(-t)


FUNCS = {'exp_t': exp_t, **gu.WEIGHT_FUNCS}


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


def test_weight_table_is_float32_for_exp_of_an_int16_array():
    table, is_f32 = weight_table(exp_t)
    assert is_f32 and table.dtype == np.float32 and table.shape == (WEIGHT_TABLE_LEN,)
    assert np.array_equal(bits(table), bits(np.exp(-np.arange(WEIGHT_TABLE_LEN, dtype=np.int16))))
    # the band the act depends on: subnormal from 88 to 103, exactly 0 from 104
    tiny = np.finfo(np.float32).tiny
    assert table[87] >= tiny and (table[88:104] > 0).all() and (table[88:104] < tiny).all() and (table[104:] == 0).all()


@pytest.mark.parametrize('name', sorted(gu.WEIGHT_FUNCS))
def test_weight_table_is_float64_for_the_fixture_functions(name):
    table, is_f32 = weight_table(gu.WEIGHT_FUNCS[name])
    assert not is_f32 and table.dtype == np.float64
    assert np.array_equal(bits(table), bits(gu.WEIGHT_FUNCS[name](np.arange(WEIGHT_TABLE_LEN, dtype=np.int16))))


def _raises(t):
    raise ZeroDivisionError


@pytest.mark.parametrize('fn', [
    lambda t: 1.0,                                  # scalar-valued
    lambda t: np.float32(0.5),
    lambda t: t / t.sum(),                          # not elementwise
    lambda t: np.exp(-0.1 * t) / len(t),
    lambda t: 1.0 / t,                              # inf at 0
    lambda t: np.log(t - 5.0),                      # nan below 5
    lambda t: t + 1,                                # an integer table
    lambda t: np.exp(-0.1 * t).astype(np.float16),
    _raises,
], ids=['scalar', 'scalar32', 'normalised', 'by_length', 'inf', 'nan', 'integer', 'float16', 'raises'])
def test_weight_table_refuses_what_no_table_can_stand_for(fn):
    assert weight_table(fn) is None


@pytest.mark.parametrize('name', sorted(FUNCS))
@pytest.mark.parametrize('P', [3, 10, 40])
def test_weighted_list_equals_the_scipy_form_bit_for_bit(name, P):
    fn = FUNCS[name]
    table, is_f32 = weight_table(fn)
    rng = np.random.RandomState(1000 + P)
    dropped = 0
    for case in range(100):
        n = int(rng.randint(1, 121))
        prods = rng.randint(0, P, size=n)
        span = int(rng.choice([3, 30, 130, 400]))            # short spans: many views per clock value; long: underflow under exp(-t)
        times = np.sort(rng.randint(0, span, size=n)) + int(rng.randint(0, 20000))
        now = int(times[-1]) + int(rng.randint(0, 3))
        want = np.asarray(weighted_views([np.int16(p) for p in prods], [np.int16(t) for t in times], np.int16(now), fn, P))
        assert want.dtype == np.float32 and want.shape == (1, P)
        got_p, got_v = weighted_list(prods, times, now, table, is_f32)
        assert got_v.dtype == np.float32
        assert np.array_equal(got_p, np.flatnonzero(want[0] != 0)), (name, P, case)
        assert np.array_equal(bits(got_v), bits(want[0][got_p])), (name, P, case)
        dropped += len(np.unique(prods)) - len(got_p)
    if name == 'exp_t':
        assert dropped > 0, 'no history of this sweep lost a product to underflow'


def test_weighted_list_refuses_clock_values_outside_the_int16_range():
    table, is_f32 = weight_table(exp_t)
    for prods, times, now in (([1], [5], 32768), ([1], [-1], 4), ([1], [9], 8)):
        with pytest.raises(ValueError):
            weighted_list(prods, times, now, table, is_f32)
    p, v = weighted_list([], [], 7, table, is_f32)
    assert len(p) == 0 and len(v) == 0 and v.dtype == np.float32


def test_weighted_list_rebuilds_the_training_features_of_the_reference():
    """hostpath_logreg_weight_history: the unmodified reference's training log and the train_data() it built from it."""
    meta, cols = gu.load('hostpath_logreg_weight_history')
    table, is_f32 = weight_table(gu.WEIGHT_FUNCS[meta['agent_args']['weight_history']])
    u, t, z, v = (cols['trainlog_' + k] for k in 'utzv')
    indptr, indices, data = cols['train_indptr'], cols['train_indices'], cols['train_data']
    row, cur, prods, times = 0, None, [], []
    for i in range(len(u)):
        if u[i] != cur:
            cur, prods, times = u[i], [], []
        if z[i] != 1:
            prods.append(int(v[i]))
            times.append(int(t[i]))
            continue
        got_p, got_v = weighted_list(prods, times, int(t[i]), table, is_f32)
        lo, hi = indptr[row], indptr[row + 1]
        assert np.array_equal(got_p, indices[lo:hi]), row
        assert np.array_equal(bits(got_v.astype(np.float64)), bits(data[lo:hi].astype(np.float64))), row
        row += 1
    assert row == len(indptr) - 1 > 1000


def test_a_weighted_agent_keeps_every_other_device_form_closed():
    P = 6
    w = np.linspace(-1, 1, 2 * P + P * P)[None, :]
    for extra in ({}, {'with_ps_all': True}):
        agent = LogregPolyFrozenAgent(Configuration({'num_products': P, 'weight_history_function': exp_t, **extra}), w, [0.5])
        assert agent.ope_policy() is None and agent.ope_policy_checked() is None
    from recogym_amd.agents import EpsilonGreedy
    from recogym_amd.agents.epsilon_greedy import epsilon_greedy_args
    inner = LogregPolyFrozenAgent(Configuration({'num_products': P, 'weight_history_function': exp_t}), w, [0.5])
    for models in (False, True):
        eg = EpsilonGreedy(Configuration({**epsilon_greedy_args, 'num_products': P, 'random_seed': 3, 'device_models': models}), inner)
        assert eg.device_policy() is None


@pytest.mark.parametrize('name,fn', [('poly_wh_exp_default', exp_t), ('poly_wh_exp02_normal', gu.WEIGHT_FUNCS['exp_0.2'])])
def test_the_contract_gives_the_reference_agent_its_actions_and_training_features(name, fn):
    """tests/make_golden_weight_history.py: the unmodified reference's LogregPolyAgent with a weight function, on the default clock
    (float32 table; products leave the list as exact zeros) and under a NormalTimeGenerator (float64 table).  weighted_list, the
    decisions in the contract's order, scipy's expit and the first maximum give every logged action; applied per bandit row of the
    training log they rebuild the reference's own train_data() bit for bit."""
    from scipy.special import expit
    from recogym_amd.agents.logreg_poly import poly_decisions, poly_split
    meta, cols = gu.load(name)
    P = meta['env_args']['num_products']
    table, is_f32 = weight_table(fn)
    assert is_f32 == meta['census']['table_f32']
    model = poly_split(cols['poly_coef'], cols['poly_intercept'], P)
    clock = cols['time'] if 'time' in cols else cols['t']

    def walk(u, z, v, t, on_act):
        cur, prods, times, acts = None, [], [], 0
        for i in range(len(u)):
            if u[i] != cur:
                cur, prods, times = u[i], [], []
            if z[i] != 1:
                prods.append(int(v[i]))
                times.append(int(np.int16(t[i])))
                continue
            on_act(acts, i, *weighted_list(prods, times, int(np.int16(t[i])), table, is_f32), len(set(prods)))
            acts += 1
        return acts

    dropped = []

    def check_action(k, i, p, val, distinct):
        assert int(np.argmax(expit(poly_decisions(p, val.astype(np.float64), *model)))) == cols['a'][i], i
        dropped.append(distinct - len(p))
    assert walk(cols['u'], cols['z'], cols['v'], clock, check_action) == meta['census']['acts']
    assert sum(dropped) == meta['census']['dropped'] and (sum(dropped) > 0) == is_f32

    indptr, indices, data = cols['train_indptr'], cols['train_indices'], cols['train_data']

    def check_row(k, i, p, val, distinct):
        lo, hi = indptr[k], indptr[k + 1]
        assert np.array_equal(p, indices[lo:hi]), k
        assert np.array_equal(bits(val.astype(np.float64)), bits(data[lo:hi].astype(np.float64))), k
    rows = walk(*(cols['trainlog_' + k] for k in 'uzvt'), check_row)
    assert rows == len(indptr) - 1 > 1000
