"""BayesianAgentVB in the device step loop (RG_POLICY_BAYES_VB, k_bayes_acts): the reference's own logs row for row
(tests/golden/bayes_*.npz, tests/make_golden_bayes_vb.py) with the census the generator recorded, generate_logs against the
per-user host route, decisions placed to the bit, random models that test the margin claim |q_device - q_reference| <= W
directly against the reference's expression, and the unresolved-act protocol.  Needs a real MI355X."""
import warnings

import numpy as np
import pytest

import adversarial_util as au
import bayes_util as bu
import golden_util as gu
from device_util import assert_frames_equal, make_env
import recogym_amd as recogym
from recogym_amd import _abi
from recogym_amd.agents import BayesianAgentVB, BayesianVBFrozenAgent, bayesian_poly_args
from recogym_amd.agents.bayesian_poly_vb import (SATURATED, UNRESOLVED, ZSAT, bayes_abs_sum, bayes_decisions, bayes_margin, bayes_rule,
                                                 bayes_transpose, bayes_z_bound, reference_act)
from recogym_amd.envs.configuration import Configuration
from recogym_amd.envs.reco_env_v1 import env_1_args

pytestmark = pytest.mark.gpu


def run_fixture(name, first_user=0, n_users=None, organic_only_below=0, ledger=False):
    """-> meta, cols, rows, counters, the raw sorted log, launches of k_bayes_acts[, the launch ledger, poly_verify's outcome and
    the unresolved list]"""
    from recogym_amd.sim import Simulator
    meta, cols = gu.load(name)
    P, n = meta['env_args']['num_products'], meta['n_users'] if n_users is None else n_users
    frozen = BayesianVBFrozenAgent(Configuration({'num_products': P}), bu.fixture_lambda(meta, cols))
    sim = Simulator(gu.env_config(meta), n, device='cuda:0', **frozen.device_policy())
    sim.reset_users(first_user, n, organic_only_below=organic_only_below)
    sim.run()
    rows, cnt, raw = sim.rows(), sim.counters(), sim.sorted_log_host()[0]
    launched = sim.get_option('launched_bayes_vb')
    extra = ()
    if ledger:
        stands = sim.poly_verify()
        extra = (au.ledger(sim), stands, sim.poly_unresolved.copy())
    sim.close()
    return (meta, cols, rows, cnt, raw, launched) + extra


def assert_log_equals_the_reference(name, meta, cols, rows, cnt, launched):
    """The rows and counters of a run of the fixture's users (of several runs: rows concatenated, counters summed) held to it."""
    gu.assert_rows_equal(rows, cols, ps_rtol=0, what=name)
    census = meta['census']
    print(name, {k: cnt[k] for k in ('lr_acts', 'lr_rows', 'bayes_saturated', 'poly_unresolved')}, census)
    assert cnt['bayes_saturated'] == census['saturated'] and cnt['poly_unresolved'] == census['unresolved'] == 0
    assert cnt['lr_acts'] == census['acts'] and launched > 0
    assert cnt['live'] == 0 and cnt['log_dropped'] == 0 and cnt['hist_overflow'] == 0


@pytest.mark.parametrize('name', bu.FIXTURES)
def test_device_log_equals_the_reference(name):
    """P = 4 with all 1000 draws, P = 10 with 120 draws (a masked last stride) under sigma_omega > 0 (lock-step rounds) and = 0,
    and the shifted model whose acts all saturate with the lowest index winning."""
    meta, cols, rows, cnt, _, launched = run_fixture(name)
    assert_log_equals_the_reference(name, meta, cols, rows, cnt, launched)


def test_two_runs_give_the_same_log():
    a, b = run_fixture('bayes_p10_s120'), run_fixture('bayes_p10_s120')
    assert np.array_equal(a[4], b[4]) and a[3] == b[3]


def trained_agent():
    """-> the meta of bayes_p4, BayesianAgentVB trained on the fixture's training log"""
    meta, cols = gu.load('bayes_p4')
    train = {k[len('trainlog_'):]: v for k, v in cols.items() if k.startswith('trainlog_')}
    from make_golden_ope import log_frame
    agent = BayesianAgentVB(Configuration({**bayesian_poly_args, 'num_products': 4, 'random_seed': 7}))
    agent.train_from_log(log_frame(train))
    return meta, agent


def test_generate_logs_with_the_trained_agent_equals_the_host_route():
    meta, agent = trained_agent()
    env = make_env(meta['env_args'])
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        got = env.generate_logs(100, agent)
    want = env._generate_logs_per_user(100, agent, 0)
    assert_frames_equal(got, want)
    assert (got['ps'].to_numpy(dtype=np.float64, na_value=np.nan)[(got['z'] == 'bandit').to_numpy()] == 1.0).all()


def test_out_of_range_combinations_are_refused():
    from device_util import handle
    import torch
    lib, h, ws = handle(_abi.RG_POLICY_BAYES_VB)
    lam = torch.zeros(100 * 2, dtype=torch.float64, device='cuda:0')
    assert lib.rg_sim_set_bayes_vb(h, lam.data_ptr(), 0) == -1 and b'num_samples' in lib.rg_last_error()
    assert lib.rg_sim_set_bayes_vb(h, None, 2) == -1 and b'NULL' in lib.rg_last_error()
    assert lib.rg_sim_set_bayes_vb(h, lam.data_ptr(), 2) == 0
    cdf = torch.ones(9, dtype=torch.float64, device='cuda:0')
    assert lib.rg_sim_set_epsilon_greedy_model(h, 0.1, 1, 1, cdf.data_ptr(), 0.01, 0.9) == -1 and b'BAYES_VB' in lib.rg_last_error()
    lib.rg_sim_destroy(h)
    lib, h, ws = handle(_abi.RG_POLICY_LOGREG_POLY)
    assert lib.rg_sim_set_bayes_vb(h, lam.data_ptr(), 2) == -4
    lib.rg_sim_destroy(h)


# ------------------------------------------------------------------------------------------------
# decisions placed to the bit, random models
# ------------------------------------------------------------------------------------------------
def debug_acts(P, lam, nd, prod, cnt):
    """rg_sim_debug_set_history + rg_sim_debug_bayes_acts -> (actions, flags, q) of the users whose histories are given."""
    from recogym_amd.sim import Simulator
    n = len(nd)
    cfg = Configuration({**env_1_args, 'random_seed': 5, 'num_products': P, 'K': 2, 'sigma_omega': 0.0})
    sim = Simulator(cfg, n, device='cuda:0', policy=_abi.RG_POLICY_BAYES_VB, policy_seed=0, ouc=dict(history_cap=max(prod.shape[1], 255)),
                    bayes_vb=dict(lam=lam), log_capacity=0)
    sim.reset_users(0, n)
    sim.debug_set_history(nd, prod, cnt)
    out = sim.debug_bayes_acts()
    sim.close()
    return out


@pytest.mark.parametrize('P', [2, 10, 65, 130])
def test_placed_decisions(P):
    cases = bu.placed(P)
    for c0 in range(0, len(cases), P):          # a case per product: the user that viewed product p once decides on lam_t[p, :, 0]
        batch = cases[c0:c0 + P]
        lam_t = np.zeros((P, P, 1))
        for p, (_, z, _, _) in enumerate(batch):
            lam_t[p, :, 0] = z
        lam = np.ascontiguousarray(lam_t.reshape(P * P, 1).T)
        assert np.array_equal(bayes_transpose(lam, P), lam_t)
        n = len(batch)
        act, fl, q = debug_acts(P, lam, np.ones(n, dtype=np.uint32), np.arange(n, dtype=np.uint32).reshape(n, 1),
                                np.ones((n, 1), dtype=np.uint32))
        for i, (name, z, want_a, want_fl) in enumerate(batch):
            dec = bayes_decisions([i], [1], lam_t)
            rule = bayes_rule(dec, 1, bayes_abs_sum([i], [1], lam_t))
            host = reference_act(np.eye(P, dtype=np.int16)[i:i + 1], lam)[0]
            print(P, name, 'device', act[i], fl[i], 'rule', rule, 'host', host)
            assert rule[1] == want_fl and (want_a is None or rule[0] == want_a), (P, name, rule)
            assert (act[i], fl[i]) == rule, (P, name, act[i], fl[i], rule)
            if not fl[i] & UNRESOLVED:
                assert act[i] == host, (P, name)
    # the empty history: action 0, resolved, every mean 0.5
    act, fl, q = debug_acts(P, np.full((3, P * P), 7.0), np.zeros(1, dtype=np.uint32), np.zeros((1, 1), dtype=np.uint32),
                            np.zeros((1, 1), dtype=np.uint32))
    assert (act[0], fl[0]) == (0, 0) and (q[0] == 0.5).all()


def models(P, S, rng):
    """Weight scales that place acts below ZSAT (means far apart), across it, above it (every decision positive: long histories
    saturate), and a model whose two best actions have identical columns (an exact tie of the means, below ZSAT)."""
    tie = rng.standard_normal((S, P, P)) * 0.0002
    top = 0.002 + rng.standard_normal((S, P)) * 0.0002
    tie[:, :, min(2, P - 1)] = top
    tie[:, :, P - 1] = top
    return dict(below=rng.standard_normal((S, P * P)) * 0.002,
                across=rng.standard_normal((S, P * P)) * 0.05 + 0.02,
                above=np.abs(rng.standard_normal((S, P * P))) + 0.5,
                tie=tie.reshape(S, P * P))


@pytest.mark.parametrize('S', [1, 63, 64, 65, 130, 1000])
@pytest.mark.parametrize('P', [10, 65, 130])
def test_random_models_and_histories(P, S):
    """Histories of 1, 15, 16, 40 and P distinct products (the first history line holds 15), counts up to 300; S below, at and
    above one stride of 64 lanes and several strides.  Per act: the device's means lie within W of the reference expression's
    (the margin claim itself); a resolved act has the host act's action; an act whose reference gap exceeds 4 W outside the
    saturated zone is resolved; the model with two identical best columns gives unresolved acts."""
    rng = np.random.RandomState(1000 * P + S)
    sizes = sorted({s for s in (1, 15, 16, 40, P) if s <= P})
    users = [s for s in sizes for _ in range(1 if P * P * S > 5_000_000 else 2)]       # (the reference expression is P x P^2 x S per act)
    n, stride = len(users), max(sizes)
    nd = np.array(users, dtype=np.uint32)
    prod = np.zeros((n, stride), dtype=np.uint32)
    cnt = np.zeros((n, stride), dtype=np.uint32)
    for i, s in enumerate(users):
        prod[i, :s] = np.sort(rng.choice(P, s, replace=False))
        cnt[i, :s] = np.where(rng.rand(s) < 0.7, rng.randint(1, 4, s), rng.randint(1, 301, s))
    seen = dict(plain=0, saturated=0, unresolved=0)
    for kind, lam in models(P, S, rng).items():
        lam_t = bayes_transpose(lam, P)
        act, fl, q = debug_acts(P, lam, nd, prod, cnt)
        for i, s in enumerate(users):
            p_i, c_i = prod[i, :s], cnt[i, :s]
            X = np.zeros((1, P), dtype=np.int16)
            X[0, p_i] = c_i
            host, q_ref = reference_act(X, lam)
            z = bayes_decisions(p_i, c_i, lam_t)
            M = bayes_abs_sum(p_i, c_i, lam_t)
            W = bayes_margin(s, M, S)
            assert bayes_z_bound(s, M) < 1.0
            err = np.abs(q[i] - q_ref).max()
            assert err <= W, (P, S, kind, i, s, err, W)
            assert bool(fl[i] & SATURATED) == bool((z.min(axis=1) >= ZSAT).any()), (P, S, kind, i)       # z is the host's to the bit
            if not fl[i] & UNRESOLVED:
                assert act[i] == host, (P, S, kind, i, s)
            top = np.sort(q_ref)[::-1]
            if not fl[i] & SATURATED and top[0] - top[1] > 4.0 * W:
                assert not fl[i] & UNRESOLVED, (P, S, kind, i, s, top[0] - top[1], W)
            if kind == 'tie':
                assert z.max() < ZSAT and set(np.argsort(q_ref)[-2:]) == {min(2, P - 1), P - 1}
                assert fl[i] == UNRESOLVED and act[i] == min(2, P - 1), (P, S, i, act[i], fl[i])
            seen['plain'] += fl[i] == 0
            seen['saturated'] += fl[i] & SATURATED
            seen['unresolved'] += (fl[i] & UNRESOLVED) >> 1
    print(P, S, seen)
    assert seen['plain'] > 0 and seen['saturated'] > 0 and seen['unresolved'] > 0


# ------------------------------------------------------------------------------------------------
# unresolved acts: confirmed by the host -> the device log stands; refuted -> the host route
# ------------------------------------------------------------------------------------------------
OVER = dict(random_seed=321, num_products=10, K=4)


def constant_agent(l1, l2, P=10):
    """One draw whose weight depends on the action alone: z[a] = l_a x (the user's views), l_1 = l1, l_2 = l2, the rest -1."""
    lam = np.full((P, P), -1.0)
    lam[:, 1], lam[:, 2] = l1, l2
    return BayesianVBFrozenAgent(Configuration({'num_products': P}), lam.reshape(1, P * P))


def test_an_unresolved_act_the_host_confirms_keeps_the_device_route():
    """Two identical columns: the two means tie exactly on the device (inside 2 W) and in the reference, whose first maximum is
    the device's action."""
    from recogym_amd.sim import Simulator
    agent = constant_agent(0.25, 0.25)
    sim = Simulator(Configuration({**env_1_args, **OVER}), 60, device='cuda:0', **agent.device_policy())
    sim.reset_users(0, 60)
    sim.run()
    cnt = sim.counters()
    assert sim.poly_verify() and not sim.poly_overflow
    assert len(sim.poly_unresolved) == cnt['poly_unresolved'] > 60 and len(sim.poly_refuted) == 0
    assert cnt['poly_unresolved'] + cnt['bayes_saturated'] == cnt['lr_acts']      # (from 160 views on the pair saturates: resolved)
    assert (sim.poly_unresolved[:, 2] == 1).all()
    sim.close()
    env = make_env(OVER)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        got = env.generate_logs(60, agent)
    assert_frames_equal(got, env._generate_logs_per_user(60, agent, 0))
    assert set(got['a'].dropna().astype(int)) == {1}


def refuted_agent():
    """After one view z[1] = 38 and z[2] = 45: the device takes the saturated action 2 and lists the act, because the mean of
    action 1 is within W of 1.0; the reference's expit(38) IS 1.0, so its first maximum is action 1.  (From two views on both
    saturate and both sides take action 1.)"""
    agent = constant_agent(38.0, 45.0)
    X = np.zeros((1, 10), dtype=np.int16)
    X[0, 3] = 1
    a, q = reference_act(X, agent.Lambda)                      # the host's own expression decides what the reference does
    assert a == 1 and q[1] == q[2] == 1.0
    z = bayes_decisions([3], [1], agent.lam_t)
    assert bayes_rule(z, 1, bayes_abs_sum([3], [1], agent.lam_t)) == (2, SATURATED | UNRESOLVED)
    return agent


def test_a_refuted_act_sends_generate_logs_to_the_host_route():
    agent = refuted_agent()
    env = make_env(OVER)
    with pytest.warns(RuntimeWarning, match='host route'):
        got = env.generate_logs(60, agent)
    assert_frames_equal(got, env._generate_logs_per_user(60, agent, 0))
    assert set(got['a'].dropna().astype(int)) == {1}          # the reference's action throughout


def test_test_agent_applies_the_protocol_too():
    """test_agent counts clicks from the device counters: with an act the host refutes it must count the host route's rows."""
    from scipy.stats.distributions import beta
    from recogym_amd.sim import Simulator
    agent, n = refuted_agent(), 300
    env = make_env(OVER)
    want = env._generate_logs_per_user(n, agent, 0)
    c = want[want['z'] == 'bandit']['c']
    s, f = int(c.sum()), int(c.shape[0]) - int(c.sum())
    sim = Simulator(Configuration({**env_1_args, **OVER}), n, device='cuda:0', **agent.device_policy())
    sim.reset_users(0, n)
    sim.run()
    dev_rows = sim.rows()
    assert not sim.poly_verify() and len(sim.poly_refuted) > 0 and (sim.poly_refuted[:, 2] == 2).all()
    sim.close()
    assert (dev_rows['a'][dev_rows['z'] == 1] == 2).any()       # the unverified device log holds the refuted action
    with pytest.warns(RuntimeWarning, match='host route'):
        got = recogym.test_agent(env, agent, 0, n)
    assert got == (beta.ppf(0.5, s + 1, f + 1), beta.ppf(0.025, s + 1, f + 1), beta.ppf(0.975, s + 1, f + 1))
    # a confirmed act: the counters of the device run stand, no warning
    ok = constant_agent(0.25, 0.25)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        got = recogym.test_agent(env, ok, 0, 60)
    c = env._generate_logs_per_user(60, ok, 0)
    c = c[c['z'] == 'bandit']['c']
    assert got[0] == beta.ppf(0.5, int(c.sum()) + 1, int(c.shape[0]) - int(c.sum()) + 1)
