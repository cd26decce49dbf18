"""BayesianAgentVB on the host: the device rule restated in numpy (bayes_rule on bayes_decisions) and the host act against the
unmodified reference's own logs (tests/golden/bayes_*.npz, tests/make_golden_bayes_vb.py), the port's build() against the
reference's posterior draws, the margin W and the rule on decisions placed to the bit, and where the agent has a device form.
No device."""
import numpy as np
import pytest
from scipy.special import expit

import bayes_util as bu
import golden_util as gu
from make_golden_ope import log_frame
from recogym_amd import _abi
from recogym_amd import agents
from recogym_amd.agents.bayesian_poly_vb import (MODEL_BYTES_CAP, SATURATED, UNRESOLVED, ZSAT, BayesianAgentVB, BayesianVBFrozenAgent,
                                                 bayes_abs_sum, bayes_decisions, bayes_margin, bayes_means, bayes_rule,
                                                 bayes_transpose, bayes_z_bound, bayesian_poly_args, reference_act)
from recogym_amd.envs.configuration import Configuration
from recogym_amd.envs.context import DefaultContext
from recogym_amd.envs.observation import Observation
from recogym_amd.envs.session import OrganicSessions


def test_agent_is_exported_with_the_reference_arguments():
    assert agents.BayesianAgentVB is BayesianAgentVB and agents.bayesian_poly_args is bayesian_poly_args
    want = dict(num_products=10, poly_degree=2, max_iter=5000, aa=1., bb=1., with_ps_all=False, num_samples=1000)
    assert {k: v for k, v in bayesian_poly_args.items() if k != 'random_seed'} == want and 'random_seed' in bayesian_poly_args
    assert _abi.RG_POLICY_BAYES_VB == 8 and _abi.RG_CNT_BAYES_SATURATED == 29 and _abi.RG_ABI_VERSION == 15
    assert (ZSAT, SATURATED, UNRESOLVED) == (40.0, 1, 2)


def test_the_policy_is_accepted_and_the_unassigned_number_stays_refused():
    """rg_sim_create is host code: policy 8 sizes a workspace with a history row and the unresolved list; 7 is not assigned."""
    import ctypes as C
    import __graft_entry__ as graft
    import make_golden_create_plan as plan
    graft.build()
    lib = _abi.load()
    need = lib.rg_sim_workspace_bytes(C.byref(plan.rg_config(plan._c(policy=_abi.RG_POLICY_BAYES_VB))), 1000)
    assert need > lib.rg_sim_workspace_bytes(C.byref(plan.rg_config(plan._c(policy=0))), 1000) > 0
    assert lib.rg_sim_workspace_bytes(C.byref(plan.rg_config(plan._c(policy=7))), 1000) == 0
    assert lib.rg_last_error() == b'unknown policy 7'
    assert lib.rg_sim_workspace_bytes(C.byref(plan.rg_config(plan._c(policy=9))), 1000) == 0


@pytest.mark.parametrize('name', bu.FIXTURES)
def test_rule_reproduces_the_reference_actions_and_the_census(name):
    meta, cols = gu.load(name)
    census = bu.rule_census(cols, meta['env_args']['num_products'], bu.fixture_lambda(meta, cols))     # asserts every action
    assert census == meta['census'] and census['unresolved'] == 0 and census['acts'] > 200


def test_some_fixture_proves_the_saturated_zone():
    c = [gu.load(n)[0]['census'] for n in bu.FIXTURES]
    assert any(x['saturated'] > 0 and x['lower_wins'] > 0 for x in c) and any(x['saturated'] == 0 for x in c)


@pytest.mark.parametrize('name', bu.FIXTURES)
def test_host_act_reproduces_the_reference_actions(name):
    """The agent driven like generate_logs drives it (the organic rows since the last act as the observation's sessions)."""
    meta, cols = gu.load(name)
    P = meta['env_args']['num_products']
    ag = BayesianVBFrozenAgent(Configuration({'num_products': P, 'with_ps_all': True}), bu.fixture_lambda(meta, cols))
    u, z, v, a, t = cols['u'], cols['z'], cols['v'], cols['a'], cols['t']
    cur, session, acts = None, None, 0
    for i in range(len(u)):
        if u[i] != cur:
            cur, session = u[i], OrganicSessions()
            ag.reset()
        if z[i] == 0:
            session.next(DefaultContext(int(t[i]), int(u[i])), int(v[i]))
        else:
            act = ag.act(Observation(DefaultContext(int(t[i]), int(u[i])), session), 0, False)
            assert act['a'] == a[i] and act['ps'] == 1.0, (name, i, act['a'], int(a[i]))
            assert act['ps-a'].sum() == 1.0 and act['ps-a'][a[i]] == 1.0
            session = OrganicSessions()
            acts += 1
    assert acts == int((z == 1).sum()) > 1000


def test_build_on_the_reference_training_log():
    """The port's build() with the agent's own stream against the reference's draws from the global stream seeded alike: Lambda
    within 64 x the deviation the generator measured (floor 1e-12; the factor covers another BLAS build), and the reference's
    actions on the evaluation log."""
    meta, cols = gu.load('bayes_p4')
    P = meta['env_args']['num_products']
    log = log_frame({k[len('trainlog_'):]: v for k, v in cols.items() if k.startswith('trainlog_')})
    ag = BayesianAgentVB(Configuration({**bayesian_poly_args, 'num_products': P, 'random_seed': meta['agent_args']['random_seed']}))
    ag.train_from_log(log)
    assert ag.frozen is None                                  # the model is built at the first act
    frozen = ag._ready()
    lam = cols['bayes_lambda']
    assert frozen.Lambda.shape == lam.shape == (1000, P * P)
    dev = np.abs(frozen.Lambda - lam).max() / np.abs(lam).max()
    print('deviation', dev, 'recorded', meta['lambda_dev'])
    assert dev <= max(64 * meta['lambda_dev'], 1e-12)
    assert np.allclose(ag.q_mu, cols['bayes_q_mu'], rtol=1e-9, atol=0)
    pol = ag.device_policy()
    assert pol['policy'] == _abi.RG_POLICY_BAYES_VB and pol['ouc'] is None and pol['bayes_vb']['lam'] is frozen.Lambda
    assert ag.ope_policy() is None and ag.ope_policy_checked() is None
    census = bu.rule_census(cols, P, frozen.Lambda)           # asserts the reference's action on every act
    assert census['unresolved'] == 0 and census['acts'] == meta['census']['acts']


def test_num_samples_is_a_key():
    _, cols = gu.load('bayes_p4')
    log = log_frame({k[len('trainlog_'):]: v[cols['trainlog_u'] < 8] for k, v in cols.items() if k.startswith('trainlog_')})
    ag = BayesianAgentVB(Configuration({**bayesian_poly_args, 'num_products': 4, 'random_seed': 3, 'num_samples': 17}))
    ag.train_from_log(log)
    assert ag._ready().Lambda.shape == (17, 16)


def test_decisions_and_transpose():
    rng = np.random.RandomState(5)
    P, S = 6, 70
    lam = rng.randn(S, P * P)
    lam_t = bayes_transpose(lam, P)
    assert lam_t.shape == (P, P, S) and lam_t.flags['C_CONTIGUOUS']
    assert all(lam_t[p, a, s] == lam[s, p * P + a] for p in range(P) for a in range(P) for s in (0, 1, S - 1))
    prods, cnts = [0, 2, 5], [3, 1, 250]
    z = bayes_decisions(prods, cnts, lam_t)
    want = np.zeros((P, S))
    for a in range(P):
        for s in range(S):
            acc = 0.0
            for p, c in zip(prods, cnts):
                acc = acc + c * lam[s, p * P + a]
            want[a, s] = acc
    assert np.array_equal(z, want)
    X = np.zeros((1, P), dtype=np.int16)
    X[0, prods] = cnts
    a_ref, q_ref = reference_act(X, lam)
    M = bayes_abs_sum(prods, cnts, lam_t)
    assert M == max(sum(abs(c * lam[s, p * P + a]) for p, c in zip(prods, cnts)) for a in range(P) for s in range(S))
    assert np.abs(bayes_means(z) - q_ref).max() <= bayes_margin(len(prods), M, S)
    # the device's order of the sum: lanes over s, then the butterfly
    e = np.r_[expit(z[1]), np.zeros(128 - S)].reshape(2, 64)
    lanes = e[0] + e[1]
    o = 32
    while o:
        lanes = lanes[:o] + lanes[o:2 * o]
        o >>= 1
    assert bayes_means(z)[1] == lanes[0] / S


def test_margin_is_made_of_ieee_operations():
    u = 2.0 ** -53
    assert bayes_z_bound(1, 1.0) == 6 * u and bayes_z_bound(10, 250.0) == 24 * u * 250.0
    assert bayes_margin(1, 0.0, 1) == 46 * u and bayes_margin(10, 250.0, 1000) == 24 * u * 250.0 / 4 + 2044 * u
    assert 1e-13 < bayes_margin(10, 250.0, 1000) < 1e-12      # against natural gaps of 1e-7
    # 2 gamma_n M <= ez for every history length of a row
    for n in (1, 15, 255, 2 ** 20):
        g = n * u / (1 - n * u)
        assert 2 * g * 3.0 <= bayes_z_bound(n, 3.0)


@pytest.mark.parametrize('P', [2, 10, 65, 130])
def test_rule_on_placed_decisions(P):
    assert expit(39.0) == 1.0 and expit(36.0) < 1.0
    for name, z, want_a, want_fl in bu.placed(P):
        lam_t = np.zeros((P, P, 1))
        lam_t[0, :, 0] = z
        dec = bayes_decisions([0], [1], lam_t)
        assert np.array_equal(dec[:, 0], z), name
        M = bayes_abs_sum([0], [1], lam_t)
        assert M == np.abs(z).max()
        a, fl = bayes_rule(dec, 1, M)
        assert fl == want_fl and (want_a is None or a == want_a), (P, name, a, fl)
        if not fl & UNRESOLVED:
            assert a == int(np.argmax(expit(z))), (P, name)
    assert bayes_rule(np.zeros((P, 1)), 0, 0.0) == (0, 0)     # the empty history
    # a z error bound of 1 or more: unresolved outright, saturated or not
    big = np.full((P, 1), 45.0)
    assert bayes_z_bound(1, 2.0 ** 52) >= 1.0 and bayes_rule(big, 1, 2.0 ** 52)[1] == UNRESOLVED


def test_device_policy_is_none_where_only_the_host_is_exact():
    lam = np.zeros((3, 16))
    assert BayesianVBFrozenAgent(Configuration({'num_products': 4}), lam).device_policy() is not None
    assert BayesianVBFrozenAgent(Configuration({'num_products': 4, 'with_ps_all': True}), lam).device_policy() is None
    weighted = BayesianVBFrozenAgent(Configuration({'num_products': 4, 'weight_history_function': lambda dt: np.exp(-0.1 * dt)}), lam)
    assert weighted.device_policy() is None and weighted.history is not None
    # beyond the cap: P P S 8 bytes (a view of one zero: no memory behind it)
    P = 128
    S = MODEL_BYTES_CAP // (8 * P * P)
    huge = np.broadcast_to(np.zeros((1, 1)), (S + 1, P * P))
    ag = BayesianVBFrozenAgent.__new__(BayesianVBFrozenAgent)
    ag.config, ag.Lambda, ag.history = Configuration({'num_products': P}), huge, None
    assert huge.size * 8 > MODEL_BYTES_CAP and ag.device_policy() is None
    ag.Lambda = huge[:S]
    assert ag.device_policy() is not None
    bad = np.zeros((3, 16))
    bad[1, 2] = np.inf
    assert BayesianVBFrozenAgent(Configuration({'num_products': 4}), bad).device_policy() is None
    for a in (weighted, BayesianVBFrozenAgent(Configuration({'num_products': 4}), lam)):
        assert a.ope_policy() is None and a.ope_policy_checked() is None


def test_weighted_history_runs_on_the_host():
    """With a weight function the act's features are the time-weighted float sums (the reference's ViewsFeaturesProvider with history)."""
    rng = np.random.RandomState(2)
    P = 4
    lam = rng.randn(9, P * P)
    fn = lambda dt: np.exp(-0.3 * dt)       # noqa: E731
    ag = BayesianVBFrozenAgent(Configuration({'num_products': P, 'weight_history_function': fn}), lam)
    session = OrganicSessions()
    for t, v in ((0, 1), (1, 3), (2, 1)):
        session.next(DefaultContext(t, 0), v)
    act = ag.act(Observation(DefaultContext(3, 0), session), 0, False)
    X = np.zeros((1, P), dtype=np.float32)
    for t, v in ((0, 1), (1, 3), (2, 1)):
        X[0, v] += np.float32(fn(np.int16(3) - np.array([np.int16(t)]))[0])
    assert act['a'] == reference_act(ag.history.features(3).reshape(1, P), lam)[0] and act['ps'] == 1.0 and act['ps-a'] == ()
    assert np.allclose(ag.history.features(3), X, rtol=1e-6)
