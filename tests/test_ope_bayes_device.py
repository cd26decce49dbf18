"""Off-policy replay of BayesianAgentVB on the device (rg_ope_replay_bayes / rg_ope_replay_bayes_eg, recogym_amd/csrc/rg_ope_bayes.hip)
against the host loop of the same call (BayesianVBFrozenAgent.act through evaluate_agent._host_ips / _host_snips / _host_recall),
the host act on hand-made histories, bayes_util's placed decisions, and itself.  Every ratio, click, IPS term and sum is compared
bit for bit; the head words of the workspace prove that the device took the acts.  Needs a real MI355X."""
import numpy as np
import pytest
import torch
from scipy.special import expit

import bayes_util as bu
import golden_util as gu
import ope_models_util as mu
from make_golden_ope import log_frame
from recogym_amd import _abi
from recogym_amd.agents.bayesian_poly_vb import SATURATED, UNRESOLVED, BayesianVBFrozenAgent
from recogym_amd.sim import DeviceLog

pytestmark = pytest.mark.gpu
DEV = mu.DEV


def fixture_agent(name):
    meta, cols = gu.load(name)
    P = meta['env_args']['num_products']
    return BayesianVBFrozenAgent(mu.cfg(P), bu.fixture_lambda(meta, cols)), log_frame(cols)


def tie_agent(P=10, S=3):
    """Lambda = 0: every mean is exactly 0.5, the device lists the act, the reference's argmax is action 0."""
    return BayesianVBFrozenAgent(mu.cfg(P), np.zeros((S, P * P)))


# ---- 1. taken, not bypassed -----------------------------------------------------------------------------------------------------
def test_the_device_takes_the_acts_and_the_estimators_equal_the_host_loop():
    ag, df = fixture_agent('bayes_p10_s120')
    r, st = mu.estimators_equal_the_host_loop(ag, df)
    assert st['acts'] > 100 and st['rows_read'] >= st['acts']


# ---- 2. fixtures and simulator logs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', bu.FIXTURES)
def test_self_evaluation_of_the_fixtures(name):
    """The model that wrote the log evaluates it: pi = 1 and ps = 1 at every row."""
    ag, df = fixture_agent(name)
    r, st = mu.estimators_equal_the_host_loop(ag, df)
    assert bool((r == 1.0).all())


@pytest.mark.parametrize('sigma', [0.0, 0.1])
def test_simulator_logs_equal_the_host_loop(sigma):
    mu.sim_log_equals_the_host_loop(mu.bayes_agent(10, 120, seed=3), sigma)


# ---- 3. history tiers -------------------------------------------------------------------------------------------------------------
def test_history_sizes_round_the_tier_boundaries():
    st = mu.check(mu.tier_users(520), mu.bayes_agent(520, 3, seed=3, scale=0.3), 'tiers', all_resolved=True)
    assert st['rows_read'] >= 513 + 512 + 511


# ---- 4. chunk geometry ------------------------------------------------------------------------------------------------------------
def test_chunk_geometry():
    ag = mu.bayes_agent(65, 5, seed=4, scale=0.3)
    users = mu.geometry_users(65)
    assert len(users[4]) == 128 and len(users[5]) == 129 and len(users[6]) == 180 and users[2][60:70] == ['b'] * 10
    mu.check(users, ag, 'geometry')
    dl, _, _ = mu.build(users, ag)
    r, c, sums, st = mu.replay(ag, dl, n_users=0)
    assert r.size == 0 and sums.tolist() == [0.0, 0.0, 0.0] and st['acts'] == 0


# ---- 5. lane and stride edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', [4, 65])
def test_lane_and_stride_edges(P):
    users = mu.random_users(P, seed=P)
    for S in (1, 63, 64, 65, 130):
        mu.check(users, mu.bayes_agent(P, S, seed=P + S, scale=0.3), f'P = {P}, S = {S}')


@pytest.mark.parametrize('S', [1, 63, 64, 65, 130])
@pytest.mark.parametrize('P', [4, 65])
def test_placed_decisions_with_the_saturated_zone(P, S):
    """bayes_util.placed: user p views product p once, so z[a][s] = lam_t[p][a][s] exactly — every sample holds the placed vector.
    The placements whose expected action the reference's expression shares (a refuted act has its own test), the saturated ones
    first, P of them at most: the resolved ones need no host, the unresolved ones are confirmed through the list; the saturated head
    word counts the saturated placements.  The logged actions are the expected action, the largest decision's index and another."""
    def host(z):
        return int(np.argmax(expit(np.tile(z[:, None], (1, S))).mean(1)))
    cases = [c for c in bu.placed(P) if c[2] is not None and host(c[1]) == c[2]]
    cases = sorted(cases, key=lambda c: not c[3] & SATURATED)[:P]
    n_sat = sum(1 for c in cases if c[3] & SATURATED)
    assert n_sat >= 3 and (P == 4 or any(c[3] & UNRESOLVED for c in cases))
    Lambda = np.zeros((S, P * P))
    raw, want = np.zeros((4 * len(cases), 4), dtype=np.uint32), []
    for p, (name, z, want_a, want_fl) in enumerate(cases):
        Lambda[:, p * P:(p + 1) * P] = z[None, :]
        raw[4 * p:4 * p + 4, 0], raw[4 * p:4 * p + 4, 1], raw[4 * p, 2] = p, np.arange(4), p
        for t, a in enumerate((want_a, int(np.argmax(z)), (want_a + 1) % P)):
            raw[4 * p + 1 + t, 2] = a | _abi.RG_EV_BANDIT
            want.append(1.0 / 0.5 if a == want_a else 0.0)
    ag = BayesianVBFrozenAgent(mu.cfg(P), Lambda)
    for p, (name, z, want_a, _) in enumerate(cases):
        assert ag.act_on([p], [1]) == want_a, name
    dl = DeviceLog(torch.from_numpy(raw.view(np.int32)).to(DEV), torch.arange(0, 4 * len(cases) + 1, 4, dtype=torch.int64, device=DEV),
                   0.5, 0, P, None)
    r, _, _, st = mu.replay(ag, dl)
    print(st)
    mu.same(r, want)
    assert (st['acts'], st['saturated']) == (len(cases), n_sat)
    assert st['unresolved'] == sum(1 for c in cases if c[3] & UNRESOLVED) and not st['overflow']


# ---- 6. the unresolved protocol ---------------------------------------------------------------------------------------------------
def test_an_exact_tie_is_listed_and_the_host_confirms_action_0():
    mu.tie_stands(tie_agent())


def test_a_refuted_act_sends_the_estimators_to_the_host_loop(monkeypatch):
    mu.refuted_takes_the_host_loop(tie_agent(), monkeypatch, 'bayes_host_act')


def test_more_unresolved_acts_than_the_list_holds():
    mu.overflow_takes_the_host_loop(tie_agent())


# ---- 7. determinism and both ways in ----------------------------------------------------------------------------------------------
def test_two_replays_both_ways_in_and_two_shards_give_the_same_bits():
    mu.determinism_and_both_ways_in(mu.bayes_agent(10, 120, seed=3))


# ---- 8. the EG form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('epsilon,pure_new', [(0.0, False), (0.3, True), (0.3, False)])
def test_the_eg_form_equals_a_host_restatement(epsilon, pure_new):
    mu.eg_form(mu.bayes_agent(10, 120, seed=3), epsilon, pure_new)


# ---- 9. recall@k and the tables ---------------------------------------------------------------------------------------------------
def test_recall_and_the_tables_equal_the_host_loops(monkeypatch):
    """(Both agents in one dict: test_ope_nn_device.py.)"""
    mu.recall_and_tables({'bayes': mu.bayes_agent(10, 30, seed=4)}, monkeypatch)
