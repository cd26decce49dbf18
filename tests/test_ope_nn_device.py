"""Off-policy replay of NnIpsAgent's argmax form on the device (rg_ope_replay_nn / rg_ope_replay_nn_eg, recogym_amd/csrc/rg_ope_nn.hip)
against the host loop of the same call (NnIpsFrozenAgent.act through evaluate_agent._host_ips / _host_snips / _host_recall), the host
act on hand-made histories, and itself.  Every ratio, click, IPS term and sum is compared bit for bit; the head words of the
workspace prove that the device took the acts.  Needs a real MI355X."""
import numpy as np
import pytest
import torch

import golden_util as gu
import nn_ips_util as nu
import ope_models_util as mu
from make_golden_ope import log_frame
from recogym_amd import _abi
from recogym_amd import evaluate_agent as ev
from recogym_amd.agents.nn_ips import COUNT_CAP, NnIpsFrozenAgent
from recogym_amd.sim import DeviceLog

pytestmark = pytest.mark.gpu
DEV = mu.DEV


def fixture_agent(name):
    meta, cols = gu.load(name)
    P = meta['env_args']['num_products']
    return NnIpsFrozenAgent(mu.cfg(P), nu.fixture_state(meta, cols)), log_frame(cols)


def tie_agent(P=10, H=5):
    """W3 = 0, b3 = 0: every logit is exactly 0, the device lists the act, torch's argmax of the uniform softmax is action 0."""
    state = mu.nn_state(P, H, seed=1)
    state['w3'][:], state['b3'][:] = 0.0, 0.0
    return NnIpsFrozenAgent(mu.cfg(P), state)


def staged(P, H):
    """rg_ope_nn.hip's rule: the layer vectors of four waves and the three matrices within kNnStageBytes = 48 KB."""
    return 8 * (2 * 4 * H + 2 * P * H + H * H) <= 48 * 1024


# ---- 1. taken, not bypassed -----------------------------------------------------------------------------------------------------
def test_the_device_takes_the_acts_and_the_estimators_equal_the_host_loop():
    ag, df = fixture_agent('nn_ips_p10')
    r, st = mu.estimators_equal_the_host_loop(ag, df)
    assert st['acts'] > 100 and st['rows_read'] >= st['acts']


# ---- 2. fixtures and simulator logs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', nu.FIXTURES)
def test_self_evaluation_of_the_fixtures(name):
    """The net that wrote the log evaluates it: pi = 1 at every row, so the ratio is 1 / the logged ps."""
    ag, df = fixture_agent(name)
    r, st = mu.estimators_equal_the_host_loop(ag, df)
    ps = df['ps'][(df['z'] == 'bandit') & (df['u'] < df['u'].max())].to_numpy(dtype=np.float64)
    mu.same(r, 1.0 / ps)


@pytest.mark.parametrize('sigma', [0.0, 0.1])
def test_simulator_logs_equal_the_host_loop(sigma):
    mu.sim_log_equals_the_host_loop(mu.nn_agent(10, 20, seed=3), sigma)


# ---- 3. history tiers -------------------------------------------------------------------------------------------------------------
def test_history_sizes_round_the_tier_boundaries():
    st = mu.check(mu.tier_users(520), mu.nn_agent(520, 4, seed=3, scale=0.1), 'tiers', all_resolved=True)
    assert st['rows_read'] >= 513 + 512 + 511


def test_a_count_beyond_2_to_24_is_listed_and_confirmed():
    """One user that views product 2 2^24 + 1 times and product 0 once: the count is not an fp32 value, so nn_act itself flags the
    act; the host confirms it (torch rounds the count to 2^24: the same action under this net) and the replay stands.  (The size is
    the case: 2^24 + 1 views are 2^24 + 1 rows of one user, which one wave inserts one by one — about 7 s, most of it that walk.)"""
    P, n = 4, COUNT_CAP + 1
    rows = torch.zeros((n + 3, 4), dtype=torch.int32, device=DEV)
    rows[:, 1] = torch.arange(n + 3, dtype=torch.int32, device=DEV)
    rows[:n, 2] = 2
    ag = mu.nn_agent(P, 4, seed=5)
    a_host = ag.act_on([0, 2], [1, n])[0]
    for i, a in enumerate((a_host, (a_host + 1) % P)):
        rows[n + 1 + i, 2] = int(np.uint32(a | _abi.RG_EV_BANDIT).view(np.int32))
    dl = DeviceLog(rows, torch.tensor([0, n + 3], dtype=torch.int64, device=DEV), 0.5, 0, P, None)
    r, _, sums, st = mu.replay(ag, dl)
    print(st)
    assert (st['acts'], st['unresolved'], st['overflow'], st['rows_read']) == (1, 1, False, 2)
    mu.same(r, [2.0, 0.0])
    mu.same(sums, [2.0, 0.0, 2.0])


# ---- 4. chunk geometry ------------------------------------------------------------------------------------------------------------
def test_chunk_geometry():
    ag = mu.nn_agent(65, 33, seed=4, scale=0.3)
    users = mu.geometry_users(65)
    assert len(users[4]) == 128 and len(users[5]) == 129 and len(users[6]) == 180 and users[2][60:70] == ['b'] * 10
    mu.check(users, ag, 'geometry')
    dl, _, _ = mu.build(users, ag)
    r, c, sums, st = mu.replay(ag, dl, n_users=0)
    assert r.size == 0 and sums.tolist() == [0.0, 0.0, 0.0] and st['acts'] == 0


# ---- 5. lane and stride edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', [63, 64, 65, 129])
def test_lane_and_stride_edges(P):
    users = mu.random_users(P, seed=P)
    for H in (1, 33, 64, 65, 130):
        mu.check(users, mu.nn_agent(P, H, seed=P + H, scale=0.3), f'P = {P}, H = {H}, staged {staged(P, H)}')
    assert P != 65 or (staged(65, 33) and not staged(65, 64))


def test_a_placed_decision_past_the_lds_opt_in():
    """H = 1024: 64 KB of layer vectors beside 28 KB of static LDS.  With W1 = W2 = 0 and zero biases both hidden layers are exactly
    0.5, so z[a] = 0.5 sum_k w3[a][k] + b3[a]: 512 x 2^-9 = 1 on top of b3 = (0, 1, 2.5, 2) for action 1 alone -> z = (0, 2, 2.5, 2)."""
    P, H = 4, 1024
    assert 8 * 2 * 4 * H + 28 * 1024 > 64 * 1024
    state = {k: np.zeros_like(v) for k, v in mu.nn_state(P, H, seed=0).items()}
    state['b3'][:] = [0.0, 1.0, 2.5, 2.0]
    state['w3'][1, :] = 2.0 ** -9
    ag = NnIpsFrozenAgent(mu.cfg(P), state)
    assert ag.act_on([3], [1])[0] == 2
    st = mu.check([[('o', 3), 'b', 'b', ('o', 0), 'b'], [('o', 1), 'b']], ag, 'H = 1024')
    assert st['acts'] == 3


# ---- 6. the unresolved protocol ---------------------------------------------------------------------------------------------------
def test_an_exact_tie_is_listed_and_the_host_confirms_action_0():
    mu.tie_stands(tie_agent())


def test_a_refuted_act_sends_the_estimators_to_the_host_loop(monkeypatch):
    mu.refuted_takes_the_host_loop(tie_agent(), monkeypatch, 'nn_host_act')


def test_more_unresolved_acts_than_the_list_holds():
    mu.overflow_takes_the_host_loop(tie_agent())


# ---- 7. determinism and both ways in ----------------------------------------------------------------------------------------------
def test_two_replays_both_ways_in_and_two_shards_give_the_same_bits():
    mu.determinism_and_both_ways_in(mu.nn_agent(10, 20, seed=3))


# ---- 8. the EG form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('epsilon,pure_new', [(0.0, False), (0.3, True), (0.3, False)])
def test_the_eg_form_equals_a_host_restatement(epsilon, pure_new):
    mu.eg_form(mu.nn_agent(10, 20, seed=3), epsilon, pure_new)


# ---- 9. recall@k and the tables ---------------------------------------------------------------------------------------------------
def test_recall_and_the_tables_equal_the_host_loops(monkeypatch):
    mu.recall_and_tables({'nn': mu.nn_agent(10, 20, seed=3), 'bayes': mu.bayes_agent(10, 30, seed=4)}, monkeypatch)
