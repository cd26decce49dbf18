"""The act list of the four model agents beyond one trip of the grid (rg_act_common.hpp: act_list_run).

The step loop's act kernels (k_poly_acts, k_bayes_acts, k_nn_acts, k_mlr_acts) walk lr_list[0 .. lr_cnt[t]) a wave per act,
grid-stride, under a grid capped at 8 blocks of 4 waves per CU.  The agents' fixtures have tens to hundreds of users: no wave of
theirs takes a second trip round the loop, and every block either has work in all its waves or returns before it stages.  Here a
population is sized from the device's CU count so that ONE step lists more acts than the grid has waves — asserted from the act
counter, step by step — and the run is held to the same users run as two shards that are each too small to reach the wave count:
the shards' log digests add up (modulo 2^64) to the whole run's, their counters sum to it, and their unresolved lists joined are
its list.  The host confirms the whole run's listed acts (poly_verify).

P = 10, synthetic models, lock-step (an event per launch).  Nearly every user enters the bandit state at event 1, with one view
behind it: that step lists about 0.9 N acts.  Every model is made to leave some acts unresolved and far fewer than the list
holds (asserted): the comparison of the lists is never one of empty lists."""
import numpy as np
import pytest

from recogym_amd import _abi
from recogym_amd.envs.configuration import Configuration
from recogym_amd.envs.reco_env_v1 import env_1_args

pytestmark = pytest.mark.gpu

P = 10
LIST_CAP = 4096                               # kPolyListCap: entries of the unresolved list
BLOCKS_PER_CU, WAVES_PER_BLOCK = 8, 4         # launch_model_acts' cap (capped_wave_grid(.., 8, CUs)), kBlock / 64
# short lives (a run of some 50 steps), and 0.9 of the organic users turn to the bandit state together
ENV = {**env_1_args, 'random_seed': 11, 'num_products': P, 'K': 5, 'prob_leave_organic': 0.05, 'prob_organic_to_bandit': 0.9,
       'prob_leave_bandit': 0.25, 'prob_bandit_to_organic': 0.5}
# the counters of the log's rows and of the acts (the float64-resolve counters follow the draw kernels' tiles, `step` is the clock)
ADDITIVE = ('organic', 'bandit', 'clicks', 'phantom', 'live', 'log_rows', 'log_dropped', 'hist_overflow', 'lr_acts', 'lr_rows',
            'poly_table', 'poly_unresolved', 'bayes_saturated')


def policy_of(agent):
    """The Simulator's policy arguments of a synthetic model of `agent`, made as the agent's own test file (or timing tool) makes its."""
    rng = np.random.RandomState(7)
    if agent == 'poly':
        # a dense model small enough that every decision stays inside |z| < 1.8, with two actions whose decisions differ by 2^-48
        # wherever the history's counts are equal: inside the margin W (at least 2^-48) and, at such z, some ulps of expit apart.
        # Where the two lead — about one act in a hundred — the higher index wins, the act is listed, and the host confirms it.
        wf, wa, wk = rng.standard_normal(P) * 0.02, rng.standard_normal(P) * 0.02, rng.standard_normal((P, P)) * 0.02
        wk[6] = wk[3]
        wa[3] -= 0.02 / 3
        wa[6] = (3 * wa[3] + 2.0 ** -48) / 6
        return dict(policy=_abi.RG_POLICY_LOGREG_POLY, policy_seed=0, logreg_poly=dict(wf=wf, wa=wa, wk=wk, intercept=0.1))
    if agent == 'bayes':
        # two actions with identical columns (test_bayes_vb_device.models' tie), far below the rest except on the rows of TWO viewed
        # products, each of which alone a decoy action wins: a history of just those two products in about equal counts — an act
        # or two in a hundred — ends in an exact tie of the two best means
        lam = rng.standard_normal((120, P, P)) * 0.05           # [sample][viewed product][action]
        top = rng.standard_normal((120, P)) * 0.05 - 0.5
        top[:, 4] += 0.7
        top[:, 7] += 0.7
        lam[:, :, 2] = top
        lam[:, :, P - 1] = top
        lam[:, 4, 0] += 0.39
        lam[:, 7, 0] -= 0.2
        lam[:, 7, 1] += 0.39
        lam[:, 4, 1] -= 0.2
        return dict(policy=_abi.RG_POLICY_BAYES_VB, policy_seed=0, bayes_vb=dict(lam=lam.reshape(120, P * P)))
    if agent == 'nn':
        import test_nn_ips_device as t
        return dict(policy=_abi.RG_POLICY_NN_IPS, policy_seed=0, nn_ips=dict(state=t.random_state(P, 20, rng, scale=2.0)))
    # integer weights: two scores tie exactly on a few histories in a thousand, so the list is not empty and far from its 4096 entries
    W = rng.randint(-64, 65, (P, P)).astype(np.float32)
    return dict(policy=_abi.RG_POLICY_MLR, policy_seed=0, mlr=dict(state=dict(W=W)))


def run(agent, first_user, n, by_hand=0):
    """Users [first_user, first_user + n) to their end -> digest, counters, the unresolved list sorted, poly_verify's verdict, and the
    largest increase of the act counter over the first `by_hand` steps (taken one rg_sim_step at a time)."""
    from recogym_amd.sim import Simulator
    sim = Simulator(Configuration(ENV), n, device='cuda:0', **policy_of(agent))
    try:
        sim.reset_users(first_user, n)
        most, acts = 0, 0
        for _ in range(by_hand):
            sim.step()
            now = sim.counters()['lr_acts']
            most, acts = max(most, now - acts), now
        sim.run()
        cnt = sim.counters()
        assert cnt['live'] == 0 and cnt['log_dropped'] == 0 and cnt['hist_overflow'] == 0, cnt
        stands = sim.poly_verify()
        listed = sim.poly_unresolved[np.lexsort(sim.poly_unresolved.T[::-1])]
        return dict(digest=sim.log_digest(), cnt=cnt, listed=listed, stands=stands and not sim.poly_overflow, most=most)
    finally:
        sim.close()


@pytest.mark.parametrize('agent', ['poly', 'bayes', 'nn', 'mlr'])
def test_a_step_beyond_the_grid_equals_its_shards(agent, monkeypatch):
    import torch
    from test_agent_run_forms import set_form
    set_form('lockstep', monkeypatch)
    waves = BLOCKS_PER_CU * WAVES_PER_BLOCK * torch.cuda.get_device_properties(0).multi_processor_count
    n = waves * 5 // 4 + 37                    # 0.9 n = 1.125 waves: the margin, waves / 8, is some thirty standard deviations of the binomial
    whole = run(agent, 0, n, by_hand=3)
    print(agent, 'waves', waves, 'users', n, 'most acts in a step', whole['most'], 'acts', whole['cnt']['lr_acts'], 'listed', len(whole['listed']))
    assert whole['most'] > waves, 'no step listed more acts than the grid has waves: the stride is not covered'
    assert whole['stands'], 'the host refutes a listed act, or the list overflowed'
    assert 0 < len(whole['listed']) < LIST_CAP, 'the run lists no unresolved act, or fills the list: the comparison of the lists is void'
    split = n // 2 - 11                        # two ragged shards; a step lists at most one act per user, so neither reaches the wave count
    shards = [run(agent, 0, split, by_hand=3), run(agent, split, n - split, by_hand=3)]
    for s, size in zip(shards, (split, n - split)):
        assert size < waves and s['most'] < waves and s['stands'], (size, s['most'], waves)
    assert [sum(s['digest'][i] for s in shards) % (1 << 64) for i in range(5)] == whole['digest']
    assert {k: sum(s['cnt'][k] for s in shards) for k in ADDITIVE} == {k: whole['cnt'][k] for k in ADDITIVE}
    joined = np.concatenate([s['listed'] for s in shards])
    assert np.array_equal(joined[np.lexsort(joined.T[::-1])], whole['listed'])
