"""The HIP-event profile of a run (rg_sim_set_profiling / rg_sim_get_profile): what each of its buckets holds, for the three
ways rg_sim_run goes to the end — run_walk, run_walk_pipe, and lock-step rounds handed to k_tail.  Needs a real MI355X."""
import math
import time

import pytest
import torch

import adversarial_util as au
from recogym_amd.envs.configuration import Configuration
from recogym_amd.envs.reco_env_v1 import env_1_args

pytestmark = pytest.mark.gpu

P, K, N_USERS = 500, 20, 2000
# the buckets whose intervals lie one after the other on the run's stream (tail_ms includes both walk rounds)
DISJOINT = ('draw_mfma_ms', 'draw_search_ms', 'draw_exact_ms', 'logreg_ms', 'advance_ms', 'tail_ms')


@pytest.mark.parametrize('form', ['run_walk', 'run_walk_pipe', 'drifting'])
def test_profile_buckets_of_a_run_to_the_end(form, monkeypatch):
    """sigma_omega = 0 as it comes (run_walk), with RECOGYM_PIPE_MIN=256 (run_walk_pipe), and sigma_omega = 0.1 (rounds, then
    k_tail).  A walked run is one step whose walk rounds are the whole of tail_ms; a drifting run counts a step per advance
    launch and has no walk time; and in every form the buckets, disjoint intervals of one stream, fit into the host's wall
    time around run() (5 % + 1 ms for the clocks' disagreement) — a larger sum means an interval was counted twice."""
    from recogym_amd.sim import Simulator
    for k in ('RECOGYM_DRAW', 'RECOGYM_WALK', 'RECOGYM_PIPE', 'RECOGYM_PIPE_MIN', 'RECOGYM_SLICES', 'RECOGYM_TAIL', 'RECOGYM_RUN_AHEAD'):
        monkeypatch.delenv(k, raising=False)
    if form == 'run_walk_pipe':
        monkeypatch.setenv('RECOGYM_PIPE_MIN', '256')
    cfg = Configuration({**env_1_args, 'random_seed': 321, 'num_products': P, 'K': K,
                         'sigma_omega': 0.1 if form == 'drifting' else 0.0})
    sim = Simulator(cfg, N_USERS, device='cuda:0')
    sim.reset_users(0, N_USERS)
    sim.set_profiling(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sim.run()
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3
    prof = sim.profile()
    led = au.ledger(sim)
    launched = {k: sim.get_option('launched_' + k) for k in ('advance', 'advance_run', 'tail')}
    sim.close()
    print(form, 'wall_ms', wall_ms, prof, launched)

    assert len(prof) == 9
    for k, v in prof.items():
        assert math.isfinite(v) and v >= 0, (k, prof)
    if form == 'drifting':
        assert led['walk'] == led['walk2'] == led['walk_solo'] == 0, led
        assert prof['steps'] == launched['advance'] + launched['advance_run'] > 0, (prof, launched)
        assert prof['walk1_ms'] == 0 == prof['walk2_ms'], prof
        assert prof['advance_ms'] > 0, prof
        assert (prof['tail_ms'] > 0) == (launched['tail'] > 0), (prof, launched)
    else:
        assert (led['sweep_xh'] > 0) == (form == 'run_walk_pipe') and led['walk2'] >= 1, led
        assert launched['advance'] == launched['advance_run'] == launched['tail'] == 0, launched
        assert prof['steps'] == 1, prof
        assert prof['walk1_ms'] > 0 and prof['draw_mfma_ms'] > 0, prof
        assert prof['advance_ms'] == 0 == prof['logreg_ms'], prof
        assert prof['tail_ms'] == pytest.approx(prof['walk1_ms'] + prof['walk2_ms'], rel=1e-9, abs=0), prof
    total = sum(prof[k] for k in DISJOINT)
    assert total <= wall_ms * 1.05 + 1.0, (total, wall_ms, prof)
