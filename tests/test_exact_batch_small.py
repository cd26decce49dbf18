"""The float64 batch of a walked run (k_exact_sums_h in its vector and matrix forms, k_exact_sums_m) at the smallest shapes where
it can go wrong, against the oracle in Philox mode: sigma_omega = 0, 600 users — two full groups of 256 and a partial one —,
every one of them parked.

K = 3, 20, 32: register blocks of 1, 5 and 8 and the k < K mask (K = 20 is the widest shape whose Gamma rows the vector form
keeps two at a time in scalar registers, K = 32 takes the other loop).  P = 100: 28 padded products with mu = -inf inside the
last 64-product chunk; P = 192: none; P = 640 (K = 20 only): work items of more than one chunk, so that the vector form's row
prefetch crosses a chunk's end.  exact_mix = 0, 1, 8: every group in the vector form, one matrix group beside two vector groups in
the same launch, every group in the matrix form (that one is k_exact_sums_m's launch: the ledger shows which).

Every organic draw of a user takes one uniform (rg_sim_debug_set_uniforms) at a boundary of the user's own float64 cdf, computed
in NumPy the way the oracle does (reco_env_v1.py:119-128), off it by 1e-9 relative in one set and by 1e-12 in the other, half the
users to each side: no 16-bit or fp32 certificate holds there, so every user parks at its first draw and float64 decides.  omega
is the oracle's own, handed to the run through rg_sim_debug_set_omega, so that the cdf the uniforms were placed on is the one the
run sums.  What such a run must log follows from the oracle as in tests/test_park_compact.py: every view of a user is the
float64 decision v* of its uniform, the OrganicUserEventCounter policy's counts sit on v* alone, its act is v* with ps = 1, and
the oracle's environment stepped with that action gives the transitions, the clicks and the phantom row."""
import functools

import numpy as np
import pytest
import torch

import adversarial_util as au
import golden_util as gu
from history_model import ROW_DTYPE
from recogym_amd import _abi
from recogym_amd.envs.configuration import Configuration
from recogym_amd.envs.reco_env_v1 import env_1_args
from test_hip_parity import assert_walk_pipe

pytestmark = pytest.mark.gpu

N = 600
POL = dict(policy=_abi.RG_POLICY_ORGANIC_USER_COUNT, policy_seed=31, ouc=dict(gu.OUC_DEFAULTS))
COLS = ('u', 't', 'z', 'v', 'a', 'c', 'ps')
WALK_ENV = ('RECOGYM_DRAW', 'RECOGYM_WALK', 'RECOGYM_WALK_HANDOVER', 'RECOGYM_PIPE_MIN', 'RECOGYM_XH', 'RECOGYM_XH_WAVES', 'RECOGYM_PIPE',
            'RECOGYM_SLICES', 'RECOGYM_BF16', 'RECOGYM_EXACT_MIX')
SHAPES = [(100, 3), (192, 3), (100, 20), (192, 20), (640, 20), (100, 32), (192, 32)]
# (exact_mix, run form): 'walk' = run_walk (the host reads the list's length), 'pipe' = run_walk_pipe (the dense list, lengths on
# the device; it has no all-matrix form: exact_mix = 8 is run_walk's)
FORMS = [(0, 'walk'), (1, 'walk'), (8, 'walk'), (0, 'pipe'), (1, 'pipe')]
CASES = [(P, K, mix, form) for P, K in SHAPES for mix, form in FORMS if form == 'walk' or K <= 20]     # (run_walk_pipe: K <= 20, k_sweep_xh)


def config(P, K):
    return Configuration({**env_1_args, 'random_seed': 5100 + P + K, 'num_products': P, 'K': K, 'sigma_omega': 0.0})


@functools.lru_cache(maxsize=None)
def reference(P, K, eps):
    """(omega, uniform per user, rows the run must log, the oracle's counters of them); once per shape and offset, read-only."""
    from oracle import oracle as orc
    cfg = config(P, K)
    env = orc.OracleEnv(cfg, rng_mode=orc.RNG_PHILOX, **POL)
    gamma, mu_o = env.tables[0], env.tables[1]
    omega = np.zeros((N, K))
    for user in range(N):
        env.reset(user)
        omega[user] = env.omega
    rng = np.random.RandomState(1000 + P + K)
    logits = omega @ gamma.T + np.asarray(mu_o).reshape(1, -1)
    logits -= logits.max(axis=1, keepdims=True)
    e = np.exp(logits)
    cdf = np.cumsum(e / e.sum(axis=1, keepdims=True), axis=1)
    cdf /= cdf[:, -1:]
    rows_i = np.arange(N)
    sign = np.where(rows_i % 2 == 0, -1.0, 1.0)                        # half the users to each side of their boundary
    # a boundary per user, drawn by mass, then moved on (cyclically) to the first one whose product on the offset's side is heavier
    # than four offsets, so that the uniform's distance to the nearest boundary IS the offset
    mass = np.diff(cdf, axis=1, prepend=0.0)
    b = np.zeros(N, dtype=np.int64)
    for i in range(N):
        k = min(max(int(np.searchsorted(cdf[i], rng.random_sample(), 'right')), 0), P - 2)
        while mass[i, k + (sign[i] > 0)] <= 4.0 * eps * cdf[i, k]:
            k = (k + 1) % (P - 1)
        b[i] = k
    u = cdf[rows_i, b] * (1.0 + sign * eps)
    v = np.array([np.searchsorted(cdf[i], u[i], 'right') for i in range(N)])
    lo = np.where(v > 0, cdf[rows_i, np.maximum(v - 1, 0)], -np.inf)
    hi = np.where(v < P - 1, cdf[rows_i, np.minimum(v, P - 1)], np.inf)
    margin = np.minimum(u - lo, hi - u) / u
    assert (margin > 0.99 * eps).all() and (margin < 1.01 * eps).all(), (margin.min(), margin.max())
    assert (v == b + (sign > 0)).all()                                 # the decision is the side the offset names
    out = []
    for user in range(N):
        a = int(v[user])
        env.reset(user)
        org, _, done = env.step(None)
        while True:
            out += [(user, r['t'], 0, a, -1, -1, np.nan, 0) for r in org]
            t = env.time
            if done:
                out.append((user, t, 1, -1, a, 0, 1.0, 1))
                break
            org, reward, done = env.step(a)
            out.append((user, t, 1, -1, a, reward, 1.0, 0))
    rows = np.array(out, dtype=ROW_DTYPE)
    ban = (rows['z'] == 1) & (rows['phantom'] == 0)
    oc = dict(organic=int((rows['z'] == 0).sum()), bandit=int(ban.sum()), clicks=int(rows['c'][ban].sum()), phantom=N)
    for x in (omega, u, rows):
        x.setflags(write=False)
    return omega, u, rows, oc


def walked(P, K, omega, u):
    """One run of the N users under the environment the caller has set -> rows, counters, ledger."""
    from recogym_amd.sim import Simulator
    sim = Simulator(config(P, K), N, device='cuda:0', p_click=False, **POL)
    sim.reset_users(0, N)
    d_om = torch.from_numpy(np.array(omega)).to('cuda:0')
    d_u = torch.from_numpy(np.array(u)).to('cuda:0')
    _abi.check(sim.lib.rg_sim_debug_set_omega(sim._h, d_om.data_ptr(), sim._stream()), 'debug_set_omega')
    _abi.check(sim.lib.rg_sim_debug_set_uniforms(sim._h, d_u.data_ptr()), 'debug_set_uniforms')
    sim.run()
    torch.cuda.synchronize()
    _abi.check(sim.lib.rg_sim_debug_set_uniforms(sim._h, None), 'debug_set_uniforms')
    rows, cnt, led = sim.rows(), sim.counters(), au.ledger(sim)
    led['exact_mix'], led['batch_users'] = sim.get_option('exact_mix'), sim.get_option('batch_users')
    sim.close()
    return rows, cnt, led


@pytest.mark.parametrize('P,K,mix,form', CASES)
def test_every_parked_user_gets_the_float64_decision(P, K, mix, form, monkeypatch):
    for k in WALK_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('RECOGYM_EXACT_MIX', str(mix))
    if form == 'pipe':
        monkeypatch.setenv('RECOGYM_PIPE_MIN', '256')
    for eps in (1e-9, 1e-12):
        omega, u, want, oc = reference(P, K, eps)
        rows, cnt, led = walked(P, K, omega, u)
        what = f'P={P} K={K} exact_mix={mix} {form} eps={eps:g}'
        print(f'{what}: exact_h {led["exact_h"]}, exact_m {led["exact_m"]}, exact_sweeps {cnt["exact_sweeps"]}, exact_draws {cnt["exact_draws"]}')
        assert led['exact_mix'] == mix
        if form == 'pipe':
            assert_walk_pipe(led)
        elif mix < 8:
            assert led['exact_h'] >= 1 and led['exact_m'] == 0 and led['walk2'] >= 2, led
        else:       # every group in the matrix form is k_exact_sums_m's launch (rg_host.hip, run_walk)
            assert led['exact_m'] >= 1 and led['exact_h'] == 0 and led['walk2'] >= 2, led
        # Every user is on the batch's list: parked at its first draw (counted as a sweep), or handed over by a wave left with
        # fewer live lanes than the hand-over threshold (the ragged last wave of 600 users).  No certificate of the 16-bit and
        # fp32 sums reaches within 1e-9 of a boundary (rho >= 2^-23), so float64 decided every organic draw of the run.
        assert led['batch_users'] == N if form == 'pipe' else led['batch_users'] >= N, led
        assert N // 2 < cnt['exact_sweeps'] <= N and cnt['exact_draws'] == oc['organic'], cnt
        gu.assert_rows_equal(rows, {k: want[k] for k in COLS}, ps_rtol=1e-12, what=what)
        assert (rows['phantom'] == want['phantom']).all()
        assert (cnt['organic'], cnt['bandit'], cnt['clicks'], cnt['phantom']) == (oc['organic'], oc['bandit'], oc['clicks'], oc['phantom'])
        assert cnt['live'] == 0 and cnt['exact_overflow'] == 0 and cnt['hist_overflow'] == 0 and cnt['log_dropped'] == 0
