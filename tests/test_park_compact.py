"""The dense list between round 1 and the float64 batch of run_walk_pipe (k_park_compact), against the oracle in Philox mode:
sigma_omega = 0, 4 096 users, the OrganicUserEventCounter policy, RECOGYM_PIPE_MIN = 256 so that run_walk_pipe serves them.  Rows
(u, t, z, v, a, c) and the phantom flag exact, ps to 1e-12.

"Adversarial": every organic draw of a user takes one uniform (rg_sim_debug_set_uniforms) placed next to a boundary of the user's
own float64 cdf as tests/adversarial_util.py places it — a boundary drawn by mass, u = cdf[b] (1 +- eps), eps from 1e-9 to
3e-3 — but on the omega the environment itself draws, so that the oracle's environment can be stepped beside it.  The oracle
takes no uniforms from outside; what such a run must log follows from it all the same: every view of a user is the float64
decision v* of its uniform, so the policy's counts sit on v* alone and its act is v* with ps = 1 whatever its own draw, and the
oracle's environment stepped with that action (history_model.py steps it the same way) gives the transitions, clicks and the
phantom row.  A user whose uniform is closer than 1e-11 (relative) to a boundary — two float64 cdfs may differ there — gets the
middle of its product's interval instead (or of its heaviest product's), so that every row can be held exact.
"Clear": the same hook with every user's uniform in the middle of its heaviest product's interval: every draw certifies.
"Addressed": the draws as the run addresses them by (seed, user, t), the oracle's own log as the reference."""
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

N = 4096
POL = dict(policy=_abi.RG_POLICY_ORGANIC_USER_COUNT, policy_seed=31, ouc=dict(gu.OUC_DEFAULTS))
COLS = ('u', 't', 'z', 'v', 'a', 'c', 'ps')
WALK_ENV = ('RECOGYM_DRAW', 'RECOGYM_WALK', 'RECOGYM_WALK_HANDOVER', 'RECOGYM_PIPE_MIN', 'RECOGYM_XH', 'RECOGYM_XH_WAVES', 'RECOGYM_PIPE',
            'RECOGYM_SLICES', 'RECOGYM_BF16')


def config(P, K):
    return Configuration({**env_1_args, 'random_seed': 8800 + P + K, 'num_products': P, 'K': K, 'sigma_omega': 0.0})


@functools.lru_cache(maxsize=None)
def adversarial_reference(P, K, clear=False):
    """(uniform per user, rows the run must log, the oracle's counters of them); computed once per shape, read-only."""
    from oracle import oracle as orc
    cfg = config(P, K)
    env = orc.OracleEnv(cfg, rng_mode=orc.RNG_PHILOX, **POL)
    gamma, mu_o = env.tables[0], env.tables[1]
    omega = np.zeros((N, K))
    for user in range(N):
        env.reset(user)
        omega[user] = env.omega
    # adversarial_util.reference's placement (reco_env_v1.py:119-128 in float64)
    rng = np.random.RandomState(77 + P)
    logits = omega @ gamma.T + np.asarray(mu_o).reshape(1, -1)
    logits -= logits.max(axis=1, keepdims=True)
    e = np.exp(logits)
    cdf = np.cumsum(e / e.sum(axis=1, keepdims=True), axis=1)
    cdf /= cdf[:, -1:]
    rows_i = np.arange(N)
    b = np.clip(np.array([np.searchsorted(cdf[i], rng.random_sample(), 'right') for i in range(N)]), 0, P - 2)
    eps = 10.0 ** rng.uniform(-9, -2.5, N)
    sign = rng.choice([-1.0, 1.0], N)
    u = np.clip(cdf[rows_i, b] * (1.0 + sign * eps), 0.0, np.nextafter(1.0, 0.0))
    heavy = np.argmax(np.diff(cdf, axis=1, prepend=0.0), axis=1)       # (a product too light for that: the user's heaviest one's)
    if clear:
        u = 0.5 * (np.where(heavy > 0, cdf[rows_i, np.maximum(heavy - 1, 0)], 0.0) + cdf[rows_i, heavy])
    for attempt in range(3):
        v = np.array([np.searchsorted(cdf[i], u[i], 'right') for i in range(N)])
        lo = np.where(v > 0, cdf[rows_i, np.maximum(v - 1, 0)], 0.0)
        hi = np.where(v < P - 1, cdf[rows_i, np.minimum(v, P - 1)], 1.0)
        margin = np.minimum(u - np.where(v > 0, lo, -np.inf), np.where(v < P - 1, hi, np.inf) - u) / np.maximum(u, 1e-300)
        if attempt == 1:
            lo, hi = np.where(heavy > 0, cdf[rows_i, np.maximum(heavy - 1, 0)], 0.0), cdf[rows_i, heavy]
        u = np.where(margin > 1e-11, u, 0.5 * (lo + hi))
    assert (margin > 1e-11).all() and (clear or (margin < 5e-7).sum() > N // 8), ((margin <= 1e-11).sum(), (margin < 5e-7).sum())
    assert not clear or (margin > 1e-3).all()
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
    for x in (u, rows):
        x.setflags(write=False)
    return u, rows, oc


@functools.lru_cache(maxsize=None)
def oracle_log(P, K):
    from oracle import oracle as orc
    env = orc.OracleEnv(config(P, K), rng_mode=orc.RNG_PHILOX, **POL)
    rows = env.generate_logs(N)
    rows.setflags(write=False)
    return rows, env.counters()


def walked(P, K, u=None, digest=False):
    """One run of the N users under the environment the caller has set -> rows, counters, the ledger with the last run's list
    counts, the order-independent digest where asked for."""
    from recogym_amd.sim import Simulator
    sim = Simulator(config(P, K), N, device='cuda:0', p_click=False, **POL)
    sim.reset_users(0, N)
    if u is not None:
        d_u = torch.from_numpy(np.array(u)).to('cuda:0')
        _abi.check(sim.lib.rg_sim_debug_set_uniforms(sim._h, d_u.data_ptr()), 'debug_set_uniforms')
    sim.run()
    torch.cuda.synchronize()
    _abi.check(sim.lib.rg_sim_debug_set_uniforms(sim._h, None), 'debug_set_uniforms')
    rows, cnt, led = sim.rows(), sim.counters(), au.ledger(sim)
    for k in ('launched_park_compact', 'park_slots', 'park_users', 'handed_over', 'batch_users'):
        led[k] = sim.get_option(k)
    dig = sim.log_digest() if digest else None
    sim.close()
    print(f'P={P} K={K}: ' + ', '.join(f'{k} {led[k]}' for k in ('park_slots', 'park_users', 'handed_over', 'batch_users')) +
          f', exact_sweeps {cnt["exact_sweeps"]}, exact_draws {cnt["exact_draws"]}')
    return rows, cnt, led, dig


def pipe_env(monkeypatch, **extra):
    for k in WALK_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('RECOGYM_PIPE_MIN', '256')
    for k, v in extra.items():
        monkeypatch.setenv(k, v)


def assert_exact(rows, cnt, want, oc, what):
    gu.assert_rows_equal(rows, {k: want[k] for k in COLS}, ps_rtol=1e-12, what=what)
    assert (rows['phantom'] == want['phantom']).all()
    assert (cnt['organic'], cnt['bandit'], cnt['clicks'], cnt['phantom']) == (oc['organic'], oc['bandit'], oc['clicks'], oc['phantom'])
    assert cnt['live'] == 0 and cnt['exact_overflow'] == 0 and cnt['hist_overflow'] == 0 and cnt['log_dropped'] == 0


def reference(P, K, draws):
    """(uniforms or None, rows, counters) the run must reproduce"""
    if draws == 'addressed':
        return (None,) + oracle_log(P, K)
    return adversarial_reference(P, K, draws == 'clear')


def assert_dense(led, cnt):
    """k_park_compact served the run, and its counts agree with the list round 1 left and with what round 2 counted."""
    assert led['launched_park_compact'] == 1
    assert led['park_users'] >= 0 and led['handed_over'] >= 0 and led['batch_users'] == led['park_users'] + led['handed_over']
    assert led['park_slots'] >= led['batch_users'] and led['park_slots'] % 64 == 0
    assert cnt['exact_sweeps'] == led['park_users']         # (round 2 counts a sweep per listed user with the pend bit)


@pytest.mark.parametrize('draws', ['adversarial', 'addressed'])
@pytest.mark.parametrize('P,K', [(640, 7), (3000, 20)])
def test_parked_and_handed_over_users_reach_the_batch_through_the_dense_list(P, K, draws, monkeypatch):
    """The default hand-over: users of both kinds, a list with unused entries between them."""
    pipe_env(monkeypatch)
    u, want, oc = reference(P, K, draws)
    rows, cnt, led, _ = walked(P, K, u)
    assert_walk_pipe(led)
    assert_dense(led, cnt)
    assert led['park_users'] > 0 and led['handed_over'] > 0 and cnt['exact_draws'] > 0
    assert_exact(rows, cnt, want, oc, f'dense list P={P} K={K} {draws}')


@pytest.mark.parametrize('P,K', [(640, 7), (545, 13)])
def test_nearly_everything_handed_over(P, K, monkeypatch):
    """RECOGYM_WALK_HANDOVER = 64, addressed draws: a wave of round 1 finds its queue empty at its first refill and hands over
    every user it still has, so only the users whose FIRST draw was uncertified (parked before that refill) carry the pend bit.
    P = 545: a ragged table."""
    pipe_env(monkeypatch, RECOGYM_WALK_HANDOVER='64')
    u, want, oc = reference(P, K, 'addressed')
    rows, cnt, led, _ = walked(P, K, u)
    assert_walk_pipe(led)
    assert_dense(led, cnt)
    assert led['batch_users'] <= N and led['handed_over'] > N // 2 > led['park_users']
    assert_exact(rows, cnt, want, oc, f'all handed over P={P} K={K}')


def test_nothing_parked_leaves_only_handed_over_users(monkeypatch):
    """(P, K) = (33, 3).  Addressed draws park 3 of the 4 096 users there (9 float64 draws), and every larger shape of the suite
    parks more, so the case takes the hook instead: clear draws, every one certified, no user parked — the dense list holds
    handed-over users only and round 2 counts no sweep."""
    pipe_env(monkeypatch)
    P, K = 33, 3
    u, want, oc = reference(P, K, 'clear')
    rows, cnt, led, _ = walked(P, K, u)
    assert_walk_pipe(led)
    assert_dense(led, cnt)
    assert cnt['exact_draws'] == 0 and led['park_users'] == 0 and led['handed_over'] > 0
    assert_exact(rows, cnt, want, oc, 'nothing parked')


@pytest.mark.parametrize('draws', ['adversarial', 'addressed'])
def test_the_log_is_that_of_the_host_counted_run(draws, monkeypatch):
    """The order-independent digest of the first mixed shape equals that of RECOGYM_PIPE = 0 (run_walk: host-side counts, no
    dense list) on the same users and uniforms."""
    P, K = 640, 7
    u = adversarial_reference(P, K)[0] if draws == 'adversarial' else None
    pipe_env(monkeypatch)
    _, cnt_p, led_p, dig_p = walked(P, K, u, digest=True)
    assert_walk_pipe(led_p)
    assert_dense(led_p, cnt_p)
    pipe_env(monkeypatch, RECOGYM_PIPE='0')
    _, cnt_h, led_h, dig_h = walked(P, K, u, digest=True)
    assert led_h['launched_park_compact'] == 0 and led_h['sweep_xh'] == 0 and led_h['walk2'] >= 2, led_h
    assert (led_h['park_users'], led_h['handed_over']) == (-1, -1) and led_h['batch_users'] == led_h['park_slots'] > 0
    assert dig_p == dig_h
    assert all(cnt_p[k] == cnt_h[k] for k in ('organic', 'bandit', 'clicks', 'phantom'))
