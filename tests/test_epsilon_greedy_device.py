"""EpsilonGreedy inside the device step loop and its off-policy replay (rg_sim_set_epsilon_greedy, rg_eg_explore_actions,
rg_ope_replay_eg) against logs of the reference's own EpsilonGreedy (tests/golden/eg_*.npz, tests/make_golden_eg.py), NumPy's
choice arithmetic, and the host forms of the same agents."""
import ctypes as C

import numpy as np
import pytest
import torch

from device_util import HostOnly, handle
import eg_util as eu
import golden_util as gu
import recogym_amd as recogym
from make_golden_ope import log_frame
from recogym_amd import _abi
from recogym_amd import evaluate_agent as ev
from recogym_amd.agents import (EpsilonGreedy, LastViewTableAgent, OrganicCount, OrganicUserEventCounterAgent, RandomAgent,
                                epsilon_greedy_args, organic_count_args, organic_user_count_args)
from recogym_amd.agents.epsilon_greedy import explore_table
from recogym_amd.envs.configuration import Configuration
from recogym_amd.envs.reco_env_v1 import env_1_args, rows_to_dataframe
from recogym_amd.sim import Simulator

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (options, the kernel that acts): an event per launch, run-ahead rounds, and the defaults (the tail kernel at these populations)
MODES = (dict(tail_below=0, run_ahead=0), dict(tail_below=0, run_ahead=32), dict())


def run(cfg, n, pol, options=(), first=0, n_users=None, organic_only_below=0):
    sim = Simulator(cfg, n, device=DEV, **{k: v for k, v in pol.items() if k != 'ps_all'})
    for k, v in dict(options).items():
        sim.set_option(k, v)
    sim.reset_users(first, n if n_users is None else n_users, organic_only_below=organic_only_below)
    sim.run()
    return sim


def run_fixture(name, options=(), first_user=0, n_users=None, organic_only_below=0):
    """-> meta, cols, the Simulator after its run (the caller closes it)"""
    meta, cols, P = eu.load(name)
    pol = eu.wrapper(meta, cols, P).device_policy()
    assert pol is not None and pol['epsilon_greedy']['epsilon'] == meta['eg_args']['epsilon']
    n = meta['n_users'] if n_users is None else n_users
    return meta, cols, run(gu.env_config(meta), n, pol, options, first_user, organic_only_below=organic_only_below)


def assert_log_is_the_fixture(what, meta, cols, rows, sims):
    """The rows of a run of the fixture's users held to it (`sims`: the Simulators that ran them; of several: their rows concatenated)."""
    is_b = cols['z'] == 1
    last = np.r_[cols['u'][1:] != cols['u'][:-1], True]
    gu.assert_rows_equal(rows, cols, ps_rtol=0, what=what)
    assert np.array_equal(eu.bits(rows['ps'][is_b]), eu.bits(cols['ps'][is_b])), f'{what}: ps bits'
    assert np.array_equal(rows['phantom'] != 0, is_b & last), 'the phantom row is every user\'s last'
    for sim in sims:
        assert sim.aux_ps is not None and not sim.uniform_ps            # the float64 side array is on by default
        if meta['env_args']['sigma_omega'] == 0.0:
            # the overlay has no walked form: the run stayed in the lock-step kernels
            with pytest.raises(_abi.RecoGymHipError, match='no walked run'):
                sim.walk_fate()
            assert sim.counters()['memo_hits'] == 0


@pytest.mark.parametrize('name', eu.LOG_FIXTURES)
def test_device_log_equals_the_reference_fixture(name):
    for options in MODES:
        meta, cols, sim = run_fixture(name, options)
        assert_log_is_the_fixture(f'{name} {options}', meta, cols, sim.rows(), [sim])
        sim.close()
    if name == 'eg_p1000_k20_table_sigma0':
        # (the same inner policy alone IS walked at this shape — BASELINE config 2's table: the check above means something)
        pol = eu.wrapper(meta, cols, meta['env_args']['num_products']).device_policy()
        plain = run(gu.env_config(meta), meta['n_users'], {k: v for k, v in pol.items() if k != 'epsilon_greedy'})
        plain.walk_fate()
        plain.close()


def _numpy_choice(P, pure_new, g, u):
    """rng.choice(P, p = product_probas) for the uniforms u, product_probas built as epsilon_greedy.py:38-42 builds them."""
    p = np.ones(P)
    if pure_new:
        p[g] = 0.0
    p = p / np.sum(p)
    cdf = p.cumsum()
    cdf /= cdf[-1]
    return cdf, cdf.searchsorted(u, side='right')


@pytest.mark.parametrize('pure_new', [True, False])
@pytest.mark.parametrize('P', [2, 3, 65, 1000, 4097])
def test_explore_search_equals_numpy_choice(P, pure_new):
    lib = _abi.load()
    r = np.random.RandomState(P)
    gs = np.arange(P) if P <= 65 else np.unique(np.r_[0, 1, P // 2, P - 2, P - 1, r.randint(0, P, size=24)])
    u_all, g_all, want = [], [], []
    for g in gs:
        cdf, _ = _numpy_choice(P, pure_new, g, 0.0)
        vals = cdf if P <= 65 else np.r_[cdf[[0, 1, g - 1 if g else 0, g, min(g + 1, P - 1), P - 2, P - 1]], cdf[r.randint(0, P, size=48)]]
        u = np.r_[0.0, 1.0 - 2.0 ** -53, vals, np.nextafter(vals, 0.0), np.nextafter(vals, 2.0), r.random_sample(16)]
        u = u[(u >= 0.0) & (u < 1.0)]
        u_all.append(u)
        g_all.append(np.full(u.size, g, dtype=np.int32))
        want.append(_numpy_choice(P, pure_new, g, u)[1])
    u_all, g_all, want = np.concatenate(u_all), np.concatenate(g_all), np.concatenate(want)
    assert want.max() <= P - 1 and (not pure_new or (want != g_all).all())
    d_cdf = torch.from_numpy(explore_table(P, pure_new)[0]).to(DEV)
    d_u, d_g = torch.from_numpy(u_all).to(DEV), torch.from_numpy(g_all).to(DEV)
    out = torch.full((u_all.size,), -1, dtype=torch.int32, device=DEV)
    assert lib.rg_eg_explore_actions(P, int(pure_new), d_cdf.data_ptr(), d_u.data_ptr(), d_g.data_ptr(), u_all.size, out.data_ptr(),
                                     None) == 0, lib.rg_last_error()
    got = out.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(int(g_all[i]), float(u_all[i]).hex(), int(got[i]), int(want[i])) for i in bad[:8]]


def _pair(kind, P, eps=0.3, eg_seed=7, pure_new=True):
    """(the wrapper that logs, the same wrapper with with_ps_all on both agents)"""
    table = np.random.RandomState(P).randint(0, P, size=P)
    def inner(all_):
        if kind == 'random':
            return RandomAgent(Configuration({'num_products': P, 'random_seed': 19, 'with_ps_all': all_}))
        return LastViewTableAgent(Configuration({'num_products': P, 'with_ps_all': all_}), table)
    def eg(all_):
        return EpsilonGreedy(Configuration({**epsilon_greedy_args, 'epsilon': eps, 'random_seed': eg_seed, 'epsilon_pure_new': pure_new,
                                            'num_products': P, 'with_ps_all': all_}), inner(all_))
    return eg(False), eg(True)


@pytest.mark.parametrize('kind', ['random', 'table'])
@pytest.mark.parametrize('P', [10, 1000])
def test_self_replay_gives_ratio_one_and_the_hosts_branches(kind, P):
    n = 300
    cfg = Configuration({**env_1_args, 'random_seed': 77, 'num_products': P, 'K': 5, 'prob_leave_bandit': 0.05, 'prob_leave_organic': 0.05})
    logger, target = _pair(kind, P)
    sim = run(cfg, n, logger.device_policy())
    dl = sim.device_log()
    assert not isinstance(dl.ps, float)
    out = {}
    r, c, sums = ev.ope_replay(target, dl, n_users=n, eg_out=out)
    assert r.numel() > 1000 and bool((r == 1.0).all())
    assert float(sums[0].item()) == r.numel() == float(sums[2].item())
    greedy, h0 = ev.epsilon_greedy_branches(target, sim)
    assert torch.equal(greedy, out['greedy']) and torch.equal(h0, out['h0'])
    rows = sim.rows()
    keep = rows['u'] < 60
    acts = eu.host_acts(logger, {k: rows[k][keep] for k in ('u', 't', 'z', 'v')})
    m = len(acts)
    assert m > 200 and np.array_equal(greedy.cpu().numpy()[:m], np.array([x['greedy'] for x in acts], dtype=np.uint8))
    # h0 is the inner action on every row: the reference reports it on explored acts, where it differs from `a`
    assert np.array_equal(h0.cpu().numpy()[:m], np.array([x['h0'] if not x['greedy'] else x['a'] for x in acts]))
    assert 0.2 < 1.0 - float(greedy.float().mean().item()) < 0.4
    sim.close()


@pytest.mark.parametrize('name', eu.OPE_FIXTURES)
def test_estimators_on_a_frame_equal_the_reference_and_the_host_loop(name, monkeypatch):
    meta, want, P = eu.load(name)
    _, cols = gu.load(meta['log'])
    df = log_frame(cols)
    df = df[df['u'] <= 150]
    target = eu.wrapper(meta, want, P, with_ps_all=True)
    assert ev.ope_policy_of(target) is not None
    c, ratio = ev.evaluate_SNIPS(target, df)
    m = len(ratio)
    assert m > 1000 and np.array_equal(eu.bits(ratio), eu.bits(want['ratio'][:m])) and np.array_equal(np.asarray(c, dtype=np.float64), want['c'][:m])
    ips = ev.evaluate_IPS(target, df)
    assert np.array_equal(eu.bits(ips), eu.bits(want['c'][:m] * want['ratio'][:m]))
    agents = {'eg': target, 'random': RandomAgent(Configuration({'num_products': P, 'random_seed': 5, 'with_ps_all': True}))}
    t_ips, t_snips = ev.verify_agents_IPS(df, agents), ev.verify_agents_SNIPS(df, agents)
    monkeypatch.setattr(ev, '_device_present', lambda: False)         # the same calls through the host loop
    assert ev.evaluate_SNIPS(target, df)[1] == list(ratio)
    assert t_ips.equals(ev.verify_agents_IPS(df, agents)) and t_snips.equals(ev.verify_agents_SNIPS(df, agents))


def test_estimators_on_a_device_log_equal_the_host_loop():
    P, n = 10, 250
    cfg = Configuration({**env_1_args, 'random_seed': 12, 'num_products': P, 'K': 5, 'prob_leave_bandit': 0.05, 'prob_leave_organic': 0.05})
    logger, _ = _pair('table', P, eps=0.5, eg_seed=3)
    sim = run(cfg, n, logger.device_policy())            # a log with full support: EpsilonGreedy at eps = 0.5, pure_new
    df = rows_to_dataframe(sim.rows(), P)
    for kind, pure_new in (('random', True), ('table', False), ('table', True)):
        _, target = _pair(kind, P, eps=0.3, eg_seed=9, pure_new=pure_new)
        c_dev, r_dev = ev.evaluate_SNIPS(target, sim)
        c_host, r_host = ev._host_snips(target, df)
        assert np.array_equal(eu.bits(r_dev.cpu().numpy()), eu.bits(r_host)) and np.array_equal(c_dev.cpu().numpy(), np.asarray(c_host, dtype=np.float64))
        ips = ev.evaluate_IPS(target, sim.device_log())
        assert np.array_equal(eu.bits(ips.cpu().numpy()), eu.bits(ev._host_ips(target, df)))
        assert np.isfinite(r_host).all()
    sim.close()


def test_shards_concatenate_and_runs_repeat():
    P, n = 10, 400
    cfg = Configuration({**env_1_args, 'random_seed': 5, 'num_products': P, 'K': 5, 'prob_leave_bandit': 0.05, 'prob_leave_organic': 0.05})
    inner = OrganicUserEventCounterAgent(Configuration({**organic_user_count_args, 'num_products': P, 'random_seed': 4}))
    pol = EpsilonGreedy(Configuration({**epsilon_greedy_args, 'epsilon': 0.3, 'random_seed': 8, 'num_products': P}), inner).device_policy()
    def log(first, count):
        sim = run(cfg, count, pol, first=first)
        rows, offsets = sim.sorted_log()
        ps, _ = sim.sorted_aux(offsets, rows.shape[0])
        out = rows.cpu().numpy().copy(), ps.cpu().numpy().copy()
        sim.close()
        return out
    whole, again = log(0, n), log(0, n)
    assert whole[0].tobytes() == again[0].tobytes() and whole[1].tobytes() == again[1].tobytes()
    a, b = log(0, 150), log(150, n - 150)
    assert np.array_equal(np.concatenate([a[0], b[0]]), whole[0])
    assert np.concatenate([a[1], b[1]]).tobytes() == whole[1].tobytes()


def test_test_agent_on_the_device_equals_the_per_user_host_path():
    env = recogym.make('reco-gym-v1')
    env.init_gym({**recogym.env_1_args, 'random_seed': 42, 'num_products': 10})
    def agent():
        return EpsilonGreedy(Configuration({**epsilon_greedy_args, 'epsilon': 0.2, 'random_seed': 6, 'num_products': 10}),
                             OrganicCount(Configuration({**organic_count_args, 'num_products': 10})))
    assert agent().device_policy()['policy'] == _abi.RG_POLICY_LAST_VIEW_TABLE
    got = recogym.test_agent(env, agent(), 200, 200)
    want = recogym.test_agent(env, HostOnly(agent()), 200, 200)
    assert got == want
    # clicks and impressions themselves, on the evaluation users of that call
    trained = agent()
    cnt, sim = env.simulate(200, None)
    trained.train_from_log(sim.device_log())
    sim.close()
    cnt, sim = env.simulate(200, trained, first_user_id=200, log=False)
    sim.close()
    df = env.generate_logs(200, HostOnly(trained), first_user_id=200)
    b = df[df['z'] == 'bandit']
    assert (cnt['clicks'], cnt['bandit'] + cnt['phantom']) == (int(b['c'].sum()), len(b))


def test_error_paths():
    table = torch.from_numpy(explore_table(10, True)[0]).to(DEV)
    for policy in (_abi.RG_POLICY_UNIFORM_ENV, _abi.RG_POLICY_EXTERNAL, _abi.RG_POLICY_LOGREG_FROZEN):
        lib, h, ws = handle(policy)
        assert lib.rg_sim_set_epsilon_greedy(h, 0.1, 7, 1, table.data_ptr(), 0.1 / 9, 0.9) == -1 and b'EpsilonGreedy wraps' in lib.rg_last_error()
        lib.rg_sim_destroy(h)
    lib, h, ws = handle(_abi.RG_POLICY_RANDOM_AGENT)
    for eps in (-0.01, 1.01, float('nan')):
        assert lib.rg_sim_set_epsilon_greedy(h, eps, 7, 1, table.data_ptr(), 0.0, 0.0) == -1 and b'epsilon' in lib.rg_last_error()
    assert lib.rg_sim_set_epsilon_greedy(h, 0.1, 7, 1, None, 0.1 / 9, 0.9) == -1 and b'NULL' in lib.rg_last_error()
    assert lib.rg_sim_set_epsilon_greedy(h, 0.1, 7, 1, table.data_ptr(), 0.1 / 9, 0.9) == 0
    lib.rg_sim_destroy(h)
    lib, h, ws = handle(_abi.RG_POLICY_RANDOM_AGENT, P=1)
    assert lib.rg_sim_set_epsilon_greedy(h, 0.1, 7, 1, table.data_ptr(), 0.1, 0.9) == -1 and b'at least 2' in lib.rg_last_error()
    assert lib.rg_sim_set_epsilon_greedy(h, 0.1, 7, 0, table.data_ptr(), 0.1, 0.9) == 0          # without pure_new one product is enough
    lib.rg_sim_destroy(h)
    # after rg_sim_reset_users: RG_ESTATE
    cfg = Configuration({**env_1_args, 'random_seed': 1, 'num_products': 10, 'K': 5})
    sim = Simulator(cfg, 32, device=DEV, policy=_abi.RG_POLICY_RANDOM_AGENT, policy_seed=3)
    sim.reset_users(0, 32)
    assert sim.lib.rg_sim_set_epsilon_greedy(sim._h, 0.1, 7, 1, table.data_ptr(), 0.1 / 9, 0.9) == -4 and b'before rg_sim_reset_users' in sim.lib.rg_last_error()
    sim.close()
    with pytest.raises(_abi.RecoGymHipError, match='EpsilonGreedy wraps'):
        Simulator(cfg, 32, device=DEV, epsilon_greedy=dict(epsilon=0.1, seed=7, pure_new=True))            # agent=None inside
    # the stateless entry points
    out = torch.zeros(4, dtype=torch.int32, device=DEV)
    u = torch.zeros(4, dtype=torch.float64, device=DEV)
    assert lib.rg_eg_explore_actions(1, 1, table.data_ptr(), u.data_ptr(), out.data_ptr(), 4, out.data_ptr(), None) == -1
    assert lib.rg_eg_explore_actions(10, 1, None, u.data_ptr(), out.data_ptr(), 4, out.data_ptr(), None) == -1
    sim = run(cfg, 40, dict(policy=_abi.RG_POLICY_RANDOM_AGENT, policy_seed=3))
    dl = sim.device_log()
    n, total = 39, int(dl.offsets[39].item())
    ratio = torch.zeros(total, dtype=torch.float64, device=DEV)
    sums = torch.zeros(3, dtype=torch.float64, device=DEV)
    def replay(kind, eps=0.1, pure_new=1, P=10, table=None, ws_bytes=None):
        inner = _abi.RgOpePolicy(kind=kind, num_products=P, policy_seed=3, ouc_select_randomly=1, ouc_exploit_explore=1,
                                 ouc_reverse_pop=0, reserved=0, ouc_epsilon=0.0, table=table)
        eg = _abi.RgOpeEg(epsilon=eps, seed=7, pure_new=pure_new, reserved=0, prob_explore=1.0 / 9)
        need = lib.rg_ope_eg_workspace_bytes(C.byref(inner), n, 4096)
        ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
        return lib.rg_ope_replay_eg(C.byref(inner), C.byref(eg), dl.rows.data_ptr(), dl.offsets.data_ptr(), n, 4096, _abi.RG_OPE_PS_CONST,
                                    None, 0.1, ratio.data_ptr(), None, sums.data_ptr(), None, None, ws.data_ptr(),
                                    need if ws_bytes is None else ws_bytes, None)
    assert replay(_abi.RG_POLICY_RANDOM_AGENT) == 0
    for kind in (_abi.RG_POLICY_ORGANIC_USER_COUNT, _abi.RG_POLICY_LOGREG_FROZEN, _abi.RG_POLICY_UNIFORM_ENV):
        assert replay(kind) == -1 and b'no replay form' in lib.rg_last_error()
    assert replay(_abi.RG_POLICY_LAST_VIEW_TABLE) == -1 and b'null table' in lib.rg_last_error()
    assert replay(_abi.RG_POLICY_RANDOM_AGENT, eps=1.5) == -1 and b'epsilon' in lib.rg_last_error()
    assert replay(_abi.RG_POLICY_RANDOM_AGENT, P=1) == -1 and b'at least 2' in lib.rg_last_error()
    assert replay(_abi.RG_POLICY_RANDOM_AGENT, ws_bytes=8) == -3
    sim.close()


def test_logs_that_do_not_qualify_go_to_the_host_loop():
    P = 10
    _, target = _pair('random', P)
    # a float clock: the target always draws, and its draw key is the event index
    from recogym_amd.envs.features.time import NormalTimeGenerator
    tg = NormalTimeGenerator(Configuration({'normal_time_mu': 0.0, 'normal_time_sigma': 1.0}))
    cfg = Configuration({**env_1_args, 'random_seed': 3, 'num_products': P, 'K': 5, 'time_generator': tg,
                         'prob_leave_bandit': 0.05, 'prob_leave_organic': 0.05})
    sim = run(cfg, 60, dict(policy=_abi.RG_POLICY_RANDOM_AGENT, policy_seed=3))
    dl = sim.device_log()
    assert dl.time is not None and ev.ope_replay(target, dl) is None and ev.epsilon_greedy_branches(target, dl) is None
    df = ev._device_log_to_frame(dl)
    assert ev._frame_to_device(df, ev.ope_policy_of(target), torch.device(DEV)) is None
    got = ev.evaluate_SNIPS(target, df)
    assert isinstance(got[1], list) and got[1] == ev._host_snips(target, df)[1]
    sim.close()
    # an OrganicUserEventCounter inside: no replay form
    cfg = Configuration({**env_1_args, 'random_seed': 3, 'num_products': P, 'K': 5, 'prob_leave_bandit': 0.05, 'prob_leave_organic': 0.05})
    sim = run(cfg, 60, dict(policy=_abi.RG_POLICY_RANDOM_AGENT, policy_seed=3))
    ouc = EpsilonGreedy(Configuration({**epsilon_greedy_args, 'epsilon': 0.3, 'random_seed': 7, 'num_products': P, 'with_ps_all': True}),
                        OrganicUserEventCounterAgent(Configuration({**organic_user_count_args, 'num_products': P, 'random_seed': 4,
                                                                   'with_ps_all': True})))
    assert ev.ope_policy_of(ouc) is None and ev._device_or_none(ouc, sim) is None
    c, r = ev.evaluate_SNIPS(ouc, sim)
    assert isinstance(r, list) and len(r) > 100 and np.isfinite(r).all()
    sim.close()
