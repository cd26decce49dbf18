"""EpsilonGreedy round the frozen LogReg argmax and the likelihood agent inside the device step loop and in the off-policy replay
(rg_sim_set_epsilon_greedy_model, rg_ope_replay_logreg_eg, rg_ope_replay_poly_eg) against logs of the reference's own wrapper round
its own trained models (tests/golden/model_eg_*.npz, tests/make_golden_eg_models.py) and this package's host route.  Every
comparison is bit for bit, except the two tables of means whose sums torch and NumPy take in different orders (bound stated
there).  Needs a real MI355X."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch
from scipy.special import expit

from device_util import HostOnly, assert_frames_equal, constant_agent, handle, make_env
import eg_models_util as mu
import eg_util as eu
import golden_util as gu
from make_golden_ope import log_frame
from recogym_amd import _abi
from recogym_amd import evaluate_agent as ev
from recogym_amd.agents import (EpsilonGreedy, LastViewTableAgent, LogregFrozenAgent, LogregPolyFrozenAgent, RandomAgent,
                                epsilon_greedy_args)
from recogym_amd.agents.epsilon_greedy import explore_table
from recogym_amd.agents.logreg_poly import poly_margin
from recogym_amd.envs.configuration import Configuration
from recogym_amd.envs.reco_env_v1 import env_1_args, rows_to_dataframe
from recogym_amd.sim import Simulator, poly_device_model

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# test_epsilon_greedy_device.MODES: an event per launch, run-ahead rounds, and the defaults
MODES = (dict(tail_below=0, run_ahead=0), dict(tail_below=0, run_ahead=32), dict())
EG = dict(epsilon=0.3, random_seed=7)


def run(cfg, n, pol, options=(), first_user=0, organic_only_below=0):
    sim = Simulator(cfg, n, device=DEV, **{k: v for k, v in pol.items() if k != 'ps_all'})
    for k, v in dict(options).items():
        sim.set_option(k, v)
    sim.reset_users(first_user, n, organic_only_below=organic_only_below)
    sim.run()
    return sim


def run_fixture(name, options=(), first_user=0, n_users=None, organic_only_below=0):
    meta, cols, P = mu.load(name)
    pol = mu.wrapper(meta, cols, P).device_policy()
    assert pol is not None and pol['epsilon_greedy']['epsilon'] == meta['eg_args']['epsilon']
    return meta, cols, P, run(gu.env_config(meta), meta['n_users'] if n_users is None else n_users, pol, options, first_user, organic_only_below)


def same(a, b):
    assert np.array_equal(eu.bits(a), eu.bits(b))


# ---- (a) the device log against the fixture --------------------------------------------------------------------------------
def assert_log_is_the_fixture(what, meta, cols, rows, cnt):
    """The rows and counters of a run of the fixture's users (of several runs: rows concatenated, counters summed) held to it."""
    is_b = cols['z'] == 1
    last = np.r_[cols['u'][1:] != cols['u'][:-1], True]
    gu.assert_rows_equal(rows, cols, ps_rtol=0, what=what)
    assert np.array_equal(eu.bits(rows['ps'][is_b]), eu.bits(cols['ps'][is_b])), f'{what}: ps bits'
    assert np.array_equal(rows['phantom'] != 0, is_b & last), 'the phantom row is every user\'s last'
    census = meta['census']
    print(what, {k: cnt[k] for k in ('lr_acts', 'lr_rows', 'poly_table', 'poly_unresolved')}, census)
    assert cnt['lr_acts'] == census['acts'], what
    if meta['inner'] == 'poly':
        assert cnt['poly_table'] == census['table'] and cnt['poly_unresolved'] == census['unresolved'] == 0, what
    assert cnt['live'] == 0 and cnt['log_dropped'] == 0 and cnt['hist_overflow'] == 0, what


@pytest.mark.parametrize('name', mu.LOG_FIXTURES)
def test_device_log_equals_the_reference_fixture(name):
    for options in MODES:
        meta, cols, P, sim = run_fixture(name, options)
        rows, cnt = sim.rows(), sim.counters()
        sim.close()
        assert_log_is_the_fixture(f'{name} {options}', meta, cols, rows, cnt)


# ---- (b) the branches ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', mu.LOG_FIXTURES)
def test_branches_and_self_replay(name):
    meta, cols, P, sim = run_fixture(name)
    target = mu.wrapper(meta, cols, P, with_ps_all=True)
    is_b = cols['z'] == 1
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        greedy, h0 = ev.epsilon_greedy_branches(target, sim)
        out, stats = {}, {}
        r, c, sums = ev.ope_replay(target, sim.device_log(), n_users=meta['n_users'], eg_out=out, stats=stats)
    sim.close()
    want_greedy, want_h0, a = cols['greedy'][is_b], cols['h0'][is_b], cols['a'][is_b]
    greedy, h0 = greedy.cpu().numpy(), h0.cpu().numpy()
    assert np.array_equal(greedy, want_greedy.astype(np.uint8))
    # h0 is the model's action on every row: the reference reports it on explored acts only, a greedy act took it
    assert np.array_equal(h0, np.where(want_greedy == 1, a, want_h0))
    assert int((greedy == 0).sum()) == meta['census']['explored']
    assert torch.equal(out['greedy'].cpu(), torch.from_numpy(greedy)) and torch.equal(out['h0'].cpu(), torch.from_numpy(h0))
    # the log replayed under the wrapper that wrote it: pi is the logged propensity, the same float64 product
    assert r.numel() == int(is_b.sum()) and bool((r == 1.0).all())
    assert float(sums[0].item()) == r.numel() == float(sums[2].item())
    assert np.array_equal(c.cpu().numpy(), cols['c'][is_b].astype(np.float64))
    assert stats['acts'] == meta['census']['acts'] and stats['error'] == 0
    if meta['inner'] == 'poly':
        assert stats['table'] == meta['census']['table'] and stats['unresolved'] == 0 and not stats['overflow']


# ---- (c) the estimators ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', mu.OPE_FIXTURES)
def test_estimators_on_a_frame_equal_the_reference(name):
    meta, want, P = mu.load(name)
    df = log_frame(gu.load(meta['log'])[1])
    target = mu.wrapper(meta, want, P, with_ps_all=True)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        assert ev._device_or_none(target, df) is not None          # the device route
        c, ratio = ev.evaluate_SNIPS(target, df)
        ips = ev.evaluate_IPS(target, df)
    assert len(ratio) == len(want['ratio']) > 20000
    same(ratio, want['ratio'])
    assert np.array_equal(np.asarray(c, dtype=np.float64), want['c'])
    same(ips, want['c'] * want['ratio'])


def table_logger(P, eps=0.5, seed=3):
    table = np.random.RandomState(P).randint(0, P, size=P)
    return EpsilonGreedy(Configuration({**epsilon_greedy_args, 'epsilon': eps, 'random_seed': seed, 'num_products': P}),
                         LastViewTableAgent(Configuration({'num_products': P}), table))


def targets(with_ps_all=True, **over):
    out = {}
    for name in ('model_eg_poly_p10', 'model_eg_logreg_p10_hidden_classes', 'model_eg_logreg_p10_not_pure_new'):
        meta, cols, P = mu.load(name)
        out[name[len('model_eg_'):]] = mu.wrapper(meta, cols, P, with_ps_all=with_ps_all, **over)
    return out


def test_verify_agents_on_a_device_log_equal_the_host_loop(monkeypatch):
    """The rows behind the tables are the host loop's bit for bit.  The tables hold means and standard errors of n < 2^15
    non-negative float64 terms, summed by torch on one side and by NumPy on the other: each sum is within n 2^-53 relative of
    the exact one whatever its order, so the entries agree to 2^15 2^-52 < 1e-11 of the largest entry of their row."""
    P, n = 10, 250
    cfg = Configuration({**env_1_args, 'random_seed': 12, 'num_products': P, 'K': 5, 'prob_leave_bandit': 0.05, 'prob_leave_organic': 0.05})
    sim = run(cfg, n, table_logger(P).device_policy())            # a log with full support: EpsilonGreedy at eps = 0.5, pure_new
    dl = sim.device_log()
    df = rows_to_dataframe(sim.rows(), P)
    agents = {**targets(), 'random': RandomAgent(Configuration({'num_products': P, 'random_seed': 5, 'with_ps_all': True}))}
    assert int(((dl.rows[:, 2] & _abi.RG_EV_BANDIT) != 0).sum()) < 2 ** 15
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        got = [ev.verify_agents_SNIPS(dl, agents), ev.verify_agents_IPS(sim, agents)]
        ratios = {k: ev.evaluate_SNIPS(a, dl) for k, a in agents.items()}
        ips = {k: ev.evaluate_IPS(a, dl) for k, a in agents.items()}
    sim.close()
    monkeypatch.setattr(ev, '_device_present', lambda: False)
    for k, a in agents.items():
        assert torch.is_tensor(ratios[k][1])
        c_host, r_host = ev._host_snips(a, df)
        same(ratios[k][1].cpu().numpy(), r_host)
        assert np.array_equal(ratios[k][0].cpu().numpy(), np.asarray(c_host, dtype=np.float64)) and np.isfinite(r_host).all()
        same(ips[k].cpu().numpy(), ev._host_ips(a, df))
    want = [ev.verify_agents_SNIPS(df, agents), ev.verify_agents_IPS(df, agents)]
    for g, w in zip(got, want):
        assert list(g['Agent']) == list(w['Agent']) == list(agents)
        gv, wv = g[['0.025', '0.500', '0.975']].to_numpy(dtype=np.float64), w[['0.025', '0.500', '0.975']].to_numpy(dtype=np.float64)
        print(gv, wv)
        assert (np.abs(gv - wv) <= 1e-11 * np.abs(wv).max(axis=1, keepdims=True)).all()


def test_a_float_clock_goes_to_the_host_loop():
    from recogym_amd.envs.features.time import NormalTimeGenerator
    P = 10
    tg = NormalTimeGenerator(Configuration({'normal_time_mu': 0.0, 'normal_time_sigma': 1.0}))
    cfg = Configuration({**env_1_args, 'random_seed': 3, 'num_products': P, 'K': 5, 'time_generator': tg,
                         'prob_leave_bandit': 0.05, 'prob_leave_organic': 0.05})
    sim = run(cfg, 40, dict(policy=_abi.RG_POLICY_RANDOM_AGENT, policy_seed=3))
    dl = sim.device_log()
    df = ev._device_log_to_frame(dl)
    sim.close()
    for target in targets().values():
        assert dl.time is not None and ev.ope_replay(target, dl) is None and ev.epsilon_greedy_branches(target, dl) is None
        pol = ev.ope_policy_of(target) or ev.ope_checked_policy_of(target)
        assert pol is not None and ev._frame_to_device(df, pol, torch.device(DEV)) is None
        got = ev.evaluate_SNIPS(target, df)
        assert isinstance(got[1], list) and got[1] == ev._host_snips(target, df)[1]


# ---- (d) small shapes against this package's host route --------------------------------------------------------------------
def logs(env, n, agent):
    """generate_logs on the device route (no warning: nothing was refuted) and on the per-user host route"""
    assert agent.device_policy() is not None
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        got = env.generate_logs(n, agent)
    want = env.generate_logs(n, HostOnly(agent))
    assert_frames_equal(got, want)
    return got


SMALL = dict(random_seed=99, num_products=10, K=4, prob_leave_bandit=0.05, prob_leave_organic=0.05)


@pytest.mark.parametrize('name', ['model_eg_poly_p10', 'model_eg_logreg_p10'])
def test_epsilon_0_is_the_unwrapped_model_and_epsilon_1_never_takes_it(name):
    meta, cols, P = mu.load(name)
    env, n = make_env(SMALL), 70
    plain = logs(env, n, mu.inner_agent(meta, cols, P))
    got = logs(env, n, mu.wrap(mu.inner_agent(meta, cols, P), P, dict(EG, epsilon=0.0)))
    assert_frames_equal(got, plain)
    ps = got['ps'].to_numpy(dtype=np.float64, na_value=np.nan)[(got['z'] == 'bandit').to_numpy()]
    same(ps, np.full(ps.size, (1.0 - 0.0) * 1.0))
    # epsilon = 1 with pure_new: every act explores and none logs the model's action
    agent = mu.wrap(mu.inner_agent(meta, cols, P), P, dict(EG, epsilon=1.0))
    got = logs(env, n, agent)
    cnt, sim = env.simulate(n, agent)
    greedy, h0 = ev.epsilon_greedy_branches(mu.wrap(mu.inner_agent(meta, cols, P, True), P, dict(EG, epsilon=1.0), with_ps_all=True), sim)
    sim.close()
    a = got['a'][got['z'] == 'bandit'].to_numpy(dtype=np.int64)
    assert a.size == greedy.numel() > 300 and not bool(greedy.any()) and (a != h0.cpu().numpy()).all()
    assert len(set(h0.cpu().numpy().tolist())) > 1
    ps = got['ps'].to_numpy(dtype=np.float64, na_value=np.nan)[(got['z'] == 'bandit').to_numpy()]
    same(ps, np.full(ps.size, 1.0 * explore_table(P, True)[1]))


def two_product_models(with_ps_all=False):
    """(LogReg argmax, likelihood agent) over two products whose action depends on HOW MANY views the user has, whichever product
    they went to (a two-product environment may show one product only): LogReg scores 1.0 against 0.4 (views), the likelihood agent
    decides on z[0] = 0 against z[1] = -1.25 + 0.5 (a count) per viewed product — no ties, multiples of 0.25 far outside the
    rule's margin."""
    cfg = Configuration({'num_products': 2, 'with_ps_all': with_ps_all})
    wk = np.array([[0.0, 0.0], [0.5, 0.5]])
    return (LogregFrozenAgent(cfg, np.array([[0.0, 0.0], [0.4, 0.4]]), np.array([1.0, 0.0]), np.array([0, 1])),
            LogregPolyFrozenAgent(cfg, np.r_[np.zeros(2), [0.0, -1.25], wk.reshape(-1)][None, :], [0.0]))


@pytest.mark.parametrize('which', [0, 1])
def test_two_products_with_pure_new_explore_the_other_one(which):
    env, n = make_env({**SMALL, 'num_products': 2}), 70
    eg_args = dict(EG, epsilon=0.5)
    agent = mu.wrap(two_product_models()[which], 2, eg_args)
    got = logs(env, n, agent)
    cnt, sim = env.simulate(n, agent)
    greedy, h0 = ev.epsilon_greedy_branches(mu.wrap(two_product_models(True)[which], 2, eg_args, with_ps_all=True), sim)
    sim.close()
    greedy, h0 = greedy.cpu().numpy(), h0.cpu().numpy()
    a = got['a'][got['z'] == 'bandit'].to_numpy(dtype=np.int64)
    assert a.size == greedy.size > 300 and 0.3 < greedy.mean() < 0.7 and len(set(h0.tolist())) == 2
    assert np.array_equal(a, np.where(greedy == 1, h0, 1 - h0))
    ps = got['ps'].to_numpy(dtype=np.float64, na_value=np.nan)[(got['z'] == 'bandit').to_numpy()]
    same(ps, np.where(greedy == 1, (1.0 - 0.5) * 1.0, 0.5 * 1.0))


# ---- (e) the unresolved-act protocol under the wrapper ---------------------------------------------------------------------
OVER = dict(random_seed=321, num_products=10, K=4)
CONFIRMED = (25.0, 25.0 + 2.0 ** -12)              # inside W(z2) = 4.9e-4, far beyond one step of expit: the host confirms action 2


def refuted_pair():
    z1 = 25.0
    z2 = next(z for z in (z1 + 2.0 ** -e for e in range(20, 46)) if expit(z) == expit(z1))      # scipy merges them: the host acts 1
    assert z2 > z1 and int(np.argmax(expit(np.array([0.0, z1, z2])))) == 1
    return z1, z2


def test_an_unresolved_greedy_act_the_host_confirms_keeps_the_device_route():
    assert 0 < CONFIRMED[1] - CONFIRMED[0] <= poly_margin(CONFIRMED[1])
    agent = mu.wrap(constant_agent(*CONFIRMED), 10, EG)
    sim = run(Configuration({**env_1_args, **OVER}), 60, agent.device_policy())
    cnt = sim.counters()
    assert sim.poly_verify() and not sim.poly_overflow
    # the list holds the GREEDY act of every act, explored ones included
    assert len(sim.poly_unresolved) == cnt['poly_unresolved'] == cnt['lr_acts'] > 60 and len(sim.poly_refuted) == 0
    assert (sim.poly_unresolved[:, 2] == 2).all()
    target = mu.wrap(constant_agent(*CONFIRMED, with_ps_all=True), 10, EG, with_ps_all=True)
    st = {}
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        r, c, sums = ev.ope_replay(target, sim.device_log(), n_users=60, stats=st)
        greedy, h0 = ev.epsilon_greedy_branches(target, sim)
    sim.close()
    assert st['unresolved'] == st['acts'] > 60 and bool((r == 1.0).all()) and bool((h0 == 2).all())
    got = logs(make_env(OVER), 60, agent)
    a = got['a'][got['z'] == 'bandit'].to_numpy(dtype=np.int64)
    assert np.array_equal(a == 2, greedy.cpu().numpy() == 1) and 0.15 < (a != 2).mean() < 0.45


def test_a_refuted_greedy_act_sends_generate_logs_to_the_host_route():
    agent = mu.wrap(constant_agent(*refuted_pair()), 10, EG)
    env = make_env(OVER)
    with pytest.warns(RuntimeWarning, match='host route') as rec:
        got = env.generate_logs(60, agent)
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    assert_frames_equal(got, env.generate_logs(60, HostOnly(agent)))
    a = got['a'].dropna().astype(int)
    assert 0.55 < (a == 1).mean() < 0.85 and 0 < (a == 2).mean() < 0.1      # greedy acts take the reference's action, 1


def test_a_refuted_greedy_act_sends_the_replay_to_the_host_loop():
    target = mu.wrap(constant_agent(*refuted_pair(), with_ps_all=True), 10, EG, with_ps_all=True)
    cfg = Configuration({**env_1_args, 'random_seed': 11, 'num_products': 10, 'K': 5})
    sim = run(cfg, 120, dict(policy=_abi.RG_POLICY_UNIFORM_ENV))
    dl = sim.device_log()
    df = ev._device_log_to_frame(dl)
    sim.close()
    with pytest.warns(RuntimeWarning, match='host loop') as rec:
        assert ev.ope_replay(target, dl) is None
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    with pytest.warns(RuntimeWarning, match='host loop'):
        assert ev.epsilon_greedy_branches(target, dl) is None
    with pytest.warns(RuntimeWarning, match='host loop') as rec:
        rewards, ratio = ev.evaluate_SNIPS(target, dl)
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    want_c, want_r = ev._host_snips(target, df)
    assert isinstance(ratio, list) and len(ratio) > 300
    same(ratio, want_r)
    same(rewards, want_c)


# ---- (f) determinism -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['model_eg_poly_p40', 'model_eg_logreg_p10'])
def test_two_runs_give_the_same_log_and_the_same_sums(name):
    raws, sums = [], []
    for _ in range(2):
        meta, cols, P, sim = run_fixture(name)
        raws.append(sim.sorted_log_host()[0].copy())
        target = mu.wrapper(meta, cols, P, with_ps_all=True)
        for _ in range(2):
            sums.append(ev.ope_replay(target, sim.device_log(), n_users=meta['n_users'])[2].cpu().numpy().copy())
        sim.close()
    assert raws[0].tobytes() == raws[1].tobytes()
    assert all(s.tobytes() == sums[0].tobytes() for s in sums)


# ---- (g) error paths -------------------------------------------------------------------------------------------------------
def test_step_loop_error_paths():
    table = torch.from_numpy(explore_table(10, True)[0]).to(DEV)
    args = (0.1, 7, 1, table.data_ptr(), 0.1 / 9, 0.9)
    for policy in (_abi.RG_POLICY_LAST_VIEW_TABLE, _abi.RG_POLICY_RANDOM_AGENT, _abi.RG_POLICY_ORGANIC_USER_COUNT, _abi.RG_POLICY_UNIFORM_ENV,
                   _abi.RG_POLICY_EXTERNAL):
        lib, h, ws = handle(policy)
        assert lib.rg_sim_set_epsilon_greedy_model(h, *args) == -1 and b'wraps the frozen LogReg argmax' in lib.rg_last_error()
        lib.rg_sim_destroy(h)
    lib, h, ws = handle(_abi.RG_POLICY_LOGREG_FROZEN, lr_select_randomly=True)
    assert lib.rg_sim_set_epsilon_greedy_model(h, *args) == -1 and b'lr_select_randomly' in lib.rg_last_error()
    lib.rg_sim_destroy(h)
    for policy in (_abi.RG_POLICY_LOGREG_FROZEN, _abi.RG_POLICY_LOGREG_POLY):
        lib, h, ws = handle(policy)
        # the old entry point still refuses a model, message included
        assert lib.rg_sim_set_epsilon_greedy(h, *args) == -1 and b'EpsilonGreedy wraps RandomAgent' in lib.rg_last_error()
        for eps in (-0.01, 1.01, float('nan')):
            assert lib.rg_sim_set_epsilon_greedy_model(h, eps, 7, 1, table.data_ptr(), 0.0, 0.0) == -1 and b'epsilon' in lib.rg_last_error()
        assert lib.rg_sim_set_epsilon_greedy_model(h, 0.1, 7, 1, None, 0.1 / 9, 0.9) == -1 and b'NULL' in lib.rg_last_error()
        assert lib.rg_sim_set_epsilon_greedy_model(h, *args) == 0
        lib.rg_sim_destroy(h)
        lib, h, ws = handle(policy, P=1)
        assert lib.rg_sim_set_epsilon_greedy_model(h, 0.1, 7, 1, table.data_ptr(), 0.1, 0.9) == -1 and b'at least 2' in lib.rg_last_error()
        assert lib.rg_sim_set_epsilon_greedy_model(h, 0.1, 7, 0, table.data_ptr(), 0.1, 0.9) == 0
        lib.rg_sim_destroy(h)
    # after rg_sim_reset_users: RG_ESTATE
    meta, cols, P = mu.load('model_eg_logreg_p10')
    sim = Simulator(gu.env_config(meta), 32, device=DEV, **mu.inner_agent(meta, cols, P).device_policy())
    sim.reset_users(0, 32)
    assert sim.lib.rg_sim_set_epsilon_greedy_model(sim._h, *args) == -4 and b'before rg_sim_reset_users' in sim.lib.rg_last_error()
    sim.close()
    # a sampling LogReg through the Simulator: refused, not run without the overlay
    sampling = dict(policy=_abi.RG_POLICY_LOGREG_FROZEN, policy_seed=3, ouc=None,
                    logreg=dict(coef_t=np.eye(P), intercept=np.zeros(P), classes=np.arange(P, dtype=np.int32), select_randomly=True))
    with pytest.raises(_abi.RecoGymHipError, match='lr_select_randomly'):
        Simulator(gu.env_config(meta), 32, device=DEV, epsilon_greedy=dict(epsilon=0.1, seed=7, pure_new=True), **sampling)


def test_replay_error_paths():
    lib = _abi.load()
    cfg = Configuration({**env_1_args, 'random_seed': 1, 'num_products': 10, 'K': 5})
    sim = run(cfg, 40, dict(policy=_abi.RG_POLICY_RANDOM_AGENT, policy_seed=3))
    dl = sim.device_log()
    n, total = 39, int(dl.offsets[39].item())
    ratio = torch.zeros(total, dtype=torch.float64, device=DEV)
    sums = torch.zeros(3, dtype=torch.float64, device=DEV)
    meta, cols, P = mu.load('model_eg_logreg_p10')
    lr, keep_lr = ev._logreg_model(mu.inner_agent(meta, cols, P, True).ope_policy()['logreg'], P, torch.device(DEV))
    meta, cols, P = mu.load('model_eg_poly_p10')
    host, keep_pl = poly_device_model(mu.inner_agent(meta, cols, P, True).ope_policy_checked()['logreg_poly'], P, torch.device(DEV))
    pl = _abi.RgOpePoly(num_products=P, n_steps=int(keep_pl[3].numel()), wf=keep_pl[0].data_ptr(), wa=keep_pl[1].data_ptr(),
                        wk_t=keep_pl[2].data_ptr(), th=keep_pl[3].data_ptr(), intercept=host[3])

    def replay(fn, size_fn, model, eps=0.1, pure_new=1, ws_bytes=None, null_eg=False):
        eg = _abi.RgOpeEg(epsilon=eps, seed=7, pure_new=pure_new, reserved=0, prob_explore=1.0 / 9)
        need = size_fn(C.byref(model), n, 4096)
        ws = torch.zeros(max(need, 8), dtype=torch.uint8, device=DEV)
        return fn(C.byref(model), None if null_eg else C.byref(eg), dl.rows.data_ptr(), dl.offsets.data_ptr(), n, 4096, _abi.RG_OPE_PS_CONST,
                  None, 0.1, ratio.data_ptr(), None, sums.data_ptr(), None, None, ws.data_ptr(), need if ws_bytes is None else ws_bytes, None)
    for fn, size_fn, model in ((lib.rg_ope_replay_logreg_eg, lib.rg_ope_logreg_workspace_bytes, lr),
                               (lib.rg_ope_replay_poly_eg, lib.rg_ope_poly_workspace_bytes, pl)):
        assert replay(fn, size_fn, model) == 0, lib.rg_last_error()
        for eps in (1.5, -0.1, float('nan')):
            assert replay(fn, size_fn, model, eps=eps) == -1 and b'epsilon' in lib.rg_last_error()
        assert replay(fn, size_fn, model, null_eg=True) == -1 and b'null eg' in lib.rg_last_error()
        assert replay(fn, size_fn, model, ws_bytes=8) == -3
        model.num_products = 1                    # (refused before anything reads the model)
        assert replay(fn, size_fn, model) == -1 and b'at least 2' in lib.rg_last_error()
        model.num_products = 10
    lr.select_randomly = 1
    assert replay(lib.rg_ope_replay_logreg_eg, lib.rg_ope_logreg_workspace_bytes, lr) == -1 and b'select_randomly' in lib.rg_last_error()
    sim.close()
