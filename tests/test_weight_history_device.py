"""The likelihood agent's act on a time-weighted view history, on the device (rg_wh_common.hpp: wh_insert, wh_list, wh_act through
rg_sim_debug_set_timed_history / rg_sim_debug_weighted_acts).  The feature list is compared with the reference's scipy form
(`weighted_views`) bit for bit, the action and the flag bits with the host restatement of the device rule on those features
(`poly_rule(poly_decisions(...))`).  Needs a real MI355X."""
import numpy as np
import pytest

import adversarial_util as au
import golden_util as gu
from recogym_amd import _abi
from recogym_amd.agents.logreg_poly import expit_steps, poly_decisions, poly_rule
from recogym_amd.agents.views_history import weight_table, weighted_views
from recogym_amd.envs.configuration import Configuration
from recogym_amd.envs.reco_env_v1 import env_1_args

pytestmark = pytest.mark.gpu


def exp_t(t):
    return np.exp(-t)


FUNCS = {'exp_t': exp_t, **gu.WEIGHT_FUNCS}          # a float32 table, two float64 tables
N_USERS, CAP, STRIDE = 256, 511, 320


@pytest.fixture(scope='module')
def th():
    return expit_steps()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def model(P, seed):
    rng = np.random.RandomState(seed)
    return rng.normal(0, 0.4, P), rng.normal(0, 0.05, P), rng.normal(0, 0.6, (P, P)), float(rng.normal())


def make_sim(P, fn, mdl, th, n=N_USERS, cap=CAP):
    from recogym_amd.sim import Simulator
    table, f32 = weight_table(fn)
    wf, wa, wk, b = mdl
    cfg = Configuration({**env_1_args, 'random_seed': 5, 'num_products': P, 'K': 2, 'sigma_omega': 0.0})
    sim = Simulator(cfg, n, device='cuda:0', policy=_abi.RG_POLICY_LOGREG_POLY, policy_seed=0, ouc=dict(history_cap=cap),
                    logreg_poly=dict(wf=wf, wa=wa, wk=wk, intercept=b, expit_steps=th, weight_history=dict(table=table, f32=f32)),
                    log_capacity=0)
    sim.reset_users(0, n)
    return sim


def histories(P, name, rng):
    """(kind, products, deltas) per user, deltas = now - time, never increasing along the views (view order)."""
    kinds = ['single', 'binades', 'band', 'zero', 'twice', 'long']
    out = []
    for i in range(N_USERS):
        kind = kinds[i % len(kinds)]
        if kind == 'single':
            prods, dl = [rng.randint(P)], [rng.randint(0, 60)]
        elif kind == 'binades':         # one product 40 times (others between), weights over 12 binades: the addition order shows
            span = 8 if name == 'exp_t' else (42 if name == 'exp_0.2' else 4095)
            dl = np.sort(rng.randint(0, span + 1, size=48))[::-1]
            dl[0], dl[-1] = span, 0
            prods = np.full(48, rng.randint(P))
            prods[rng.choice(np.arange(1, 47), 8, replace=False)] = rng.randint(0, P, size=8)
        elif kind == 'band':            # exp(-t): normal at 87, subnormal 88 .. 103, zero from 104 — products drop, n changes
            dl = np.sort(np.r_[np.arange(87, 105), 150, rng.randint(85, 108, size=12)])[::-1]
            prods = rng.randint(0, P, size=len(dl))
        elif kind == 'zero':            # exp(-t) and exp(-0.2 t) underflow to exactly 0: the empty list (1 / (1 + t) never does)
            lo = 104 if name == 'exp_t' else 3800
            dl = np.sort(rng.randint(lo, lo + 500, size=rng.randint(1, 9)))[::-1]
            prods = rng.randint(0, P, size=len(dl))
        elif kind == 'twice':           # the same product twice at one truncated time: two equal words in the row
            d0 = rng.randint(0, 30)
            p0 = rng.randint(P)
            dl = np.sort(np.r_[d0, d0, rng.randint(0, 40, size=5)])[::-1]
            prods = rng.randint(0, P, size=len(dl))
            prods[np.flatnonzero(dl == d0)[:2]] = p0
        else:                           # 300 views: beyond the entries a wave stages in LDS (and, at P > 256, a list beyond it)
            dl = np.sort(rng.randint(0, 90 if name == 'exp_t' else 400, size=300))[::-1]
            prods = rng.permutation(300) % P if P > 256 else rng.randint(0, P, size=300)
        out.append((kind, np.asarray(prods, dtype=np.int64), np.asarray(dl, dtype=np.int64)))
    return out


@pytest.mark.parametrize('P', [10, 65, 130, 300])
@pytest.mark.parametrize('name', sorted(FUNCS))
def test_the_device_function_on_preset_lists(name, P, th):
    fn = FUNCS[name]
    rng = np.random.RandomState(100 * P + len(name))
    mdl = model(P, P)
    hist = histories(P, name, rng)
    now = rng.randint(4500, 32768, size=N_USERS)
    n_views = np.array([len(h[1]) for h in hist])
    products = np.zeros((N_USERS, STRIDE), dtype=np.uint32)
    times = np.zeros((N_USERS, STRIDE), dtype=np.uint16)
    for i, (_, prods, dl) in enumerate(hist):
        products[i, :len(prods)] = prods
        times[i, :len(dl)] = now[i] - dl
    sim = make_sim(P, fn, mdl, th)
    sim.debug_set_timed_history(n_views, products, times)
    act, fl, ln, lp, lv = sim.debug_weighted_acts(now, stride=STRIDE)
    cnt, launched, on = sim.counters(), sim.get_option('launched_logreg_poly_w'), sim.get_option('weight_history')
    sim.close()
    assert on == 1 and launched == 1 and cnt['hist_overflow'] == 0 and cnt['wh_clock_range'] == 0
    seen = {'empty': 0, 'dropped': 0, 'long_list': 0}
    for i, (kind, prods, dl) in enumerate(hist):
        t = now[i] - dl
        want = np.asarray(weighted_views([np.int16(p) for p in prods], [np.int16(x) for x in t], np.int16(now[i]), fn, P))[0]
        keep = np.flatnonzero(want != 0)
        assert ln[i] == len(keep) and np.array_equal(lp[i, :ln[i]], keep), (i, kind)
        assert np.array_equal(bits(lv[i, :ln[i]]), bits(want[keep])), (i, kind)
        a, f = poly_rule(poly_decisions(keep, want[keep].astype(np.float64), *mdl), th)
        assert (act[i], fl[i]) == (a, f), (i, kind, act[i], fl[i], a, f)
        seen['empty'] += len(keep) == 0
        seen['dropped'] += len(keep) < len(np.unique(prods))
        seen['long_list'] += len(keep) > 256
    # the cases are what they claim to be
    if name != 'inverse':
        assert seen['empty'] >= N_USERS // 6
    if name == 'exp_t':
        assert seen['dropped'] > seen['empty']
    if P > 256:
        assert seen['long_list'] >= N_USERS // 6 - 1


@pytest.mark.parametrize('name', ['exp_t', 'exp_0.2'])
def test_a_full_row_drops_views_and_counts_each(name, th):
    """hist_cap = 32 (ouc_history_cap 31): the row keeps 31 VIEWS.  Users preset with 30, 31, 32 and 33 views drop 0, 0, 1 and 2; the
    act is taken on the views kept (the first 31 in view order)."""
    P, keep = 10, 31
    fn = FUNCS[name]
    rng = np.random.RandomState(7)
    mdl = model(P, 3)
    n_views = np.array([keep - 1, keep, keep + 1, keep + 2])
    products = rng.randint(0, P, size=(4, 40)).astype(np.uint32)
    times = np.sort(rng.randint(100, 140, size=(4, 40)), axis=1).astype(np.uint16)
    now = np.full(4, 141)
    sim = make_sim(P, fn, mdl, th, n=4, cap=keep)
    assert sim.get_option('hist_cap') == keep + 1
    sim.debug_set_timed_history(n_views, products, times)
    cnt = sim.counters()
    act, fl, ln, lp, lv = sim.debug_weighted_acts(now)
    sim.close()
    assert cnt['hist_overflow'] == 3
    for i in range(4):
        k = min(n_views[i], keep)
        want = np.asarray(weighted_views([np.int16(p) for p in products[i, :k]], [np.int16(x) for x in times[i, :k]], np.int16(141), fn, P))[0]
        nz = np.flatnonzero(want != 0)
        assert np.array_equal(lp[i, :ln[i]], nz) and np.array_equal(bits(lv[i, :ln[i]]), bits(want[nz])), i
        assert (act[i], fl[i]) == poly_rule(poly_decisions(nz, want[nz].astype(np.float64), *mdl), th), i


def test_a_clock_value_outside_the_int16_range_is_counted(th):
    """An act past 32 767, a view past 32 767 and a view after the act: one count each, none for the user inside the range."""
    P = 10
    mdl = model(P, 4)
    sim = make_sim(P, exp_t, mdl, th, n=4)
    products = np.tile(np.arange(4, dtype=np.uint32), (4, 1))
    times = np.array([[10, 11, 12, 13], [10, 11, 12, 13], [10, 11, 12, 40000], [10, 11, 12, 13]], dtype=np.uint16)
    sim.debug_set_timed_history(np.full(4, 4), products, times)
    act, fl, ln, lp, lv = sim.debug_weighted_acts(np.array([20, 32768, 20, 12], dtype=np.uint16))
    cnt = sim.counters()
    sim.close()
    assert cnt['wh_clock_range'] == 3
    want = np.asarray(weighted_views([np.int16(p) for p in range(4)], [np.int16(x) for x in (10, 11, 12, 13)], np.int16(20), exp_t, P))[0]
    assert ln[0] == 4 and np.array_equal(bits(lv[0, :4]), bits(want[:4]))
    assert ((0 <= act) & (act < P)).all()


def test_the_table_comes_before_the_reset_and_needs_a_log(th):
    P = 10
    sim = make_sim(P, exp_t, model(P, 5), th, n=8)
    with pytest.raises(_abi.RecoGymHipError, match='before rg_sim_reset_users'):
        _abi.check(sim.lib.rg_sim_set_weight_history(sim._h, sim.wh_table.data_ptr(), 32768, 1), 'rg_sim_set_weight_history')
    with pytest.raises(_abi.RecoGymHipError, match='from the log'):       # (make_sim attaches none)
        sim.run()
    sim.close()


# ------------------------------------------------------------------------------------------------
# the step loop: generate_logs with the key set against the same agent without it (the per-user host route)
# ------------------------------------------------------------------------------------------------
def agents(P, fn, seed=11, **extra):
    from recogym_amd.agents import LogregPolyFrozenAgent
    wf, wa, wk, b = model(P, seed)
    coef, icpt = np.r_[wf, wa, wk.reshape(-1)][None, :], [b]
    cfg = {'num_products': P, 'weight_history_function': fn, **extra}
    return (LogregPolyFrozenAgent(Configuration({**cfg, 'device_weight_history': True}), coef, icpt),
            LogregPolyFrozenAgent(Configuration(cfg), coef, icpt))


def env_of(clock, **over):
    from device_util import make_env
    if clock == 'normal':
        from recogym_amd.envs.features.time import NormalTimeGenerator
        over['time_generator'] = NormalTimeGenerator(Configuration({'normal_time_mu': over.pop('mu', 0.0), 'normal_time_sigma': 1.5}))
    over.pop('mu', None)
    return make_env(over)


def device_run(env, agent, n, seen=None, **users):
    """generate_logs as it is called, with the launches and counters of the device run it made (None: it made none); `seen`
    collects them for a caller that expects the call to raise.  `users`: generate_logs' num_organic_offline_users / first_user_id."""
    from recogym_amd.envs.reco_env_v1 import RecoEnv1
    seen = [] if seen is None else seen
    real = RecoEnv1.simulate

    def spy(self, *a, **k):
        cnt, sim = real(self, *a, **k)
        seen.append(dict(cnt, launched=sim.get_option('launched_logreg_poly_w'), hist_cap=sim.get_option('hist_cap'), ledger=au.ledger(sim)))
        return cnt, sim
    RecoEnv1.simulate = spy
    try:
        df = env.generate_logs(n, agent, **users)
    finally:
        RecoEnv1.simulate = real
    return df, (seen[-1] if seen else None)


@pytest.mark.parametrize('clock', ['default', 'normal'])
@pytest.mark.parametrize('name', ['exp_t', 'exp_0.2'])
def test_generate_logs_on_the_device_equals_the_host_route(name, clock):
    import warnings
    from device_util import assert_frames_equal
    P, n = 40, 200
    dev, host = agents(P, FUNCS[name])
    assert dev.device_policy()['logreg_poly']['weight_history']['f32'] == (name == 'exp_t') and host.device_policy() is None
    over = {'random_seed': 42, 'num_products': P, 'K': 8, 'sigma_omega': 0.1}
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        got, run = device_run(env_of(clock, **over), dev, n)
    want = env_of(clock, **over).generate_logs(n, host)
    print(name, clock, len(got), run)
    assert run is not None and run['launched'] > 0, 'the call took the host route'
    assert run['hist_overflow'] == 0 and run['wh_clock_range'] == 0 and run['live'] == 0 and run['log_dropped'] == 0
    assert run['lr_acts'] == run['bandit'] + run['phantom']              # a fresh act for every bandit event and trailing row
    assert_frames_equal(got, want)
    assert (got['ps'].to_numpy(dtype=np.float64, na_value=np.nan)[(got['z'] == 'bandit').to_numpy()] == 1.0).all()


def test_a_history_longer_than_its_row_is_run_again_with_a_longer_one():
    """ouc_history_cap 15: the row keeps 15 views, most users have more.  simulate counts every dropped view and runs again with
    rows twice as long until nothing is dropped; the rows are the host route's."""
    from device_util import assert_frames_equal
    from recogym_amd.envs.reco_env_v1 import device_policy_of
    P, n = 10, 60
    dev, host = agents(P, exp_t)
    pol = device_policy_of(dev)
    over = {'random_seed': 9, 'num_products': P, 'K': 4}
    env = env_of('default', **over)
    sim = env.make_simulator(n, dev, policy=dict(pol, ouc=dict(history_cap=15)))
    sim.reset_users(0, n)
    sim.run()
    cnt, cols = sim.counters(), sim.log_columns()
    sim.close()
    views = np.bincount(cols['u'][~cols['is_bandit']], minlength=n)
    assert cnt['hist_overflow'] == np.maximum(views - 15, 0).sum() > 0      # one per dropped view
    dev15 = agents(P, exp_t)[0]
    dev15.device_policy = lambda: dict(pol, ouc=dict(history_cap=15))
    got, run = device_run(env_of('default', **over), dev15, n)
    assert run['hist_overflow'] == 0 and run['hist_cap'] - 1 >= views.max() and run['launched'] > 0
    assert_frames_equal(got, env_of('default', **over).generate_logs(n, host))


def test_a_clock_past_the_int16_range_sends_the_call_to_the_host_route():
    """NormalTimeGenerator with mu = 20 000: every user's third event lies past 32 767.  The device run counts it, generate_logs
    warns once and gives the host route's answer — which is the host agent's own np.int16 cast of such a time: rows where NumPy
    wraps the value, OverflowError where it refuses to."""
    from device_util import assert_frames_equal
    P, n = 10, 30
    dev, host = agents(P, FUNCS['exp_0.2'])
    over = {'random_seed': 3, 'num_products': P, 'K': 4, 'mu': 20000.0}
    try:
        want = env_of('normal', **over).generate_logs(n, host)
    except OverflowError as e:
        want = type(e)
    seen, got = [], None
    with pytest.warns(RuntimeWarning) as rec:
        try:
            got, _ = device_run(env_of('normal', **over), dev, n, seen)
        except OverflowError as e:
            got = type(e)
    assert len([w for w in rec if 'generate_logs repeats the call' in str(w.message)]) == 1
    assert seen and seen[-1]['wh_clock_range'] > 0 and seen[-1]['launched'] > 0
    if isinstance(want, type):
        assert got is want
    else:
        assert_frames_equal(got, want)


# ------------------------------------------------------------------------------------------------
# the unmodified reference's own logs (tests/make_golden_weight_history.py)
# ------------------------------------------------------------------------------------------------
REF = {'poly_wh_exp_default': exp_t, 'poly_wh_exp02_normal': FUNCS['exp_0.2']}


def run_fixture(name, first_user=0, n_users=None, organic_only_below=0):
    """generate_logs over the fixture's users (or n_users of them from first_user on, the ids below organic_only_below organic only)
    -> meta, cols, the frame, device_run's record of the device run"""
    import warnings
    from recogym_amd.agents import LogregPolyFrozenAgent
    meta, cols = gu.load(name)
    P, n = meta['env_args']['num_products'], meta['n_users'] if n_users is None else n_users
    agent = LogregPolyFrozenAgent(Configuration({'num_products': P, 'weight_history_function': REF[name], 'device_weight_history': True}),
                                  cols['poly_coef'], cols['poly_intercept'])
    nt = meta.get('normal_time')
    env = env_of('normal', mu=nt['mu'], **meta['env_args']) if nt else env_of('default', **meta['env_args'])
    if nt:
        assert nt['sigma'] == 1.5
    n_org = max(0, min(n, organic_only_below - first_user))
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        got, run = device_run(env, agent, n - n_org, num_organic_offline_users=n_org, first_user_id=first_user)
    return meta, cols, got, run


def assert_frame_is_the_reference_log(name, meta, cols, got, run):
    """The frame and the record of a run of the fixture's users (of several runs: frames concatenated, counters summed) held to it."""
    nt = meta.get('normal_time')
    assert run is not None and run['launched'] > 0, 'the call took the host route'
    assert run['hist_overflow'] == 0 and run['wh_clock_range'] == 0 and run['poly_unresolved'] == 0
    assert len(got) == len(cols['u'])
    is_b = (got['z'] == 'bandit').to_numpy()
    assert np.array_equal(is_b, cols['z'] == 1)
    assert np.array_equal(got['u'].to_numpy(dtype=np.int64), cols['u'].astype(np.int64))
    assert np.array_equal(got['v'].to_numpy(dtype=np.float64, na_value=-1)[~is_b], cols['v'][~is_b].astype(np.float64))
    assert np.array_equal(got['a'].to_numpy(dtype=np.float64, na_value=-1)[is_b], cols['a'][is_b].astype(np.float64))
    assert np.array_equal(got['c'].to_numpy(dtype=np.float64, na_value=-1)[is_b], cols['c'][is_b].astype(np.float64))
    t = got['t'].to_numpy(dtype=np.float64)
    if nt:      # the generator's clock, at the float32 resolution of the reference's `t` column
        np.testing.assert_allclose(t, cols['time'], rtol=2e-7, atol=0)
    else:
        assert np.array_equal(t, cols['t'].astype(np.float64))
    assert (got['ps'].to_numpy(dtype=np.float64, na_value=np.nan)[is_b] == 1.0).all()


@pytest.mark.parametrize('name', sorted(REF))
def test_generate_logs_with_the_key_gives_the_reference_log(name):
    assert_frame_is_the_reference_log(name, *run_fixture(name))


# ------------------------------------------------------------------------------------------------
# the training feed from a device log (rg_weighted_feed)
# ------------------------------------------------------------------------------------------------
def assert_same_training_set(got, want):
    from scipy import sparse
    for x in (got, want):
        assert sparse.issparse(x[0])
    g, w = sparse.csr_matrix(got[0]), sparse.csr_matrix(want[0])
    g.sort_indices()
    w.sort_indices()
    assert g.shape == w.shape and g.dtype == w.dtype == np.float32
    assert np.array_equal(g.indptr, w.indptr) and np.array_equal(g.indices, w.indices)
    assert np.array_equal(bits(g.data), bits(w.data))
    for k in (1, 2, 3):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), k


@pytest.mark.parametrize('name,clock', [('exp_t', 'default'), ('exp_0.2', 'normal')])      # a float32 and a float64 table
def test_the_device_feed_equals_the_host_loop(name, clock):
    from recogym_amd.agents.feature_feed import train_data_from_log
    P, n = 20, 300
    env = env_of(clock, random_seed=17, num_products=P, K=5)
    cnt, sim = env.simulate(n, None)
    dl, cols = sim.device_log(), sim.log_columns()
    got = train_data_from_log(dl, P, weight_history_function=FUNCS[name])
    sim.close()
    want = train_data_from_log(cols, P, weight_history_function=FUNCS[name])
    assert got[0].shape[0] == cnt['bandit'] + cnt['phantom'] and got[0].nnz > 0
    assert_same_training_set(got, want)


def fixture_device_log(cols):
    import torch
    from recogym_amd.sim import DeviceLog
    u, t, z, v, a, c = (cols['trainlog_' + k].astype(np.int64) for k in 'utzvac')
    code = np.where(z == 1, _abi.RG_EV_BANDIT | np.where(c == 1, _abi.RG_EV_CLICK, 0) | a, v)
    rows = np.stack([u, t, code, np.zeros_like(u)], axis=1).astype(np.uint32).view(np.int32)
    offsets = np.r_[0, np.flatnonzero(np.r_[u[1:] != u[:-1], True]) + 1].astype(np.int64)
    assert len(offsets) == u.max() + 2
    dev = 'cuda:0'
    return DeviceLog(torch.from_numpy(rows).to(dev), torch.from_numpy(offsets).to(dev), torch.from_numpy(cols['trainlog_ps']).to(dev), 0, 10, None)


@pytest.mark.parametrize('name', sorted(REF))
def test_the_device_feed_rebuilds_the_reference_training_set(name):
    from scipy import sparse
    from recogym_amd.agents.feature_feed import train_data_from_log
    meta, cols = gu.load(name)
    P = meta['env_args']['num_products']
    got = train_data_from_log(fixture_device_log(cols), P, weight_history_function=REF[name])
    want = (sparse.csr_matrix((cols['train_data'], cols['train_indices'], cols['train_indptr']), shape=(len(cols['train_actions']), P)),
            cols['train_actions'], cols['train_deltas'], cols['train_pss'])
    assert str(cols['train_data_dtype']) == 'float32'
    assert_same_training_set(got, want)


def test_a_feed_row_outside_the_clock_range_takes_the_host_loop():
    import torch
    from recogym_amd.agents.feature_feed import weighted_train_data_device
    meta, cols = gu.load('poly_wh_exp_default')
    dl = fixture_device_log(cols)
    table, f32 = weight_table(exp_t)
    assert weighted_train_data_device(dl, 10, table, f32) is not None
    rows = dl.rows.clone()
    rows[5, 1] = 40000
    assert weighted_train_data_device(dl._replace(rows=rows), 10, table, f32) is None


def test_test_agent_trains_from_the_device_log_to_the_same_model():
    import recogym_amd as recogym
    from recogym_amd.agents import LogregPolyAgent, logreg_poly_args
    P = 10
    seen = {}

    def trained(**extra):
        agent = LogregPolyAgent(Configuration({**logreg_poly_args, 'num_products': P, 'random_seed': 7, 'weight_history_function': exp_t,
                                               **extra}))
        real = LogregPolyAgent.train_from_log
        logs = []

        def spy(self, log, *a, **k):
            logs.append(type(log).__name__)
            seen[bool(extra)] = self
            return real(self, log, *a, **k)
        LogregPolyAgent.train_from_log = spy
        try:
            res = recogym.test_agent(env_of('default', random_seed=42, num_products=P, K=5), agent, 60, 30)
        finally:
            LogregPolyAgent.train_from_log = real
        return res, logs
    with_key, logs_key = trained(device_weight_history=True)
    without, logs_host = trained()
    assert logs_key == ['DeviceLog'] and logs_host == ['dict']
    assert LogregPolyAgent(Configuration({**logreg_poly_args, 'num_products': P, 'weight_history_function': exp_t,
                                          'device_weight_history': True})).accepts_device_log
    assert not LogregPolyAgent(Configuration({**logreg_poly_args, 'num_products': P, 'weight_history_function': exp_t})).accepts_device_log
    assert not LogregPolyAgent(Configuration({**logreg_poly_args, 'num_products': P, 'weight_history_function': lambda t: t / t.sum(),
                                              'device_weight_history': True})).accepts_device_log
    a, b = seen[True].logreg, seen[False].logreg
    assert a is not None and b is not None
    assert np.array_equal(a.coef_, b.coef_) and np.array_equal(a.intercept_, b.intercept_)
    assert with_key == without
