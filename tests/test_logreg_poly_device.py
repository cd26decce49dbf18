"""The likelihood agent in the device step loop (RG_POLICY_LOGREG_POLY, k_poly_acts): the reference's own logs row for row
(tests/golden/poly_*.npz, tests/make_golden_logreg_poly.py) with the path counters the generator recorded, generate_logs against
the per-user host route, adversarial placements of the decisions around expit's steps — every case checked against the host act
(scipy's expit) AND by its flag bits, so the path is proven, not assumed — and the unresolved-act protocol.  Every comparison is
bit for bit.  Needs a real MI355X."""
import warnings

import numpy as np
import pytest
import torch
from scipy.special import expit

import adversarial_util as au
from device_util import assert_frames_equal, constant_agent, make_env
import golden_util as gu
import recogym_amd as recogym
from recogym_amd import _abi
from recogym_amd.agents import LogregPolyAgent, LogregPolyFrozenAgent, logreg_poly_args
from recogym_amd.agents.logreg_poly import expit_steps, poly_decisions, poly_margin, poly_rule
from recogym_amd.envs.configuration import Configuration
from recogym_amd.envs.reco_env_v1 import env_1_args

pytestmark = pytest.mark.gpu

TABLE, UNRESOLVED, MERGE = 1, 2, 4
FIXTURES = ['poly_p10', 'poly_p10_sigma0', 'poly_p40', 'poly_p10_ips', 'poly_p10_shifted']


@pytest.fixture(scope='module')
def th():
    return expit_steps()


def frozen_of(cols, P, **cfg):
    return LogregPolyFrozenAgent(Configuration({'num_products': P, **cfg}), cols['poly_coef'], cols['poly_intercept'])


def run_fixture(name, first_user=0, n_users=None, organic_only_below=0, ledger=False):
    """-> meta, cols, rows, counters, the raw sorted log[, the launch ledger and the unresolved list (poly_verify's outcome)]"""
    from recogym_amd.sim import Simulator
    meta, cols = gu.load(name)
    P, n = meta['env_args']['num_products'], meta['n_users'] if n_users is None else n_users
    sim = Simulator(gu.env_config(meta), n, device='cuda:0', **frozen_of(cols, P).device_policy())
    sim.reset_users(first_user, n, organic_only_below=organic_only_below)
    sim.run()
    rows, cnt, raw = sim.rows(), sim.counters(), sim.sorted_log_host()[0]
    extra = ()
    if ledger:
        stands = sim.poly_verify()
        extra = (au.ledger(sim), stands, sim.poly_unresolved.copy())
    sim.close()
    return (meta, cols, rows, cnt, raw) + extra


def assert_log_equals_the_reference(name, meta, cols, rows, cnt):
    """The rows and counters of a run of the fixture's users (of several runs: rows concatenated, counters summed) held to it."""
    gu.assert_rows_equal(rows, cols, ps_rtol=0, what=name)
    census = meta['census']
    print(name, {k: cnt[k] for k in ('lr_acts', 'lr_rows', 'poly_table', 'poly_unresolved')}, census)
    assert cnt['poly_table'] == census['table'] and cnt['poly_unresolved'] == census['unresolved'] == 0
    assert cnt['lr_acts'] == census['acts']
    assert cnt['live'] == 0 and cnt['log_dropped'] == 0 and cnt['hist_overflow'] == 0


@pytest.mark.parametrize('name', FIXTURES)
def test_device_log_equals_the_reference(name):
    """sigma_omega > 0 (lock-step rounds) and = 0, P = 10 and P = 40 (saturated acts), the IPS-weighted fit, and the shifted model
    whose acts all lie on the step table with lower indices winning merges."""
    meta, cols, rows, cnt, _ = run_fixture(name)
    assert_log_equals_the_reference(name, meta, cols, rows, cnt)


def test_some_fixture_proves_the_table_and_a_merge():
    c = [gu.load(n)[0]['census'] for n in FIXTURES]
    assert any(x['table'] > 0 and x['merges'] > 0 for x in c) and any(0 < x['table'] < x['acts'] for x in c)


def test_two_runs_give_the_same_log():
    a, b = run_fixture('poly_p40'), run_fixture('poly_p40')
    assert np.array_equal(a[4], b[4]) and a[3] == b[3]


def trained_agent():
    """-> the meta of poly_p10, LogregPolyAgent trained on the fixture's training log"""
    meta, cols = gu.load('poly_p10')
    train = {k[len('trainlog_'):]: v for k, v in cols.items() if k.startswith('trainlog_')}
    from make_golden_ope import log_frame
    agent = LogregPolyAgent(Configuration({**logreg_poly_args, 'num_products': 10, 'random_seed': 7}))
    agent.train_from_log(log_frame(train))
    return meta, agent


def test_generate_logs_with_the_trained_agent_equals_the_host_route():
    meta, agent = trained_agent()
    env = make_env(meta['env_args'])
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        got = env.generate_logs(200, agent)
    want = env._generate_logs_per_user(200, agent, 0)
    assert_frames_equal(got, want)
    assert (got['ps'].to_numpy(dtype=np.float64, na_value=np.nan)[(got['z'] == 'bandit').to_numpy()] == 1.0).all()


# ------------------------------------------------------------------------------------------------
# adversarial: decisions placed to the bit
# ------------------------------------------------------------------------------------------------
def debug_acts(P, wf, wa, wk, b, nd, prod, cnt, th):
    """rg_sim_debug_set_history + rg_sim_debug_poly_acts -> (actions, flags) of the users whose histories are given."""
    from recogym_amd.sim import Simulator
    n, stride = len(nd), prod.shape[1]
    cfg = Configuration({**env_1_args, 'random_seed': 5, 'num_products': P, 'K': 2, 'sigma_omega': 0.0})
    hist_cap = max(stride, 255)
    sim = Simulator(cfg, n, device='cuda:0', policy=_abi.RG_POLICY_LOGREG_POLY, policy_seed=0, ouc=dict(history_cap=hist_cap),
                    logreg_poly=dict(wf=wf, wa=wa, wk=wk, intercept=b, expit_steps=th), log_capacity=0)
    sim.reset_users(0, n)
    dev = 'cuda:0'
    d = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)).to(dev) for x in (nd, prod, cnt)]
    act = torch.full((n,), -1, dtype=torch.int32, device=dev)
    fl = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    _abi.check(sim.lib.rg_sim_debug_set_history(sim._h, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), stride, sim._stream()),
               'debug_set_history')
    _abi.check(sim.lib.rg_sim_debug_poly_acts(sim._h, act.data_ptr(), fl.data_ptr(), sim._stream()), 'debug_poly_acts')
    torch.cuda.synchronize()
    out = act.cpu().numpy().astype(np.int64), fl.cpu().numpy().astype(np.int64)
    sim.close()
    return out


def placements(P, th):
    """(name, z vector, expected action, expected flags): with a one-view history (count 1) and wf = wa = 0, b = 0 the decision
    of action a is wk[a, p] exactly."""
    K = len(th)
    lo, hi = (0, 1) if P == 2 else (P // 3, P - 1)
    k = next(i for i in range(400, K) if th[i] < th[i - 1])        # an inner step that decisions reach (thresholds coincide in pairs)
    below = np.nextafter(th[K - 1], -np.inf)                # z* one double below the table
    W = poly_margin(below)
    inside = below - W
    while below - inside > W:
        inside = np.nextafter(inside, np.inf)
    outside = below - W
    while below - outside <= W:
        outside = np.nextafter(outside, -np.inf)
    assert below - inside <= W < below - outside and outside < inside and inside - outside < 1e-12 * W + 4 * np.spacing(below)

    def vec(z_lo, z_hi, base=-3.0):
        z = np.full(P, base)
        z[lo], z[hi] = z_lo, z_hi
        return z
    last = np.full(P, -1.0)
    last[P - 1] = 7.0
    first_only = np.full(P, -745.0)
    first_only[0] = -720.0
    last_lane = max((a for a in range(P) if a % 64 == 63), default=None)       # lane 63's last action (P >= 64)
    lane63 = np.full(P, -1.0)
    if last_lane is not None:
        lane63[last_lane] = 7.0
    return [
        ('saturated pair, larger z at the higher index', vec(th[0] + 1.0, th[0] + 3.0), lo, TABLE | MERGE),
        ('saturated exactly from th[0]', vec(th[0], 90.0), lo, TABLE | MERGE),
        ('one double below th[0] is another step', vec(np.nextafter(th[0], -np.inf), th[0]), hi, TABLE),
        ('same inner step', vec(th[k], np.nextafter(th[k - 1], -np.inf)), lo, TABLE | MERGE),
        ('adjacent inner steps', vec(np.nextafter(th[k], -np.inf), th[k]), hi, TABLE),
        ('the last step of the table', vec(th[K - 1], np.nextafter(th[K - 2], -np.inf) if th[K - 2] > th[K - 1] else th[K - 1]), lo,
         TABLE | (MERGE if th[K - 2] > th[K - 1] else 0)),
        ('below the table, lower index just inside W', vec(inside, below), hi, UNRESOLVED),
        ('below the table, lower index just outside W', vec(outside, below), hi, 0),
        ('below the table, HIGHER index inside W', vec(below, inside), lo, 0),
        ('exact tie below the table', vec(3.25, 3.25), lo, 0),
        ('exact tie on the table', vec(th[0] + 1.0, th[0] + 1.0), lo, TABLE),
        ('the maximum in the last action', last, P - 1, 0),
        ('negative decisions', vec(-700.0, -699.0, base=-745.0), hi, 0),
        ('below -700 expit leaves the normal doubles: unresolved', vec(-730.0, -701.0, base=-745.0), hi, UNRESOLVED),
        ('below -700 with the best decision at index 0', first_only, 0, 0),
    ] + ([('the maximum in the last action of the last lane', lane63, last_lane, 0)] if last_lane is not None else [])


@pytest.mark.parametrize('P', [2, 10, 65, 130])
def test_placed_decisions(P, th):
    cases = placements(P, th)
    for c0 in range(0, len(cases), P):          # a case per product: the user that viewed product p once decides on wk[:, p]
        batch = cases[c0:c0 + P]
        wk = np.zeros((P, P))
        for p, (_, z, _, _) in enumerate(batch):
            wk[:, p] = z
        n = len(batch)
        nd = np.ones(n, dtype=np.uint32)
        prod = np.arange(n, dtype=np.uint32).reshape(n, 1)
        cnt = np.ones((n, 1), dtype=np.uint32)
        act, fl = debug_acts(P, np.zeros(P), np.zeros(P), wk, 0.0, nd, prod, cnt, th)
        for i, (name, z, want_a, want_fl) in enumerate(batch):
            assert np.array_equal(poly_decisions([i], [1], np.zeros(P), np.zeros(P), wk, 0.0), z), name
            host = int(np.argmax(expit(z)))
            assert poly_rule(z, th) == (want_a, want_fl), (name, poly_rule(z, th))
            print(P, name, 'device', act[i], fl[i], 'host', host)
            assert (act[i], fl[i]) == (want_a, want_fl), (P, name, act[i], fl[i])
            if not want_fl & UNRESOLVED:
                assert act[i] == host, (P, name)


@pytest.mark.parametrize('P,sizes', [(10, (1, 3, 10)), (65, (1, 15, 16, 40)), (130, (1, 15, 16, 40, 130)), (300, (255, 256, 257, 300))])
def test_random_models_and_histories(P, sizes, th):
    """Histories of 1, 15, 16 and 40 distinct products (the first history line holds 15), n = P, histories round the 256 entries a
    wave keeps in LDS (P = 300 with a raised history cap: the rest is read from the row), counts up to 300; weights whose
    scale puts decisions below, on and above the table.  The device's action and flags equal the numpy restatement of its rule
    on the host's decisions (so the decisions are the host's bit for bit), and the host act wherever the act is resolved."""
    rng = np.random.RandomState(P)
    scales = (0.0005, 0.02, 3.0) if P >= 300 else (0.02, 0.3, 3.0)       # (long histories: smaller weights keep some acts below the table)
    users = [(s, scale) for s in sizes for scale in scales for _ in range(6)]
    n, stride = len(users), max(sizes)
    nd = np.array([s for s, _ in users], dtype=np.uint32)
    prod = np.zeros((n, stride), dtype=np.uint32)
    cnt = np.zeros((n, stride), dtype=np.uint32)
    for i, (s, _) in enumerate(users):
        prod[i, :s] = np.sort(rng.choice(P, s, replace=False))
        cnt[i, :s] = np.where(rng.rand(s) < 0.7, rng.randint(1, 4, s), rng.randint(1, 301, s))
    seen = dict(table=0, merge=0, plain=0)
    for scale in scales:
        wf, wa, wk, b = rng.randn(P) * scale, rng.randn(P) * scale / P, rng.randn(P, P) * scale, float(rng.randn())
        act, fl = debug_acts(P, wf, wa, wk, b, nd, prod, cnt, th)
        ag = LogregPolyFrozenAgent(Configuration({'num_products': P}), np.r_[wf, wa, wk.reshape(-1)][None, :], [b])
        for i, (s, _) in enumerate(users):
            z = ag.decisions(prod[i, :s], cnt[i, :s])
            assert (act[i], fl[i]) == poly_rule(z, th), (P, scale, i, s, act[i], fl[i], poly_rule(z, th))
            if not fl[i] & UNRESOLVED:
                assert act[i] == int(np.argmax(expit(z))), (P, scale, i, s)
            seen['table'] += fl[i] & TABLE
            seen['merge'] += (fl[i] & MERGE) >> 2
            seen['plain'] += fl[i] == 0
    print(P, seen)
    assert seen['table'] > 0 and seen['plain'] > 0 and (P == 10 or seen['merge'] > 0)


# ------------------------------------------------------------------------------------------------
# unresolved acts: confirmed by the host -> the device log stands; refuted -> the host route
# ------------------------------------------------------------------------------------------------
OVER = dict(random_seed=321, num_products=10, K=4)


def test_an_unresolved_act_the_host_confirms_keeps_the_device_route():
    from recogym_amd.sim import Simulator
    z1, z2 = 25.0, 25.0 + 2.0 ** -12                         # inside W(z2) = 4.9e-4, far beyond one step of expit (1.6e-5 here)
    assert 0 < z2 - z1 <= poly_margin(z2) and expit(z1) < expit(z2)
    agent = constant_agent(z1, z2)
    sim = Simulator(Configuration({**env_1_args, **OVER}), 60, device='cuda:0', **agent.device_policy())
    sim.reset_users(0, 60)
    sim.run()
    cnt = sim.counters()
    assert sim.poly_verify() and not sim.poly_overflow
    assert len(sim.poly_unresolved) == cnt['poly_unresolved'] == cnt['lr_acts'] > 60 and len(sim.poly_refuted) == 0
    assert (sim.poly_unresolved[:, 2] == 2).all()
    sim.close()
    env = make_env(OVER)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        got = env.generate_logs(60, agent)
    assert_frames_equal(got, env._generate_logs_per_user(60, agent, 0))
    assert set(got['a'].dropna().astype(int)) == {2}


def test_a_refuted_act_sends_generate_logs_to_the_host_route():
    z1 = 25.0
    z2 = next(z for z in (z1 + 2.0 ** -e for e in range(20, 46)) if expit(z) == expit(z1))      # found by search: scipy merges them
    assert z2 > z1 and int(np.argmax(expit(np.array([0.0, z1, z2])))) == 1
    agent = constant_agent(z1, z2)
    env = make_env(OVER)
    with pytest.warns(RuntimeWarning, match='host route'):
        got = env.generate_logs(60, agent)
    assert_frames_equal(got, env._generate_logs_per_user(60, agent, 0))
    assert set(got['a'].dropna().astype(int)) == {1}          # the reference's action: the lower index of the merged pair


def history_agent(P=10):
    """Decisions that DEPEND on the history: z[2] = 25 exactly, z[1] = 25 + 2^-16 sum_j c_(n + j) // P g[p_j] with g in -3 .. 3 — the
    pair is within W = 4.9e-4 of each other for every history, a step of expit is 1.6e-5 wide here, and which of the two is larger,
    by how much, and whether scipy merges them changes with the views and their counts."""
    rng = np.random.RandomState(17)
    wa = np.zeros(P)
    wa[1], wa[2] = 25.0, 12.5
    wk = np.zeros((P, P))
    wk[1] = rng.randint(-3, 4, P) * 2.0 ** -16
    return LogregPolyFrozenAgent(Configuration({'num_products': P}), np.r_[np.zeros(P), wa, wk.reshape(-1)][None, :], [0.0])


def test_unresolved_acts_of_a_history_dependent_model_are_judged_on_the_right_history():
    """The listed (user, t, action) against an independent truth, the per-user host route's log: the bandit rows an act serves —
    the user's bandit rows from event t up to its next organic row — carry the reference's action exactly where the host
    confirmed the act, and every row on which the two logs differ is served by a refuted act."""
    from recogym_amd.sim import Simulator
    agent, n = history_agent(), 80
    env = make_env(OVER)
    want = env._generate_logs_per_user(n, agent, 0)
    sim = Simulator(Configuration({**env_1_args, **OVER}), n, device='cuda:0', **agent.device_policy())
    sim.reset_users(0, n)
    sim.run()
    rows = sim.rows()
    stands = sim.poly_verify()
    listed, refuted = sim.poly_unresolved, {tuple(int(x) for x in r) for r in sim.poly_refuted}
    sim.close()
    assert len(rows) == len(want) and not sim.poly_overflow
    wa_ = want['a'].to_numpy(dtype=np.float64, na_value=-1).astype(np.int64)
    u, t, z = rows['u'].astype(np.int64), rows['t'].astype(np.int64), rows['z']
    assert np.array_equal(z == 1, (want['z'] == 'bandit').to_numpy())
    differ = (z == 1) & (rows['a'] != wa_)
    covered = np.zeros(len(rows), dtype=bool)
    deep = 0
    for user, t_act, a in listed:
        mine = np.flatnonzero(u == user)
        later_organic = mine[(t[mine] > t_act) & (z[mine] == 0)]
        end = t[later_organic[0]] if len(later_organic) else np.iinfo(np.int64).max
        served = mine[(t[mine] >= t_act) & (t[mine] < end) & (z[mine] == 1)]
        assert len(served) and (rows['a'][served] == a).all(), (user, t_act, a)
        confirmed = (int(user), int(t_act), int(a)) not in refuted
        assert ((wa_[served] == a).all() if confirmed else (wa_[served] != a).all()), (user, t_act, a, confirmed)
        covered[served] |= not confirmed
        deep += int((z[mine] == 0)[t[mine] <= t_act].sum() > 1)
    print('unresolved', len(listed), 'refuted', len(refuted), 'with more than one view', deep, 'rows that differ', int(differ.sum()))
    assert np.array_equal(differ, covered) and stands == (len(refuted) == 0)
    assert len(listed) > 10 and deep > 5
    if refuted:
        with pytest.warns(RuntimeWarning, match='host route'):
            got = env.generate_logs(n, agent)
    else:
        got = env.generate_logs(n, agent)
    assert_frames_equal(got, want)


def test_test_agent_applies_the_protocol_too():
    """test_agent counts clicks from the device counters: with an act the host refutes it must count the host route's rows."""
    from scipy.stats.distributions import beta
    from recogym_amd.sim import Simulator
    z1 = 25.0
    z2 = next(z for z in (z1 + 2.0 ** -e for e in range(20, 46)) if expit(z) == expit(z1))
    agent, n = constant_agent(z1, z2), 300
    env = make_env(OVER)
    want = env._generate_logs_per_user(n, agent, 0)
    c = want[want['z'] == 'bandit']['c']
    s, f = int(c.sum()), int(c.shape[0]) - int(c.sum())
    sim = Simulator(Configuration({**env_1_args, **OVER}), n, device='cuda:0', log_capacity=0, **agent.device_policy())
    sim.reset_users(0, n)
    sim.run()
    dev_clicks = sim.counters()['clicks']
    sim.close()
    print('clicks: device alone', dev_clicks, 'host route', s)
    assert dev_clicks != s                                   # the unverified device counters would have been wrong
    with pytest.warns(RuntimeWarning, match='host route'):
        got = recogym.test_agent(env, agent, 0, n)
    assert got == (beta.ppf(0.5, s + 1, f + 1), beta.ppf(0.025, s + 1, f + 1), beta.ppf(0.975, s + 1, f + 1))
    # a confirmed act: the counters of the device run stand, no warning
    ok = constant_agent(25.0, 25.0 + 2.0 ** -12)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        got = recogym.test_agent(env, ok, 0, 60)
    c = env._generate_logs_per_user(60, ok, 0)
    c = c[c['z'] == 'bandit']['c']
    assert got[0] == beta.ppf(0.5, int(c.sum()) + 1, int(c.shape[0]) - int(c.sum()) + 1)
