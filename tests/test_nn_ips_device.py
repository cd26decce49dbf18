"""NnIpsAgent in the device step loop (RG_POLICY_NN_IPS, k_nn_acts): the reference's own logs row for row
(tests/golden/nn_ips_*.npz, tests/make_golden_nn_ips.py) with ps inside the proven bound, the device's unresolved set against the
host restatement of the rule, decisions placed to the bit over products x hidden units, constructed near-ties, generate_logs
against the per-user host route, and the unresolved-act protocol.  Needs a real MI355X."""
import warnings

import numpy as np
import pytest

import adversarial_util as au
import golden_util as gu
import nn_ips_util as nu
from device_util import make_env
import recogym_amd as recogym
from recogym_amd import _abi
from recogym_amd.agents import NnIpsAgent, NnIpsFrozenAgent, nn_ips_args
from recogym_amd.agents.nn_ips import UNRESOLVED, NnModel, nn_forward, nn_margin, nn_ps_bound, nn_rule
from recogym_amd.envs.configuration import Configuration
from recogym_amd.envs.reco_env_v1 import env_1_args

pytestmark = pytest.mark.gpu

K_POLY_HIST = 256           # kPolyHist: history entries a wave keeps in LDS


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def run_fixture(name, first_user=0, n_users=None, organic_only_below=0, ledger=False):
    from recogym_amd.sim import Simulator
    meta, cols = gu.load(name)
    P, n = meta['env_args']['num_products'], meta['n_users'] if n_users is None else n_users
    state = nu.fixture_state(meta, cols)
    frozen = NnIpsFrozenAgent(Configuration({'num_products': P}), state)
    sim = Simulator(gu.env_config(meta), n, device='cuda:0', **frozen.device_policy())
    sim.reset_users(first_user, n, organic_only_below=organic_only_below)
    sim.run()
    rows, cnt, raw = sim.rows(), sim.counters(), sim.sorted_log_host()[0]
    stands = sim.poly_verify()
    listed, refuted, overflow = sim.poly_unresolved.copy(), sim.poly_refuted.copy(), sim.poly_overflow
    launched = sim.get_option('launched_nn_ips')
    led = au.ledger(sim) if ledger else None
    sim.close()
    return dict(meta=meta, cols=cols, state=state, rows=rows, cnt=cnt, raw=raw, stands=stands, listed=listed, refuted=refuted,
                overflow=overflow, launched=launched, ledger=led)


def assert_run_equals_the_fixture(name, r, lockstep=False):
    """The results of a run of the fixture's users (run_fixture's dict; of several runs: rows and lists concatenated, counters
    summed) held to the fixture.  `lockstep`: the run took an event per launch (not the run-ahead rounds of the default form), where
    the device lists an unresolved act of a bandit user under the act's own event (nu.rule_over_log's t_lockstep)."""
    rows, cols, P = r['rows'], r['cols'], r['meta']['env_args']['num_products']
    no_ps = rows.copy()
    no_ps['ps'] = cols['ps']                                 # the integer columns here; ps below, against its own bound
    gu.assert_rows_equal(no_ps, cols, ps_rtol=0, what=name)
    acts = nu.rule_over_log(cols, P, r['state'])
    worst = 0.0
    for act in acts:
        for i in act['rows']:
            assert bits(rows['ps'][i]) == bits(act['ps']), (name, i, rows['ps'][i], act['ps'])        # the restatement, to the bit
            err = abs(rows['ps'][i] / cols['ps'][i] - 1.0)
            worst = max(worst, err / act['bound'])
            assert err <= act['bound'], (name, i, rows['ps'][i], cols['ps'][i], act['bound'])
    want = {(a['user'], a['t_lockstep' if lockstep else 't']) for a in acts if a['flags'] & UNRESOLVED}
    got = {(int(u), int(t)) for u, t, _ in r['listed']}
    print(name, {k: r['cnt'][k] for k in ('lr_acts', 'lr_rows', 'poly_unresolved')}, r['meta']['census'], 'worst ps error / bound', worst)
    assert r['stands'] and not r['overflow'] and len(r['refuted']) == 0
    assert got == want and r['cnt']['poly_unresolved'] == len(want) == r['meta']['census']['unresolved']
    assert r['cnt']['lr_acts'] == len(acts) and r['launched'] > 0
    assert 10 * len(want) <= len(acts)                      # at least 90 % of the acts are resolved on the device
    assert r['cnt']['live'] == 0 and r['cnt']['log_dropped'] == 0 and r['cnt']['hist_overflow'] == 0


@pytest.mark.parametrize('name', nu.FIXTURES)
def test_device_log_equals_the_fixture(name):
    assert_run_equals_the_fixture(name, run_fixture(name))


def test_two_runs_give_the_same_log():
    a, b = run_fixture('nn_ips_p40_loaded'), run_fixture('nn_ips_p40_loaded')
    assert np.array_equal(a['raw'], b['raw']) and a['cnt'] == b['cnt'] and np.array_equal(bits(a['rows']['ps']), bits(b['rows']['ps']))


# ------------------------------------------------------------------------------------------------
# decisions placed to the bit
# ------------------------------------------------------------------------------------------------
def random_state(P, H, rng, scale=0.5):
    shapes = dict(w1=(H, P), b1=(H,), w2=(H, H), b2=(H,), w3=(P, H), b3=(P,))
    return {k: (rng.standard_normal(s) * scale).astype(np.float32) for k, s in shapes.items()}


def debug_acts(P, state, nd, prod, cnt):
    """rg_sim_debug_set_history + rg_sim_debug_nn_acts -> (actions, flags, z, ps) of the users whose histories are given."""
    from recogym_amd.sim import Simulator
    n = len(nd)
    cfg = Configuration({**env_1_args, 'random_seed': 5, 'num_products': P, 'K': 2, 'sigma_omega': 0.0})
    sim = Simulator(cfg, n, device='cuda:0', policy=_abi.RG_POLICY_NN_IPS, policy_seed=0, ouc=dict(history_cap=max(prod.shape[1], 255)),
                    nn_ips=dict(state=state), log_capacity=0)
    sim.reset_users(0, n)
    sim.debug_set_history(nd, prod, cnt)
    out = sim.debug_nn_acts()
    sim.close()
    return out


def random_histories(P, rng):
    """0, 1, kPolyHist and kPolyHist + 1 distinct products (as many as P has), a few sizes between, counts up to 2^24 (the largest
    the rule resolves) and, on the last two users, beyond it."""
    sizes = sorted({min(s, P) for s in (0, 1, 2, 7, 16, K_POLY_HIST, K_POLY_HIST + 1)})
    users = [s for s in sizes for _ in range(3)] + [min(2, P)] * 2
    n, stride = len(users), max(max(sizes), 1)
    prod = np.zeros((n, stride), dtype=np.uint32)
    cnt = np.zeros((n, stride), dtype=np.uint32)
    for i, s in enumerate(users):
        prod[i, :s] = np.sort(rng.choice(P, s, replace=False))
        cnt[i, :s] = np.where(rng.rand(s) < 0.7, rng.randint(1, 4, s), rng.randint(1, 301, s))
        if s and i % 3 == 2:
            cnt[i, rng.randint(s)] = 1 << 24
    cnt[n - 2, 0], cnt[n - 1, 0] = (1 << 24) + 1, 0xFFFFFFFF
    return np.array(users, dtype=np.uint32), prod, cnt


def check_against_restatement(P, H, state, nd, prod, cnt, what):
    frozen = NnIpsFrozenAgent(Configuration({'num_products': P}), state)
    m = frozen.model
    act, fl, z, ps = debug_acts(P, state, nd, prod, cnt)
    seen = dict(resolved=0, unresolved=0)
    for i, s in enumerate(nd):
        p_i, c_i = prod[i, :s], cnt[i, :s]
        a_w, fl_w, z_w, ps_w = nn_rule(p_i, c_i, m)
        assert (act[i], fl[i]) == (a_w, fl_w), (what, i, s, act[i], fl[i], a_w, fl_w)
        assert np.array_equal(bits(z[i]), bits(z_w)), (what, i, s, np.abs(z[i] - z_w).max())
        assert bits(ps[i]) == bits(ps_w), (what, i, s, ps[i], ps_w)
        if not fl[i] & UNRESOLVED:
            host_a, host_ps = frozen.act_on(p_i, c_i)
            assert act[i] == host_a, (what, i, s)
            M1 = nn_forward(p_i, c_i, m)[3]
            assert abs(ps[i] / host_ps - 1.0) <= nn_ps_bound(s, M1, H, m.A2, m.A3, P), (what, i, s, ps[i], host_ps)
        seen['unresolved' if fl[i] & UNRESOLVED else 'resolved'] += 1
    return act, fl, seen


@pytest.mark.parametrize('H', [1, 20, 32, 33, 64, 65, 130])
@pytest.mark.parametrize('P', [2, 10, 65, 130])
def test_placed_decisions(P, H):
    """Random nets on random histories: the device's actions, flags, logits and ps are the NumPy restatement's to the bit, and every
    resolved action is the torch forward's, its ps within nn_ps_bound.  (The three matrices fit the block's LDS at P = 65, H = 33 and no longer at
    P = 65, H = 64: both forms of the weight reads are met.)"""
    rng = np.random.RandomState(1000 * P + H)
    state = random_state(P, H, rng)
    nd, prod, cnt = random_histories(P, rng)
    act, fl, seen = check_against_restatement(P, H, state, nd, prod, cnt, (P, H))
    print(P, H, seen)
    assert fl[-1] & UNRESOLVED and fl[-2] & UNRESOLVED       # a count that is not an fp32 value
    assert seen['resolved'] > 0 or P == 2 or H == 1


@pytest.mark.parametrize('H', [830, 1024])
def test_placed_decisions_at_the_hidden_cap(H):
    """The largest net the device form accepts, and one just past the point where the layer vectors (64 H bytes of dynamic LDS) plus
    the kernel's 12.3 KB of static LDS leave 64 KiB although the dynamic part alone does not: the launch needs the opt-in on
    the total."""
    P = 10
    rng = np.random.RandomState(H)
    nd, prod, cnt = random_histories(P, rng)
    act, fl, seen = check_against_restatement(P, H, random_state(P, H, rng, 0.05), nd, prod, cnt, ('cap', H))
    print(H, seen)
    assert seen['resolved'] > 0


def test_histories_beyond_the_lds_row():
    """kPolyHist and kPolyHist + 1 distinct products need more than 256 products: P = 300, H = 20."""
    P, H = 300, 20
    rng = np.random.RandomState(77)
    nd, prod, cnt = random_histories(P, rng)
    assert K_POLY_HIST in nd and K_POLY_HIST + 1 in nd
    act, fl, seen = check_against_restatement(P, H, random_state(P, H, rng, 0.2), nd, prod, cnt, 'P300')
    assert seen['resolved'] > 0


@pytest.mark.parametrize('P,H', [(10, 20), (130, 65)])
def test_constructed_near_ties(P, H):
    """Two identical rows of W3 (the best two actions by a wide margin), b3 differing by 0, W / 2 and 4 W: unresolved for 0 and W / 2,
    resolved with the right action for 4 W; the exact tie is confirmed by the host as the first index wherever the host's own two
    logits are equal (its BLAS may add two identical rows in different orders: then either of the two is its answer, which is why the
    device lists the act)."""
    rng = np.random.RandomState(31 * P + H)
    lo, hi = 1, P - 1
    base = random_state(P, H, rng, 0.3)
    base['w3'][lo] = np.abs(base['w3'][lo]) + 1.0            # h2 > 0: these two logits lead the rest by about H / 2
    base['w3'][hi] = base['w3'][lo]
    base['b3'][lo] = base['b3'][hi] = 0.0
    nd = np.array([1, 2, 0], dtype=np.uint32)
    prod = np.array([[3 % P, 0], [1, P - 1], [0, 0]], dtype=np.uint32)
    cnt = np.array([[2, 0], [1, 5], [0, 0]], dtype=np.uint32)
    m0 = NnModel(base)
    W = max(float(nn_margin(s, nn_forward(prod[i, :s], cnt[i, :s], m0)[3], H, m0.A2, m0.A3)) for i, s in enumerate(nd))
    for name, delta, want_fl, want_a in (('tie', 0.0, UNRESOLVED, lo), ('W / 2', W / 2, UNRESOLVED, None), ('4 W', 4 * W, 0, hi),
                                         ('4 W, the lower index', -4 * W, 0, lo)):
        state = {k: v.copy() for k, v in base.items()}
        state['b3'][hi] = np.float32(delta)
        act, fl, seen = check_against_restatement(P, H, state, nd, prod, cnt, (P, H, name))
        assert (fl == want_fl).all(), (name, fl)
        if want_a is not None:
            assert (act == want_a).all(), (name, act)
        if name == 'tie':
            import torch
            frozen = NnIpsFrozenAgent(Configuration({'num_products': P}), state)
            for i, s in enumerate(nd):
                x = np.zeros((1, P), dtype=np.float32)
                x[0, prod[i, :s]] = cnt[i, :s]
                with torch.no_grad():
                    logits = frozen.net[:5](torch.from_numpy(x))[0].numpy()
                host = frozen.act_on(prod[i, :s], cnt[i, :s])[0]
                assert host in (lo, hi) and (host == lo or logits[lo] != logits[hi]), (i, host, logits[lo], logits[hi])


# ------------------------------------------------------------------------------------------------
# routes
# ------------------------------------------------------------------------------------------------
OVER = dict(random_seed=321, num_products=10, K=4)


def assert_frames_equal_ps_bounded(got, want, P, state):
    """Every column but ps equal; ps within the act's nn_ps_bound of the host route's (torch's fp32 value)."""
    assert len(got) == len(want)
    for k in ('t', 'u', 'v', 'a', 'c'):
        assert np.array_equal(got[k].to_numpy(dtype=np.float64, na_value=np.nan), want[k].to_numpy(dtype=np.float64, na_value=np.nan), equal_nan=True), k
    assert ((got['z'] == 'bandit') == (want['z'] == 'bandit')).all()
    cols = dict(u=want['u'].to_numpy(dtype=np.int64), z=(want['z'] == 'bandit').to_numpy().astype(np.int64),
                v=want['v'].to_numpy(dtype=np.float64, na_value=0).astype(np.int64))
    g, w = got['ps'].to_numpy(dtype=np.float64, na_value=np.nan), want['ps'].to_numpy(dtype=np.float64, na_value=np.nan)
    for act in nu.rule_over_log(dict(cols, a=want['a'].to_numpy(dtype=np.float64, na_value=-1).astype(np.int64)), P, state):
        for i in act['rows']:
            assert abs(g[i] / w[i] - 1.0) <= act['bound'], (i, g[i], w[i], act['bound'])
    assert np.array_equal(np.isnan(g), np.isnan(w))


def trained_agent():
    """-> the meta of nn_ips_p10, NnIpsAgent trained on the fixture's training log"""
    import torch
    from make_golden_ope import log_frame
    meta, cols = gu.load('nn_ips_p10')
    train = {k[len('trainlog_'):]: v for k, v in cols.items() if k.startswith('trainlog_')}
    agent = NnIpsAgent(Configuration({**nn_ips_args, 'num_products': 10, 'random_seed': 7}))
    agent.train_from_log(log_frame(train))
    torch.manual_seed(7)
    agent.build()
    return meta, agent


def test_generate_logs_with_the_trained_agent_equals_the_host_route():
    meta, agent = trained_agent()
    env = make_env(meta['env_args'])
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        got = env.generate_logs(100, agent)
    want = env._generate_logs_per_user(100, agent, 0)
    assert_frames_equal_ps_bounded(got, want, 10, agent.frozen.state())
    ps = got['ps'].to_numpy(dtype=np.float64, na_value=np.nan)[(got['z'] == 'bandit').to_numpy()]
    assert ((ps > 0.0) & (ps < 1.0)).all()                    # a model output, not the constant 1


def tie_agent(b_hi, P=10, H=4):
    """w1 = w2 = 0 and two identical rows of w3: whatever the history, z[1] = c and z[2] = c + b_hi lead the rest."""
    state = dict(w1=np.zeros((H, P)), b1=np.zeros(H), w2=np.zeros((H, H)), b2=np.zeros(H), w3=np.zeros((P, H)), b3=np.full(P, -5.0))
    state['w3'][1] = state['w3'][2] = 1.0
    state['b3'][1], state['b3'][2] = 0.0, b_hi
    return NnIpsFrozenAgent(Configuration({'num_products': P}), {k: v.astype(np.float32) for k, v in state.items()})


def test_an_unresolved_act_the_host_confirms_keeps_the_device_route():
    from recogym_amd.sim import Simulator
    agent = tie_agent(0.0)
    sim = Simulator(Configuration({**env_1_args, **OVER}), 60, device='cuda:0', **agent.device_policy())
    sim.reset_users(0, 60)
    sim.run()
    cnt = sim.counters()
    assert sim.poly_verify() and not sim.poly_overflow
    assert len(sim.poly_unresolved) == cnt['poly_unresolved'] == cnt['lr_acts'] > 60 and len(sim.poly_refuted) == 0
    assert (sim.poly_unresolved[:, 2] == 1).all()
    sim.close()
    env = make_env(OVER)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        got = env.generate_logs(60, agent)
    assert_frames_equal_ps_bounded(got, env._generate_logs_per_user(60, agent, 0), 10, agent.state())
    assert set(got['a'].dropna().astype(int)) == {1}


def refuted_agent():
    """b3[2] = 2^-30: the device's float64 logits put action 2 ahead by 2^-30, inside the margin, so the act is listed; in torch's
    fp32 forward the sum 2 + 2^-30 rounds to 2, the two logits tie and the first maximum is action 1."""
    agent = tie_agent(2.0 ** -30)
    a, fl, z, _ = nn_rule([3], [1], agent.model)
    assert (a, fl) == (2, UNRESOLVED) and z[2] - z[1] == 2.0 ** -30
    assert agent.act_on([3], [1])[0] == 1                      # the host's own forward decides what the reference does
    return agent


def test_a_refuted_act_sends_generate_logs_to_the_host_route():
    agent = refuted_agent()
    env = make_env(OVER)
    with pytest.warns(RuntimeWarning, match='host route'):
        got = env.generate_logs(60, agent)
    want = env._generate_logs_per_user(60, agent, 0)
    from device_util import assert_frames_equal
    assert_frames_equal(got, want)                            # the host route itself: its ps too
    assert set(got['a'].dropna().astype(int)) == {1}


def test_test_agent_applies_the_protocol():
    """test_agent counts clicks from the device counters: with an act the host refutes it must count the host route's rows."""
    from scipy.stats.distributions import beta
    agent, n = refuted_agent(), 300
    env = make_env(OVER)
    want = env._generate_logs_per_user(n, agent, 0)
    c = want[want['z'] == 'bandit']['c']
    s, f = int(c.sum()), int(c.shape[0]) - int(c.sum())
    with pytest.warns(RuntimeWarning, match='host route'):
        got = recogym.test_agent(env, agent, 0, n)
    assert got == (beta.ppf(0.5, s + 1, f + 1), beta.ppf(0.025, s + 1, f + 1), beta.ppf(0.975, s + 1, f + 1))
    ok = tie_agent(0.0)                                        # a confirmed act: the counters of the device run stand, no warning
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        got = recogym.test_agent(env, ok, 0, 60)
    c = env._generate_logs_per_user(60, ok, 0)
    c = c[c['z'] == 'bandit']['c']
    assert got[0] == beta.ppf(0.5, int(c.sum()) + 1, int(c.shape[0]) - int(c.sum()) + 1)


def test_out_of_range_combinations_are_refused():
    from device_util import handle
    import torch
    lib, h, ws = handle(_abi.RG_POLICY_NN_IPS)
    H = 4
    arr = [torch.zeros(n, dtype=torch.float64, device='cuda:0') for n in (10 * H, H, H * H, H, H * 10, 10)]
    ptr = [a.data_ptr() for a in arr]
    assert lib.rg_sim_set_nn_ips(h, *ptr, 0) == -1 and b'num_hidden' in lib.rg_last_error()
    assert lib.rg_sim_set_nn_ips(h, *ptr, 1025) == -1 and b'num_hidden' in lib.rg_last_error()
    assert lib.rg_sim_set_nn_ips(h, *ptr[:3], None, *ptr[4:], H) == -1 and b'NULL' in lib.rg_last_error()
    arr[2][1] = float('inf')
    assert lib.rg_sim_set_nn_ips(h, *ptr, H) == -1 and b'finite' in lib.rg_last_error()
    arr[2][1] = 0.0
    assert lib.rg_sim_set_nn_ips(h, *ptr, H) == 0
    cdf = torch.ones(9, dtype=torch.float64, device='cuda:0')
    assert lib.rg_sim_set_epsilon_greedy_model(h, 0.1, 1, 1, cdf.data_ptr(), 0.01, 0.9) == -1 and b'NN_IPS' in lib.rg_last_error()
    lib.rg_sim_destroy(h)
    lib, h, ws = handle(_abi.RG_POLICY_LOGREG_POLY)
    assert lib.rg_sim_set_nn_ips(h, *ptr, H) == -4
    lib.rg_sim_destroy(h)
    lib, h, ws = handle(_abi.RG_POLICY_NN_IPS, P=4001)
    assert lib.rg_sim_set_nn_ips(h, *ptr, H) == -1 and b'products' in lib.rg_last_error()
    lib.rg_sim_destroy(h)


def test_select_randomly_batched_host_route_equals_the_per_user_route():
    """select_randomly has no device form; its host act draws one addressed policy uniform, so the per-slot copies of the batched
    host route give the per-user route's rows."""
    from device_util import assert_frames_equal
    rng = np.random.RandomState(8)
    agent = NnIpsFrozenAgent(Configuration({'num_products': 10, 'select_randomly': True, 'random_seed': 5}), random_state(10, 20, rng, 1.0))
    assert agent.device_policy() is None
    env = make_env(OVER)
    got = env._generate_logs_batched(40, agent, 0)
    assert_frames_equal(got, env._generate_logs_per_user(40, agent, 0))
    assert len(set(got['a'].dropna().astype(int))) > 3
