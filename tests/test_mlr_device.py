"""PyTorchMLRAgent in the device step loop (RG_POLICY_MLR, k_mlr_acts): the reference's own logs row for row
(tests/golden/mlr_*.npz, tests/make_golden_mlr.py), the device's unresolved set against the host restatement of the rule, every run
form, two shards and offset ids, decisions placed to the bit, constructed near-ties, generate_logs and test_agent against the
per-user host route, and the unresolved-act protocol.  Needs a real MI355X."""
import warnings

import numpy as np
import pytest

import adversarial_util as au
import golden_util as gu
import mlr_util as mu
from device_util import assert_frames_equal, make_env
from test_agent_run_forms import SPLIT, assert_form, cat_rows, set_form, sum_counters
import recogym_amd as recogym
from recogym_amd import _abi
from recogym_amd.agents import PyTorchMLRAgent, PyTorchMLRFrozenAgent, pytorch_mlr_args
from recogym_amd.agents.pytorch_mlr import COUNT_CAP, UNRESOLVED, mlr_forward, mlr_margin, mlr_rule, mlr_table
from recogym_amd.envs.configuration import Configuration
from recogym_amd.envs.reco_env_v1 import env_1_args

pytestmark = pytest.mark.gpu

K_POLY_HIST = 256           # kPolyHist: history entries a wave keeps in LDS
ACT = ('mlr',)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def ledger(sim):
    return dict(au.ledger(sim), mlr=sim.get_option('launched_mlr'))


def run_fixture(name, first_user=0, n_users=None, organic_only_below=0):
    from recogym_amd.sim import Simulator
    meta, cols = gu.load(name)
    P, n = meta['env_args']['num_products'], meta['n_users'] if n_users is None else n_users
    W = mu.fixture_weight(meta, cols)
    frozen = PyTorchMLRFrozenAgent(Configuration({'num_products': P}), W)
    pol = {k: v for k, v in frozen.device_policy().items() if k != 'ps_all'}
    sim = Simulator(gu.env_config(meta), n, device='cuda:0', **pol)
    sim.reset_users(first_user, n, organic_only_below=organic_only_below)
    sim.run()
    rows, cnt, raw = sim.rows(), sim.counters(), sim.sorted_log_host()[0]
    stands = sim.poly_verify()
    listed, refuted, overflow = sim.poly_unresolved.copy(), sim.poly_refuted.copy(), sim.poly_overflow
    led = ledger(sim)
    sim.close()
    return dict(meta=meta, cols=cols, W=W, rows=rows, cnt=cnt, raw=raw, stands=stands, listed=listed, refuted=refuted, overflow=overflow,
                ledger=led)


def join(rs):
    return dict(rs[0], rows=cat_rows([x['rows'] for x in rs]), cnt=sum_counters([x['cnt'] for x in rs]),
                listed=np.concatenate([x['listed'] for x in rs]), refuted=np.concatenate([x['refuted'] for x in rs]),
                overflow=any(x['overflow'] for x in rs), stands=all(x['stands'] for x in rs))


def assert_run_equals_the_fixture(name, r, lockstep=False):
    """The rows, ps (the constant 1) and the counters are the reference's log bit for bit; the listed unresolved acts are mlr_rule's
    over the log; the host confirms every one of them.  `lockstep`: the run took an event per launch, where the device lists an
    unresolved act of a bandit user under the act's own event (mlr_util.rule_over_log's t_lockstep)."""
    rows, cols, P = r['rows'], r['cols'], r['meta']['env_args']['num_products']
    gu.assert_rows_equal(rows, cols, ps_rtol=0, what=name)
    is_b = cols['z'] == 1
    assert np.array_equal(bits(rows['ps'][is_b]), bits(np.ones(int(is_b.sum()))))
    acts = mu.rule_over_log(cols, P, r['W'])
    want = {(a['user'], a['t_lockstep' if lockstep else 't']) for a in acts if a['flags'] & UNRESOLVED}
    got = {(int(u), int(t)) for u, t, _ in r['listed']}
    print(name, {k: r['cnt'][k] for k in ('lr_acts', 'lr_rows', 'poly_unresolved')}, r['meta']['census'])
    assert r['stands'] and not r['overflow'] and len(r['refuted']) == 0
    assert got == want and r['cnt']['poly_unresolved'] == len(want) == len(r['listed']) == r['meta']['census']['unresolved']
    assert r['cnt']['lr_acts'] == len(acts) and r['ledger']['mlr'] > 0
    assert r['cnt']['organic'] == int((cols['z'] == 0).sum()) and r['cnt']['bandit'] + r['cnt']['phantom'] == int(is_b.sum()) and r['cnt']['clicks'] == int((cols['c'] == 1).sum())
    assert r['cnt']['live'] == 0 and r['cnt']['log_dropped'] == 0 and r['cnt']['hist_overflow'] == 0
    if name == 'mlr_p10_ties':
        assert 5 * len(want) >= len(acts) and {int(a) for _, _, a in r['listed']} == {1}      # the lowest index of the tied pair


@pytest.mark.parametrize('name', mu.FIXTURES)
def test_device_log_equals_the_fixture(name, monkeypatch):
    set_form('default', monkeypatch)
    assert_run_equals_the_fixture(name, run_fixture(name))


THREE = ('lockstep', 'repack_lockstep', 'repack_rounds')
FORM_CASES = [(n, f) for n in ('mlr_p40_a05', 'mlr_p10_ties') for f in THREE] + [('mlr_p10_sigma0', f) for f in ('repack_lockstep', 'nocache_rounds')]


@pytest.mark.parametrize('name,form', FORM_CASES)
def test_fixture_in_form(name, form, monkeypatch):
    set_form(form, monkeypatch)
    r = run_fixture(name)
    print(name, form, {k: v for k, v in r['ledger'].items() if v and k not in au.DESCRIPTORS})
    assert_form(r['ledger'], form, ACT)
    assert_run_equals_the_fixture(name, r, lockstep=r['ledger']['advance_run'] == 0)


def test_fixture_as_two_shards(monkeypatch):
    """Users [0, 37) in the default form and [37, n) in repacked rounds: the rows concatenated, the lists joined and the counters
    summed are the fixture's."""
    name = 'mlr_p40_a05'
    n = gu.load(name)[0]['n_users']
    assert 0 < SPLIT < n and (n - SPLIT) % 64
    set_form('default', monkeypatch)
    a = run_fixture(name, first_user=0, n_users=SPLIT)
    set_form('repack_rounds', monkeypatch)
    b = run_fixture(name, first_user=SPLIT, n_users=n - SPLIT)
    assert_form(b['ledger'], 'repack_rounds', ACT)
    assert a['ledger']['mlr'] > 0 and (a['ledger']['advance_run'] == 0) == (b['ledger']['advance_run'] == 0)
    assert_run_equals_the_fixture(name, join([a, b]), lockstep=a['ledger']['advance_run'] == 0)


def test_two_runs_give_the_same_log(monkeypatch):
    set_form('default', monkeypatch)
    a, b = run_fixture('mlr_p40_a05'), run_fixture('mlr_p40_a05')
    assert np.array_equal(a['raw'], b['raw']) and a['cnt'] == b['cnt'] and np.array_equal(a['listed'], b['listed'])


# ------------------------------------------------------------------------------------------------
# decisions placed to the bit
# ------------------------------------------------------------------------------------------------
def debug_acts(P, W, nd, prod, cnt):
    """rg_sim_debug_set_history + rg_sim_debug_mlr_acts -> (actions, flags, z) of the users whose histories are given."""
    from recogym_amd.sim import Simulator
    n = len(nd)
    cfg = Configuration({**env_1_args, 'random_seed': 5, 'num_products': P, 'K': 2, 'sigma_omega': 0.0})
    sim = Simulator(cfg, n, device='cuda:0', policy=_abi.RG_POLICY_MLR, policy_seed=0, ouc=dict(history_cap=max(prod.shape[1], 255)),
                    mlr=dict(state=dict(W=W)), log_capacity=0)
    sim.reset_users(0, n)
    sim.debug_set_history(nd, prod, cnt)
    out = sim.debug_mlr_acts()
    sim.close()
    return out


def placed_histories(P, rng, sizes):
    """Per size three random histories (the third with a count of 2^24, the largest the rule resolves), the empty one, one product,
    all products, and on the last two users a count of 2^24 + 1 and of 2^32 - 1."""
    sizes = sorted({min(s, P) for s in sizes} | {0, 1, P})
    users = [s for s in sizes for _ in range(3)] + [min(2, P)] * 2
    n, stride = len(users), max(max(sizes), 1)
    prod = np.zeros((n, stride), dtype=np.uint32)
    cnt = np.zeros((n, stride), dtype=np.uint32)
    for i, s in enumerate(users):
        prod[i, :s] = np.sort(rng.choice(P, s, replace=False))
        cnt[i, :s] = np.where(rng.rand(s) < 0.7, rng.randint(1, 4, s), rng.randint(1, 301, s))
        if s and i % 3 == 2:
            cnt[i, rng.randint(s)] = COUNT_CAP
    cnt[n - 2, 0], cnt[n - 1, 0] = COUNT_CAP + 1, 0xFFFFFFFF
    return np.array(users, dtype=np.uint32), prod, cnt


def check_against_restatement(P, W, nd, prod, cnt, what):
    frozen = PyTorchMLRFrozenAgent(Configuration({'num_products': P}), W)
    wt = mlr_table(W)
    act, fl, z = debug_acts(P, W, nd, prod, cnt)
    seen = dict(resolved=0, unresolved=0)
    for i, s in enumerate(nd):
        p_i, c_i = prod[i, :s], cnt[i, :s]
        a_w, fl_w, z_w = mlr_rule(p_i, c_i, wt)
        assert (act[i], fl[i]) == (a_w, fl_w), (what, i, s, act[i], fl[i], a_w, fl_w)
        assert np.array_equal(bits(z[i]), bits(z_w)), (what, i, s, np.abs(z[i] - z_w).max())
        if not fl[i] & UNRESOLVED:
            assert act[i] == frozen.act_on(p_i, c_i)[0], (what, i, s)
        seen['unresolved' if fl[i] & UNRESOLVED else 'resolved'] += 1
    return act, fl, seen


@pytest.mark.parametrize('P', [2, 10, 64, 65, 130])
def test_placed_decisions(P):
    """Random weights on placed histories: the device's actions, flags and scores are the NumPy restatement's to the bit, and every
    resolved action is the host act's.  (The table is in the block's LDS up to P = 78: 64 and 65 are staged over one and two passes
    of the lanes, 130 reads global memory.)"""
    rng = np.random.RandomState(1000 + P)
    W = (rng.standard_normal((P, P)) * 0.5).astype(np.float32)
    nd, prod, cnt = placed_histories(P, rng, (2, 7, 16))
    act, fl, seen = check_against_restatement(P, W, nd, prod, cnt, P)
    print(P, seen)
    assert fl[-1] & UNRESOLVED and fl[-2] & UNRESOLVED       # a count that is not an fp32 value
    assert fl[0] & UNRESOLVED and act[0] == 0 and nd[0] == 0  # the empty history
    assert seen['resolved'] > 0


def test_histories_beyond_the_lds_row():
    """290 distinct viewed products of P = 300: more than the kPolyHist = 256 entries a wave keeps in LDS (and 256, 257 beside)."""
    P = 300
    rng = np.random.RandomState(77)
    nd, prod, cnt = placed_histories(P, rng, (K_POLY_HIST, K_POLY_HIST + 1, 290))
    assert {K_POLY_HIST, K_POLY_HIST + 1, 290, 300} <= set(nd.tolist())
    act, fl, seen = check_against_restatement(P, (rng.standard_normal((P, P)) * 0.2).astype(np.float32), nd, prod, cnt, 'P300')
    assert seen['resolved'] > 0


@pytest.mark.parametrize('P', [10, 130])
def test_constructed_near_ties(P):
    """Two rows of W (actions lo < hi) that lead the rest by a wide margin on the histories of test_nn_ips_device's near-tie test;
    hi's row is lo's plus delta on the viewed products: a score difference of exactly 0, of just under 2 E, of just over 2 E (both
    ways round).  The flag is set exactly where mlr_rule sets it — unresolved, unresolved, resolved — and the lowest index wins the
    exact tie."""
    rng = np.random.RandomState(31 * P)
    lo, hi = 1, P - 1
    base = (rng.standard_normal((P, P)) * 0.3).astype(np.float32)
    base[lo] = np.abs(base[lo]) + 4.0
    nd = np.array([1, 2], dtype=np.uint32)
    prod = np.array([[3 % P, 0], [1, P - 1]], dtype=np.uint32)
    cnt = np.array([[2, 0], [1, 5]], dtype=np.uint32)
    for name, ulps, want_fl, want_a in (('tie', 0, UNRESOLVED, lo), ('under', None, UNRESOLVED, hi), ('over', None, 0, hi),
                                        ('over, the lower index', None, 0, lo)):
        for i in range(2):
            W = base.copy()
            W[hi] = W[lo]
            p_i, c_i = prod[i, :nd[i]], cnt[i, :nd[i]]
            if ulps is None:
                # move hi's weight of the first viewed product by whole fp32 ulps until the device's gap is on the wanted side of 2 E
                p0, sign = int(p_i[0]), -1.0 if name.endswith('index') else 1.0
                step = np.spacing(W[lo, p0])
                k_over = next(k for k in range(1, 1 << 12) if _gap(W, lo, hi, p0, sign * k * step, p_i, c_i) > 0)
                k = k_over if name.startswith('over') else k_over - 1
                assert k >= 1, 'no whole ulp lies under 2 E: widen the counts'
                W[hi, p0] = W[lo, p0] + np.float32(sign * k * step)
            act, fl, _ = check_against_restatement(P, W, nd[i:i + 1], prod[i:i + 1], cnt[i:i + 1], (P, name, i))
            assert fl[0] == want_fl and act[0] == want_a, (name, i, fl, act)


def _gap(W, lo, hi, p0, delta, prods, cnts):
    """(best - second best) - 2 E of the device's rule with W[hi][p0] = W[lo][p0] + delta."""
    W = W.copy()
    W[hi, p0] = W[lo, p0] + np.float32(delta)
    z, a, M1 = mlr_forward(prods, cnts, mlr_table(W))
    return abs(z[hi] - z[lo]) - 2.0 * mlr_margin(len(prods), M1)


# ------------------------------------------------------------------------------------------------
# routes
# ------------------------------------------------------------------------------------------------
OVER = dict(random_seed=321, num_products=10, K=4)


def trained_agent():
    """-> the meta of mlr_p10_a05, PyTorchMLRAgent trained on the fixture's training log"""
    import torch
    from make_golden_ope import log_frame
    meta, _ = gu.load('mlr_p10_a05')
    agent = PyTorchMLRAgent(Configuration({**pytorch_mlr_args, 'num_products': 10, 'random_seed': 7, 'alpha': 0.5}))
    agent.train_from_log(log_frame(mu.training_log('mlr_p10_a05')))
    torch.manual_seed(7)
    agent.build()
    return meta, agent


@pytest.fixture(scope='module')
def trained():
    return trained_agent()


def assert_frames_equal_with_ps_all(got, want, P):
    """Column for column, `ps-a` too: the one-hot vector at the action on bandit rows, None on organic rows."""
    assert_frames_equal(got, want)
    is_b = (want['z'] == 'bandit').to_numpy()
    for g, w, b, a in zip(got['ps-a'], want['ps-a'], is_b, want['a']):
        if b:
            assert np.array_equal(g, w) and g.shape == (P,) and g[int(a)] == 1.0 and g.sum() == 1.0
        else:
            assert g is None or (hasattr(g, '__len__') and len(g) == 0)
            assert w is None or (hasattr(w, '__len__') and len(w) == 0)


def test_generate_logs_with_the_trained_agent_equals_the_host_route(trained, monkeypatch):
    set_form('default', monkeypatch)
    meta, agent = trained
    env = make_env(meta['env_args'])
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        got = env.generate_logs(100, agent)
    want = env._generate_logs_per_user(100, agent, 0)
    assert_frames_equal_with_ps_all(got, want, 10)
    assert len(set(got['a'].dropna().astype(int))) >= 3
    assert (got['ps'][got['z'] == 'bandit'] == 1.0).all()


FIRST_ID, N_ORGANIC, N_OFFLINE = 65530, 10, 40          # the ids cross 65 535: the frame's `u` column goes to 32 bits


def test_offset_ids_with_organic_only_users_equal_the_host_route(trained, monkeypatch):
    from recogym_amd.envs.reco_env_v1 import RecoEnv1
    meta, agent = trained
    set_form('default', monkeypatch)
    env = make_env(meta['env_args'])
    want = env._generate_logs_per_user(N_OFFLINE, agent, N_ORGANIC, FIRST_ID)
    u, is_b = want['u'].to_numpy(dtype=np.int64), (want['z'] == 'bandit').to_numpy()
    assert u.min() == FIRST_ID and u.max() == FIRST_ID + N_OFFLINE + N_ORGANIC - 1 > 65535
    assert not is_b[u < FIRST_ID + N_ORGANIC].any() and is_b[u >= FIRST_ID + N_ORGANIC].any()
    seen, real = [], RecoEnv1.simulate

    def spy(self, *a, **k):
        cnt, sim = real(self, *a, **k)
        seen.append(ledger(sim))
        return cnt, sim
    monkeypatch.setattr(RecoEnv1, 'simulate', spy)
    for form in ('default', 'repack_tail'):            # (repack_tail's switches: the repack on, the rest as generate_logs runs by default)
        set_form(form, monkeypatch)
        del seen[:]
        with warnings.catch_warnings():
            warnings.simplefilter('error', RuntimeWarning)       # a fallback to the host route warns: it fails here
            got = make_env(meta['env_args']).generate_logs(N_OFFLINE, agent, num_organic_offline_users=N_ORGANIC, first_user_id=FIRST_ID)
        assert len(seen) == 1, 'generate_logs made no device run, or more than one'
        led = seen[0]
        assert (led['repack'] > 0) == (form != 'default') and led['tail'] == 0 and led['mlr'] > 0, led
        assert_frames_equal_with_ps_all(got, want, 10)
        ids, gb = got['u'].to_numpy(dtype=np.int64), (got['z'] == 'bandit').to_numpy()
        assert not gb[ids < FIRST_ID + N_ORGANIC].any(), 'an organic-only user logged a bandit row'


def tie_agent(w_hi, P=10):
    """Rows 1 and 2 of W lead the rest on every history: W[1] = 1 everywhere, W[2] = 1 but for W[2][3] = w_hi, the rest -5."""
    W = np.full((P, P), -5.0, dtype=np.float32)
    W[1] = W[2] = 1.0
    W[2, 3] = w_hi
    return PyTorchMLRFrozenAgent(Configuration({'num_products': P}), W)


def test_an_unresolved_act_the_host_confirms_keeps_the_device_route(monkeypatch):
    from recogym_amd.sim import Simulator
    set_form('default', monkeypatch)
    agent = tie_agent(1.0)
    pol = {k: v for k, v in agent.device_policy().items() if k != 'ps_all'}
    sim = Simulator(Configuration({**env_1_args, **OVER}), 60, device='cuda:0', **pol)
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
    assert_frames_equal_with_ps_all(got, env._generate_logs_per_user(60, agent, 0), 10)
    assert set(got['a'].dropna().astype(int)) == {1}


def patch_host_act(monkeypatch, action):
    """The host act of the confirmation (sim.mlr_host_act) patched to answer `action`: it disagrees with every listed act."""
    from recogym_amd import sim as sim_module
    monkeypatch.setattr(sim_module, 'mlr_host_act', lambda views, P, agent: action)


def test_a_refuted_act_sends_generate_logs_to_the_host_route(monkeypatch):
    set_form('default', monkeypatch)
    agent = tie_agent(1.0)
    patch_host_act(monkeypatch, 2)
    env = make_env(OVER)
    with pytest.warns(RuntimeWarning, match='PyTorchMLRAgent.*host route'):
        got = env.generate_logs(60, agent)
    want = env._generate_logs_per_user(60, agent, 0)
    assert_frames_equal_with_ps_all(got, want, 10)            # the host route itself
    assert set(got['a'].dropna().astype(int)) == {1}


def test_test_agent_applies_the_protocol(trained, monkeypatch):
    """test_agent with the training agent: the offline protocol trains it from a device log, the evaluation runs k_mlr_acts, and the
    result is the host route's.  With an act the host refutes it counts the host route's rows, after the warning."""
    from scipy.stats.distributions import beta
    import torch
    set_form('default', monkeypatch)
    env = make_env(OVER)
    agent = PyTorchMLRAgent(Configuration({**pytorch_mlr_args, 'num_products': 10, 'random_seed': 7}))
    torch.manual_seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        got = recogym.test_agent(env, agent, 60, 80)
    # the same protocol by hand: train on the uniform log of users [0, 60), evaluate users [60, 140) on the per-user host route
    cnt, sim = env.simulate(60, None, 0, first_user_id=0)
    again = PyTorchMLRAgent(Configuration({**pytorch_mlr_args, 'num_products': 10, 'random_seed': 7}))
    again.train_from_log(sim.log_columns(), 0)
    sim.close()
    torch.manual_seed(3)
    again.build()
    c = env._generate_logs_per_user(80, again, 0, 60)
    c = c[c['z'] == 'bandit']['c']
    s, f = int(c.sum()), int(c.shape[0]) - int(c.sum())
    assert got == (beta.ppf(0.5, s + 1, f + 1), beta.ppf(0.025, s + 1, f + 1), beta.ppf(0.975, s + 1, f + 1))
    # a refuted act: the host route's rows, after the warning
    tie = tie_agent(1.0)
    want = env._generate_logs_per_user(100, tie, 0)
    c = want[want['z'] == 'bandit']['c']
    s, f = int(c.sum()), int(c.shape[0]) - int(c.sum())
    patch_host_act(monkeypatch, 2)
    with pytest.warns(RuntimeWarning, match='host route'):
        got = recogym.test_agent(env, tie, 0, 100)
    assert got == (beta.ppf(0.5, s + 1, f + 1), beta.ppf(0.025, s + 1, f + 1), beta.ppf(0.975, s + 1, f + 1))


def test_out_of_range_combinations_are_refused():
    from device_util import handle
    import torch
    lib, h, ws = handle(_abi.RG_POLICY_MLR)
    wt = torch.zeros(100, dtype=torch.float64, device='cuda:0')
    assert lib.rg_sim_set_mlr(h, None) == -1 and b'NULL' in lib.rg_last_error()
    assert lib.rg_sim_set_mlr(None, wt.data_ptr()) == -1
    for bad in (float('inf'), float('nan')):
        wt[37] = bad
        assert lib.rg_sim_set_mlr(h, wt.data_ptr()) == -1 and b'finite' in lib.rg_last_error()
    wt[37] = 0.0
    assert lib.rg_sim_debug_mlr_acts(h, wt.data_ptr(), wt.data_ptr(), wt.data_ptr(), None) == -4       # no model yet
    assert lib.rg_sim_set_mlr(h, wt.data_ptr()) == 0
    assert lib.rg_sim_debug_mlr_acts(h, None, wt.data_ptr(), wt.data_ptr(), None) == -1
    cdf = torch.ones(9, dtype=torch.float64, device='cuda:0')
    assert lib.rg_sim_set_epsilon_greedy_model(h, 0.1, 1, 1, cdf.data_ptr(), 0.01, 0.9) == -1 and b'MLR' in lib.rg_last_error()
    assert lib.rg_sim_set_epsilon_greedy_model_ps(h, 0.1, 1, 1, cdf.data_ptr(), 0.01, 0.9) == -1
    lib.rg_sim_destroy(h)
    lib, h, ws = handle(_abi.RG_POLICY_NN_IPS)
    assert lib.rg_sim_set_mlr(h, wt.data_ptr()) == -4
    lib.rg_sim_destroy(h)
    lib, h, ws = handle(_abi.RG_POLICY_MLR, P=4001)
    assert lib.rg_sim_set_mlr(h, wt.data_ptr()) == -1 and b'products' in lib.rg_last_error()
    lib.rg_sim_destroy(h)
