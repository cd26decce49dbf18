"""EpsilonGreedy round NnIpsAgent (argmax form) and BayesianAgentVB inside the device step loop (rg_sim_set_epsilon_greedy_model_ps) and
in the off-policy replay (rg_ope_replay_nn_eg, rg_ope_replay_bayes_eg), reached through the wrapper's own hooks, against logs of the
reference's own wrapper round its own agents (tests/golden/nn_eg_*.npz, bayes_eg_*.npz, tests/make_golden_eg_nn_bayes.py) and this
package's host route.

Every comparison is bit for bit but one: the propensity of a GREEDY NnIpsAgent row is (1 - epsilon) * prob[a], and prob[a] is the
device's float64 forward on one side and torch's fp32 forward on the other.  The two lie within nn_ps_bound (agents/nn_ips.py, proven
in DESIGN.md 4i) of each other, and each side rounds its product by the same 1 - epsilon once: |ps_dev / ps_ref - 1| <= nn_ps_bound +
2^-51.  Needs a real MI355X."""
import functools
import warnings

import numpy as np
import pytest
import torch

import adversarial_util as au
import eg_nn_bayes_util as xu
import eg_util as eu
import golden_util as gu
import nn_ips_util as nu
from device_util import HostOnly, assert_frames_equal, handle, make_env
from make_golden_ope import log_frame
from recogym_amd import _abi
from recogym_amd import evaluate_agent as ev
from recogym_amd.agents.bayesian_poly_vb import BayesianVBFrozenAgent
from recogym_amd.agents.epsilon_greedy import explore_table
from recogym_amd.agents.nn_ips import NnIpsFrozenAgent
from recogym_amd.envs.configuration import Configuration
from recogym_amd.envs.reco_env_v1 import env_1_args
from recogym_amd.sim import Simulator

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# test_eg_models_device.MODES: an event per launch, run-ahead rounds, and the defaults
MODES = (dict(tail_below=0, run_ahead=0), dict(tail_below=0, run_ahead=32), dict())
EG = dict(epsilon=0.3, random_seed=7)
TWO_ROUNDINGS = 2.0 ** -51          # each side's product by 1 - epsilon rounds once: 2^-53 relative each, 2^-51 with room
ACT_KERNEL = {'nn': 'nn_ips', 'bayes': 'bayes_vb'}


def run(cfg, n, pol, options=(), first_user=0, organic_only_below=0):
    sim = Simulator(cfg, n, device=DEV, **{k: v for k, v in pol.items() if k != 'ps_all'})
    for k, v in dict(options).items():
        sim.set_option(k, v)
    sim.reset_users(first_user, n, organic_only_below=organic_only_below)
    sim.run()
    return sim


def run_fixture(name, options=(), first_user=0, n_users=None, organic_only_below=0, keep=False):
    """-> the record of a run of the fixture's users under the wrapper's own device_policy() (`keep`: with the open Simulator)"""
    meta, cols, P = xu.load(name)
    pol = xu.wrapper(meta, cols, P).device_policy()
    assert pol is not None and pol['epsilon_greedy']['epsilon'] == meta['eg_args']['epsilon']
    sim = run(gu.env_config(meta), meta['n_users'] if n_users is None else n_users, pol, options, first_user, organic_only_below)
    r = dict(meta=meta, cols=cols, P=P, rows=sim.rows(), cnt=sim.counters(), stands=sim.poly_verify(), listed=sim.poly_unresolved.copy(),
             refuted=sim.poly_refuted.copy(), overflow=sim.poly_overflow, ledger=au.ledger(sim), act=(ACT_KERNEL[meta['inner']],))
    if keep:
        r['sim'] = sim
    else:
        sim.close()
    return r


def same(a, b):
    assert np.array_equal(eu.bits(a), eu.bits(b))


@functools.lru_cache(maxsize=None)
def row_bounds(name):
    """per row of an NnIpsAgent fixture: nn_ps_bound of the act that serves it (computed once per fixture)"""
    meta, cols, P = xu.load(name)
    return xu.nn_row_bounds(meta, cols, P)[0]


def assert_ps(what, name, meta, cols, ps):
    """The float64 propensities of a run against the fixture's: bit for bit on explored rows and on every BayesianAgentVB row; on
    greedy NnIpsAgent rows within the proven bound of the act plus the two roundings."""
    is_b, greedy = cols['z'] == 1, cols['greedy'] == 1
    explored = is_b & ~greedy
    assert np.array_equal(eu.bits(ps[explored]), eu.bits(cols['ps'][explored])), f'{what}: ps bits on explored rows'
    if meta['inner'] == 'bayes':
        assert np.array_equal(eu.bits(ps[is_b]), eu.bits(cols['ps'][is_b])), f'{what}: ps bits'
        return
    bound = row_bounds(name)
    err = np.abs(ps[greedy] / cols['ps'][greedy] - 1.0)
    print(what, 'greedy rows', int(greedy.sum()), 'worst |ps_dev / ps_ref - 1|', float(err.max()), 'worst error / bound',
          float((err / (bound[greedy] + TWO_ROUNDINGS)).max()))
    assert (bound[greedy] > 0).all() and (err <= bound[greedy] + TWO_ROUNDINGS).all(), f'{what}: ps on greedy rows'
    assert ((ps[greedy] > 0.0) & (ps[greedy] < 1.0 - meta['eg_args']['epsilon'])).all()       # (1 - eps) * a model output below 1


# ---- (a) the device log against the fixture --------------------------------------------------------------------------------
def assert_log_is_the_fixture(what, name, rs):
    """The records of the runs that together cover the fixture's users (rows concatenated, counters summed) held to it."""
    meta, cols = rs[0]['meta'], rs[0]['cols']
    rows = rs[0]['rows'] if len(rs) == 1 else np.concatenate([r['rows'] for r in rs])
    cnt = {k: sum(r['cnt'][k] for r in rs) for k in rs[0]['cnt']}
    is_b = cols['z'] == 1
    last = np.r_[cols['u'][1:] != cols['u'][:-1], True]
    no_ps = rows.copy()
    no_ps['ps'] = cols['ps']                                 # the integer columns (the action among them) here; ps below
    gu.assert_rows_equal(no_ps, cols, ps_rtol=0, what=what)
    assert np.array_equal(rows['phantom'] != 0, is_b & last), 'the phantom row is every user\'s last'
    assert_ps(what, name, meta, cols, rows['ps'])
    census = meta['census']
    print(what, {k: cnt[k] for k in ('lr_acts', 'lr_rows', 'poly_unresolved')}, census)
    assert cnt['lr_acts'] == census['acts'] and cnt['poly_unresolved'] == census['unresolved'], what
    # the confirm-or-repeat protocol: the listed acts are GREEDY acts, and the host confirms every one of them
    assert all(r['stands'] and not r['overflow'] and len(r['refuted']) == 0 for r in rs), what
    listed = np.concatenate([r['listed'] for r in rs])
    assert len(listed) == census['unresolved'], what
    g = xu.greedy_actions(cols)
    first = {}
    for i, u in enumerate(cols['u'].tolist()):
        first.setdefault(u, i)
    for u, t, a in listed.tolist():
        at = first[u] + t                                    # the listed event, or the row after it, is a bandit row of this act
        row = at if cols['z'][at] == 1 else at + 1
        assert cols['z'][row] == 1 and g[row] == a, (what, u, t, a)
    assert cnt['live'] == 0 and cnt['log_dropped'] == 0 and cnt['hist_overflow'] == 0, what


@pytest.mark.parametrize('name', xu.LOG_FIXTURES)
def test_device_log_equals_the_reference_fixture(name):
    for options in MODES:
        r = run_fixture(name, options)
        assert r['ledger'][r['act'][0]] > 0 and r['ledger']['walk'] == r['ledger']['walk2'] == 0
        assert_log_is_the_fixture(f'{name} {options}', name, [r])


# ---- (b) the branches and the log replayed under the wrapper that wrote it ---------------------------------------------------
@pytest.mark.parametrize('name', xu.LOG_FIXTURES)
def test_branches_and_self_replay(name):
    r0 = run_fixture(name, keep=True)
    meta, cols, P, sim = r0['meta'], r0['cols'], r0['P'], r0['sim']
    target = xu.wrapper(meta, cols, P, with_ps_all=True)
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
    r = r.cpu().numpy()
    assert r.size == int(is_b.sum()) and float(sums[0].item()) == r.size
    assert np.array_equal(c.cpu().numpy(), cols['c'][is_b].astype(np.float64))
    explored = want_greedy == 0
    # an explored row: pi = epsilon * (1 / n), the logged propensity itself
    assert (r[explored] == 1.0).all()
    if meta['inner'] == 'bayes':
        # pi is the logged propensity, the same float64 product, on every row
        assert (r == 1.0).all() and float(sums[2].item()) == r.size
    else:
        # a greedy row: pi = (1 - epsilon) * 1 (the inner `ps-a` is one-hot) over the logged (1 - epsilon) * prob[a]
        want = (1.0 - meta['eg_args']['epsilon']) / cols['ps'][is_b][~explored]
        bound = row_bounds(name)[is_b][~explored]
        err = np.abs(r[~explored] / want - 1.0)
        print(name, 'worst ratio error / bound', float((err / (bound + TWO_ROUNDINGS)).max()))
        assert (err <= bound + TWO_ROUNDINGS).all() and (r[~explored] > 1.0).all()
    assert stats['acts'] == meta['census']['acts'] and stats['error'] == 0
    assert stats['unresolved'] == meta['census']['unresolved'] and not stats['overflow']


# ---- (c) the estimators ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', xu.OPE_FIXTURES)
def test_estimators_on_a_frame_equal_the_reference(name):
    meta, want, P = xu.load(name)
    df = log_frame(gu.load(meta['log'])[1])
    target = xu.wrapper(meta, want, P, with_ps_all=True)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        assert ev._device_or_none(target, df) is not None          # the device route
        c, ratio = ev.evaluate_SNIPS(target, df)
        ips = ev.evaluate_IPS(target, df)
    assert len(ratio) == len(want['ratio']) > 20000
    same(ratio, want['ratio'])
    assert np.array_equal(np.asarray(c, dtype=np.float64), want['c'])
    same(ips, want['c'] * want['ratio'])


def test_tables_and_recall_on_a_device_log_equal_the_host_loop(monkeypatch):
    """verify_agents_IPS / _SNIPS / _recall_at_k and evaluate_recall_at_k with the two wrappers as targets, over a device log with
    full support: the rows behind the tables are the host loop's bit for bit, the tables the estimators' own reductions of them."""
    from ope_models_util import bits, table
    agents = {}
    for name in ('nn_eg_p10', 'bayes_eg_p10_s120_not_pure_new'):
        meta, cols, P = xu.load(name)
        agents[name] = xu.wrapper(meta, cols, P, with_ps_all=True)
        assert ev._recall_form(ev._replay_policy_of(agents[name])) == 'table'
    sim = run(Configuration({**env_1_args, 'random_seed': 11, 'num_products': 10, 'K': 5}), 60, dict(policy=_abi.RG_POLICY_UNIFORM_ENV))
    dl = sim.device_log()
    df = ev._device_log_to_frame(dl)
    sim.close()
    ks = (1, 5)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        hits = {(name, k): ev.evaluate_recall_at_k(ag, dl, k=k) for name, ag in agents.items() for k in ks}
        got = dict(ips=ev.verify_agents_IPS(dl, agents), snips=ev.verify_agents_SNIPS(dl, agents),
                   recall=ev.verify_agents_recall_at_k(dl, agents, k=5))
    monkeypatch.setattr(ev, '_device_present', lambda: False)
    for frame in got.values():
        assert list(frame['Agent']) == list(agents)
    for i, (name, ag) in enumerate(agents.items()):
        for k in ks:
            want = ev._host_recall(ag, df, k)
            assert torch.is_tensor(hits[name, k]) and hits[name, k].cpu().tolist() == want and len(want) > 0, (name, k)
        rewards, ratio = ev._host_snips(ag, df)
        ips = np.asarray(ev._host_ips(ag, df), dtype=np.float64)
        want = dict(ips=table(ips), snips=table(np.asarray(rewards, dtype=np.float64) * np.asarray(ratio), snips_ratio=ratio),
                    recall=table(ev._host_recall(ag, df, 5)))
        for what, frame in got.items():
            row = tuple(float(frame[q][i]) for q in ('0.025', '0.500', '0.975'))
            assert bits(row).tolist() == bits(want[what]).tolist(), (name, what, row, want[what])


# ---- (d) small shapes against this package's host route --------------------------------------------------------------------
def assert_frames_match(got, want, inner):
    """A device frame against the host route's: every column but ps equal; ps bit for bit, except where it carries the net's own
    output (a greedy NnIpsAgent row), there within the act's bound plus the two roundings."""
    if not isinstance(inner, NnIpsFrozenAgent):
        return assert_frames_equal(got, want)
    assert len(got) == len(want)
    for k in ('t', 'u', 'v', 'a', 'c'):
        assert np.array_equal(got[k].to_numpy(dtype=np.float64, na_value=np.nan), want[k].to_numpy(dtype=np.float64, na_value=np.nan), equal_nan=True), k
    assert ((got['z'] == 'bandit') == (want['z'] == 'bandit')).all()
    cols = dict(u=want['u'].to_numpy(dtype=np.int64), z=(want['z'] == 'bandit').to_numpy().astype(np.int64),
                v=want['v'].to_numpy(dtype=np.float64, na_value=0).astype(np.int64), a=want['a'].to_numpy(dtype=np.float64, na_value=-1).astype(np.int64))
    g, w = got['ps'].to_numpy(dtype=np.float64, na_value=np.nan), want['ps'].to_numpy(dtype=np.float64, na_value=np.nan)
    assert np.array_equal(np.isnan(g), np.isnan(w))
    P = int(inner.config.num_products)
    for act in nu.rule_over_log(cols, P, inner.state()):                # (the bound of an act depends on its history alone)
        for i in act['rows']:
            assert eu.bits(g[i]) == eu.bits(w[i]) or abs(g[i] / w[i] - 1.0) <= act['bound'] + TWO_ROUNDINGS, (i, g[i], w[i], act['bound'])


def logs(env, n, agent):
    """generate_logs on the device route (no warning: nothing was refuted) and on the per-user host route"""
    assert agent.device_policy() is not None
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        got = env.generate_logs(n, agent)
    want = env.generate_logs(n, HostOnly(agent))
    assert_frames_match(got, want, agent.agent)
    return got


def bandit(df, k, dtype=np.float64):
    return df[k].to_numpy(dtype=np.float64, na_value=np.nan)[(df['z'] == 'bandit').to_numpy()].astype(dtype)


SMALL = dict(random_seed=99, num_products=10, K=4, prob_leave_bandit=0.05, prob_leave_organic=0.05)


@pytest.mark.parametrize('name', ['nn_eg_p10', 'bayes_eg_p10_s120'])
def test_epsilon_0_is_the_unwrapped_agent_and_epsilon_1_never_takes_its_action(name):
    meta, cols, P = xu.load(name)
    env, n = make_env(SMALL), 70
    inner = xu.inner_agent(meta, cols, P)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        plain = env.generate_logs(n, inner)
    got = logs(env, n, xu.wrap(xu.inner_agent(meta, cols, P), P, dict(EG, epsilon=0.0)))
    assert_frames_equal(got, plain)                      # (1.0 - 0.0) * ps is ps: the unwrapped device log, its ps bits included
    if meta['inner'] == 'bayes':
        same(bandit(got, 'ps'), np.full(bandit(got, 'ps').size, (1.0 - 0.0) * 1.0))
    # epsilon = 1 with pure_new: every act explores and none logs the model's action
    agent = xu.wrap(xu.inner_agent(meta, cols, P), P, dict(EG, epsilon=1.0))
    got = logs(env, n, agent)
    cnt, sim = env.simulate(n, agent)
    greedy, h0 = ev.epsilon_greedy_branches(xu.wrap(xu.inner_agent(meta, cols, P, True), P, dict(EG, epsilon=1.0), with_ps_all=True), sim)
    sim.close()
    a = bandit(got, 'a', np.int64)
    assert a.size == greedy.numel() > 300 and not bool(greedy.any()) and (a != h0.cpu().numpy()).all()
    assert len(set(h0.cpu().numpy().tolist())) > 1
    same(bandit(got, 'ps'), np.full(a.size, 1.0 * explore_table(P, True)[1]))


def two_product_models(with_ps_all=False):
    """(NnIpsAgent, BayesianAgentVB) over two products whose action depends on HOW MANY views the user has, whichever product they
    went to (a two-product environment may show one product only).  The net: one hidden unit per layer, h1 = sigmoid(0.5 v - 1),
    h2 = sigmoid(h1), logits 0 and 40 (h2 - 0.637): -0.58 up to two views, +0.55 from three on.  The posterior: two draws, action 0
    with weights (0.2, 0.2) per view — mean expit(0.2 v) — and action 1 with (4, -0.1): action 1 wins up to four views (by 0.0106 at
    four), action 0 from five on (by 0.042 at five).  Both far outside the rules' margins."""
    extra = {'device_replay': True} if with_ps_all else {}
    cfg = Configuration({'num_products': 2, 'with_ps_all': with_ps_all, **extra})
    f = lambda x: np.asarray(x, dtype=np.float32)       # noqa: E731
    state = dict(w1=f([[0.5, 0.5]]), b1=f([-1.0]), w2=f([[1.0]]), b2=f([0.0]), w3=f([[0.0], [40.0]]), b3=f([0.0, -40.0 * 0.637]))
    lam = np.array([[0.2, 4.0, 0.2, 4.0], [0.2, -0.1, 0.2, -0.1]])           # [draw][viewed product * 2 + action]
    return NnIpsFrozenAgent(cfg, state), BayesianVBFrozenAgent(cfg, lam)


@pytest.mark.parametrize('which', [0, 1])
def test_two_products_with_pure_new_explore_the_other_one(which):
    inner = two_product_models()[which]
    few, many = ((0, 1), (1, 0))[which]
    from ope_models_util import host_action
    assert host_action(inner, [0], [1]) == host_action(inner, [1], [2]) == few and host_action(inner, [0, 1], [3, 3]) == many
    env, n = make_env({**SMALL, 'num_products': 2}), 70
    eg_args = dict(EG, epsilon=0.5)
    agent = xu.wrap(inner, 2, eg_args)
    got = logs(env, n, agent)
    cnt, sim = env.simulate(n, agent)
    greedy, h0 = ev.epsilon_greedy_branches(xu.wrap(two_product_models(True)[which], 2, eg_args, with_ps_all=True), sim)
    sim.close()
    greedy, h0 = greedy.cpu().numpy(), h0.cpu().numpy()
    a = bandit(got, 'a', np.int64)
    assert a.size == greedy.size > 300 and 0.3 < greedy.mean() < 0.7 and len(set(h0.tolist())) == 2
    assert np.array_equal(a, np.where(greedy == 1, h0, 1 - h0))
    ps = bandit(got, 'ps')
    same(ps[greedy == 0], np.full(int((greedy == 0).sum()), 0.5 * 1.0))
    if which == 1:
        same(ps[greedy == 1], np.full(int((greedy == 1).sum()), (1.0 - 0.5) * 1.0))
    else:
        assert ((ps[greedy == 1] > 0.25) & (ps[greedy == 1] < 0.5)).all()       # (1 - 0.5) * prob[a], prob[a] in (1/2, 1)


@pytest.mark.parametrize('name', ['nn_eg_p10', 'bayes_eg_p4'])
def test_test_agent_returns_the_host_routes_quantiles(name):
    import recogym_amd as recogym
    meta, cols, P = xu.load(name)
    env = make_env({**SMALL, 'num_products': P})
    agent = xu.wrapper(meta, cols, P)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        got = recogym.test_agent(env, agent, 0, 60)
    assert got == recogym.test_agent(env, HostOnly(agent), 0, 60)


# ---- (e) the other run forms -------------------------------------------------------------------------------------------------
# fixture -> forms (tests/test_agent_run_forms.FORM_ENV); the whole-fixture cases hold the relabelling of a repack (shown without a
# GPU in test_eg_nn_bayes_host.py), the shards the id offset
FORMS = {'nn_eg_p40': ('repack_lockstep', 'repack_rounds'), 'nn_eg_p10_sigma0': ('repack_lockstep', 'nocache_rounds'),
         'bayes_eg_p10_s120': ('repack_lockstep', 'repack_rounds')}
SHARDS = [('nn_eg_p40', 'repack_rounds'), ('bayes_eg_p10_s120_not_pure_new', 'repack_rounds')]


@pytest.mark.parametrize('name,form', [(n, f) for n, forms in FORMS.items() for f in forms])
def test_fixture_in_form(name, form, monkeypatch):
    import test_agent_run_forms as rf
    rf.set_form(form, monkeypatch)
    r = run_fixture(name)
    print(name, form, {k: v for k, v in r['ledger'].items() if v and k not in au.DESCRIPTORS})
    rf.assert_form(r['ledger'], form, r['act'])
    assert_log_is_the_fixture(f'{name} {form}', name, [r])


@pytest.mark.parametrize('name,form', SHARDS)
def test_fixture_as_two_shards(name, form, monkeypatch):
    """Users [0, 37) in the default form and [37, n) with the state repack on: the rows concatenated, the unresolved lists joined
    and the counters summed are the fixture's."""
    import test_agent_run_forms as rf
    n = xu.load(name)[0]['n_users']
    rf.set_form('default', monkeypatch)
    a = run_fixture(name, first_user=0, n_users=rf.SPLIT)
    rf.set_form(form, monkeypatch)
    b = run_fixture(name, first_user=rf.SPLIT, n_users=n - rf.SPLIT)
    rf.assert_form(b['ledger'], form, b['act'])
    assert a['ledger'][a['act'][0]] > 0
    assert_log_is_the_fixture(f'{name} shards', name, [a, b])


@pytest.mark.parametrize('name', ['nn_eg_p10', 'bayes_eg_p10_s120'])
def test_offset_ids_with_organic_only_users_equal_the_host_route(name, monkeypatch):
    import test_agent_run_forms as rf
    from recogym_amd.envs.reco_env_v1 import RecoEnv1
    meta, cols, P = xu.load(name)
    agent = xu.wrapper(meta, cols, P)
    rf.set_form('default', monkeypatch)
    env = make_env(meta['env_args'])
    want = env._generate_logs_per_user(rf.N_OFFLINE, agent, rf.N_ORGANIC, rf.FIRST_ID)
    u, is_b = want['u'].to_numpy(dtype=np.int64), (want['z'] == 'bandit').to_numpy()
    assert u.min() == rf.FIRST_ID and u.max() == rf.FIRST_ID + rf.N_OFFLINE + rf.N_ORGANIC - 1 > 65535
    assert not is_b[u < rf.FIRST_ID + rf.N_ORGANIC].any() and is_b[u >= rf.FIRST_ID + rf.N_ORGANIC].any()
    seen, real = [], RecoEnv1.simulate

    def spy(self, *a, **k):
        cnt, sim = real(self, *a, **k)
        seen.append(au.ledger(sim))
        return cnt, sim
    monkeypatch.setattr(RecoEnv1, 'simulate', spy)
    for form in ('default', 'repack_tail'):            # (repack_tail's switches: the repack on, the rest as generate_logs runs by default)
        rf.set_form(form, monkeypatch)
        del seen[:]
        with warnings.catch_warnings():
            warnings.simplefilter('error', RuntimeWarning)       # a fallback to the host route warns: it fails here
            got = make_env(meta['env_args']).generate_logs(rf.N_OFFLINE, agent, num_organic_offline_users=rf.N_ORGANIC, first_user_id=rf.FIRST_ID)
        assert len(seen) == 1, 'generate_logs made no device run, or more than one'
        led = seen[0]
        assert (led['repack'] > 0) == (form != 'default') and led['tail'] == 0 and led[ACT_KERNEL[meta['inner']]] > 0, led
        assert_frames_match(got, want, agent.agent)
        ids, gb = got['u'].to_numpy(dtype=np.int64), (got['z'] == 'bandit').to_numpy()
        assert not gb[ids < rf.FIRST_ID + rf.N_ORGANIC].any(), 'an organic-only user logged a bandit row'
        # explored rows and greedy rows (BayesianAgentVB: the two constants; NnIpsAgent: model outputs besides)
        assert len(set(bandit(got, 'ps').tolist())) > (2 if meta['inner'] == 'nn' else 1)


# ---- (f) the unresolved-act protocol under the wrapper ---------------------------------------------------------------------
OVER = dict(random_seed=321, num_products=10, K=4)


def protocol_agents(kind, refuted, with_ps_all=False):
    """The constructions of the agents' own device tests, rebuilt with the configuration a replay target needs: an agent whose every
    (NnIpsAgent) or first-view (BayesianAgentVB) act the device lists — the host confirms it (-> its action 1) or refutes it (device
    action 2, host action 1).  Margin cases of the decision rules: nothing here runs a kernel outside its contract."""
    extra = {'device_replay': True} if with_ps_all else {}
    cfg = Configuration({'num_products': 10, 'with_ps_all': with_ps_all, **extra})
    if kind == 'nn':
        import test_nn_ips_device as t
        base = t.refuted_agent() if refuted else t.tie_agent(0.0)
        return NnIpsFrozenAgent(cfg, base.state())
    import test_bayes_vb_device as t
    base = t.refuted_agent() if refuted else t.constant_agent(0.25, 0.25)
    return BayesianVBFrozenAgent(cfg, base.Lambda)


@pytest.mark.parametrize('kind', ['nn', 'bayes'])
def test_an_unresolved_greedy_act_the_host_confirms_keeps_the_device_route(kind):
    agent = xu.wrap(protocol_agents(kind, False), 10, EG)
    sim = run(Configuration({**env_1_args, **OVER}), 60, agent.device_policy())
    cnt = sim.counters()
    assert sim.poly_verify() and not sim.poly_overflow
    # the list holds the GREEDY act of every listed act, explored ones included
    assert len(sim.poly_unresolved) == cnt['poly_unresolved'] > 60 and len(sim.poly_refuted) == 0
    assert kind == 'bayes' or cnt['poly_unresolved'] == cnt['lr_acts']
    assert (sim.poly_unresolved[:, 2] == 1).all()
    target = xu.wrap(protocol_agents(kind, False, True), 10, EG, with_ps_all=True)
    st = {}
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        r, c, sums = ev.ope_replay(target, sim.device_log(), n_users=60, stats=st)
        greedy, h0 = ev.epsilon_greedy_branches(target, sim)
    sim.close()
    assert st['unresolved'] > 60 and st['acts'] == cnt['lr_acts'] and bool((h0 == 1).all())
    assert kind == 'nn' or bool((r == 1.0).all())
    got = logs(make_env(OVER), 60, agent)
    a = bandit(got, 'a', np.int64)
    assert np.array_equal(a == 1, greedy.cpu().numpy() == 1) and 0.15 < (a != 1).mean() < 0.45


@pytest.mark.parametrize('kind', ['nn', 'bayes'])
def test_a_refuted_greedy_act_sends_generate_logs_to_the_host_route(kind):
    agent = xu.wrap(protocol_agents(kind, True), 10, EG)
    env = make_env(OVER)
    with pytest.warns(RuntimeWarning, match='host route') as rec:
        got = env.generate_logs(60, agent)
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    assert_frames_equal(got, env.generate_logs(60, HostOnly(agent)))          # the host route itself: its ps too
    a = got['a'].dropna().astype(int)
    assert 0.55 < (a == 1).mean() < 0.85 and 0 < (a == 2).mean() < 0.1      # greedy acts take the reference's action, 1


@pytest.mark.parametrize('kind', ['nn', 'bayes'])
def test_a_refuted_greedy_act_sends_the_replay_to_the_host_loop(kind):
    target = xu.wrap(protocol_agents(kind, True, True), 10, EG, with_ps_all=True)
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


# ---- (g) determinism -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['nn_eg_p40', 'bayes_eg_p10_s120'])
def test_two_runs_give_the_same_log_and_the_same_sums(name):
    raws, sums = [], []
    for _ in range(2):
        r = run_fixture(name, keep=True)
        sim = r['sim']
        raws.append(sim.sorted_log_host()[0].copy())
        target = xu.wrapper(r['meta'], r['cols'], r['P'], with_ps_all=True)
        for _ in range(2):
            sums.append(ev.ope_replay(target, sim.device_log(), n_users=r['meta']['n_users'])[2].cpu().numpy().copy())
        sim.close()
    assert raws[0].tobytes() == raws[1].tobytes()
    assert all(s.tobytes() == sums[0].tobytes() for s in sums)


# ---- (h) error paths: arguments only ---------------------------------------------------------------------------------------
def test_step_loop_error_paths():
    table = torch.from_numpy(explore_table(10, True)[0]).to(DEV)
    args = (0.1, 7, 1, table.data_ptr(), 0.1 / 9, 0.9)
    for policy in (_abi.RG_POLICY_LAST_VIEW_TABLE, _abi.RG_POLICY_RANDOM_AGENT, _abi.RG_POLICY_ORGANIC_USER_COUNT, _abi.RG_POLICY_UNIFORM_ENV,
                   _abi.RG_POLICY_EXTERNAL, _abi.RG_POLICY_LOGREG_FROZEN, _abi.RG_POLICY_LOGREG_POLY):
        lib, h, ws = handle(policy)
        assert lib.rg_sim_set_epsilon_greedy_model_ps(h, *args) == -1 and b'wraps NnIpsAgent or BayesianAgentVB' in lib.rg_last_error()
        lib.rg_sim_destroy(h)
    lib, h, ws = handle(_abi.RG_POLICY_LOGREG_FROZEN, lr_select_randomly=True)
    assert lib.rg_sim_set_epsilon_greedy_model_ps(h, *args) == -1 and b'wraps NnIpsAgent or BayesianAgentVB' in lib.rg_last_error()
    lib.rg_sim_destroy(h)
    for policy, word in ((_abi.RG_POLICY_NN_IPS, b'RG_POLICY_NN_IPS: host path'), (_abi.RG_POLICY_BAYES_VB, b'RG_POLICY_BAYES_VB: host path')):
        lib, h, ws = handle(policy)
        # the two older entry points still refuse these policies, messages included
        assert lib.rg_sim_set_epsilon_greedy(h, *args) == -1 and b'EpsilonGreedy wraps RandomAgent' in lib.rg_last_error()
        assert lib.rg_sim_set_epsilon_greedy_model(h, *args) == -1 and word in lib.rg_last_error()
        for eps in (-0.01, 1.01, float('nan')):
            assert lib.rg_sim_set_epsilon_greedy_model_ps(h, eps, 7, 1, table.data_ptr(), 0.0, 0.0) == -1 and b'epsilon' in lib.rg_last_error()
        assert lib.rg_sim_set_epsilon_greedy_model_ps(h, 0.1, 7, 1, None, 0.1 / 9, 0.9) == -1 and b'NULL' in lib.rg_last_error()
        assert lib.rg_sim_set_epsilon_greedy_model_ps(None, *args) == -1 and b'sim is NULL' in lib.rg_last_error()
        for eps in (0.0, 1.0, 0.1):
            assert lib.rg_sim_set_epsilon_greedy_model_ps(h, eps, 7, 1, table.data_ptr(), 0.1 / 9, 0.9) == 0
        lib.rg_sim_destroy(h)
        lib, h, ws = handle(policy, P=1)
        assert lib.rg_sim_set_epsilon_greedy_model_ps(h, 0.1, 7, 1, table.data_ptr(), 0.1, 0.9) == -1 and b'at least 2' in lib.rg_last_error()
        assert lib.rg_sim_set_epsilon_greedy_model_ps(h, 0.1, 7, 0, table.data_ptr(), 0.1, 0.9) == 0
        lib.rg_sim_destroy(h)
    # after rg_sim_reset_users: RG_ESTATE
    for name in ('nn_eg_p10', 'bayes_eg_p10_s120'):
        meta, cols, P = xu.load(name)
        sim = Simulator(gu.env_config(meta), 32, device=DEV, **xu.inner_agent(meta, cols, P).device_policy())
        sim.reset_users(0, 32)
        assert sim.lib.rg_sim_set_epsilon_greedy_model_ps(sim._h, *args) == -4 and b'before rg_sim_reset_users' in sim.lib.rg_last_error()
        sim.close()
    # one product with pure_new through the Simulator: refused, not run without the overlay
    one = NnIpsFrozenAgent(Configuration({'num_products': 1}), {k: np.zeros(s, dtype=np.float32) for k, s in
                                                                 dict(w1=(3, 1), b1=(3,), w2=(3, 3), b2=(3,), w3=(1, 3), b3=(1,)).items()})
    with pytest.raises(_abi.RecoGymHipError, match='at least 2'):
        Simulator(Configuration({**env_1_args, 'random_seed': 1, 'num_products': 1, 'K': 2}), 32, device=DEV,
                  epsilon_greedy=dict(epsilon=0.1, seed=7, pure_new=True), **one.device_policy())
