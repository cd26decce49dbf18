"""Every device agent on every run form, repacked and sharded.

The base policies are held to the oracle on every execution form in tests/test_hip_parity.py.  The agents whose act is a kernel of its own
(NnIpsAgent: k_nn_acts, the likelihood agent: k_poly_acts and its time-weighted k_wh_insert / k_poly_acts_w, BayesianAgentVB:
k_bayes_acts, the frozen LogReg) and the two EpsilonGreedy overlays have a device test file each, and each of those files runs its
fixtures from user id 0, without organic-only users and below the population from which the state repack is on — so slot == user
index == user id throughout, and a kernel that took one for another would pass.  Here the same fixtures (the reference's own logs,
tests/golden/) run

  * in every form of the step loop the agent has — lock-step, run-ahead rounds, each with the state repack forced on (RECOGYM_REPACK_MIN=1),
    the tail kernel behind a repack for the overlay over the base policies, the rounds of a sigma_omega = 0 run without its sum cache;
  * as two shards, users [0, 37) and [37, n), the second repacked: ids that do not start at 0;
  * through generate_logs at ids 65 530 ... with ten organic-only users in front, against the per-user host route.

The rows, propensities and counters are held to the fixture by the helpers of the agents' own test files (nothing is asserted about
rows here that they do not assert, with their tolerances); what is added is the form, proven from the launch ledger, and — without a
GPU — that the fixtures are populations on which these forms differ from the default one (a repack that relabels, acts on every path,
two ragged shards)."""
import warnings

import numpy as np
import pytest

import adversarial_util as au
import golden_util as gu
from recogym_amd import _abi
from recogym_amd.envs.configuration import Configuration
from recogym_amd.envs.reco_env_v1 import env_1_args

gpu = pytest.mark.gpu
RG_EINVAL = -1        # include/recogym_hip.h

# form -> switches (set before the Simulator is created: rg_sim_create reads them once)
FORM_ENV = {
    'default': {},
    'lockstep': {'RECOGYM_RUN_AHEAD': '0', 'RECOGYM_TAIL': '0'},
    'rounds': {'RECOGYM_RUN_AHEAD': '32', 'RECOGYM_TAIL': '0'},
    'repack_lockstep': {'RECOGYM_REPACK_MIN': '1', 'RECOGYM_REPACK': '3', 'RECOGYM_RUN_AHEAD': '0', 'RECOGYM_TAIL': '0'},
    'repack_rounds': {'RECOGYM_REPACK_MIN': '1', 'RECOGYM_REPACK': '2', 'RECOGYM_RUN_AHEAD': '32', 'RECOGYM_TAIL': '0'},
    'repack_tail': {'RECOGYM_REPACK_MIN': '1', 'RECOGYM_REPACK': '2'},
    'nocache_rounds': {'RECOGYM_CACHE': '0', 'RECOGYM_RUN_AHEAD': '32', 'RECOGYM_TAIL': '0'},
}
SPLIT = 37          # odd and below a wave: both shards end in a ragged wave

THREE = ('lockstep', 'repack_lockstep', 'repack_rounds')
SIGMA0 = ('repack_lockstep', 'nocache_rounds')
REPACKED = ('repack_lockstep', 'repack_rounds')
# family -> fixture -> forms, in the order of their priority.  (The EpsilonGreedy files' MODES run lockstep, rounds and the default.)
CASES = {
    'nn_ips': {'nn_ips_p40_loaded': THREE, 'nn_ips_p10': THREE, 'nn_ips_p10_sigma0': SIGMA0},
    'poly_wh': {'poly_wh_exp_default': ('repack_lockstep',), 'poly_wh_exp02_normal': ('repack_lockstep',)},      # lock-step by design
    'bayes': {'bayes_p10_s120': THREE, 'bayes_p4_shifted': THREE, 'bayes_p10_s120_sigma0': SIGMA0},
    'poly': {'poly_p40': THREE, 'poly_p10_shifted': THREE, 'poly_p10_sigma0': SIGMA0},
    'eg_model': {'model_eg_poly_p10_long_users': REPACKED, 'model_eg_logreg_p10_hidden_classes': REPACKED, 'model_eg_poly_p40': REPACKED,
                 'model_eg_poly_p10_sigma0': ('repack_lockstep',)},
    'eg': {'eg_p10_eps03_ouc': REPACKED + ('repack_tail',), 'eg_p1000_k20_random': REPACKED + ('repack_tail',),
           'eg_p10_not_pure_new_table': REPACKED + ('repack_tail',), 'eg_p1000_k20_table_sigma0': ('repack_lockstep',)},
    'logreg': {'philox_logreg': REPACKED},
}
FORM_CASES = [(family, name, form) for family, fixtures in CASES.items() for name, forms in fixtures.items() for form in forms]
# the fixture of each family that runs as two shards, and the form of the second
SHARDS = [('nn_ips', 'nn_ips_p40_loaded', 'repack_rounds'), ('bayes', 'bayes_p10_s120', 'repack_rounds'), ('poly', 'poly_p40', 'repack_rounds'),
          ('poly_wh', 'poly_wh_exp_default', 'repack_lockstep'), ('eg_model', 'model_eg_poly_p10', 'repack_rounds'),
          ('eg', 'eg_p10_eps03_ouc', 'repack_rounds')]
# the census entry that counts the acts of a family's second path (the step table, the saturated zone, an act listed for the host,
# a view whose weight vanished, an explored act)
SECOND_PATH = {'nn_ips': ('unresolved',), 'poly': ('table', 'unresolved'), 'bayes': ('saturated', 'unresolved'),
               'poly_wh': ('dropped', 'unresolved'), 'eg_model': ('table', 'unresolved', 'explored')}


def set_form(form, monkeypatch):
    from test_history_capacity import SWITCHES
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in FORM_ENV[form].items():
        monkeypatch.setenv(k, v)


# ---------------------------------------------------------------------------------------------------------------------------
# one adapter per family: run(name, **users) -> a record with its 'ledger'; hold(what, name, records) holds the records of the
# runs that together cover the fixture's users to it, through the family's own helper
# ---------------------------------------------------------------------------------------------------------------------------
def sum_counters(cnts):
    return {k: sum(c[k] for c in cnts) for k in cnts[0]}


def cat_rows(rows):
    return rows[0] if len(rows) == 1 else np.concatenate(rows)


class NnIps:
    act = ('nn_ips',)

    @staticmethod
    def run(name, **users):
        import test_nn_ips_device as t
        return t.run_fixture(name, ledger=True, **users)

    @staticmethod
    def hold(what, name, rs):
        import test_nn_ips_device as t
        r = dict(rs[0], rows=cat_rows([x['rows'] for x in rs]), cnt=sum_counters([x['cnt'] for x in rs]),
                 listed=np.concatenate([x['listed'] for x in rs]), refuted=np.concatenate([x['refuted'] for x in rs]),
                 overflow=any(x['overflow'] for x in rs), stands=all(x['stands'] for x in rs), launched=min(x['launched'] for x in rs))
        # an event per launch lists a bandit user's unresolved act one event later than a round does (nu.rule_over_log): by design
        lockstep = {x['ledger']['advance_run'] == 0 for x in rs}
        assert len(lockstep) == 1, 'shards in forms that list their unresolved acts differently'
        t.assert_run_equals_the_fixture(name, r, lockstep=lockstep.pop())


class Poly:
    act = ('logreg_poly',)
    module = 'test_logreg_poly_device'

    @classmethod
    def run(cls, name, **users):
        t = __import__(cls.module)
        out = t.run_fixture(name, ledger=True, **users)
        return dict(out=out[:-3], ledger=out[-3], stands=out[-2], listed=out[-1])

    @classmethod
    def hold(cls, what, name, rs):
        t = __import__(cls.module)
        meta, cols = rs[0]['out'][:2]
        assert all(r['stands'] for r in rs) and sum(len(r['listed']) for r in rs) == meta['census']['unresolved']
        # (out[4] is the raw log, which the helper does not take; BayesianAgentVB's helper also takes the launches of k_bayes_acts)
        t.assert_log_equals_the_reference(name, meta, cols, cat_rows([r['out'][2] for r in rs]), sum_counters([r['out'][3] for r in rs]),
                                          *([min(r['out'][5] for r in rs)] if len(rs[0]['out']) > 5 else []))


class Bayes(Poly):
    act = ('bayes_vb',)
    module = 'test_bayes_vb_device'


class PolyWh:
    act = ('logreg_poly_w',)

    @staticmethod
    def run(name, **users):
        import test_weight_history_device as t
        meta, cols, got, run = t.run_fixture(name, **users)
        return dict(meta=meta, cols=cols, got=got, run=run, ledger=run['ledger'])

    @staticmethod
    def hold(what, name, rs):
        import pandas as pd
        import test_weight_history_device as t
        runs = [r['run'] for r in rs]
        run = {k: (min if k == 'launched' else sum)(x[k] for x in runs) for k in runs[0] if k not in ('ledger', 'hist_cap')}
        got = rs[0]['got'] if len(rs) == 1 else pd.concat([r['got'] for r in rs], ignore_index=True)
        t.assert_frame_is_the_reference_log(name, rs[0]['meta'], rs[0]['cols'], got, run)


class EgModel:
    @staticmethod
    def act_of(meta):
        return ('logreg_poly',) if meta['inner'] == 'poly' else ('logreg_screen', 'logreg_acts')

    @staticmethod
    def run(name, **users):
        import test_eg_models_device as t
        meta, cols, P, sim = t.run_fixture(name, **users)
        try:
            return dict(meta=meta, cols=cols, rows=sim.rows(), cnt=sim.counters(), ledger=au.ledger(sim), act=EgModel.act_of(meta))
        finally:
            sim.close()

    @staticmethod
    def hold(what, name, rs):
        import test_eg_models_device as t
        t.assert_log_is_the_fixture(what, rs[0]['meta'], rs[0]['cols'], cat_rows([r['rows'] for r in rs]), sum_counters([r['cnt'] for r in rs]))


class Eg:
    act = ()            # the base policies act inside the advance kernels

    @staticmethod
    def run(name, **users):
        import test_epsilon_greedy_device as t
        meta, cols, sim = t.run_fixture(name, **users)
        return dict(meta=meta, cols=cols, sim=sim, rows=sim.rows(), ledger=au.ledger(sim))

    @staticmethod
    def hold(what, name, rs):
        import test_epsilon_greedy_device as t
        try:
            t.assert_log_is_the_fixture(what, rs[0]['meta'], rs[0]['cols'], cat_rows([r['rows'] for r in rs]), [r['sim'] for r in rs])
        finally:
            for r in rs:
                r['sim'].close()


class Logreg:
    act = ('logreg_screen', 'logreg_acts')

    @staticmethod
    def run(name, **users):
        import test_hip_parity as t
        meta, cols, rows, cnt, led = t.run_fixture(name, with_ledger=True, **users)
        return dict(meta=meta, cols=cols, rows=rows, cnt=cnt, ledger=led)

    @staticmethod
    def hold(what, name, rs):
        import test_hip_parity as t
        t.assert_rows_are_the_reference_fixture(name, rs[0]['meta'], rs[0]['cols'], cat_rows([r['rows'] for r in rs]),
                                                sum_counters([r['cnt'] for r in rs]))


FAMILY = {'nn_ips': NnIps, 'poly': Poly, 'bayes': Bayes, 'poly_wh': PolyWh, 'eg_model': EgModel, 'eg': Eg, 'logreg': Logreg}


def assert_form(led, form, act):
    """The launch ledger shows the form (the table of the module's forms) and the family's act kernel; none of these agents is walked."""
    assert led['walk'] == led['walk2'] == led['walk_solo'] == 0, led
    if form == 'lockstep':
        assert led['advance'] > 0 and led['advance_run'] == led['tail'] == led['repack'] == 0, led
    elif form == 'rounds':
        assert led['advance_run'] > 0 and led['advance'] == 0, led
    elif form == 'repack_lockstep':
        assert led['repack'] > 0 and led['advance'] > 0 and led['advance_run'] == led['tail'] == 0, led
    elif form == 'repack_rounds':
        assert led['repack'] > 0 and led['advance_run'] > 0 and led['advance'] == led['tail'] == 0, led
    elif form == 'repack_tail':
        assert led['repack'] > 0 and led['tail'] > 0, led
    elif form == 'nocache_rounds':
        assert led['draw_cached'] == 0 and led['advance_run'] > 0 and led['advance'] == led['tail'] == 0, led
    else:
        assert form == 'default' and led['repack'] == 0, led
    assert not act or sum(led[k] for k in act) > 0, (act, led)


def run_in_form(family, name, form, monkeypatch, **users):
    fam = FAMILY[family]
    set_form(form, monkeypatch)
    r = fam.run(name, **users)
    print(f'{family} {name} {form} {users}: ledger', {k: v for k, v in r['ledger'].items() if v and k not in au.DESCRIPTORS})
    return r


@gpu
@pytest.mark.parametrize('family,name,form', FORM_CASES)
def test_fixture_in_form(family, name, form, monkeypatch):
    r = run_in_form(family, name, form, monkeypatch)
    try:
        assert_form(r['ledger'], form, r.get('act', getattr(FAMILY[family], 'act', ())))
    except AssertionError:
        if 'sim' in r:
            r['sim'].close()
        raise
    FAMILY[family].hold(f'{name} {form}', name, [r])


@gpu
@pytest.mark.parametrize('family,name,form', SHARDS)
def test_fixture_as_two_shards(family, name, form, monkeypatch):
    """Users [0, 37) in the default form and [37, n) with the state repack on: the rows concatenated, the unresolved lists joined
    and the counters summed are the fixture's."""
    n = gu.load(name)[0]['n_users']
    a = run_in_form(family, name, 'default', monkeypatch, first_user=0, n_users=SPLIT)
    b = run_in_form(family, name, form, monkeypatch, first_user=SPLIT, n_users=n - SPLIT)
    try:
        act = b.get('act', getattr(FAMILY[family], 'act', ()))
        assert_form(b['ledger'], form, act)
        assert not act or sum(a['ledger'][k] for k in act) > 0, a['ledger']
    except AssertionError:
        for r in (a, b):
            if 'sim' in r:
                r['sim'].close()
        raise
    FAMILY[family].hold(f'{name} shards', name, [a, b])


# ---------------------------------------------------------------------------------------------------------------------------
# offset ids with organic-only users in front, against the per-user host route
# ---------------------------------------------------------------------------------------------------------------------------
FIRST_ID, N_ORGANIC, N_OFFLINE = 65530, 10, 40          # the ids cross 65 535: the frame's `u` column goes to 32 bits


def host_route_agent(family):
    """-> env arguments, the agent, the frame comparison of the family's own file (got, want), the act kernels"""
    from device_util import assert_frames_equal
    if family == 'nn_ips':
        import test_nn_ips_device as t
        meta, agent = t.trained_agent()
        return meta['env_args'], agent, lambda got, want: t.assert_frames_equal_ps_bounded(got, want, 10, agent.frozen.state()), ('nn_ips',)
    if family == 'eg_model':
        import eg_models_util as mu
        meta, cols, P = mu.load('model_eg_poly_p10')
        return meta['env_args'], mu.wrapper(meta, cols, P), assert_frames_equal, ('logreg_poly',)
    t = __import__({'poly': 'test_logreg_poly_device', 'bayes': 'test_bayes_vb_device'}[family])
    meta, agent = t.trained_agent()
    return meta['env_args'], agent, assert_frames_equal, ({'poly': 'logreg_poly', 'bayes': 'bayes_vb'}[family],)


@gpu
@pytest.mark.parametrize('family', ['nn_ips', 'poly', 'bayes', 'eg_model'])
def test_offset_ids_with_organic_only_users_equal_the_host_route(family, monkeypatch):
    from device_util import make_env
    from recogym_amd.envs.reco_env_v1 import RecoEnv1
    env_args, agent, compare, act = host_route_agent(family)
    set_form('default', monkeypatch)
    env = make_env(env_args)
    want = env._generate_logs_per_user(N_OFFLINE, agent, N_ORGANIC, FIRST_ID)
    u, is_b = want['u'].to_numpy(dtype=np.int64), (want['z'] == 'bandit').to_numpy()
    assert u.min() == FIRST_ID and u.max() == FIRST_ID + N_OFFLINE + N_ORGANIC - 1 > 65535
    assert not is_b[u < FIRST_ID + N_ORGANIC].any() and is_b[u >= FIRST_ID + N_ORGANIC].any()
    seen, real = [], RecoEnv1.simulate

    def spy(self, *a, **k):
        cnt, sim = real(self, *a, **k)
        seen.append(au.ledger(sim))
        return cnt, sim
    monkeypatch.setattr(RecoEnv1, 'simulate', spy)
    for form in ('default', 'repack_tail'):            # (repack_tail's switches: the repack on, the rest as generate_logs runs by default)
        set_form(form, monkeypatch)
        del seen[:]
        with warnings.catch_warnings():
            warnings.simplefilter('error', RuntimeWarning)       # a fallback to the host route warns: it fails here
            got = make_env(env_args).generate_logs(N_OFFLINE, agent, num_organic_offline_users=N_ORGANIC, first_user_id=FIRST_ID)
        assert len(seen) == 1, 'generate_logs made no device run, or more than one'
        led = seen[0]
        print(f'{family} ids from {FIRST_ID}, {form}: ledger', {k: v for k, v in led.items() if v and k not in au.DESCRIPTORS})
        assert (led['repack'] > 0) == (form != 'default') and led['tail'] == 0 and sum(led[k] for k in act) > 0, led
        compare(got, want)
        ids, gb = got['u'].to_numpy(dtype=np.int64), (got['z'] == 'bandit').to_numpy()
        assert not gb[ids < FIRST_ID + N_ORGANIC].any(), 'an organic-only user logged a bandit row'


# ---------------------------------------------------------------------------------------------------------------------------
# without a GPU: the cases mean something
# ---------------------------------------------------------------------------------------------------------------------------
def lives(cols, first_user=0):
    """-> per user index: its number of rows, and per row its event index (the position among its user's rows)"""
    u = cols['u'].astype(np.int64) - first_user
    starts = np.flatnonzero(np.r_[True, u[1:] != u[:-1]])
    n_rows = np.diff(np.r_[starts, len(u)])
    return u, n_rows, np.arange(len(u)) - np.repeat(starts, n_rows)


def assert_repack_relabels(name, every, first_user=0):
    """At the second repack of a run that repacks every `every` launches, a user has stopped and a user with a higher id lives on
    to a bandit row: from then on that user's slot is not its index.  A launch takes a live user through at least one event and
    at most one organic event (a round ends at the first transition that is not 'bandit'), so in lock-step and in rounds alike a
    user of at most T = 2 x every rows has stopped at launch T, and a bandit row behind more than T organic rows is logged
    after it."""
    cols = gu.load(name)[1]
    keep = cols['u'] >= first_user
    cols = {k: cols[k][keep] for k in ('u', 'z')}
    u, n_rows, _ = lives(cols, first_user)
    T = 2 * every
    organic_before = np.concatenate([np.cumsum(cols['z'][u == i] == 0) for i in range(len(n_rows))])
    later = np.unique(u[(cols['z'] == 1) & (organic_before > T)])
    stopped = np.flatnonzero(n_rows <= T)
    assert len(stopped) and len(later) and later.max() > stopped.min(), (name, every, stopped[:4], later[:4])
    return len(stopped), len(later)


def test_the_repack_relabels_in_every_repacked_case():
    for family, name, form in FORM_CASES:
        if form.startswith('repack'):
            every = int(FORM_ENV[form]['RECOGYM_REPACK'])
            print(name, form, assert_repack_relabels(name, every))
    # The second shards: those of the two 40-user fixtures are users 37, 38 and 39, who all outlive the second repack — these two
    # shard cases hold the id offset (first_user + uidx against uidx) and a three-user wave, not the relabelling, which the
    # whole-fixture cases above hold for their families.  Stated, so that a regenerated fixture cannot change it unnoticed.
    three_users = {'bayes_p10_s120', 'poly_wh_exp_default'}
    for family, name, form in SHARDS:
        every = int(FORM_ENV[form]['RECOGYM_REPACK'])
        if name in three_users:
            assert gu.load(name)[0]['n_users'] - SPLIT == 3
            with pytest.raises(AssertionError):
                assert_repack_relabels(name, every, SPLIT)
        else:
            print(name, 'second shard', form, assert_repack_relabels(name, every, SPLIT))


def test_the_act_paths_are_exercised():
    for family, keys in SECOND_PATH.items():
        names = list(CASES[family]) + [n for f, n, _ in SHARDS if f == family]
        census = {n: gu.load(n)[0]['census'] for n in names}
        assert all(c['acts'] > 0 for c in census.values()), census
        assert any(c.get(k, 0) > 0 for c in census.values() for k in keys), (family, census)
    # the frozen LogReg fixture and the overlay over the base policies keep no census: bandit rows served by more than one action
    for name in list(CASES['logreg']) + list(CASES['eg']):
        cols = gu.load(name)[1]
        assert len(set(cols['a'][cols['z'] == 1].tolist())) > 1, name


def test_the_shards_are_ragged():
    for family, name, form in SHARDS:
        n = gu.load(name)[0]['n_users']
        assert 0 < SPLIT < n and SPLIT % 64 and (n - SPLIT) % 64, (name, n)
        cols = gu.load(name)[1]
        assert (cols['u'] < SPLIT).any() and (cols['u'] >= SPLIT).any() and (cols['z'][cols['u'] >= SPLIT] == 1).any()


# ---------------------------------------------------------------------------------------------------------------------------
# rg_sim_set_option("tail_below"): the create-time rule holds after create (host-only calls)
# ---------------------------------------------------------------------------------------------------------------------------
def test_tail_below_is_refused_where_create_keeps_it_zero(monkeypatch):
    from recogym_amd.envs.features.time import NormalTimeGenerator
    set_form('default', monkeypatch)
    lib = _abi.load()
    base = {**env_1_args, 'random_seed': 3, 'num_products': 12, 'K': 4}
    clock = NormalTimeGenerator(Configuration({'normal_time_mu': 0.0, 'normal_time_sigma': 1.5}))
    refused = [('LOGREG_FROZEN', base, dict(policy=_abi.RG_POLICY_LOGREG_FROZEN, policy_seed=0)),
               ('LOGREG_POLY', base, dict(policy=_abi.RG_POLICY_LOGREG_POLY, policy_seed=0)),
               ('BAYES_VB', base, dict(policy=_abi.RG_POLICY_BAYES_VB, policy_seed=0)),
               ('NN_IPS', base, dict(policy=_abi.RG_POLICY_NN_IPS, policy_seed=0)),
               ('time_mode', {**base, 'time_generator': clock}, dict(policy=_abi.RG_POLICY_ORGANIC_USER_COUNT, policy_seed=5, ouc=dict(gu.OUC_DEFAULTS)))]
    for what, args, pol in refused:
        h = au.host_sim(lib, Configuration(args), **pol)
        assert h is not None, (what, lib.rg_last_error())
        assert au.host_option(lib, h, 'tail_below') == 0, what              # what plan_repack_tail decided
        for v in (1, 64, 4096):
            assert lib.rg_sim_set_option(h, b'tail_below', v) == RG_EINVAL, (what, v)
            err = lib.rg_last_error()
            assert b'tail_below' in err and (b'time_mode' if what == 'time_mode' else b'LogReg family') in err, (what, err)
            assert au.host_option(lib, h, 'tail_below') == 0, what
        assert lib.rg_sim_set_option(h, b'tail_below', 0) == 0, (what, lib.rg_last_error())      # the EpsilonGreedy files set it
        assert lib.rg_sim_set_option(h, b'run_ahead', 0) == 0, what                               # (the other options are as they were)
        lib.rg_sim_destroy(h)
    h = au.host_sim(lib, Configuration(base), policy=_abi.RG_POLICY_ORGANIC_USER_COUNT, policy_seed=5, ouc=dict(gu.OUC_DEFAULTS))
    assert au.host_option(lib, h, 'tail_below') == 4096
    for v in (0, 7, 4096):
        assert lib.rg_sim_set_option(h, b'tail_below', v) == 0 and au.host_option(lib, h, 'tail_below') == v
    assert lib.rg_sim_set_option(h, b'tail_below', 1 << 32) == RG_EINVAL and b'2^32' in lib.rg_last_error()
    lib.rg_sim_destroy(h)
