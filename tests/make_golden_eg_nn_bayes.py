"""Writes tests/golden/nn_eg_*.npz and bayes_eg_*.npz: logs of the reference's own EpsilonGreedy (recogym/agents/epsilon_greedy.py),
unmodified, round the reference's own NnIpsAgent (argmax form) and BayesianAgentVB.

    python tests/make_golden_eg_nn_bayes.py   (needs the reference package; never imported by a test)

(The files are not called model_eg_*: tests/eg_models_util.py lists every model_eg_*.npz as a fixture of the LogReg / likelihood
tests, which rebuild a LogReg from whatever they find there.)

The wrapper's `rng` is ref_harness.InjectedAgentRng(env_rng, eg_seed), as in make_golden_eg.py (flip: words 0,1 of the policy block
of (eg_seed, user, t); explore action: words 2,3), and `act` is wrapped to record `greedy` and `h0` of every bandit row.  The inner
agents draw nothing.  They are built as the plain fixtures' generators build them — make_golden_nn_ips.reference_agent (with its
dense feature provider) and load_weights with the scale and seed the plain loaded fixture recorded; make_golden_bayes_vb.reference_agent
on the same training log, Lambda cut to S_CUT draws at P = 10 — and the generator asserts that the model so built IS the one the plain
fixture stores, so the new files name that fixture (`weights_from` / `lambda_from`) instead of storing the model again.  The
environments are the plain fixtures' (the organic process does not depend on the actions: the greedy acts see the histories those
fixtures saw; prob_leave_* = 0.01 there, so users pass 64 rows), plus a BayesianAgentVB one with prob_leave_* = 0.05 (many users, many
trailing rows; the loaded net takes fewer than P / 2 distinct actions on histories that short).

Every file carries the log columns, `greedy`, `h0` (-1 on greedy acts and organic rows) and the meta with the census of the device
rule over the GREEDY acts: acts, explored, unresolved.  The generator ASSERTS, as conditions of the fixtures: the device rule
restated in NumPy (nn_ips_util.rule_over_log / bayes_util.rule_census on the log with `a` replaced by the greedy action) gives the
reference's greedy action on every act it resolves; this package's host act (sim.nn_host_act / sim.bayes_host_act, what
Simulator.poly_verify judges by) confirms every act, the unresolved ones included; unresolved <= 10 % of the acts; at least one
explored and one greedy act; for the loaded nets at least P / 2 distinct greedy actions; and on a greedy NnIpsAgent row the logged
ps is the float64 product (1 - epsilon) * prob[a] of a float32 prob[a].

nn_eg_ope / bayes_eg_ope: the reference's evaluate_SNIPS of the wrapper (with_ps_all on both agents) round each model on the
uniform-logger log philox_p10, the wrapper's stream keyed by the evaluated observation's (user, t) as in make_golden_ope.py; IPS is
pinned as c * ratio (c in {0, 1}: the same double; the reference's evaluate_IPS raises on a `ps-a` array under this numpy)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import bayes_util as bu  # noqa: E402
import eg_nn_bayes_util as xu  # noqa: E402
import golden_util as gu  # noqa: E402
import make_golden_bayes_vb as mb  # noqa: E402
import make_golden_eg as me  # noqa: E402
import make_golden_nn_ips as mn  # noqa: E402
import make_golden_ope as mo  # noqa: E402
import nn_ips_util as nu  # noqa: E402
import ref_harness as rh  # noqa: E402

EG = dict(epsilon=0.3, random_seed=7)
SHORT = dict(prob_leave_bandit=0.05, prob_leave_organic=0.05)

# name -> (inner kind, the plain fixture whose model and environment it takes, env overrides, users, eg args)
CASES = {
    'nn_eg_p10': ('nn', 'nn_ips_p10_loaded', {}, 80, EG),
    'nn_eg_p10_not_pure_new': ('nn', 'nn_ips_p10_loaded', {}, 100, dict(EG, epsilon_pure_new=False)),
    'nn_eg_p10_sigma0': ('nn', 'nn_ips_p10_loaded', dict(sigma_omega=0.0), 150, EG),
    'nn_eg_p40': ('nn', 'nn_ips_p40_loaded', {}, 150, EG),
    'bayes_eg_p4': ('bayes', 'bayes_p4', {}, 40, EG),
    'bayes_eg_p10_s120': ('bayes', 'bayes_p10_s120', {}, 40, EG),
    'bayes_eg_p10_s120_not_pure_new': ('bayes', 'bayes_p10_s120', dict(SHORT, random_seed=213), 120, dict(EG, epsilon_pure_new=False)),
}
OPE_LOG = 'philox_p10'
OPE_CASES = {'nn_eg_ope': ('nn', 'nn_ips_p10_loaded', EG),
             'bayes_eg_ope': ('bayes', 'bayes_p10_s120', dict(EG, epsilon=0.2, epsilon_pure_new=False))}

_BUILT = {}


def set_with_ps_all(config):
    object.__setattr__(config, 'with_ps_all', True)         # (the reference's Configuration ignores a plain assignment)


def reference_inner(kind, source, with_ps_all=False):
    """The reference's agent carrying the model of the plain fixture `source`, built as that fixture's generator built it."""
    smeta, scols = gu.load(source)
    args = smeta['env_args']
    P = args['num_products']
    plain_args = {**args, 'random_seed': 42, 'sigma_omega': 0.1, 'sigma_mu_organic': 3}      # (the training log's environment)
    key = (kind, source)
    if key not in _BUILT:
        if kind == 'nn':
            _BUILT[key] = rh.make_reference_env({**plain_args, 'random_seed': 1042}).generate_logs(mn.N_TRAIN)
        else:
            train = rh.make_reference_env({**plain_args, 'random_seed': 1042}).generate_logs(mb.N_TRAIN)
            ref = mb.reference_agent(P, train)
            _BUILT[key] = np.asarray(ref.model.Lambda, dtype=np.float64)[:scols['bayes_lambda'].shape[0]]
    if kind == 'nn':
        agent = mn.reference_agent(P, _BUILT[key], **({'with_ps_all': True} if with_ps_all else {}))
        mn.load_weights(agent, P, int(agent.config.num_hidden), smeta['weight_scale'], smeta['weight_seed'])
        state = mn.state_of(agent)
        assert all(np.array_equal(state[k], scols['nn_' + k]) for k in nu.KEYS), 'the net is not the one the plain fixture stores'
        return agent, P, args
    train = rh.make_reference_env({**plain_args, 'random_seed': 1042}).generate_logs(2)        # (any log: Lambda is set below)
    agent = mb.reference_agent(P, train)
    # the fit's Lambda on this machine against the stored one (BLAS may order its sums otherwise: the stored draws are the model)
    dev = float(np.abs(_BUILT[key] - scols['bayes_lambda']).max() / np.abs(scols['bayes_lambda']).max())
    assert dev < 1e-9, dev
    agent.model.Lambda = scols['bayes_lambda'].copy()
    if with_ps_all:
        set_with_ps_all(agent.config)
        set_with_ps_all(agent.model.config)
        assert agent.model.config.with_ps_all and agent.config.with_ps_all
    return agent, P, args


def host_confirms(kind, cols, P, model):
    """This package's host act on every act of the log against the log's action -> the number of acts."""
    from recogym_amd import sim
    from recogym_amd.agents.nn_ips import NnIpsFrozenAgent
    from recogym_amd.envs.configuration import Configuration
    host = NnIpsFrozenAgent(Configuration({'num_products': P}), model) if kind == 'nn' else None
    acts = nu.acts_of_log(cols, P)
    for rows, prods, cnts in acts:
        views = np.repeat(prods, cnts)
        got = sim.nn_host_act(views, P, host) if kind == 'nn' else sim.bayes_host_act(views, P, model)
        assert all(got == cols['a'][i] for i in rows), (kind, int(cols['u'][rows[0]]), rows[0], got)
    return len(acts)


def census_of(kind, cols, P, model, eg_args, loaded):
    is_b = cols['z'] == 1
    g = xu.greedy_cols(cols)
    out = dict(explored=int(np.sum(cols['greedy'][is_b] == 0)), greedy=int(np.sum(cols['greedy'][is_b] == 1)))
    if kind == 'nn':
        from recogym_amd.agents.nn_ips import UNRESOLVED
        acts = nu.rule_over_log(g, P, model)
        for act in acts:
            if not act['flags'] & UNRESOLVED:
                assert all(act['action'] == g['a'][i] for i in act['rows']), (act['user'], act['rows'][0], act['action'])
            for i in act['rows']:
                if cols['greedy'][i] == 1:
                    # the logged value: (1.0 - epsilon) * float(prob[a]), and the restated ps within the proven bound of prob[a]
                    p32 = np.float32(cols['ps'][i] / (1.0 - eg_args['epsilon']))
                    assert (1.0 - eg_args['epsilon']) * float(p32) == cols['ps'][i], (i, cols['ps'][i])
                    if act['action'] == g['a'][i]:
                        assert abs(act['ps'] / float(p32) - 1.0) <= act['bound'], (i, act['ps'], float(p32), act['bound'])
        out.update(acts=len(acts), unresolved=sum(1 for a in acts if a['flags'] & UNRESOLVED),
                   distinct_greedy_actions=len(set(g['a'][is_b].tolist())))
        assert not loaded or 2 * out['distinct_greedy_actions'] >= P, out
    else:
        c = bu.rule_census(g, P, model)
        out.update(acts=int(c['acts']), unresolved=int(c['unresolved']), saturated=int(c['saturated']))
        assert bool((cols['ps'][is_b & (cols['greedy'] == 1)] == (1.0 - eg_args['epsilon']) * 1.0).all())
    assert host_confirms(kind, g, P, model) == out['acts']
    assert 10 * out['unresolved'] <= out['acts'], out
    assert out['explored'] > 0 and out['greedy'] > 0, out
    return out


def run_case(name, kind, source, env_over, n_users, eg_args):
    inner, P, src_args = reference_inner(kind, source)
    args = {**src_args, **env_over}
    eg = me.make_eg(eg_args, inner, P)
    env = rh.make_reference_env(args)
    env_rng = rh.inject_counter_rng(env, None, None)
    eg.rng = rh.InjectedAgentRng(env_rng, eg_args['random_seed'])
    greedy, h0 = [], []
    act = eg.act

    def recording(observation, reward, done):
        out = act(observation, reward, done)
        greedy.append(bool(out['greedy']))
        h0.append(int(out['h0']) if 'h0' in out else -1)
        assert ('h0' in out) == (not out['greedy'])
        return out
    eg.act = recording
    df = env.generate_logs(n_users, eg)
    arrays = rh.log_to_arrays(df)
    is_b = arrays['z'] == 1
    assert is_b.sum() == len(greedy)
    g_col, h_col = np.full(len(df), -1, dtype=np.int8), np.full(len(df), -1, dtype=np.int32)
    g_col[is_b], h_col[is_b] = greedy, h0
    small = dict(t=arrays['t'].astype(np.int32), u=arrays['u'].astype(np.int32), z=arrays['z'].astype(np.int8),
                 v=arrays['v'].astype(np.int32), a=arrays['a'].astype(np.int32), c=arrays['c'].astype(np.int8), ps=arrays['ps'],
                 greedy=g_col, h0=h_col)
    smeta, scols = gu.load(source)
    model = nu.fixture_state(smeta, scols) if kind == 'nn' else scols['bayes_lambda']
    census = census_of(kind, small, P, model, eg_args, loaded='weight_scale' in smeta)
    lens = np.bincount(small['u'])
    meta = dict(env_args=args, n_users=n_users, eg_args={'epsilon_pure_new': True, **eg_args}, inner=kind,
                **({'weights_from': source} if kind == 'nn' else {'lambda_from': source}), rng='philox', census=census,
                longest_user=int(lens.max()))
    path = os.path.join(gu.GOLDEN, name + '.npz')
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **small)
    size = os.path.getsize(path)
    print(f'{name}: {len(df)} rows, longest user {lens.max()}, {census} -> {size / 1024:.0f} KiB')
    assert size <= 228 * 1024, size
    return meta, small


def crosses_a_chunk(cols):
    """Bandit rows that share one act cross a 64-row chunk of the replay: rows 63 and 64 of a user are both bandit rows."""
    u, z = cols['u'], cols['z']
    start = np.flatnonzero(np.r_[True, u[1:] != u[:-1]])
    return any(s + 64 < len(u) and u[s + 64] == u[s] and z[s + 63] == 1 and z[s + 64] == 1 for s in start)


def run_ope_case(name, kind, source, eg_args):
    import importlib
    ev = importlib.import_module('recogym.evaluate_agent')
    meta, cols = gu.load(OPE_LOG)
    P = meta['env_args']['num_products']
    inner, P_model, _ = reference_inner(kind, source, with_ps_all=True)
    assert P_model == P
    eg = me.make_eg(eg_args, inner, P, with_ps_all=True)
    rng = mo.ContextAgentRng(eg_args['random_seed'])
    eg.rng = rng
    act = eg.act

    def keyed(observation, reward, done):
        ctx = observation.context()
        rng.user, rng.t = int(ctx.user()), int(ctx.time())
        return act(observation, reward, done)
    eg.act = keyed
    rewards, ratio = ev.evaluate_SNIPS(eg, mo.log_frame(cols))
    path = os.path.join(gu.GOLDEN, name + '.npz')
    np.savez_compressed(path, meta=np.array(json.dumps(dict(log=OPE_LOG, num_products=P, eg_args={'epsilon_pure_new': True, **eg_args},
                                                            inner=kind, **({'weights_from': source} if kind == 'nn' else {'lambda_from': source}),
                                                            ips_from='c * ratio of evaluate_SNIPS'))),
                        c=np.asarray(rewards, dtype=np.float64), ratio=np.asarray(ratio, dtype=np.float64))
    nz = int(np.count_nonzero(ratio))
    print(f'{name}: {len(ratio)} ratios, != 0: {nz} -> {os.path.getsize(path) / 1024:.0f} KiB')
    assert 0 < nz < len(ratio)


def main():
    assert rh.reference_available(), 'needs the reference package'
    rh.import_reference()
    only = sys.argv[1:]
    done = {name: run_case(name, *case) for name, case in CASES.items() if not only or name in only}
    for name in ('nn_eg_p10', 'bayes_eg_p4'):
        if name in done:
            assert done[name][0]['longest_user'] > 64 and crosses_a_chunk(done[name][1]), f'{name}: no act crosses a chunk'
    for name, case in OPE_CASES.items():
        if not only or name in only:
            run_ope_case(name, *case)


if __name__ == '__main__':
    main()
