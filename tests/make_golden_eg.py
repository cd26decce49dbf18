"""Writes tests/golden/eg_*.npz: logs of the reference's own EpsilonGreedy (recogym/agents/epsilon_greedy.py), unmodified, with the
counter RNG injected.

    python tests/make_golden_eg.py          (needs the reference package; see ref_harness.import_reference)

The wrapper's `rng` is ref_harness.InjectedAgentRng(env_rng, eg_seed) — its explore flip `choice([True, False], p)` reads words
0,1 of the policy block of (eg_seed, user, t), its explore action `choice(P, p)` words 2,3: the draw contract of
include/recogym_rng.h — and the inner agent is injected by inject_counter_rng with its own seed.  The log comes from the
reference's env.generate_logs; `act` is wrapped to record `greedy` and `h0` (-1 on greedy acts) of every bandit row.

Inner agents: the reference's RandomAgent and OrganicUserEventCounterAgent, and TableAgent below (a = table[last view] with a
float64 `ps` table, on the reference's Agent base), which stands for the trained count agents without their training.

Two more fixtures (eg_ope_*.npz) hold the reference's evaluate_SNIPS of EpsilonGreedy targets with with_ps_all over the
uniform-logger log philox_p10, the agents' streams keyed by the (user, t) of the evaluated observation as in make_golden_ope.py
(c in {0, 1}: evaluate_IPS's c * pi / ps is c * ratio, the same double)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import golden_util as gu  # noqa: E402
import make_golden as mg  # noqa: E402
import make_golden_ope as mo  # noqa: E402
import ref_harness as rh  # noqa: E402

ENV = {**mg.BASE, 'prob_leave_bandit': 0.05, 'prob_leave_organic': 0.05}

# name -> (env overrides, users, eg args, inner kind, inner args)
CASES = {
    'eg_p10_eps0_table': (dict(random_seed=101), 60, dict(epsilon=0.0, random_seed=7), 'table', dict(table_seed=1)),
    'eg_p10_eps03_random': (dict(random_seed=102), 80, dict(epsilon=0.3, random_seed=7), 'random', dict(random_seed=19)),
    'eg_p10_eps03_random_same_seed': (dict(random_seed=103), 60, dict(epsilon=0.3, random_seed=19), 'random', dict(random_seed=19)),
    'eg_p10_eps1_ouc': (dict(random_seed=104), 60, dict(epsilon=1.0, random_seed=7), 'ouc', dict(random_seed=23)),
    'eg_p10_eps03_ouc': (dict(random_seed=105), 80, dict(epsilon=0.3, random_seed=23), 'ouc', dict(random_seed=23)),
    'eg_p10_eps03_ouc_argmax_sigma0': (dict(random_seed=106, sigma_omega=0.0), 80, dict(epsilon=0.3, random_seed=7), 'ouc',
                                       dict(random_seed=23, select_randomly=False)),
    'eg_p10_eps03_table_sigma0': (dict(random_seed=107, sigma_omega=0.0), 100, dict(epsilon=0.3, random_seed=7), 'table',
                                  dict(table_seed=2)),
    'eg_p2_pure_new_table': (dict(random_seed=108, num_products=2), 60, dict(epsilon=0.5, random_seed=7), 'table', dict(table_seed=3)),
    'eg_p1000_k20_table_sigma0': (dict(random_seed=109, num_products=1000, K=20, sigma_omega=0.0), 50, dict(epsilon=0.3, random_seed=7),
                                  'table', dict(table_seed=4)),
    'eg_p1000_k20_random': (dict(random_seed=110, num_products=1000, K=20), 50, dict(epsilon=0.3, random_seed=7), 'random',
                            dict(random_seed=19)),
    'eg_p10_not_pure_new_random': (dict(random_seed=111), 80, dict(epsilon=0.3, random_seed=7, epsilon_pure_new=False), 'random',
                                   dict(random_seed=19)),
    'eg_p10_not_pure_new_table': (dict(random_seed=112), 60, dict(epsilon=0.3, random_seed=7, epsilon_pure_new=False), 'table',
                                  dict(table_seed=5)),
}

OPE_LOG = 'philox_p10'
OPE_CASES = {
    'eg_ope_random': (dict(epsilon=0.3, random_seed=7), 'random', dict(random_seed=19)),
    'eg_ope_table_not_pure_new': (dict(epsilon=0.2, random_seed=7, epsilon_pure_new=False), 'table', dict(table_seed=6)),
}


def tables(P, seed):
    """The TableAgent's two tables: an action and a float64 propensity per last viewed product."""
    r = np.random.RandomState(seed)
    return r.randint(0, P, size=P).astype(np.int32), r.uniform(0.05, 1.0, size=P)


def table_agent_class():
    rh.import_reference()
    from recogym.agents import Agent

    class TableAgent(Agent):
        def __init__(self, config, table, ps):
            super().__init__(config)
            self.table, self.ps, self.last_product_viewed = table, ps, None

        def act(self, observation, reward, done):
            if observation.sessions():
                self.last_product_viewed = int(observation.sessions()[-1]['v'])
            a = int(self.table[self.last_product_viewed])
            ps_all = ()
            if self.config.with_ps_all:
                ps_all = np.zeros(self.config.num_products)
                ps_all[a] = 1.0
            return {**super().act(observation, reward, done), 'a': a, 'ps': float(self.ps[self.last_product_viewed]), 'ps-a': ps_all}
    return TableAgent


def make_inner(kind, args, P, with_ps_all=False):
    rh.import_reference()
    from recogym import Configuration
    if kind == 'table':
        table, ps = tables(P, args['table_seed'])
        return table_agent_class()(Configuration({'num_products': P, 'with_ps_all': with_ps_all}), table, ps), dict(table=table, table_ps=ps)
    return mg.make_agent(kind, {**args, 'num_products': P, 'with_ps_all': with_ps_all}), {}


def make_eg(eg_args, inner, P, with_ps_all=False):
    from recogym import Configuration
    from recogym.agents.epsilon_greedy import EpsilonGreedy, epsilon_greedy_args
    return EpsilonGreedy(Configuration({**epsilon_greedy_args, **eg_args, 'num_products': P, 'with_ps_all': with_ps_all}), inner)


def run_case(name, env_over, n_users, eg_args, kind, inner_args):
    args = {**ENV, **env_over}
    P = args['num_products']
    env = rh.make_reference_env(args)
    inner, extra = make_inner(kind, inner_args, P)
    eg = make_eg(eg_args, inner, P)
    env_rng = rh.inject_counter_rng(env, None if kind == 'table' else inner, inner_args.get('random_seed'))
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
                 greedy=g_col, h0=h_col, **extra)
    meta = dict(env_args=args, n_users=n_users, eg_args={'epsilon_pure_new': True, **eg_args}, inner=kind, inner_args=inner_args,
                rng='philox')
    path = os.path.join(gu.GOLDEN, name + '.npz')
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **small)
    n_b = int(is_b.sum())
    print(f'{name}: {len(df)} rows, {n_b} acts, {n_b - int(np.sum(greedy))} explored -> {os.path.getsize(path) / 1024:.0f} KiB')


def run_ope_case(name, eg_args, kind, inner_args):
    import importlib
    ev = importlib.import_module('recogym.evaluate_agent')
    meta, cols = gu.load(OPE_LOG)
    P = meta['env_args']['num_products']
    inner, extra = make_inner(kind, inner_args, P, with_ps_all=True)
    eg = make_eg(eg_args, inner, P, with_ps_all=True)
    rngs = [mo.ContextAgentRng(eg_args['random_seed'])]
    eg.rng = rngs[0]
    if kind != 'table':
        rngs.append(mo.ContextAgentRng(inner_args['random_seed']))
        inner.rng = rngs[1]
    act = eg.act

    def keyed(observation, reward, done):
        ctx = observation.context()
        for r in rngs:
            r.user, r.t = int(ctx.user()), int(ctx.time())
        return act(observation, reward, done)
    eg.act = keyed
    rewards, ratio = ev.evaluate_SNIPS(eg, mo.log_frame(cols))
    path = os.path.join(gu.GOLDEN, name + '.npz')
    np.savez_compressed(path, meta=np.array(json.dumps(dict(log=OPE_LOG, num_products=P, eg_args={'epsilon_pure_new': True, **eg_args},
                                                            inner=kind, inner_args=inner_args))),
                        c=np.asarray(rewards, dtype=np.float64), ratio=np.asarray(ratio, dtype=np.float64), **extra)
    print(f'{name}: {len(ratio)} ratios -> {os.path.getsize(path) / 1024:.0f} KiB')


def main():
    for name, case in CASES.items():
        run_case(name, *case)
    for name, case in OPE_CASES.items():
        run_ope_case(name, *case)


if __name__ == '__main__':
    main()
