"""Writes tests/golden/evo_*.npz: the reference's own evaluate_agent (recogym/evaluate_agent.py:51-146), unmodified, over its own
OrganicCount / BanditCount inside its own EpsilonGreedy, with the counter RNG injected.

    python tests/make_golden_evolution.py          (needs the reference package; see ref_harness.import_reference)

The env's rng is ref_harness.inject_counter_rng's; the wrapper's `rng` is an InjectedAgentRng whose __deepcopy__ returns itself:
evaluate_agent deep-copies the agent, and every copy must keep reading the (user, t) of the live env.  Nothing of the reference
is edited: `env.step`, the agent class's `act` / `train` and the `deepcopy` name of the reference's module are wrapped for the
run and restored after it.  A fixture records

  the rewards dict        success / success_greedy / failure / failure_greedy (one per step), actions (P, steps + 1)
  every row, in order     phase (0 = the initial users, s = step s), u, t, z, v, a, c and, per bandit row, greedy (1 / 0; -1 where
                          the act reported none) and trained (1 where a train call followed the act)
  the training agent      after every phase: its tables (dense at P = 10, coordinate lists with a phase column above) and its
                          last_product_viewed (-1 = None)
  meta                    the arguments, and the names and values of the reference's constants.py enums

No initial user of a fixture ends its episode in its first organic session (this package leaves such a user out of the initial
phase, the reference lets it act once more: DESIGN.md 8): the generator moves on to the next seed until that holds."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import golden_util as gu  # noqa: E402
import make_golden as mg  # noqa: E402
import ref_harness as rh  # noqa: E402

ENV = {**mg.BASE, 'num_products': 10, 'prob_leave_organic': 0.01, 'prob_leave_bandit': 0.01, 'prob_organic_to_bandit': 0.25,
       'prob_bandit_to_organic': 0.25}
BIG = dict(num_products=1000, K=20, sigma_omega=0.0)
EG = dict(epsilon=0.3, random_seed=7)
SHAPE = dict(n_init=10, n_step_users=15, num_steps=3)

# name -> dict(agent 'oc' | 'bc', eg = EpsilonGreedy arguments or None, approach, window, seed = the first env seed tried, ...)
CASES = {}
for _i, _ag in enumerate(('oc', 'bc')):
    for _j, (_tag, _approach, _window) in enumerate((('all', 'ALL_DATA', 10000), ('explore', 'ALL_EXPLORATION_DATA', 10000),
                                                     ('slide7', 'SLIDING_WINDOW_ALL_DATA', 7),
                                                     ('slide_explore3', 'SLIDING_WINDOW_EXPLORATION_DATA', 3),
                                                     ('last_step', 'LAST_STEP', 10000))):
        CASES[f'evo_{_ag}_{_tag}'] = dict(agent=_ag, eg=EG, approach=_approach, window=_window, seed=200 + 10 * _i + _j)
CASES['evo_bc_noinit_explore'] = dict(agent='bc', eg=EG, approach='ALL_EXPLORATION_DATA', window=10000, seed=230, n_init=0,
                                      min_none_rows=2)
CASES['evo_oc_not_pure_new'] = dict(agent='oc', eg=dict(EG, epsilon_pure_new=False), approach='ALL_DATA', window=10000, seed=231)
CASES['evo_oc_plain'] = dict(agent='oc', eg=None, approach='ALL_DATA', window=10000, seed=232)
CASES['evo_bc_p1000'] = dict(agent='bc', eg=EG, approach='ALL_EXPLORATION_DATA', window=10000, seed=233, env=BIG)


class StoppedInitialUser(Exception):
    pass


def sticky_rng_class():
    class StickyAgentRng(rh.InjectedAgentRng):
        def __deepcopy__(self, memo):
            return self
    return StickyAgentRng


def make_agent(kind, eg_args, P, env_rng):
    rh.import_reference()
    from recogym import Configuration
    from recogym.agents import BanditCount, OrganicCount, bandit_count_args, organic_count_args
    from recogym.agents.epsilon_greedy import EpsilonGreedy, epsilon_greedy_args
    if kind == 'oc':
        inner = OrganicCount(Configuration({**organic_count_args, 'num_products': P}))
    else:
        inner = BanditCount(Configuration({**bandit_count_args, 'num_products': P}))
    if eg_args is None:
        return inner
    agent = EpsilonGreedy(Configuration({**epsilon_greedy_args, **eg_args, 'num_products': P}), inner)
    agent.rng = sticky_rng_class()(env_rng, eg_args['random_seed'])
    return agent


def inner_of(agent):
    return agent.agent if hasattr(agent, 'agent') else agent


def snapshot(agent):
    inner = inner_of(agent)
    lpv = getattr(inner, 'last_product_viewed', None)
    out = dict(lpv=-1 if lpv is None else int(lpv))
    for name in ('co_counts', 'pulls_a', 'clicks_a'):
        if hasattr(inner, name):
            x = np.asarray(getattr(inner, name))
            assert np.array_equal(x, np.rint(x))
            out[name] = x.astype(np.int64)
    return out


def constants_record():
    import recogym
    return {name: {m.name: m.value for m in getattr(recogym, name)}
            for name in ('AgentStats', 'AgentInit', 'TrainingApproach', 'EvolutionCase', 'RoiMetrics')}


def run_once(case, seed):
    """One run of the reference's evaluate_agent -> (rewards, rows, snapshots); StoppedInitialUser where the seed does not qualify."""
    import importlib
    import recogym
    ev = importlib.import_module('recogym.evaluate_agent')
    args = {**ENV, **case.get('env', {}), 'random_seed': seed}
    P = args['num_products']
    shape = {**SHAPE, **{k: case[k] for k in SHAPE if k in case}}
    n_init, n_step = shape['n_init'], shape['n_step_users']
    env = rh.make_reference_env(args)
    env_rng = rh.inject_counter_rng(env)
    agent = make_agent(case['agent'], case['eg'], P, env_rng)
    rows, snaps, copies = [], [], []
    state = dict(greedy=-1, last_bandit=None)

    def phase_of(u):
        return 0 if u < n_init else 1 + (u - n_init) // n_step

    env_step = env.step

    def step(action_id):
        u, t_b = int(env_rng.user), int(env_rng.t)
        out = env_step(action_id)
        obs, reward, done, _ = out
        if action_id is None:
            if done and u < n_init:
                raise StoppedInitialUser(u)
        else:
            rows.append([phase_of(u), u, t_b, 1, -1, int(action_id), int(reward), state['greedy'], 0])
            state['last_bandit'] = len(rows) - 1
            state['greedy'] = -1
        for s in obs.sessions():
            rows.append([phase_of(u), int(s['u']), int(s['t']), 0, int(s['v']), -1, -1, -1, -1])
        return out
    env.step = step

    cls = type(agent)
    cls_act, cls_train, ev_deepcopy = cls.act, cls.train, ev.deepcopy

    def act(self, observation, reward, done):
        out = cls_act(self, observation, reward, done)
        state['greedy'] = int(bool(out['greedy'])) if 'greedy' in out else -1
        return out

    def train(self, observation, action, reward, done=False):
        assert action is not None
        rows[state['last_bandit']][8] = 1
        return cls_train(self, observation, action, reward, done)

    def deepcopy(x, *a, **k):
        # call 0: initial_agent; call 1: the training agent after the initial phase; call k >= 2: the one after step k - 1
        if len(copies) == 1:
            snaps.append(snapshot(x))
        elif len(copies) >= 2:
            snaps.append(snapshot(copies[-1]))
        copies.append(ev_deepcopy(x, *a, **k))
        return copies[-1]

    cls.act, cls.train, ev.deepcopy = act, train, deepcopy
    try:
        rewards = ev.evaluate_agent(env, agent, n_init, n_step, shape['num_steps'], getattr(recogym.TrainingApproach, case['approach']),
                                    case['window'])
    finally:
        cls.act, cls.train, ev.deepcopy = cls_act, cls_train, ev_deepcopy
    assert len(snaps) == shape['num_steps'] + 1
    return rewards, np.asarray(rows, dtype=np.int64), snaps, args, shape


def none_rows(rows, snaps):
    """How many trained rows of step 1 met last_product_viewed = None (BanditCount, no initial users)."""
    from recogym_amd.agents import count_tables as ct
    r = rows[rows[:, 0] == 1]
    is_b = r[:, 3] == 1
    ix, _, _, _ = ct.online_bandit_updates(r[:, 1], is_b, np.where(is_b, 0, r[:, 4]), np.where(is_b, r[:, 5], 0), r[:, 6] == 1, 1 << 20,
                                           is_b & (r[:, 8] == 1), None)
    return int((ix < 0).sum())


def run_case(name, case):
    import recogym
    seed = case['seed']
    while True:
        try:
            rewards, rows, snaps, args, shape = run_once(case, seed)
        except StoppedInitialUser:
            seed += 1000
            continue
        if case.get('min_none_rows') and none_rows(rows, snaps) < case['min_none_rows']:
            seed += 1000
            continue
        break
    first = {}
    for r in rows:                       # no initial user ends in its first session: every one of them has a bandit row
        first.setdefault(int(r[1]), []).append(int(r[3]))
    assert all(any(z) for u, z in first.items() if u < shape['n_init'])
    P = args['num_products']
    EC = recogym.EvolutionCase
    out = dict(success=np.asarray(rewards[EC.SUCCESS], dtype=np.int64), success_greedy=np.asarray(rewards[EC.SUCCESS_GREEDY], dtype=np.int64),
               failure=np.asarray(rewards[EC.FAILURE], dtype=np.int64), failure_greedy=np.asarray(rewards[EC.FAILURE_GREEDY], dtype=np.int64),
               actions=np.asarray([rewards[EC.ACTIONS][a] for a in range(P)], dtype=np.int64),
               phase=rows[:, 0].astype(np.int8), u=rows[:, 1].astype(np.int32), t=rows[:, 2].astype(np.int32), z=rows[:, 3].astype(np.int8),
               v=rows[:, 4].astype(np.int32), a=rows[:, 5].astype(np.int32), c=rows[:, 6].astype(np.int8), greedy=rows[:, 7].astype(np.int8),
               trained=rows[:, 8].astype(np.int8), lpv=np.asarray([s['lpv'] for s in snaps], dtype=np.int64))
    for tab in ('co_counts', 'pulls_a', 'clicks_a'):
        if tab in snaps[0]:
            if P <= 10:
                out[tab] = np.stack([s[tab] for s in snaps])
            else:
                coo = [np.c_[np.full(len(r), k), r, c, s[tab][r, c]] for k, s in enumerate(snaps) for r, c in [np.nonzero(s[tab])]]
                out[tab + '_coo'] = np.concatenate(coo).astype(np.int64)
    meta = dict(env_args=args, agent=case['agent'], eg_args=None if case['eg'] is None else {'epsilon_pure_new': True, **case['eg']},
                approach=case['approach'], window=case['window'], rng='philox', constants=constants_record(), **shape)
    path = os.path.join(gu.GOLDEN, name + '.npz')
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **out)
    is_b = rows[:, 3] == 1
    print(f'{name}: seed {seed}, {len(rows)} rows, {int(is_b.sum())} acts, {int((rows[:, 8] == 1).sum())} trained, '
          f'{int((rows[:, 7] == 0).sum())} explored -> {os.path.getsize(path) / 1024:.0f} KiB')
    assert os.path.getsize(path) < 229606, 'a fixture must stay below the largest one already committed'


def main():
    rh.import_reference()
    only = sys.argv[1:]
    for name, case in CASES.items():
        if not only or name in only:
            run_case(name, case)


if __name__ == '__main__':
    main()
