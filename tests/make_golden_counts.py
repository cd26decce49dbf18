"""Writes tests/golden/counts_*.npz: the reference's own OrganicCount and BanditCount after the reference's cached-log training
loop (bench_agents.py:90-166) over committed fixture logs.

    python tests/make_golden_counts.py          (needs the reference package; see ref_harness.import_reference)

The loop lives inside the reference's `_collect_stats`; it is run as it is, with `_cached_data` answering with the fixture's
DataFrame, `deepcopy` left out (so that the agent handed in is the one trained) and an evaluation of zero users.  The tables
are stored as coordinate lists (they are all integers): co_counts, pulls_a, clicks_a; beside them the two argmax tables,
BanditCount's `ps` per last viewed product (float64, the reference's ctr at the argmax), the agent's last_product_viewed after
training, and what `act` returns for a few observations."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import golden_util as gu  # noqa: E402
import ref_harness as rh  # noqa: E402

LOGS = ('philox_p10', 'philox_p10_sigma0', 'philox_ouc_eps', 'philox_p1000_k20', 'philox_bandit_mf', 'mt_config1')


def log_frame(cols):
    """Fixture columns -> the DataFrame the reference's cached loop reads row by row: v / a / c as floats with NaN where a
    row has none (the loop asserts with np.isnan), in generate_logs' column order (t, u, z, v, a, c, ps, ps-a)."""
    import pandas as pd
    is_b = cols['z'] == 1
    return pd.DataFrame({
        't': cols['t'].astype(np.float32),
        'u': cols['u'].astype(np.int64),
        'z': np.where(is_b, 'bandit', 'organic').astype(object),
        'v': np.where(is_b, np.nan, cols['v']).astype(np.float64),
        'a': np.where(is_b, cols['a'], np.nan).astype(np.float64),
        'c': np.where(is_b, cols['c'], np.nan).astype(np.float64),
        'ps': np.where(is_b, cols['ps'], np.nan).astype(np.float64),
        'ps-a': [None] * is_b.size,
    })


class _NoUsersEnv:
    """The evaluation half of _collect_stats, for zero users."""

    def generate_logs(self, num_offline_users, agent=None):
        import pandas as pd
        return pd.DataFrame({'a': np.zeros(0), 'c': np.zeros(0)})


def train_reference(agent, df):
    import importlib
    ba = importlib.import_module('recogym.bench_agents')
    saved = ba._cached_data, ba.deepcopy, ba.tqdm
    ba._cached_data = lambda env, n_organic, n_users: df
    ba.deepcopy = lambda x: x

    class _Bar:
        def __init__(self, *a, **k):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def update(self, *a):
            pass
    ba.tqdm = _Bar
    out = sys.stdout
    sys.stdout = open(os.devnull, 'w')
    try:
        ba._collect_stats(dict(env=_NoUsersEnv(), agent=agent, num_offline_users=0, num_online_users=0,
                               num_organic_offline_users=0, epoch_with_random_reset=False, epoch=0, with_cache=True))
    finally:
        sys.stdout.close()
        sys.stdout = out
        ba._cached_data, ba.deepcopy, ba.tqdm = saved
    return agent


def coo(table):
    r, c = np.nonzero(table)
    vals = table[r, c]
    assert np.array_equal(vals, np.rint(vals)), 'a count that is not an integer'
    return np.stack([r, c, vals.astype(np.int64)]).astype(np.int64)


def main():
    recogym = rh.import_reference()
    from recogym import Configuration, DefaultContext, Observation
    from recogym.agents import BanditCount, OrganicCount, bandit_count_args, organic_count_args
    from recogym.envs.session import OrganicSessions
    for name in LOGS:
        meta, cols = gu.load(name)
        P = meta['env_args']['num_products']
        df = log_frame(cols)
        oc = train_reference(OrganicCount(Configuration({**organic_count_args, 'num_products': P, 'with_ps_all': True})), df)
        bc = train_reference(BanditCount(Configuration({**bandit_count_args, 'num_products': P})), df)
        ctr = (bc.clicks_a + 1) / (bc.pulls_a + 2)
        assert np.array_equal(ctr, bc.ctr), 'the reference keeps ctr in step with its tables'
        o_arg = oc.co_counts.argmax(axis=1)
        b_arg = bc.ctr.argmax(axis=1)
        lpv = int(bc.last_product_viewed)           # (before the acts below move it)
        # a few acts: the observation's session ends in view l
        acts = []
        for l in sorted({0, 1, P // 2, P - 1}):
            s = OrganicSessions()
            s.next(DefaultContext(3, 7), np.int16(l))
            obs = Observation(DefaultContext(4, 7), s)
            ao, ab = oc.act(obs, 0, False), bc.act(obs, 0, False)
            assert sorted(ao) == sorted(ab) == ['a', 'ps', 'ps-a', 't', 'u']
            acts.append([l, int(ao['a']), float(ao['ps']), int(np.argmax(ao['ps-a'])), int(ab['a']), float(ab['ps'])])
        res = dict(co=coo(oc.co_counts), pulls=coo(bc.pulls_a), clicks=coo(bc.clicks_a),
                   organic_argmax=o_arg.astype(np.int32), bandit_argmax=b_arg.astype(np.int32),
                   bandit_ps=bc.ctr[np.arange(P), b_arg].astype(np.float64), acts=np.asarray(acts, dtype=np.float64))
        tied = int((np.sort(oc.co_counts, axis=1)[:, -1] == np.sort(oc.co_counts, axis=1)[:, -2]).sum())
        out = os.path.join(gu.GOLDEN, f'counts_{name}.npz')
        np.savez_compressed(out, meta=json.dumps(dict(
            log=name, num_products=P, last_product_viewed=lpv, organic_rows_tied=tied,
            organic_args=organic_count_args, bandit_args=bandit_count_args)), **res)
        print(out, os.path.getsize(out), 'tied rows', tied)


if __name__ == '__main__':
    main()
