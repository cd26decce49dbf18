"""Writes tests/golden/ope_*.npz: the reference's own evaluate_IPS / evaluate_SNIPS / evaluate_recall_at_k on fixture logs.

    python tests/make_golden_ope.py          (needs the reference package; see ref_harness.import_reference)

The reference's agents draw from their own MT19937 streams; here those are swapped for the addressed policy draw of the
(user, t) of the DefaultContext the evaluation passes (ContextAgentRng), so that this package's agents — which draw the
same way — are pinned by the same numbers.  Under the numpy installed here the reference's evaluate_IPS raises on every
agent that returns a `ps-a` vector (`np.ones(5)/5 != ()`); its per-row values are pinned through evaluate_SNIPS
(c in {0, 1}: c * pi / ps and c * (pi / ps) are the same double), the empty case through evaluate_IPS itself."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import golden_util as gu  # noqa: E402
import ref_harness as rh  # noqa: E402

LOGS = ('philox_p10', 'philox_ouc_eps', 'philox_bandit_mf')

# every OrganicUserEventCounter variant: select_randomly x exploit_explore x epsilon x reverse_pop
OUC_VARIANTS = [dict(select_randomly=sr, exploit_explore=ee, epsilon=eps, reverse_pop=rp)
                for sr in (True, False) for ee in (True, False) for eps in (0.0, 0.1) for rp in (False, True)]


class ContextAgentRng:
    """Duck-typed agent rng keyed by the (user, t) of the Observation the agent is acting on."""

    def __init__(self, policy_seed):
        self.policy_seed = policy_seed
        self.user = 0
        self.t = 0

    def choice(self, a, p=None):
        w = rh.draw(self.policy_seed, self.user, self.t, 0, rh.DRAW_POLICY)
        if p is None:
            return rh.bounded(w[0], w[1], int(a))
        if not isinstance(a, (int, np.integer)):
            return rh.numpy_choice_with_p(a, p, rh.uniform(w[0], w[1]))
        return rh.numpy_choice_with_p(a, p, rh.uniform(w[2], w[3]))


def keyed(agent, seed):
    """Wrap agent.act so that the agent's rng sees the (user, t) of each act."""
    rng = ContextAgentRng(seed)
    if hasattr(agent, 'model_builder'):
        # a ModelBasedAgent builds its model (and the model its RandomState) at its first act
        build0 = agent.model_builder.build

        def build():
            fp, model = build0()
            model.rng = rng
            return fp, model
        agent.model_builder.build = build
        if getattr(agent, 'model', None) is not None:
            agent.model.rng = rng
    else:
        agent.rng = rng
    act = agent.act

    def wrapped(observation, reward, done):
        ctx = observation.context()
        rng.user, rng.t = int(ctx.user()), int(ctx.time())
        return act(observation, reward, done)
    agent.act = wrapped
    return agent


def log_frame(cols):
    """Fixture columns -> the reference's DataFrame (generate_logs' dtypes, abstract.py:318-327)."""
    import pandas as pd
    is_b = cols['z'] == 1
    n = is_b.size
    return pd.DataFrame({
        't': cols['t'].astype(np.float32),
        'u': cols['u'].astype(np.int64),
        'z': np.where(is_b, 'bandit', 'organic').astype(object),
        'v': pd.array([None if b else int(x) for b, x in zip(is_b, cols['v'])], dtype=pd.UInt16Dtype()),
        'a': pd.array([int(x) if b else None for b, x in zip(is_b, cols['a'])], dtype=pd.UInt16Dtype()),
        'c': np.where(is_b, cols['c'], np.nan).astype(np.float32),
        'ps': np.where(is_b, cols['ps'], np.nan).astype(np.float64),
        'ps-a': [None] * n,
    })


def agents(recogym, P, cols):
    from recogym.agents import (BanditMFSquare, OrganicUserEventCounterAgent, RandomAgent, bandit_mf_square_args,
                                organic_user_count_args, random_args)
    from recogym import Configuration
    out = [('random', dict(), keyed(RandomAgent(Configuration({**random_args, 'num_products': P, 'random_seed': 5,
                                                               'with_ps_all': True})), 5))]
    out.append(('random_nopsall', dict(), keyed(RandomAgent(Configuration({**random_args, 'num_products': P,
                                                                           'random_seed': 5})), 5)))
    for i, v in enumerate(OUC_VARIANTS):
        ag = OrganicUserEventCounterAgent(Configuration({**organic_user_count_args, **v, 'num_products': P,
                                                        'random_seed': 11, 'with_ps_all': True}))
        out.append((f'ouc{i}', v, keyed(ag, 11)))
    if 'bmf_product_embedding' in cols:
        import torch
        bmf = BanditMFSquare(Configuration({**bandit_mf_square_args, 'num_products': P, 'with_ps_all': True}))
        with torch.no_grad():
            bmf.product_embedding.weight.copy_(torch.from_numpy(cols['bmf_product_embedding']))
            bmf.user_embedding.weight.copy_(torch.from_numpy(cols['bmf_user_embedding']))
        out.append(('bmf', dict(), bmf))
    return out


def main():
    recogym = rh.import_reference()
    import importlib
    ev = importlib.import_module('recogym.evaluate_agent')
    for name in LOGS:
        meta, cols = gu.load(name)
        P = meta['env_args']['num_products']
        df = log_frame(cols)
        res = {}
        names = {}
        for key, params, ag in agents(recogym, P, cols):
            if key == 'random_nopsall':
                res[f'{key}__ips'] = np.asarray(ev.evaluate_IPS(ag, df), dtype=np.float64)
                continue
            rewards, ratio = ev.evaluate_SNIPS(ag, df)
            res[f'{key}__c'] = np.asarray(rewards, dtype=np.float64)
            res[f'{key}__ratio'] = np.asarray(ratio, dtype=np.float64)
            res[f'{key}__recall'] = np.asarray(ev.evaluate_recall_at_k(ag, df, k=5), dtype=np.int8)
            names[key] = params
        out = os.path.join(gu.GOLDEN, f'ope_{name}.npz')
        np.savez_compressed(out, meta=json.dumps(dict(log=name, num_products=P, agents=names, random_seed=5, ouc_seed=11)),
                            **res)
        print(out, os.path.getsize(out))


if __name__ == '__main__':
    main()
