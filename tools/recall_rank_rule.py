"""Why recall@k has a table form and a ranking form, and no device form for OrganicUserEventCounter: the rank rule

    certain hit: at most k entries have pi >= pi[v];   certain miss: at least k entries have pi > pi[v];   a tie otherwise

against np.argpartition on the host loop's own `ps-a`, over the fixture logs of tests/golden/ope_*.npz (CPU only).

    python tools/recall_rank_rule.py [k ...]          (default 1 5 P) >> profiles/recall/rank_rule_ties.txt"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import golden_util as gu  # noqa: E402
from make_golden_ope import LOGS, OUC_VARIANTS, log_frame  # noqa: E402
from recogym_amd import evaluate_agent as ev  # noqa: E402
from recogym_amd.agents import LastViewTableAgent, OrganicUserEventCounterAgent, RandomAgent  # noqa: E402
from recogym_amd.envs.configuration import Configuration  # noqa: E402


def target(key, P, cols):
    if key == 'random':
        return RandomAgent(Configuration({'num_products': P, 'random_seed': 5, 'with_ps_all': True}))
    if key == 'bmf':
        return LastViewTableAgent.from_bandit_mf(Configuration({'num_products': P, 'with_ps_all': True}),
                                                 cols['bmf_product_embedding'], cols['bmf_user_embedding'])
    return OrganicUserEventCounterAgent(Configuration({'num_products': P, 'random_seed': 11, 'weight_history_function': None,
                                                       'with_ps_all': True, **OUC_VARIANTS[int(key[3:])]}))


def main():
    for name in LOGS:
        meta, cols = gu.load(name)
        P = meta['env_args']['num_products']
        ks = [int(x) for x in sys.argv[1:]] or [1, 5, P]
        df = log_frame(cols)
        agents = json.loads(str(np.load(f'{gu.GOLDEN}/ope_{name}.npz')['meta']))['agents']
        for key in agents:
            tally = {k: [0, 0, 0] for k in ks}                  # counted rows, ties, wrong verdicts

            def visit(uid, idx, jj, pi, c):
                i = idx[jj]
                if jj + 1 < len(idx) and not c['is_b'][idx[jj + 1]] and not c['c'][i]:
                    v = c['v'][idx[jj + 1]]
                    ge, gt = int((pi >= pi[v]).sum()), int((pi > pi[v]).sum())
                    for k in ks:
                        hit = v in set(np.argpartition(pi, -k)[-k:])
                        t = tally[k]
                        t[0] += 1
                        if ge <= k:
                            t[2] += not hit
                        elif gt >= k:
                            t[2] += hit
                        else:
                            t[1] += 1
            ev._host_loop(target(key, P, cols), df, visit)
            for k in ks:
                n, ties, wrong = tally[k]
                print(f'{name:18s} {key:6s} {json.dumps(agents[key]):90s} k = {k:2d}: counted {n:5d}  ties {ties:5d} ({100 * ties / max(n, 1):5.1f} %)  '
                      f'wrong verdicts {wrong}', flush=True)


if __name__ == '__main__':
    main()
