"""Time rg_ope_replay and rg_ope_replay_eg on a C3 log (P = 10 000, K = 20, OrganicUserEventCounter logger, 10^7 users by
default) built on the device.  Three target sets: Random, LastViewTable and OUC (epsilon = 0); one dense OUC form (epsilon
smoothing); EpsilonGreedy (epsilon = 0.05) over a LastViewTable.  Warm-up, then device events (profiler off); bytes from the
log's shapes: 16 B row + 8 B ps per row read, 8 B ratio per bandit row written.  Per timed target the sha256 of the ratios'
and of the three sums' bytes (two builds of the library compute the same: equal digests).
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/ope_timing.py`.  Prints one JSON line; with --out the
line is appended to that file.  --host-users 0 skips the host loop.

    python tools/ope_timing.py [--users N] [--reps R] [--host-users 10000] [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from recogym_amd import _abi  # noqa: E402
from recogym_amd import evaluate_agent as ev  # noqa: E402
from recogym_amd.agents import (EpsilonGreedy, LastViewTableAgent, OrganicUserEventCounterAgent, RandomAgent,  # noqa: E402
                                epsilon_greedy_args)
from recogym_amd.envs.configuration import Configuration  # noqa: E402
from recogym_amd.envs.reco_env_v1 import env_1_args, rows_to_dataframe  # noqa: E402
from recogym_amd.sim import Simulator  # noqa: E402


def ouc(P, **v):
    return OrganicUserEventCounterAgent(Configuration({'num_products': P, 'random_seed': 11, 'weight_history_function': None,
                                                      'with_ps_all': True, **v}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=10_000_000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--host-users', type=int, default=10_000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    P, n = 10_000, args.users
    cfg = Configuration({**env_1_args, 'random_seed': 42, 'num_products': P, 'K': 20})
    o = dict(select_randomly=True, exploit_explore=True, epsilon=0.0, reverse_pop=False)
    sim = Simulator(cfg, n, device='cuda:0', policy=_abi.RG_POLICY_ORGANIC_USER_COUNT, policy_seed=11, ouc=o)
    sim.reset_users(0, n)
    sim.run()
    dl = sim.device_log()
    rows = int(dl.rows.shape[0])
    code = dl.rows[:, 2]
    bandit = int(((code & _abi.RG_EV_BANDIT) != 0).sum().item())
    lens = dl.offsets[1:] - dl.offsets[:-1]
    table = np.random.RandomState(3).randint(0, P, size=P)
    sets = {
        'random_lvt_ouc': [RandomAgent(Configuration({'num_products': P, 'random_seed': 5, 'with_ps_all': True})),
                           LastViewTableAgent(Configuration({'num_products': P, 'with_ps_all': True}), table), ouc(P, **o)],
        'ouc_dense_eps': [ouc(P, select_randomly=True, exploit_explore=False, epsilon=0.1, reverse_pop=False)],
        'eg_table': [EpsilonGreedy(Configuration({**epsilon_greedy_args, 'epsilon': 0.05, 'random_seed': 7, 'num_products': P,
                                                  'with_ps_all': True}),
                                   LastViewTableAgent(Configuration({'num_products': P, 'with_ps_all': True}), table))],
    }
    res = dict(users=n, rows=rows, bandit_rows=bandit, max_user_rows=int(lens.max().item()), P=P,
               bytes_per_replay=rows * (16 + 8) + bandit * 8)
    for name, agents in sets.items():
        per, sha = {}, {}
        for ag in agents:
            r, _, sums = ev.ope_replay(ag, dl)          # warm-up (and the workspace / output allocations of the pass)
            torch.cuda.synchronize()
            sha[type(ag).__name__] = dict(ratio=hashlib.sha256(r.cpu().numpy().tobytes()).hexdigest(),
                                          sums=hashlib.sha256(sums.cpu().numpy().tobytes()).hexdigest())
            del r
            ms = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                ev.ope_replay(ag, dl)
                b.record()
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b))
            per[type(ag).__name__] = min(ms)
        res[name + '_ms'] = per
        res[name + '_total_ms'] = sum(per.values())
        res[name + '_sha256'] = sha
    # the host loop at --host-users users (a DataFrame of the log's first users)
    hu = min(args.host_users, n)
    if hu:
        end = int(dl.offsets[hu].item())
        from recogym_amd.sim import decode_rows
        ps = dl.ps[:end].cpu().numpy() if dl.ps is not None and not isinstance(dl.ps, float) else None
        df = rows_to_dataframe(decode_rows(dl.rows[:end].cpu().numpy(), ps64=ps), P)
        t0 = time.perf_counter()
        ev._host_snips(ouc(P, **o), df)
        res['host_loop_s'] = dict(users=hu, rows=end, ouc_s=time.perf_counter() - t0)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
