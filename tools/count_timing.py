"""Time the count agents' training on a C3 log (P = 10 000, K = 20, sigma_omega = 0, uniform logger, 10^7 users by default)
built on the device: train_from_log of OrganicCount and of BanditCount (rg_count_train), rg_count_policy of both, and beside them
rg_ope_replay of RandomAgent on the same log in the same process — the cost of streaming the rows once, the floor the training
kernel is judged against.  Warm-up, then device events (profiler off).  Also: cell updates the log stands for vs global atomics
issued (the rest was summed in LDS), and the vectorised host form on the log's first --host-users users.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/count_timing.py` (no counters in the same run).
Prints one JSON line; with --out the line is appended to that file (profiles/counts/count_timing.txt).

    python tools/count_timing.py [--users N] [--reps R] [--host-users 10000] [--products P] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from recogym_amd import _abi  # noqa: E402
from recogym_amd import evaluate_agent as ev  # noqa: E402
from recogym_amd.agents import RandomAgent  # noqa: E402
from recogym_amd.agents import count_tables as ct  # noqa: E402
from recogym_amd.envs.configuration import Configuration  # noqa: E402
from recogym_amd.envs.reco_env_v1 import env_1_args  # noqa: E402
from recogym_amd.sim import Simulator  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    out = None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return min(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=10_000_000)
    ap.add_argument('--products', type=int, default=10_000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--host-users', type=int, default=10_000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    P, n = args.products, args.users
    cfg = Configuration({**env_1_args, 'random_seed': 42, 'num_products': P, 'K': 20, 'sigma_omega': 0.0})
    sim = Simulator(cfg, n, device='cuda:0')
    sim.reset_users(0, n)
    sim.run()
    dl = sim.device_log()
    dev = dl.rows.device
    rows = int(dl.rows.shape[0])
    bandit = int(((dl.rows[:, 2] & _abi.RG_EV_BANDIT) != 0).sum().item())
    lens = dl.offsets[1:] - dl.offsets[:-1]
    res = dict(users=n, P=P, rows=rows, organic_rows=rows - bandit, bandit_rows=bandit, max_user_rows=int(lens.max().item()),
               log_bytes=rows * 16)
    co = torch.zeros((P, P), dtype=torch.int64, device=dev)
    pulls, clicks = torch.zeros_like(co), torch.zeros_like(co)
    res['organic_train_ms'], (_, st) = timed(lambda: ct.count_train(dl, P, co=co), args.reps)
    res['organic_updates'], res['organic_global_atomics'] = st['updates'], st['global_atomics']
    res['bandit_train_ms'], (_, st) = timed(lambda: ct.count_train(dl, P, pulls=pulls, clicks=clicks), args.reps)
    res['bandit_updates'], res['bandit_global_atomics'] = st['updates'], st['global_atomics']
    res['organic_policy_ms'], _ = timed(lambda: ct.count_policy(P, _abi.RG_COUNT_ORGANIC, co=co), args.reps)
    res['bandit_policy_ms'], _ = timed(lambda: ct.count_policy(P, _abi.RG_COUNT_BANDIT, pulls=pulls, clicks=clicks), args.reps)
    rnd = RandomAgent(Configuration({'num_products': P, 'random_seed': 5, 'with_ps_all': True}))
    res['stream_floor_ope_random_ms'], _ = timed(lambda: ev.ope_replay(rnd, dl), args.reps)
    res['organic_over_floor'] = res['organic_train_ms'] / res['stream_floor_ope_random_ms']
    res['bandit_over_floor'] = res['bandit_train_ms'] / res['stream_floor_ope_random_ms']
    # the vectorised host form on the first --host-users users
    hu = min(args.host_users, n)
    end = int(dl.offsets[hu].item())
    raw = dl.rows[:end].cpu().numpy().view(np.uint32)
    is_b = (raw[:, 2] & _abi.RG_EV_BANDIT) != 0
    idx = (raw[:, 2] & _abi.RG_EV_INDEX_MASK).astype(np.int64)
    u = raw[:, 0].astype(np.int64)
    click = (raw[:, 2] & _abi.RG_EV_CLICK) != 0
    t0 = time.perf_counter()
    ct.organic_updates(u, is_b, np.where(is_b, 0, idx), P)
    t1 = time.perf_counter()
    ct.bandit_updates(u, is_b, np.where(is_b, 0, idx), np.where(is_b, idx, 0), click, P, None)
    res['host_form_s'] = dict(users=hu, rows=end, organic_s=t1 - t0, bandit_s=time.perf_counter() - t1)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
