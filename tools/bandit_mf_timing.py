"""Time BanditMFSquare's training on the log of N offline users built on the device (uniform logger, reco-gym-v1 defaults):
train_from_log on the device route (rg_bmf_samples + rg_bmf_steps; wall clock around the whole call, device events around the step
kernel alone) and, with --host, on the host route of the same commit — the reference's arithmetic, which stands in for the
reference's own class where that cannot run.  A warm-up, then the minimum of --reps runs, each on a fresh agent with the same
initial weights.  Prints one JSON line per size; with --out the lines are appended to that file (profiles/bandit_mf/).

    python tools/bandit_mf_timing.py [--products 10|100|1000|10000] [--users 2000,20000,200000] [--host-users 2000] [--reps 3] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from recogym_amd.agents import BanditMFSquareAgent, bandit_mf_square_args  # noqa: E402
from recogym_amd.envs.configuration import Configuration  # noqa: E402
from recogym_amd.envs.reco_env_v1 import env_1_args  # noqa: E402
from recogym_amd.sim import Simulator  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--products', type=int, default=10)
    ap.add_argument('--users', default='2000,20000,200000')
    ap.add_argument('--host-users', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--budget-s', type=float, default=300.0, help='a size whose step kernel is predicted (from the size before it) to '
                    'take longer than this over all its runs is run once after the warm-up; beyond 4 times this it is left out')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    P = args.products
    torch.manual_seed(7)
    first = BanditMFSquareAgent(Configuration({**bandit_mf_square_args, 'num_products': P}))
    init = [p.detach().numpy().copy() for p in first._params()]

    def fresh(device_training):
        return BanditMFSquareAgent(Configuration({**bandit_mf_square_args, 'num_products': P, 'device_training': device_training}), *init)

    us_per_user = None
    for n in [int(x) for x in args.users.split(',')]:
        reps = args.reps
        if us_per_user is not None:
            predicted = us_per_user * n * 1e-6 * (args.reps + 1)
            if predicted > 4 * args.budget_s:
                print(json.dumps(dict(users=n, P=P, skipped=f'predicted {predicted:.0f} s of step kernel over {args.reps + 1} runs')), flush=True)
                continue
            if predicted > args.budget_s:
                reps = 1
        sim = Simulator(Configuration({**env_1_args, 'random_seed': 42, 'num_products': P}), n, device='cuda:0')
        sim.reset_users(0, n)
        sim.run()
        dl = sim.device_log()
        res = dict(users=n, P=P, E=5, mini_batch=32, rows=int(dl.rows.shape[0]))
        best, best_steps = None, None
        for rep in range(reps + 1):                            # (the first run is the warm-up)
            agent = fresh(True)
            assert agent.device_route()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            agent.train_from_log(dl, 0)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep:
                best = dt if best is None else min(best, dt)
                ms = agent.last_device_stats['steps_ms']
                best_steps = ms if best_steps is None else min(best_steps, ms)
        st = agent.last_device_stats
        us_per_user = 1e3 * best_steps / n
        res.update(runs=reps, calls=st['calls'], steps=st['steps'], empty_steps=st['empty_steps'], samples=st['samples'], device_route_s=best,
                   step_kernel_ms=best_steps, us_per_step=1e3 * best_steps / max(st['steps'], 1),
                   calls_per_s=st['calls'] / best)
        if n <= args.host_users:
            lc = sim.log_columns()
            t_host = None
            for rep in range(args.reps + 1):
                host = fresh(False)
                t0 = time.perf_counter()
                host.train_from_log(lc, 0)
                dt = time.perf_counter() - t0
                if rep:
                    t_host = dt if t_host is None else min(t_host, dt)
            res.update(host_route_s=t_host, host_calls_per_s=st['calls'] / t_host, speedup=t_host / best,
                       same_table=bool(np.array_equal(host.frozen().table, agent.frozen().table)),
                       max_weight_difference=max(float(np.abs(a.detach().numpy() - b.detach().numpy()).max())
                                                 for a, b in zip(host._params(), agent._params())))
        sim.close()
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'a') as fh:
                fh.write(line + '\n')


if __name__ == '__main__':
    main()
