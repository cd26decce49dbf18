"""Time one evolution step of evaluate_agent's device route on BASELINE config 3's shape (P = 10 000, K = 20, sigma_omega = 0) at
10^6 users: EpsilonGreedy(epsilon = 0.05) over an OrganicCount trained from a device log of --train-users users.
  run            reset_users + run to the end with the log attached (what env.simulate does per step)
  stats          rg_evolution_stats over the step's sorted log
  train_*        rg_count_train_online into the co_counts table with mask NULL, the explored rows only, every 10^4-th act
and, in the same process on the same log, the two kernels they are judged against:
  stream_floor   rg_ope_replay of RandomAgent: the cost of streaming the rows once
  count_train    rg_count_train: the unfiltered reduction (it also counts phantom rows and trailing sessions)
1 warm-up, then --reps timed repetitions of each with device events; every repetition is listed, min / median / spread
(max - min over median) are reported: the spread is the run-to-run noise a difference has to exceed.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/evolve_timing.py` (no counters in the same run).
Prints one JSON line; with --out the line is appended to that file (profiles/evolve/evolve_timing.txt).

    python tools/evolve_timing.py [--users N] [--reps 5] [--train-users 100000] [--epsilon 0.05] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from recogym_amd import _abi  # noqa: E402
from recogym_amd import evaluate_agent as ev  # noqa: E402
from recogym_amd.agents import EpsilonGreedy, OrganicCount, RandomAgent, epsilon_greedy_args, organic_count_args  # noqa: E402
from recogym_amd.agents import count_tables as ct  # noqa: E402
from recogym_amd.envs.configuration import Configuration  # noqa: E402
from recogym_amd.envs.reco_env_v1 import env_1_args  # noqa: E402
from recogym_amd.sim import Simulator  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    med = statistics.median(ms)
    return dict(ms=min(ms), median_ms=med, spread=(max(ms) - min(ms)) / med, ms_all=ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=1_000_000)
    ap.add_argument('--products', type=int, default=10_000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--train-users', type=int, default=100_000)
    ap.add_argument('--epsilon', type=float, default=0.05)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    P, n = args.products, args.users
    cfg = Configuration({**env_1_args, 'random_seed': 42, 'num_products': P, 'K': 20, 'sigma_omega': 0.0})
    oc = OrganicCount(Configuration({**organic_count_args, 'num_products': P}))
    sim = Simulator(cfg, args.train_users, device='cuda:0')
    sim.reset_users(n, args.train_users)             # (training users: ids behind the timed ones)
    sim.run()
    oc.train_online_from_log(sim.device_log())
    sim.close()
    del sim
    agent = EpsilonGreedy(Configuration({**epsilon_greedy_args, 'epsilon': args.epsilon, 'random_seed': 7, 'num_products': P}), oc)
    sim = Simulator(cfg, n, device='cuda:0', **agent.device_policy())

    def run():
        sim.reset_users(0, n)
        sim.run()
    res = dict(users=n, P=P, K=20, epsilon=args.epsilon, reps=args.reps, train_users=args.train_users)
    res['run'] = timed(run, args.reps)
    dl = sim.device_log()
    dev = dl.rows.device
    code = dl.rows[:, 2]
    is_act = ((code & _abi.RG_EV_BANDIT) != 0) & ((code & _abi.RG_EV_PHANTOM) == 0)
    rows, acts = int(dl.rows.shape[0]), int(is_act.sum().item())
    res.update(rows=rows, acts=acts, log_bytes=rows * 16)
    eg = agent._overlay()
    res['stats'] = timed(lambda: ev.evolution_stats_device(dl, eg), args.reps)
    counts, _, explored = ev.evolution_stats_device(dl, eg)
    res['counts'] = counts.cpu().tolist()
    every, _ = ev.training_mask(ev.TrainingApproach.SLIDING_WINDOW_ALL_DATA, is_act, None, 0, 10_000)
    co = torch.zeros((P, P), dtype=torch.int64, device=dev)
    for key, mask in (('train_null', None), ('train_explored', explored), ('train_every_10000th', every)):
        m = None if mask is None else mask.to(torch.uint8)
        res[key] = timed(lambda: ct.count_train_online(dl, P, co=co, mask=m), args.reps)
        res[key].update(counted=acts if m is None else int((m.bool() & is_act).sum().item()),
                        **ct.count_train_online(dl, P, co=co, mask=m)[1])
    rnd = RandomAgent(Configuration({'num_products': P, 'random_seed': 5, 'with_ps_all': True}))
    res['stream_floor_ope_random'] = timed(lambda: ev.ope_replay(rnd, dl), args.reps)
    res['count_train'] = timed(lambda: ct.count_train(dl, P, co=co), args.reps)
    res['count_train'].update(ct.count_train(dl, P, co=co)[1])
    res['stats_over_floor'] = res['stats']['median_ms'] / res['stream_floor_ope_random']['median_ms']
    for key in ('train_null', 'train_explored', 'train_every_10000th'):
        res[key + '_over_count_train'] = res[key]['median_ms'] / res['count_train']['median_ms']
    sim.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
