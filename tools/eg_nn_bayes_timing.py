"""Time EpsilonGreedy round NnIpsAgent and BayesianAgentVB: the step loop with and without the overlay, and generate_logs on the
device route against the host route.

Seeded random models (a 10-20-20-10 net, 120 posterior draws) at P = 10, K = 5, the default drift sigma_omega = 0.1.
  --mode step  per agent a simulator of --users users (10^5) with the log and its float64 `ps` side array attached, unwrapped and
               (--what both) with the overlay (epsilon = 0.05, pure_new).  A step = reset_users + run to the end, timed with device
               events; one warm-up, then --reps alternating repetitions; min and max are reported, `overlay_step_loop` = wrapped /
               unwrapped (the minimum of each).  --what unwrapped times the unwrapped loop alone: with --package-root that of another
               checkout (the parent commit, which has no device form of the wrapped loop), in a process of its own.
  --mode logs  generate_logs of --log-users users (2 000) under the wrapper: --route device (the wrapper's key `device_models`) or
               --route host (without the key: the route every checkout has), wall clock, one warm-up of 50 users first.
Prints one JSON line per agent; with --out the lines are appended to that file (profiles/eg_nn_bayes/).

    python tools/eg_nn_bayes_timing.py --mode step [--what both|unwrapped] [--users N] [--reps 3] [--package-root DIR] [--out FILE]
    python tools/eg_nn_bayes_timing.py --mode logs --route device|host [--log-users N] [--package-root DIR] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

P, K, HIDDEN, DRAWS = 10, 5, 20, 120
OVERLAY = dict(epsilon=0.05, seed=7, pure_new=True)


def models():
    rng = np.random.RandomState(0)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)       # noqa: E731
    state = dict(w1=f(HIDDEN, P), b1=f(HIDDEN), w2=f(HIDDEN, HIDDEN), b2=f(HIDDEN), w3=f(P, HIDDEN), b3=f(P))
    return dict(nn=state, bayes=rng.standard_normal((DRAWS, P * P)) * 0.5)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def emit(res, out):
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'a') as f:
            f.write(line + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=('step', 'logs'), required=True)
    ap.add_argument('--what', choices=('both', 'unwrapped'), default='both')
    ap.add_argument('--route', choices=('device', 'host'), default='device')
    ap.add_argument('--users', type=int, default=100_000)
    ap.add_argument('--log-users', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--package-root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--label', default='')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import recogym_amd as recogym
    from recogym_amd import _abi
    from recogym_amd.agents import EpsilonGreedy, epsilon_greedy_args
    from recogym_amd.agents.bayesian_poly_vb import BayesianVBFrozenAgent
    from recogym_amd.agents.nn_ips import NnIpsFrozenAgent
    from recogym_amd.envs.configuration import Configuration
    from recogym_amd.envs.reco_env_v1 import env_1_args
    from recogym_amd.sim import Simulator
    env_args = {**env_1_args, 'random_seed': 42, 'num_products': P, 'K': K}
    cfg = Configuration(env_args)
    m = models()
    inner = dict(nn=NnIpsFrozenAgent(Configuration({'num_products': P}), m['nn']),
                 bayes=BayesianVBFrozenAgent(Configuration({'num_products': P}), m['bayes']))
    base = dict(mode=args.mode, label=args.label, P=P, K=K)
    for kind, agent in inner.items():
        if args.mode == 'step':
            n = args.users
            common = dict(device='cuda:0', ps_float64=True, **agent.device_policy())
            sims = dict(unwrapped=Simulator(cfg, n, **common))
            if args.what == 'both':
                sims['wrapped'] = Simulator(cfg, n, epsilon_greedy=OVERLAY, **common)

            def step(sim):
                sim.reset_users(0, n)
                sim.run()
            ms, cnt = {k: [] for k in sims}, {}
            for rep in range(args.reps + 1):                   # rep 0 warms up
                for k, sim in sims.items():
                    t, _ = timed(lambda: step(sim))
                    cnt[k] = sim.counters()
                    if rep:
                        ms[k].append(t)
            res = dict(base, agent=kind, users=n, epsilon=OVERLAY['epsilon'], reps=args.reps)
            for k, sim in sims.items():
                c = cnt[k]
                res[k] = dict(ms=dict(min=min(ms[k]), max=max(ms[k])), events=c['organic'] + c['bandit'], acts=c['lr_acts'],
                              unresolved=c['poly_unresolved'], clicks=c['clicks'], steps=c['step'])
                sim.close()
            if 'wrapped' in sims:
                res['overlay_step_loop'] = res['wrapped']['ms']['min'] / res['unwrapped']['ms']['min']
            emit(res, args.out)
            del sims
            torch.cuda.empty_cache()
        else:
            key = {'device_models': True} if args.route == 'device' else {}
            eg = EpsilonGreedy(Configuration({**epsilon_greedy_args, 'epsilon': OVERLAY['epsilon'], 'random_seed': OVERLAY['seed'],
                                              'num_products': P, **key}), agent)
            assert (eg.device_policy() is not None) == (args.route == 'device'), 'this checkout has no such route'
            env = recogym.make('reco-gym-v1')
            env.init_gym(env_args)
            env.generate_logs(50, eg)                          # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            df = env.generate_logs(args.log_users, eg)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            emit(dict(base, agent=kind, route=args.route, users=args.log_users, rows=int(len(df)), seconds=dt,
                      bandit_rows=int((df['z'] == 'bandit').sum())), args.out)
            env.close()
    _ = _abi


if __name__ == '__main__':
    main()
