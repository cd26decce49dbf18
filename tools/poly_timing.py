"""Time the likelihood agent's act kernel against the existing frozen-LogReg act on the same population and histories.

At P = 1 000 and P = 10 000 (K = 20, the default drift: lock-step rounds) two simulations of the same users run to the end:
  1. RG_POLICY_LOGREG_POLY with a dense random model (wf, wa, wk): k_logreg_select + k_poly_acts;
  2. RG_POLICY_LOGREG_FROZEN with a dense random model of P classes on its float64-only path
     (logreg=dict(fp32=False, fp16=False)): k_logreg_select + k_logreg_acts -> logreg_act_wave.
Both read the same bytes per act (n rows of P doubles for a history of n products) — the yardstick is the existing kernel.  The
view histories do not depend on the actions (change_omega_for_bandits is off); the acts each run computed are reported (they
differ by a fraction of a percent: where a round ends a bandit run depends on the actions' click probabilities), and every
per-act figure divides by the run's own count.
us per act = the library's profiling slot of the act kernels (HIP events round k_logreg_select + the act kernel of every step,
rg_sim_set_profiling) / RG_CNT_LR_ACTS.  One warm-up run of each, then `--reps` alternating pairs; min and max are reported.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/poly_timing.py --reps 1` (no counters in the same run).
Prints one JSON line per P; with --out the lines are appended to that file (profiles/poly/poly_timing.txt).

    python tools/poly_timing.py [--users N] [--products 1000,10000] [--reps R] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from recogym_amd import _abi  # noqa: E402
from recogym_amd.agents.logreg_poly import expit_steps  # noqa: E402
from recogym_amd.envs.configuration import Configuration  # noqa: E402
from recogym_amd.envs.reco_env_v1 import env_1_args  # noqa: E402
from recogym_amd.sim import Simulator  # noqa: E402


def one_run(sim, n):
    sim.reset_users(0, n)
    sim.set_profiling(True)
    before = sim.profile()['logreg_ms']
    sim.run()
    cnt = sim.counters()
    ms = sim.profile()['logreg_ms'] - before
    sim.set_profiling(False)
    return ms, cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=100_000)
    ap.add_argument('--products', default='1000,10000')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    n = args.users
    th = expit_steps()
    for P in [int(x) for x in args.products.split(',')]:
        cfg = Configuration({**env_1_args, 'random_seed': 42, 'num_products': P, 'K': 20})
        rng = np.random.RandomState(0)
        dense = rng.standard_normal((P, P)) * 0.1
        vec = rng.standard_normal((3, P)) * 0.1
        sims = dict(
            poly=Simulator(cfg, n, device='cuda:0', log_capacity=0, policy=_abi.RG_POLICY_LOGREG_POLY, policy_seed=0,
                           logreg_poly=dict(wf=vec[0], wa=vec[1] / P, wk=dense, intercept=0.1, expit_steps=th)),
            frozen=Simulator(cfg, n, device='cuda:0', log_capacity=0, policy=_abi.RG_POLICY_LOGREG_FROZEN, policy_seed=0,
                             logreg=dict(coef_t=dense.T, intercept=vec[2], classes=np.arange(P, dtype=np.int32), fp32=False, fp16=False)))
        ms = {k: [] for k in sims}
        cnt = {}
        for rep in range(args.reps + 1):                   # rep 0 warms up
            for k, sim in sims.items():
                t, cnt[k] = one_run(sim, n)
                if rep:
                    ms[k].append(t)
        acts, rows = cnt['poly']['lr_acts'], cnt['poly']['lr_rows']
        res = dict(P=P, users=n, acts={k: cnt[k]['lr_acts'] for k in sims}, history_rows={k: cnt[k]['lr_rows'] for k in sims},
                   history_rows_per_act=rows / acts, bytes_per_act=rows / acts * P * 8, reps=args.reps,
                   poly_table=cnt['poly']['poly_table'], poly_unresolved=cnt['poly']['poly_unresolved'],
                   frozen_float64_acts=cnt['frozen']['lr_exact'])
        for k in sims:
            res[f'{k}_ms'] = dict(min=min(ms[k]), max=max(ms[k]))
            res[f'{k}_us_per_act'] = 1e3 * min(ms[k]) / cnt[k]['lr_acts']
        res['ratio_poly_over_frozen'] = res['poly_us_per_act'] / res['frozen_us_per_act']
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')
        for sim in sims.values():
            sim.close()
        del sims, dense


if __name__ == '__main__':
    main()
