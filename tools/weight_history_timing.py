"""Time the likelihood agent's act on a time-weighted view history (k_wh_insert + k_poly_acts_w) beside its act on view counts
(k_logreg_select + k_poly_acts) on the same model and population.

10^5 users, K = 20, sigma_omega = 0.1, a dense random model at P = 1 000, two simulations of the same users run to the end:
  1. counts:   RG_POLICY_LOGREG_POLY — an act per change of a user's history that an event needed;
  2. weighted: the same handle with a weight table (exp(-0.2 t), float64) — a fresh act for every bandit event and every trailing
     row, at the event's clock value, so it computes several times as many acts: both counts are reported, and every per-act
     figure divides by the run's own count.
us per act = the library's profiling slot of the act kernels (HIP events round them in every step, rg_sim_set_profiling) /
RG_CNT_LR_ACTS.  One warm-up run of each, then `--reps` alternating pairs; min and max are reported.
Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/weight_history_timing.py --reps 1` (no counters in the same run).
Then the training feed: the device feed's wall time (rg_weighted_feed, both passes and the transfers) beside the host loop
train_data_weighted on a uniform-policy log of `--feed-users` users (2 000) of the same configuration (0 skips it).
Prints one JSON line each; with --out they are appended to that file (profiles/weight_history/weight_history_timing.txt).

    python tools/weight_history_timing.py [--users N] [--products P] [--reps R] [--feed-users M] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from recogym_amd import _abi  # noqa: E402
from recogym_amd.agents.logreg_poly import expit_steps  # noqa: E402
from recogym_amd.agents.views_history import weight_table  # noqa: E402
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


def feed_timing(cfg, n, table, f32, out):
    """The training feed on a uniform-policy log of `n` users of the same configuration: rg_weighted_feed (both passes, the
    transfers and the CSR on the host; one warm-up, then two calls) beside the host loop train_data_weighted, once."""
    import time
    import torch
    from recogym_amd.agents.feature_feed import train_data_from_log, weighted_train_data_device
    sim = Simulator(cfg, n, device='cuda:0', policy=_abi.RG_POLICY_UNIFORM_ENV, policy_seed=cfg.random_seed)
    sim.reset_users(0, n)
    sim.run()
    dl, cols = sim.device_log(), sim.log_columns()
    dev_s = []
    for rep in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = weighted_train_data_device(dl, cfg.num_products, table, f32)
        dev_s.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    want = train_data_from_log(cols, cfg.num_products, weight_history_function=lambda t: np.exp(-0.2 * t))
    host_s = time.perf_counter() - t0
    want[0].sort_indices()
    same = (np.array_equal(got[0].indptr, want[0].indptr) and np.array_equal(got[0].indices, want[0].indices)
            and np.array_equal(got[0].data.view(np.uint32), want[0].data.view(np.uint32)))
    line = json.dumps(dict(feed_users=n, log_rows=int(dl.rows.shape[0]), feature_rows=int(got[0].shape[0]), nnz=int(got[0].nnz),
                           device_feed_s=dict(min=min(dev_s[1:]), max=max(dev_s[1:])), host_loop_s=host_s,
                           speedup=host_s / min(dev_s[1:]), identical=bool(same)))
    print(line, flush=True)
    if out:
        with open(out, 'a') as f:
            f.write(line + '\n')
    sim.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=100_000)
    ap.add_argument('--products', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--feed-users', type=int, default=2000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    n, P = args.users, args.products
    cfg = Configuration({**env_1_args, 'random_seed': 42, 'num_products': P, 'K': 20, 'sigma_omega': 0.1})
    rng = np.random.RandomState(0)
    model = dict(wf=rng.standard_normal(P) * 0.1, wa=rng.standard_normal(P) * 0.1 / P, wk=rng.standard_normal((P, P)) * 0.1, intercept=0.1,
                 expit_steps=expit_steps())
    table, f32 = weight_table(lambda t: np.exp(-0.2 * t))
    sims = dict(
        counts=Simulator(cfg, n, device='cuda:0', log_capacity=0, policy=_abi.RG_POLICY_LOGREG_POLY, policy_seed=0, logreg_poly=model),
        # (the weighted run reads the step's views back from the log: it needs one)
        weighted=Simulator(cfg, n, device='cuda:0', policy=_abi.RG_POLICY_LOGREG_POLY, policy_seed=0,
                           logreg_poly=dict(model, weight_history=dict(table=table, f32=f32))))
    ms, cnt = {k: [] for k in sims}, {}
    for rep in range(args.reps + 1):                   # rep 0 warms up
        for k, sim in sims.items():
            t, cnt[k] = one_run(sim, n)
            if rep:
                ms[k].append(t)
    res = dict(P=P, users=n, reps=args.reps, acts={k: cnt[k]['lr_acts'] for k in sims},
               list_entries_per_act={k: cnt[k]['lr_rows'] / cnt[k]['lr_acts'] for k in sims},
               events={k: cnt[k]['bandit'] + cnt[k]['phantom'] for k in sims},
               hist_overflow=cnt['weighted']['hist_overflow'], wh_clock_range=cnt['weighted']['wh_clock_range'],
               poly_unresolved={k: cnt[k]['poly_unresolved'] for k in sims})
    for k in sims:
        res[f'{k}_ms'] = dict(min=min(ms[k]), max=max(ms[k]))
        res[f'{k}_us_per_act'] = 1e3 * min(ms[k]) / cnt[k]['lr_acts']
    res['ratio_weighted_over_counts_per_act'] = res['weighted_us_per_act'] / res['counts_us_per_act']
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write(line + '\n')
    for sim in sims.values():
        sim.close()
    if args.feed_users:
        feed_timing(cfg, args.feed_users, table, f32, args.out)


if __name__ == '__main__':
    main()
