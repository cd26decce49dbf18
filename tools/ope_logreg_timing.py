"""Time the off-policy replay of the frozen LogReg policy at BASELINE config 5's shape (P = 10 000, K = 20, uniform logger,
10^6 users by default) with a dense random model of P classes:
  1. rg_ope_replay_logreg (argmax form) on the uniform log;
  2. rg_ope_replay of RandomAgent on the same log in the same process — the cost of streaming the rows once, the floor;
  3. a simulation of the same population UNDER that model with logreg=dict(fp16=False): the step loop's own fp32 act path
     (k_logreg_select + k_logreg_acts), its profiling slot and RG_CNT_LR_ACTS — the yardstick: the same bytes per act and the
     same arithmetic.
Reported: ms per act of the replay and of the step loop.  Warm-up, then device events (profiler off).
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/ope_logreg_timing.py` (no counters in the same run).
replay_sha256: the digests of the replay's ratios and of its three sums (two builds of the library compute the same: equal digests).
Prints one JSON line; with --out the line is appended to that file (profiles/ope/ope_logreg_timing.txt).

    python tools/ope_logreg_timing.py [--users N] [--products P] [--reps R] [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from recogym_amd import _abi  # noqa: E402
from recogym_amd import evaluate_agent as ev  # noqa: E402
from recogym_amd.agents import LogregFrozenAgent, RandomAgent  # noqa: E402
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
    ap.add_argument('--users', type=int, default=1_000_000)
    ap.add_argument('--products', type=int, default=10_000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    P, n = args.products, args.users
    cfg = Configuration({**env_1_args, 'random_seed': 42, 'num_products': P, 'K': 20})
    rng = np.random.RandomState(0)
    lr = LogregFrozenAgent(Configuration({'num_products': P, 'with_ps_all': True}), rng.standard_normal((P, P)) * 0.1,
                           rng.standard_normal(P) * 0.1, np.arange(P, dtype=np.int32))
    sim = Simulator(cfg, n, device='cuda:0')
    sim.reset_users(0, n)
    sim.run()
    dl = sim.device_log()
    rows = int(dl.rows.shape[0])
    bandit = int(((dl.rows[:, 2] & _abi.RG_EV_BANDIT) != 0).sum().item())
    lens = dl.offsets[1:] - dl.offsets[:-1]
    res = dict(users=n, P=P, classes=P, rows=rows, bandit_rows=bandit, max_user_rows=int(lens.max().item()), log_bytes=rows * 16)
    # the model on the device once (ope_replay moves a host model per call: 1.2 GB at this size, not what is measured here)
    pol = ev.ope_policy_of(lr)
    dev = dl.rows.device
    pol['logreg'] = dict(pol['logreg'], **{k: torch.as_tensor(pol['logreg'][k]).to(dev) for k in ('coef_t', 'intercept', 'classes')})
    st = {}
    res['replay_ms'], out = timed(lambda: ev.ope_replay(lr, dl, pol, stats=st), args.reps)
    res['replay_sha256'] = dict(ratio=hashlib.sha256(out[0].cpu().numpy().tobytes()).hexdigest(),
                                sums=hashlib.sha256(out[2].cpu().numpy().tobytes()).hexdigest())
    del out
    res['replay_acts'], res['replay_exact'], res['replay_rows_read'] = st['acts'], st['exact'], st['rows_read']
    # (the fp32 copy and the certificate's bounds are derived per call: timed alone, subtracted below)
    res['model_prep_ms'], _ = timed(lambda: ev._logreg_model(pol['logreg'], P, dev), args.reps)
    rnd = RandomAgent(Configuration({'num_products': P, 'random_seed': 5, 'with_ps_all': True}))
    res['stream_floor_ope_random_ms'], _ = timed(lambda: ev.ope_replay(rnd, dl), args.reps)
    del sim, dl, pol
    # the step loop under the same model, fp32 act path only
    tsim = Simulator(cfg, n, device='cuda:0', policy=_abi.RG_POLICY_LOGREG_FROZEN, policy_seed=0, log_capacity=0,
                     logreg=dict(coef_t=lr.coef_t, intercept=lr.intercept, classes=lr.classes, fp16=False))
    for rep in range(2):                                   # (warm-up, then the profiled run)
        tsim.set_profiling(rep == 1)
        tsim.reset_users(0, n)
        tsim.run()
    prof, cnt = tsim.profile(), tsim.counters()
    res['step_loop_logreg_ms'], res['step_loop_acts'], res['step_loop_exact'] = prof['logreg_ms'], cnt['lr_acts'], cnt['lr_exact']
    res['step_loop_rows_read'] = cnt['lr_rows']
    res['replay_ms_per_act'] = (res['replay_ms'] - res['model_prep_ms']) / max(res['replay_acts'], 1)
    res['step_loop_ms_per_act'] = res['step_loop_logreg_ms'] / max(res['step_loop_acts'], 1)
    res['replay_over_step_loop'] = res['replay_ms_per_act'] / res['step_loop_ms_per_act'] if res['step_loop_ms_per_act'] else None
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
