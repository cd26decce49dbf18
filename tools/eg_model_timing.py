"""Time EpsilonGreedy round the likelihood agent against the same agent unwrapped, in the step loop and in the off-policy replay.

At P = 1 000 and P = 10 000 (10^5 users, K = 20, the default drift sigma_omega = 0.1: lock-step rounds) with the dense random
likelihood models of tools/poly_timing.py:
  step loop  two simulators of the same users, RG_POLICY_LOGREG_POLY alone and with the overlay (epsilon = 0.05, pure_new), both
             with the log and its float64 `ps` side array attached.  A step = reset_users + run to the end, timed with device
             events; `overlay_step_loop` = wrapped / unwrapped (the minimum of each).
  replay     the unwrapped run's log replayed under the plain target (rg_ope_replay_poly) and under the wrapped one
             (rg_ope_replay_poly_eg), the model kept on the device between calls; evaluate_agent.ope_replay is timed whole, so both
             sides include the validation pass, the read-back of the head words and the host's confirmation of the listed acts;
             `overlay_replay` = wrapped / plain.
One warm-up of everything, then --reps alternating repetitions; min and max are reported.  Kernel times: run under
`rocprofv3 --kernel-trace --stats -- python tools/eg_model_timing.py --reps 1` (no counters in the same run).
Prints one JSON line per P; with --out the lines are appended to that file (profiles/eg_model/eg_model_timing.txt).

    python tools/eg_model_timing.py [--users N] [--products 1000,10000] [--reps 2] [--epsilon 0.05] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from recogym_amd import _abi  # noqa: E402
from recogym_amd import evaluate_agent as ev  # noqa: E402
from recogym_amd.agents.logreg_poly import expit_steps  # noqa: E402
from recogym_amd.envs.configuration import Configuration  # noqa: E402
from recogym_amd.envs.reco_env_v1 import env_1_args  # noqa: E402
from recogym_amd.sim import Simulator, poly_device_model  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=100_000)
    ap.add_argument('--products', default='1000,10000')
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--epsilon', type=float, default=0.05)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    n = args.users
    th = expit_steps()
    overlay = dict(epsilon=args.epsilon, seed=7, pure_new=True)
    for P in [int(x) for x in args.products.split(',')]:
        cfg = Configuration({**env_1_args, 'random_seed': 42, 'num_products': P, 'K': 20})
        rng = np.random.RandomState(0)
        dense = rng.standard_normal((P, P)) * 0.1
        vec = rng.standard_normal((3, P)) * 0.1
        model = dict(wf=vec[0], wa=vec[1] / P, wk=dense, intercept=0.1, expit_steps=th)
        common = dict(device='cuda:0', policy=_abi.RG_POLICY_LOGREG_POLY, policy_seed=0, logreg_poly=model, ps_float64=True)
        sims = dict(unwrapped=Simulator(cfg, n, **common), wrapped=Simulator(cfg, n, epsilon_greedy=overlay, **common))

        def step(sim):
            sim.reset_users(0, n)
            sim.run()
        ms = {k: [] for k in sims}
        cnt = {}
        for rep in range(args.reps + 1):                   # rep 0 warms up
            for k, sim in sims.items():
                t, _ = timed(lambda: step(sim))
                cnt[k] = sim.counters()
                if rep:
                    ms[k].append(t)
        res = dict(P=P, users=n, K=20, epsilon=args.epsilon, reps=args.reps)
        for k in sims:
            c = cnt[k]
            res[k] = dict(ms=dict(min=min(ms[k]), max=max(ms[k])), events=c['organic'] + c['bandit'], acts=c['lr_acts'],
                          poly_table=c['poly_table'], poly_unresolved=c['poly_unresolved'], clicks=c['clicks'], steps=c['step'])
        res['overlay_step_loop'] = res['wrapped']['ms']['min'] / res['unwrapped']['ms']['min']
        # the replay, on the unwrapped run's log
        dl = sims['unwrapped'].device_log()
        sims['wrapped'].close()
        device_model = poly_device_model(model, P, dl.rows.device)
        plain = dict(kind=_abi.RG_POLICY_LOGREG_POLY, num_products=P, policy_seed=0, logreg_poly=dict(model, device_model=device_model))
        pols = dict(replay_plain=plain, replay_wrapped=dict(plain, epsilon_greedy=overlay))
        rms = {k: [] for k in pols}
        stats = {k: {} for k in pols}
        for rep in range(args.reps + 1):
            for k, pol in pols.items():
                t, out = timed(lambda: ev.ope_replay(None, dl, pol, stats=stats[k]))
                assert out is not None, 'the host refuted an unresolved act: pick another model seed'
                if rep:
                    rms[k].append(t)
        for k in pols:
            res[k] = dict(ms=dict(min=min(rms[k]), max=max(rms[k])), acts=stats[k]['acts'], unresolved=stats[k]['unresolved'],
                          rows_read=stats[k]['rows_read'])
        res['bandit_rows'] = int(((dl.rows[:, 2] & _abi.RG_EV_BANDIT) != 0).sum().item())
        res['overlay_replay'] = res['replay_wrapped']['ms']['min'] / res['replay_plain']['ms']['min']
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'a') as f:
                f.write(line + '\n')
        sims['unwrapped'].close()
        del sims, dense, dl, device_model, plain, pols
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
