"""Time the off-policy replay of the likelihood agent against the step loop's act kernels under the same model.

At P = 1 000 and P = 10 000 (uniform logger, K = 20, sigma_omega = 0.1, 10^5 users by default) with a dense random model (wf, wa, wk):
  1. rg_ope_replay_poly on the uniform log (the model stays on the device between calls: `device_model`);
  2. rg_ope_replay of RandomAgent on the same log in the same process — the cost of streaming the rows once, the floor;
  3. a simulation of the same population UNDER that model: the step loop's k_logreg_select + k_poly_acts, their profiling slot over
     RG_CNT_LR_ACTS — the yardstick (profiles/poly/poly_timing.txt): the same bytes per act and the same act function.
Reported: us per act of the replay (event time of the WHOLE ope_replay call — workspace allocation, the validation's and the head
words' read-backs and the compaction of the ratio tensor count — and with the floor, which pays the same, taken off) and of the step
loop (a kernel-only profiling slot), and their ratio: an upper bound of the kernels' ratio, which the kernel trace gives.  One warm-up of each, then `--reps` alternating repetitions; the minimum counts, min and max are reported.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/ope_poly_timing.py --reps 1` (no counters in the same run).
Prints one JSON line per P; with --out the lines are appended to that file (profiles/ope_poly/ope_poly_timing.txt).

    python tools/ope_poly_timing.py [--users N] [--products 1000,10000] [--reps R] [--out FILE]"""
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
from recogym_amd.agents import RandomAgent  # noqa: E402
from recogym_amd.agents.logreg_poly import LogregPolyFrozenAgent, expit_steps  # noqa: E402
from recogym_amd.envs.configuration import Configuration  # noqa: E402
from recogym_amd.envs.reco_env_v1 import env_1_args  # noqa: E402
from recogym_amd.sim import Simulator, poly_device_model  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def step_loop(sim, n):
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
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    n = args.users
    th = expit_steps()
    for P in [int(x) for x in args.products.split(',')]:
        cfg = Configuration({**env_1_args, 'random_seed': 42, 'num_products': P, 'K': 20, 'sigma_omega': 0.1})
        rng = np.random.RandomState(0)
        dense = rng.standard_normal((P, P)) * 0.1
        vec = rng.standard_normal((2, P)) * 0.1
        model = dict(wf=vec[0], wa=vec[1] / P, wk=dense, intercept=0.1, expit_steps=th)
        ag = LogregPolyFrozenAgent(Configuration({'num_products': P, 'with_ps_all': True}),
                                   np.r_[model['wf'], model['wa'], dense.reshape(-1)][None, :], [0.1])
        rnd = RandomAgent(Configuration({'num_products': P, 'random_seed': 5, 'with_ps_all': True}))
        log_sim = Simulator(cfg, n, device='cuda:0')
        log_sim.reset_users(0, n)
        log_sim.run()
        dl = log_sim.device_log()
        log_sim.close()
        rows = int(dl.rows.shape[0])
        bandit = int(((dl.rows[:, 2] & _abi.RG_EV_BANDIT) != 0).sum().item())
        pol = ev.ope_checked_policy_of(ag)
        pol['logreg_poly'] = dict(model, device_model=poly_device_model(model, P, dl.rows.device))
        act_sim = Simulator(cfg, n, device='cuda:0', log_capacity=0, policy=_abi.RG_POLICY_LOGREG_POLY, policy_seed=0, logreg_poly=model)
        ms = dict(replay=[], floor=[], step_loop=[])
        st, out, cnt = {}, None, None
        for rep in range(args.reps + 1):                   # rep 0 warms up
            t_replay, out = event_ms(lambda: ev.ope_replay(ag, dl, pol, stats=st))
            t_floor, _ = event_ms(lambda: ev.ope_replay(rnd, dl))
            t_step, cnt = step_loop(act_sim, n)
            if rep:
                ms['replay'].append(t_replay); ms['floor'].append(t_floor); ms['step_loop'].append(t_step)
        assert out is not None, 'the replay did not stand (an unresolved act the host refuted)'
        res = dict(P=P, users=n, rows=rows, bandit_rows=bandit, max_user_rows=int((dl.offsets[1:] - dl.offsets[:-1]).max().item()),
                   reps=args.reps, replay_acts=st['acts'], replay_rows_read=st['rows_read'], replay_table=st['table'],
                   replay_lower=st['lower'], replay_unresolved=st['unresolved'], history_rows_per_act=st['rows_read'] / max(st['acts'], 1),
                   step_loop_acts=cnt['lr_acts'], step_loop_rows_read=cnt['lr_rows'], step_loop_table=cnt['poly_table'],
                   step_loop_unresolved=cnt['poly_unresolved'],
                   replay_sha256=dict(ratio=hashlib.sha256(out[0].cpu().numpy().tobytes()).hexdigest(),
                                      sums=hashlib.sha256(out[2].cpu().numpy().tobytes()).hexdigest()))
        for k, v in ms.items():
            res[f'{k}_ms'] = dict(min=min(v), max=max(v))
        res['replay_us_per_act'] = 1e3 * min(ms['replay']) / max(st['acts'], 1)
        res['replay_less_floor_us_per_act'] = 1e3 * (min(ms['replay']) - min(ms['floor'])) / max(st['acts'], 1)
        res['step_loop_us_per_act'] = 1e3 * min(ms['step_loop']) / max(cnt['lr_acts'], 1)
        res['replay_over_step_loop'] = res['replay_us_per_act'] / res['step_loop_us_per_act'] if res['step_loop_us_per_act'] else None
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'a') as f:
                f.write(line + '\n')
        act_sim.close()
        del act_sim, dl, pol, out, dense, model, ag
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
