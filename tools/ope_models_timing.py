"""Time the off-policy replay of NnIpsAgent and BayesianAgentVB on the device against the host loop they took before.

For both agents at P = 10 (NN: H = 20; Bayes: S = 1 000 posterior samples), on logs of the uniform logger (K = 5, sigma_omega = 0.1):
  1. evaluate_IPS of a 2 000-user device log on the device route (`device_replay = True`: rg_ope_replay_nn / rg_ope_replay_bayes and
     the host's confirmation of the listed acts) — wall clock of the whole call, the device synchronised, the minimum of `--reps`
     calls after one warm-up;
  2. evaluate_IPS of the same log with `device_replay` unset: the per-row host loop, the only route before the replay units — wall
     clock of one call;
  3. the replay entry point alone on 10^5 users, through ctypes with the model, the outputs and the workspace allocated beforehand,
     between two HIP events: the validation pass, the replay kernel and the reduction, nothing of Python's — the minimum of `--reps`
     calls after one warm-up.  (The kernel by itself: `rocprofv3 --kernel-trace --stats -- python tools/ope_models_timing.py --reps 1`,
     no counters in the same run.)
The two routes' IPS terms are compared bit for bit before a line is written.  Prints one JSON line per agent; with --out the lines
are appended to that file (profiles/ope_models/ope_models_timing.txt).

    python tools/ope_models_timing.py [--users 2000] [--kernel-users 100000] [--reps R] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from recogym_amd import _abi  # noqa: E402
from recogym_amd import evaluate_agent as ev  # noqa: E402
from recogym_amd.agents.bayesian_poly_vb import BayesianVBFrozenAgent  # noqa: E402
from recogym_amd.agents.nn_ips import NnIpsFrozenAgent  # noqa: E402
from recogym_amd.envs.configuration import Configuration  # noqa: E402
from recogym_amd.envs.reco_env_v1 import env_1_args  # noqa: E402
from recogym_amd.sim import Simulator  # noqa: E402

P, H, S = 10, 20, 1000


def uniform_log(n):
    sim = Simulator(Configuration({**env_1_args, 'random_seed': 42, 'num_products': P, 'K': 5, 'sigma_omega': 0.1}), n, device='cuda:0')
    sim.reset_users(0, n)
    sim.run()
    dl = sim.device_log()
    sim.close()
    return dl


def agents(device_replay):
    cfg = Configuration({'num_products': P, 'random_seed': 7, 'with_ps_all': True, **({'device_replay': True} if device_replay else {})})
    rng = np.random.RandomState(0)
    shapes = dict(w1=(H, P), b1=(H,), w2=(H, H), b2=(H,), w3=(P, H), b3=(P,))
    state = {k: rng.standard_normal(s).astype(np.float32) for k, s in shapes.items()}
    return dict(nn=NnIpsFrozenAgent(cfg, state), bayes=BayesianVBFrozenAgent(cfg, rng.standard_normal((S, P * P)) * 0.3))


def wall_s(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def entry_ms(ag, dl, reps):
    """The unit's replay entry point alone over every user of `dl` but the last -> (min ms, max ms, head words)."""
    target = ev._replay_target(ev.ope_checked_policy_of(ag), dl.rows.device)
    n_eval, offsets, max_rows = ev._replay_users(dl, {}, None)
    need = target.size_fn(C.byref(target.structs[0]), n_eval, max_rows)
    ws = torch.empty(need, dtype=torch.uint8, device=dl.rows.device)
    ratio = torch.empty(int(offsets[-1].item()), dtype=torch.float64, device=dl.rows.device)
    sums = torch.empty(3, dtype=torch.float64, device=dl.rows.device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ms = []
    for rep in range(reps + 1):                        # rep 0 warms up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _abi.check(target.replay_fn(C.byref(target.structs[0]), dl.rows.data_ptr(), offsets.data_ptr(), n_eval, max_rows, _abi.RG_OPE_PS_CONST,
                                    None, float(dl.ps), ratio.data_ptr(), None, sums.data_ptr(), ws.data_ptr(), need, stream), target.what)
        b.record()
        torch.cuda.synchronize()
        if rep:
            ms.append(a.elapsed_time(b))
    return min(ms), max(ms), ev._replay_head(ws, target.head), n_eval


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=2000)
    ap.add_argument('--kernel-users', type=int, default=100_000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    small, large = uniform_log(args.users), uniform_log(args.kernel_users)
    assert isinstance(small.ps, float) and isinstance(large.ps, float)
    device, host = agents(True), agents(False)
    for name in ('nn', 'bayes'):
        assert ev.ope_checked_policy_of(host[name]) is None and ev.ope_checked_policy_of(device[name]) is not None
        st = {}
        assert ev.ope_replay(device[name], small, stats=st) is not None, 'the replay did not stand (an unresolved act the host refuted)'
        dev_s = []
        for rep in range(args.reps + 1):               # rep 0 warms up
            t, got = wall_s(lambda: ev.evaluate_IPS(device[name], small))
            if rep:
                dev_s.append(t)
        host_s, want = wall_s(lambda: ev.evaluate_IPS(host[name], small))
        assert torch.is_tensor(got) and isinstance(want, list)
        assert got.cpu().numpy().tobytes() == np.asarray(want, dtype=np.float64).tobytes(), 'the two routes disagree'
        lo, hi, head, n_eval = entry_ms(device[name], large, args.reps)
        res = dict(agent=name, P=P, **(dict(H=H) if name == 'nn' else dict(S=S)), users=args.users, bandit_rows=len(want), reps=args.reps,
                   acts=st['acts'], unresolved=st['unresolved'],
                   evaluate_IPS_device_s=dict(min=min(dev_s), max=max(dev_s)), evaluate_IPS_host_loop_s=host_s,
                   host_over_device=host_s / min(dev_s), host_loop_us_per_bandit_row=1e6 * host_s / max(len(want), 1),
                   entry_users=n_eval, entry_rows=int(large.offsets[n_eval].item()), entry_acts=head['acts'], entry_unresolved=head['unresolved'],
                   entry_ms=dict(min=lo, max=hi), entry_acts_per_s=head['acts'] / (lo * 1e-3), entry_ns_per_act=1e6 * lo / max(head['acts'], 1))
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
