"""Time generate_logs with a frozen NnIpsAgent on the device route (RG_POLICY_NN_IPS: k_logreg_select + k_nn_acts) against the
host route of the same commit — the batched host loop that calls the agent's Python act (a torch forward) per bandit event, which
is the only route an agent without a device form has.

Shapes: P = 10, H = 20 (the reference's defaults), sigma_omega = 0 and 0.1 (K = 5).  The net is a random stand-in (standard normal
weights times 2: several distinct actions, decisions far apart).  The host route is wrapped so that generate_logs sees no
device_policy.  Both routes produce the same frame but for ps, which the device computes in float64 (asserted: every other column
equal, ps within 1e-4 relative — the proven per-act bound is the tests' business).  Per configuration one JSON line: users, acts,
wall seconds of both routes, device acts per second from the library's profiling slot of the act kernels (HIP events round
k_logreg_select + k_nn_acts of every step) on a larger population, and the ratio.  Kernel shares: run under
`rocprofv3 --kernel-trace --stats -- python tools/nn_ips_timing.py --device-only` (no counters in the same run).  With --out the
lines are appended to that file (profiles/nn_ips/nn_ips_timing.txt).

    python tools/nn_ips_timing.py [--users N] [--device-users M] [--hidden H] [--out FILE] [--device-only]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import recogym_amd as recogym  # noqa: E402
from recogym_amd.agents import NnIpsFrozenAgent  # noqa: E402
from recogym_amd.envs.configuration import Configuration  # noqa: E402
from recogym_amd.envs.reco_env_v1 import env_1_args  # noqa: E402
from recogym_amd.sim import Simulator  # noqa: E402


class HostRoute:
    """The agent without its device form: act / reset only."""

    def __init__(self, agent):
        self.agent = agent
        self.config = agent.config

    def act(self, observation, reward, done):
        return self.agent.act(observation, reward, done)

    def reset(self):
        return self.agent.reset()


def frame_key(df):
    return [df[k].to_numpy(dtype=np.float64, na_value=np.nan) for k in ('t', 'u', 'v', 'a', 'c')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=2000)
    ap.add_argument('--device-users', type=int, default=100_000)
    ap.add_argument('--hidden', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--device-only', action='store_true')
    args = ap.parse_args()
    P, H = 10, args.hidden
    rng = np.random.RandomState(0)
    shapes = dict(w1=(H, P), b1=(H,), w2=(H, H), b2=(H,), w3=(P, H), b3=(P,))
    agent = NnIpsFrozenAgent(Configuration({'num_products': P}), {k: (rng.standard_normal(s) * 2.0).astype(np.float32) for k, s in shapes.items()})
    for sigma in (0.0, 0.1):
        over = {**env_1_args, 'random_seed': 42, 'num_products': P, 'K': 5, 'sigma_omega': sigma}
        res = dict(P=P, H=H, sigma_omega=sigma, model_bytes=(2 * P * H + H * H + 2 * H + P) * 8)
        # the act kernels alone, on a larger population
        n = args.device_users
        sim = Simulator(Configuration(over), n, device='cuda:0', log_capacity=0, **agent.device_policy())
        ms = []
        for rep in range(3):                               # rep 0 warms up
            sim.reset_users(0, n)
            sim.set_profiling(True)
            before = sim.profile()['logreg_ms']
            t0 = time.perf_counter()
            sim.run()
            cnt = sim.counters()
            wall = time.perf_counter() - t0
            if rep:
                ms.append((sim.profile()['logreg_ms'] - before, wall))
            sim.set_profiling(False)
        sim.close()
        act_ms, run_s = min(ms)
        res.update(device_users=n, device_acts=cnt['lr_acts'], history_rows_per_act=cnt['lr_rows'] / cnt['lr_acts'],
                   unresolved=cnt['poly_unresolved'], act_kernels_ms=act_ms, run_s=run_s,
                   device_acts_per_s=cnt['lr_acts'] / (act_ms * 1e-3), act_share_of_run=act_ms * 1e-3 / run_s)
        if not args.device_only:
            env = recogym.make('reco-gym-v1')
            env.init_gym(over)
            env.generate_logs(50, agent)                   # warm-up of both routes
            env.generate_logs(50, HostRoute(agent))
            t0 = time.perf_counter()
            dev = env.generate_logs(args.users, agent)
            t_dev = time.perf_counter() - t0
            t0 = time.perf_counter()
            host = env.generate_logs(args.users, HostRoute(agent))
            t_host = time.perf_counter() - t0
            assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(frame_key(dev), frame_key(host)))
            ps_d, ps_h = (f['ps'].to_numpy(dtype=np.float64, na_value=np.nan) for f in (dev, host))
            assert np.allclose(ps_d, ps_h, rtol=1e-4, atol=0, equal_nan=True)
            bandit = int((host['z'] == 'bandit').sum())
            res.update(users=args.users, bandit_rows=bandit, distinct_actions=int(host['a'].dropna().nunique()), device_route_s=t_dev,
                       host_route_s=t_host, host_us_per_bandit_row=1e6 * t_host / bandit, ratio_host_over_device=t_host / t_dev)
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
