"""Time PyTorchMLRAgent's three device forms against the host routes of the same commit.

  1. generate_logs of `--users` users at P = 10 with a frozen PyTorchMLRAgent on the device route (RG_POLICY_MLR: k_logreg_select +
     k_mlr_acts, the host's confirmation of the listed acts) against the host route — the batched host loop that calls the agent's
     Python act per bandit event, the only route an agent without a device form has (the agent is wrapped so that generate_logs sees
     no device_policy).  Both routes produce the same frame, `ps-a` too (asserted).
  2. The act kernels alone at P = 10 and P = 1000 on a larger population: acts per second from the library's profiling slot of the
     act kernels (HIP events round k_logreg_select + k_mlr_acts of every step).  At P = 10 the table is in LDS, at P = 1000 (8 MB)
     in global memory.
  3. evaluate_IPS of a `--users`-user device log of the uniform logger with `device_replay` (rg_ope_replay_mlr) against the per-row
     host loop, and the replay entry point alone on `--kernel-users` users between two HIP events.  The two routes' IPS terms are
     compared bit for bit.
The weight is a random stand-in (standard normal: several distinct actions, decisions far apart).  One JSON line per measurement;
with --out the lines are appended to that file (profiles/mlr/mlr_timing.txt).

    python tools/mlr_timing.py [--users 2000] [--device-users 100000] [--kernel-users 100000] [--reps 3] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import recogym_amd as recogym  # noqa: E402
from recogym_amd import _abi  # noqa: E402
from recogym_amd import evaluate_agent as ev  # noqa: E402
from recogym_amd.agents import PyTorchMLRFrozenAgent  # noqa: E402
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


def agent_of(P, **cfg):
    W = np.random.RandomState(0).standard_normal((P, P)).astype(np.float32)
    return PyTorchMLRFrozenAgent(Configuration({'num_products': P, 'random_seed': 7, **cfg}), W)


def env_args(P, sigma=0.1):
    return {**env_1_args, 'random_seed': 42, 'num_products': P, 'K': 5, 'sigma_omega': sigma}


def emit(res, out):
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'a') as f:
            f.write(line + '\n')


def act_kernels(P, n, out):
    agent = agent_of(P)
    pol = {k: v for k, v in agent.device_policy().items() if k != 'ps_all'}
    sim = Simulator(Configuration(env_args(P)), n, device='cuda:0', log_capacity=0, **pol)
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
    emit(dict(what='act_kernels', P=P, table_bytes=8 * P * P, device_users=n, device_acts=cnt['lr_acts'],
              history_rows_per_act=cnt['lr_rows'] / cnt['lr_acts'], unresolved=cnt['poly_unresolved'], act_kernels_ms=act_ms, run_s=run_s,
              device_acts_per_s=cnt['lr_acts'] / (act_ms * 1e-3), act_share_of_run=act_ms * 1e-3 / run_s), out)


def frame_key(df):
    return [df[k].to_numpy(dtype=np.float64, na_value=np.nan) for k in ('t', 'u', 'v', 'a', 'c', 'ps')]


def routes(users, out):
    P = 10
    agent = agent_of(P)
    for sigma in (0.0, 0.1):
        env = recogym.make('reco-gym-v1')
        env.init_gym(env_args(P, sigma))
        env.generate_logs(50, agent)                   # warm-up of both routes
        env.generate_logs(50, HostRoute(agent))
        t0 = time.perf_counter()
        dev = env.generate_logs(users, agent)
        t_dev = time.perf_counter() - t0
        t0 = time.perf_counter()
        host = env.generate_logs(users, HostRoute(agent))
        t_host = time.perf_counter() - t0
        assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(frame_key(dev), frame_key(host)))
        is_b = (host['z'] == 'bandit').to_numpy()
        assert all(np.array_equal(g, w) for g, w in zip(dev['ps-a'][is_b], host['ps-a'][is_b]))
        bandit = int(is_b.sum())
        emit(dict(what='generate_logs', P=P, sigma_omega=sigma, users=users, bandit_rows=bandit, distinct_actions=int(host['a'].dropna().nunique()),
                  device_route_s=t_dev, host_route_s=t_host, host_us_per_bandit_row=1e6 * t_host / bandit, ratio_host_over_device=t_host / t_dev), out)


def uniform_log(P, n):
    sim = Simulator(Configuration(env_args(P)), n, device='cuda:0')
    sim.reset_users(0, n)
    sim.run()
    dl = sim.device_log()
    sim.close()
    return dl


def wall_s(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


def entry_ms(ag, dl, reps):
    """The replay entry point alone over every user of `dl` but the last -> (min ms, max ms, head words, users)."""
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


def replay(users, kernel_users, reps, out):
    P = 10
    small, large = uniform_log(P, users), uniform_log(P, kernel_users)
    device, host = agent_of(P, device_replay=True), agent_of(P)
    assert ev.ope_checked_policy_of(host) is None and ev.ope_checked_policy_of(device) is not None
    st = {}
    assert ev.ope_replay(device, small, stats=st) is not None, 'the replay did not stand (an unresolved act the host refuted)'
    dev_s = []
    for rep in range(reps + 1):                        # rep 0 warms up
        t, got = wall_s(lambda: ev.evaluate_IPS(device, small))
        if rep:
            dev_s.append(t)
    host_s, want = wall_s(lambda: ev.evaluate_IPS(host, small))
    assert torch.is_tensor(got) and isinstance(want, list)
    assert got.cpu().numpy().tobytes() == np.asarray(want, dtype=np.float64).tobytes(), 'the two routes disagree'
    lo, hi, head, n_eval = entry_ms(device, large, reps)
    emit(dict(what='replay', P=P, users=users, bandit_rows=len(want), reps=reps, acts=st['acts'], unresolved=st['unresolved'],
              evaluate_IPS_device_s=dict(min=min(dev_s), max=max(dev_s)), evaluate_IPS_host_loop_s=host_s, host_over_device=host_s / min(dev_s),
              host_loop_us_per_bandit_row=1e6 * host_s / max(len(want), 1), entry_users=n_eval, entry_rows=int(large.offsets[n_eval].item()),
              entry_acts=head['acts'], entry_unresolved=head['unresolved'], entry_ms=dict(min=lo, max=hi),
              entry_acts_per_s=head['acts'] / (lo * 1e-3), entry_ns_per_act=1e6 * lo / max(head['acts'], 1)), out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=2000)
    ap.add_argument('--device-users', type=int, default=100_000)
    ap.add_argument('--kernel-users', type=int, default=100_000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    for P in (10, 1000):
        act_kernels(P, args.device_users, args.out)
    routes(args.users, args.out)
    replay(args.users, args.kernel_users, args.reps, args.out)


if __name__ == '__main__':
    main()
