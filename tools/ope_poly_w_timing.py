"""Time the off-policy replay of the time-weighted likelihood agent (rg_ope_replay_poly_w) against the host loop it replaces.

At P = 10 with the weight function exp(-0.2 t) and a dense random model:
  1. evaluate_IPS of a 2 000-user device log (written by the weighted agent itself in the step loop) on the device route — wall time
     of the whole call, synchronised: one warm-up, then the minimum of three calls;
  2. the host loop of the same commit on the same log (evaluate_agent._host_ips on the log's frame), once.
     The two results must be equal bit for bit before any time counts.
  3. the entry point alone between two HIP events on a 10^5-user log (uniform logger, the event index as the clock), buffers
     allocated beforehand: acts per second (the call includes the validation pass and its one synchronisation).
Prints one JSON line; with --out the line is appended to that file (profiles/ope_poly_w/ope_poly_w_timing.txt).

    python tools/ope_poly_w_timing.py [--users 2000] [--entry-users 100000] [--out FILE]"""
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
from recogym_amd.agents.feature_feed import device_clock16  # noqa: E402
from recogym_amd.agents.logreg_poly import LogregPolyFrozenAgent  # noqa: E402
from recogym_amd.envs.configuration import Configuration  # noqa: E402
from recogym_amd.envs.reco_env_v1 import env_1_args  # noqa: E402
from recogym_amd.sim import Simulator  # noqa: E402

P = 10


def weight(t):
    return np.exp(-0.2 * t)


def agent(seed, **cfg):
    rng = np.random.RandomState(seed)
    w = np.r_[rng.normal(0, 0.4, P), rng.normal(0, 0.05, P), rng.normal(0, 0.6, P * P)][None, :]
    return LogregPolyFrozenAgent(Configuration({'num_products': P, 'weight_history_function': weight, 'device_weight_history': True, **cfg}),
                                 w, [float(rng.normal())])


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def entry_alone(ag, n):
    """rg_ope_replay_poly_w on an n-user uniform log between two HIP events -> (ms, acts)."""
    cfg = Configuration({**env_1_args, 'random_seed': 42, 'num_products': P, 'K': 5, 'sigma_omega': 0.1})
    sim = Simulator(cfg, n, device='cuda:0')
    sim.reset_users(0, n)
    sim.run()
    dl = sim.device_log()
    sim.close()
    device = dl.rows.device
    target = ev._replay_target(ag.ope_policy_checked(), device)
    offsets = dl.offsets.contiguous()
    max_rows = int((offsets[1:] - offsets[:-1]).max().item())
    total = int(offsets[-1].item())
    need = target.size_fn(C.byref(target.structs[0]), n, max_rows)
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    ratio = torch.empty(total, dtype=torch.float64, device=device)
    sums = torch.empty(3, dtype=torch.float64, device=device)
    t16 = device_clock16(dl.rows[:, 1].to(torch.float32))
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    def call():
        _abi.check(target.replay_fn(C.byref(target.structs[0]), dl.rows.data_ptr(), offsets.data_ptr(), n, max_rows, t16.data_ptr(),
                                    _abi.RG_OPE_PS_CONST, None, float(dl.ps), ratio.data_ptr(), None, sums.data_ptr(), None, ws.data_ptr(), need,
                                    stream), target.what)
    call()                                              # warm-up
    best = None
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        best = a.elapsed_time(b) if best is None else min(best, a.elapsed_time(b))
    head = ev._replay_head(ws, target.head)
    assert head['error'] == 0 and head['range'] == 0 and head['acts'] == int(sums[0].item()), head
    return best, head, max_rows, need


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=2000)
    ap.add_argument('--entry-users', type=int, default=100_000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    env = recogym.make('reco-gym-v1')
    env.init_gym({**env_1_args, 'random_seed': 42, 'num_products': P, 'K': 5, 'sigma_omega': 0.1})
    cnt, sim = env.simulate(args.users, agent(11))
    dl = sim.device_log()
    frame = ev._device_log_to_frame(dl)
    sim.close()
    ag = agent(12, with_ps_all=True)
    st = {}
    assert ev.ope_replay(ag, dl, stats=st) is not None, 'the device route gave the call up'
    wall_ms(lambda: ev.evaluate_IPS(ag, dl))           # warm-up
    device = [wall_ms(lambda: ev.evaluate_IPS(ag, dl)) for _ in range(3)]
    got = device[0][1].cpu().numpy()
    t0 = time.perf_counter()
    want = np.asarray(ev._host_ips(ag, frame), dtype=np.float64)
    host_ms = 1e3 * (time.perf_counter() - t0)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64)), 'the device route and the host loop differ'
    device_ms = min(ms for ms, _ in device)
    entry_ms, head, max_rows, ws_bytes = entry_alone(ag, args.entry_users)
    res = dict(P=P, weight='exp(-0.2 t)', users=args.users, bandit_rows=int(want.size), acts=st['acts'], unresolved=st['unresolved'],
               list_entries_per_act=st['rows_read'] / max(st['acts'], 1), device_ms=dict(min=device_ms, max=max(ms for ms, _ in device)),
               host_loop_ms=host_ms, host_over_device=host_ms / device_ms,
               entry=dict(users=args.entry_users, acts=head['acts'], max_user_rows=max_rows, workspace_bytes=ws_bytes, ms=entry_ms,
                          acts_per_second=head['acts'] / (1e-3 * entry_ms), unresolved=head['unresolved']))
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
