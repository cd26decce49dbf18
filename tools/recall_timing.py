"""evaluate_recall_at_k on a Simulator log of 20 000 users at P = 1000, k = 5: the device route (a last-view table, the frozen
LogReg argmax, the sampling LogReg's ranking form) against the host loop of the same commit.

    python tools/recall_timing.py [OUT]          (default profiles/recall/recall_timing.txt; needs an MI355X)"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
from recogym_amd import _abi  # noqa: E402
from recogym_amd import evaluate_agent as ev  # noqa: E402
from recogym_amd.agents import LastViewTableAgent  # noqa: E402
from recogym_amd.envs.configuration import Configuration  # noqa: E402
from recogym_amd.envs.reco_env_v1 import env_1_args  # noqa: E402
from recogym_amd.sim import Simulator  # noqa: E402
from test_ope_logreg_host import frozen  # noqa: E402

OUT = open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'recall', 'recall_timing.txt'), 'w')


def say(*a):
    line = ' '.join(str(x) for x in a)
    print(line, flush=True)
    OUT.write(line + '\n')
    OUT.flush()


N, P, K, WARM, REPS = 20000, 1000, 5, 3, 9
cfg = Configuration({**env_1_args, 'random_seed': 7, 'num_products': P, 'K': 5})
sim = Simulator(cfg, N, device='cuda:0')
sim.reset_users(0, N)
sim.run()
dl = sim.device_log()
total = int(dl.offsets[N - 1].item())
say(f'evaluate_recall_at_k, Simulator log: {N} users, P = {P}, k = {K}; rows of the {N - 1} evaluated users: {total}')
say(f'device: {torch.cuda.get_device_name(0)}; {WARM} warm-up calls, then {REPS} timed; wall = time.perf_counter round the call with a')
say('device synchronise on either side; kernel = device events round the one recall entry point (the ranking form\'s includes its log '
    'validation); every repetition listed, the minimum taken')

lib = _abi.load()
real_sets, real_hits, real_rank = ev.recall_sets, lib.rg_ope_recall_hits, lib.rg_ope_recall_logreg
clock = {}


def timed_sets(*a):
    t0 = time.perf_counter()
    out = real_sets(*a)
    clock['sets'] = time.perf_counter() - t0
    clock['keys'] = len(a[1])
    return out


class Evented:
    def __init__(self, fn, name):
        self.fn, self.name = fn, name

    def __call__(self, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = self.fn(*a)
        e1.record()
        e1.synchronize()
        clock[self.name] = e0.elapsed_time(e1) * 1e-3
        return rc


class Lib:
    def __getattr__(self, name):
        if name == 'rg_ope_recall_hits':
            return Evented(real_hits, 'kernel')
        if name == 'rg_ope_recall_logreg':
            return Evented(real_rank, 'kernel')
        return getattr(lib, name)


ev.recall_sets = timed_sets
ev._abi.load = lambda: Lib()


def fmt(xs):
    return '[' + ', '.join(f'{1e3 * x:.3f}' for x in xs) + '] ms'


def device_route(name, agent):
    walls, sets, kernels = [], [], []
    for i in range(WARM + REPS):
        clock.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = ev.evaluate_recall_at_k(agent, dl, k=K)
        torch.cuda.synchronize()
        w = time.perf_counter() - t0
        assert isinstance(got, torch.Tensor), 'the device route was left out'
        if i >= WARM:
            walls.append(w)
            sets.append(clock.get('sets', 0.0))
            kernels.append(clock['kernel'])
    say(f'{name}: device route, counted rows {got.numel()}, hits {int(got.sum().item())}')
    say(f'  wall per call      {fmt(walls)}  min {1e3 * min(walls):.3f} ms')
    say(f'  recall kernel      {fmt(kernels)}  min {1e3 * min(kernels):.3f} ms (device events)')
    if 'keys' in clock:
        say(f'  sets table (host)  {fmt(sets)}  min {1e3 * min(sets):.3f} ms; distinct keys {clock["keys"]};'
            f' share of the wall time (minimum over minimum) {100 * min(sets) / min(walls):.1f} %')
    return got, min(walls)


def host_route(name, agent, got, dev_wall):
    t0 = time.perf_counter()
    want = ev._host_recall(agent, dl, K)
    w = time.perf_counter() - t0
    same = got.cpu().numpy().tolist() == want
    say(f'{name}: host loop (device log -> DataFrame -> one act per bandit row), ONE run: {w:.2f} s; equal hits: {same};'
        f' device route faster by {w / dev_wall:.0f}x')


table = LastViewTableAgent(Configuration({'num_products': P, 'with_ps_all': True}), np.random.RandomState(3).randint(0, P, size=P))
argmax = frozen(P, with_ps_all=True)
sampling = frozen(P, with_ps_all=True, select_randomly=True)
res = {}
for name, agent in (('last-view table', table), ('frozen LogReg argmax', argmax)):
    res[name] = device_route(name, agent)
stats = {}
out = ev.recall_replay(sampling, dl, K, stats=stats)
say(f'sampling LogReg (ranking form): head {stats}')
res['sampling LogReg'] = device_route('sampling LogReg (ranking form)', sampling)
for name, agent in (('last-view table', table), ('frozen LogReg argmax', argmax)):
    host_route(name, agent, *res[name])
say('(the ranking form\'s host loop at this shape was not timed: one softmax over 1000 classes per act on top of the argmax model\'s loop)')
OUT.close()
