"""The order in which the three off-policy replay entry points (rg_ope_replay, rg_ope_replay_logreg, rg_ope_replay_eg) add up
d_sums = (n, sum c r, sum r): the documented one (recogym_amd/csrc/rg_ope_common.hpp), emulated in NumPy float64
from the device's own per-row ratios and the log's click bits, must give d_sums bit for bit.  (The other replay tests check that
two runs agree; a reordered reduction would pass them.)

The log is the smallest that takes every branch of that order: 5200 users exceed both wave caps (5120 and 4096: the
`user += W` stride), users of 130 / 64 / 65 / 63 rows straddle the 64-row chunk, one user has a single organic row, one is
empty.  ps is an array of uneven floats, so the order shows in the last bits of the sums."""
import numpy as np
import pytest
import torch

from recogym_amd import _abi
from recogym_amd import evaluate_agent as ev
from recogym_amd.agents import (EpsilonGreedy, LastViewTableAgent, OrganicUserEventCounterAgent, RandomAgent,
                                epsilon_greedy_args)
from recogym_amd.agents.logreg_frozen import LogregFrozenAgent
from recogym_amd.envs.configuration import Configuration
from recogym_amd.sim import DeviceLog

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
P, N_USERS = 8, 5200
CAP = {'rg_ope_replay': 5120, 'rg_ope_replay_logreg': 4096, 'rg_ope_replay_eg': 5120}


def _targets():
    rng = np.random.RandomState(8)
    table = rng.randint(0, P, size=P)
    coef, intercept = rng.standard_normal((P, P)), rng.standard_normal(P)
    def cfg(**kw):
        return Configuration({'num_products': P, 'with_ps_all': True, **kw})
    def logreg(select_randomly):
        return LogregFrozenAgent(cfg(random_seed=7, select_randomly=select_randomly), coef, intercept, np.arange(P, dtype=np.int32))
    return {
        'random': ('rg_ope_replay', RandomAgent(cfg(random_seed=5))),
        'table': ('rg_ope_replay', LastViewTableAgent(cfg(), table)),
        'ouc': ('rg_ope_replay', OrganicUserEventCounterAgent(cfg(random_seed=11, weight_history_function=None, select_randomly=True,
                                                                  exploit_explore=True, epsilon=0.0, reverse_pop=False))),
        'logreg_argmax': ('rg_ope_replay_logreg', logreg(False)),
        'logreg_softmax': ('rg_ope_replay_logreg', logreg(True)),
        'eg_table': ('rg_ope_replay_eg', EpsilonGreedy(cfg(**{**epsilon_greedy_args, 'epsilon': 0.3, 'random_seed': 9, 'num_products': P,
                                                               'with_ps_all': True}), LastViewTableAgent(cfg(), table))),
    }


@pytest.fixture(scope='module')
def log():
    """-> (DeviceLog, offsets, is_bandit, click as float64) of the seeded log; every non-empty user opens with an organic row."""
    rng = np.random.RandomState(2024)
    lens = np.full(N_USERS, 3, dtype=np.int64)
    lens[:6] = [130, 64, 65, 63, 1, 0]
    offsets = np.r_[0, np.cumsum(lens)]
    total = int(offsets[-1])
    user = np.repeat(np.arange(N_USERS), lens)
    t = np.arange(total) - offsets[user]
    is_b = np.where(user < 6, rng.random_sample(total) < 0.6, True) & (t > 0)
    click = is_b & (rng.random_sample(total) < 0.3)
    raw = np.zeros((total, 4), dtype=np.uint32)
    raw[:, 0], raw[:, 1] = user, t
    raw[:, 2] = rng.randint(0, P, size=total).astype(np.uint32) | np.where(is_b, _abi.RG_EV_BANDIT, 0).astype(np.uint32) \
        | np.where(click, _abi.RG_EV_CLICK, 0).astype(np.uint32)
    ps = rng.uniform(0.05, 1.0, size=total)
    raw[:, 3] = ps.astype(np.float32).view(np.uint32)
    dl = DeviceLog(torch.from_numpy(raw.view(np.int32)).to(DEV), torch.from_numpy(offsets).to(DEV), torch.from_numpy(ps).to(DEV), 0, P, None)
    return dl, offsets, is_b, click.astype(np.float64)


def documented_sums(ratio, click, is_b, offsets, cap):
    """(n, sum c r, sum r) in the replay's order: W = clamp(n_users rounded up to 4, 4, cap) waves; wave w walks users w, w + W, ...;
    lane l adds its rows chunk by chunk; xor butterfly; reduce thread i adds slots i, i + 256, ...; the 256-wide tree."""
    n_users = offsets.size - 1
    W = min(max((n_users + 3) // 4 * 4, 4), cap)
    lane = np.arange(64)
    acc = np.zeros((3, W, 64))
    for first in range(0, n_users, W):                          # every wave's next user
        u = np.arange(first, min(first + W, n_users))
        b, e = offsets[u], offsets[u + 1]
        for base in range(0, int((e - b).max()), 64):           # that user's next chunk
            row = b[:, None] + base + lane[None, :]
            on = row < e[:, None]
            row = np.where(on, row, 0)
            on &= is_b[row]
            r, c = ratio[row], click[row]
            a = acc[:, :u.size]
            a[0] = np.where(on, a[0] + 1.0, a[0])
            a[1] = np.where(on, a[1] + c * r, a[1])
            a[2] = np.where(on, a[2] + r, a[2])
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, lane ^ o]
    slots = acc[:, :, 0]                                        # [3][W]
    sh = np.zeros((3, 256))
    for i in range(0, W, 256):
        m = min(256, W - i)
        sh[:, :m] += slots[:, i:i + m]
    s = 128
    while s:
        sh[:, :s] += sh[:, s:2 * s]
        s >>= 1
    return sh[:, 0].copy()


@pytest.mark.parametrize('name', ['random', 'table', 'ouc', 'logreg_argmax', 'logreg_softmax', 'eg_table'])
def test_sums_follow_the_documented_order(log, name):
    dl, offsets, is_b, click = log
    entry, agent = _targets()[name]
    r, c, sums = ev.ope_replay(agent, dl, n_users=N_USERS)
    got = sums.cpu().numpy()
    assert r.numel() == int(is_b.sum()) and np.array_equal(c.cpu().numpy(), click[is_b])
    ratio = np.zeros(is_b.size)
    ratio[is_b] = r.cpu().numpy()
    assert np.isfinite(ratio).all() and (ratio > 0).any()
    want = documented_sums(ratio, click, is_b, offsets, CAP[entry])
    print(name, entry, [x.hex() for x in got], [x.hex() for x in want])
    assert got[0] == float(is_b.sum())
    assert got.tobytes() == want.tobytes(), (name, [x.hex() for x in got], [x.hex() for x in want])
    r2, _, sums2 = ev.ope_replay(agent, dl, n_users=N_USERS)
    assert sums2.cpu().numpy().tobytes() == got.tobytes() and torch.equal(r2, r)
