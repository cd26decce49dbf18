"""Shared by the device tests of the replay units, the EpsilonGreedy forms and the agents trained from a device log: the per-user host
route of an agent, frame comparison, the tolerance check of a replay's ratios, the constant likelihood agent and a raw rg_sim handle."""
import ctypes as C

import numpy as np
import torch

import recogym_amd as recogym
from recogym_amd import _abi
from recogym_amd.agents import LogregPolyFrozenAgent
from recogym_amd.envs.configuration import Configuration
from recogym_amd.envs.reco_env_v1 import env_1_args

DEV = 'cuda:0'


class HostOnly:
    """The agent as an arbitrary Python agent: act / train / reset only, so that generate_logs and test_agent take the per-user host path."""
    per_user_path = True

    def __init__(self, agent):
        self.agent = agent
        self.config = agent.config

    def act(self, observation, reward, done):
        return self.agent.act(observation, reward, done)

    def train(self, observation, action, reward, done=False):
        return self.agent.train(observation, action, reward, done)

    def reset(self):
        return self.agent.reset()


def make_env(over):
    env = recogym.make('reco-gym-v1')
    env.init_gym({**env_1_args, **over})
    return env


def frame_key(df):
    return [df[k].to_numpy(dtype=np.float64, na_value=np.nan) for k in ('t', 'u', 'v', 'a', 'c', 'ps')] + [(df['z'] == 'bandit').to_numpy()]


def assert_frames_equal(got, want):
    assert len(got) == len(want)
    for g, w in zip(frame_key(got), frame_key(want)):
        assert np.array_equal(g, w, equal_nan=True)


def close(got, want, rel):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    if rel == 0:
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), np.nonzero(got != want)[0][:8]
    else:
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.all(np.abs(got[ok] - want[ok]) <= rel * np.abs(want[ok])), np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok]))


def constant_agent(z1, z2, P=10, with_ps_all=False):
    """wf = wk = 0: every history decides on z[a] = a wa[a] + 0 — z[1] = z1, z[2] = z2 (2 wa[2]: exact), the rest 0."""
    wa = np.zeros(P)
    wa[1], wa[2] = z1, z2 / 2.0
    assert 2.0 * wa[2] == z2
    return LogregPolyFrozenAgent(Configuration({'num_products': P, 'with_ps_all': with_ps_all}),
                                 np.r_[np.zeros(P), wa, np.zeros(P * P)][None, :], [0.0])


def handle(policy, P=10, **cfg_over):
    """-> (lib, a raw rg_sim handle of 64 users under `policy`, the workspace tensor that keeps it alive)"""
    from recogym_amd.envs.static_params import make_rg_config
    lib = _abi.load()
    sel = cfg_over.pop('lr_select_randomly', False)
    cfg = make_rg_config(Configuration({**env_1_args, 'random_seed': 1, 'num_products': P, 'K': 5, **cfg_over}), 1, policy, 3,
                         lr_select_randomly=sel)
    need = lib.rg_sim_workspace_bytes(C.byref(cfg), 64)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    h = C.c_void_p()
    assert lib.rg_sim_create(C.byref(h), C.byref(cfg), 64, ws.data_ptr(), need) == 0
    return lib, h, ws
