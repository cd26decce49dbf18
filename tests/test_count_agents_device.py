"""OrganicCount / BanditCount trained on the device (rg_count_train + rg_count_policy): against the reference's fixtures, against
the vectorised host form on simulator logs, the overflow paths, test_agent end to end, and the error paths.  Exact throughout."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from device_util import HostOnly
import golden_util as gu
import recogym_amd as recogym
from make_golden_counts import LOGS
from recogym_amd import _abi
from recogym_amd import evaluate_agent as ev
from recogym_amd.agents import BanditCount, OrganicCount, bandit_count_args, organic_count_args
from recogym_amd.agents import count_tables as ct
from recogym_amd.envs.configuration import Configuration
from recogym_amd.envs.reco_env_v1 import env_1_args, rows_to_dataframe
from recogym_amd.sim import Simulator

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def agents(P, with_ps_all=False):
    return (OrganicCount(Configuration({**organic_count_args, 'num_products': P, 'with_ps_all': with_ps_all})),
            BanditCount(Configuration({**bandit_count_args, 'num_products': P, 'with_ps_all': with_ps_all})))


def fixture_device_log(cols, P):
    is_b = cols['z'] == 1
    return ct.columns_to_device_log(cols['u'].astype(np.int64), is_b, np.where(is_b, 0, cols['v']).astype(np.int64),
                                    np.where(is_b, cols['a'], 0).astype(np.int64), is_b & (cols['c'] == 1), P, torch.device(DEV))


def dense(coo, P):
    out = np.zeros((P, P), dtype=np.int64)
    out[coo[0], coo[1]] = coo[2]
    return out


@pytest.mark.parametrize('name', LOGS)
def test_device_equals_reference_fixture(name):
    meta, cols = gu.load(name)
    P = meta['env_args']['num_products']
    z = np.load(os.path.join(gu.GOLDEN, f'counts_{name}.npz'))
    want_meta = json.loads(str(z['meta']))
    oc, bc = agents(P)
    dl = fixture_device_log(cols, P)
    oc.train_from_log(dl)
    bc.train_from_log(dl)
    assert oc._co.dev is not None and bc._pulls.dev is not None          # trained where the log is
    assert np.array_equal(oc._co.dev.cpu().numpy(), dense(z['co'], P))
    assert np.array_equal(bc._pulls.dev.cpu().numpy(), dense(z['pulls'], P))
    assert np.array_equal(bc._clicks.dev.cpu().numpy(), dense(z['clicks'], P))
    assert np.array_equal(oc.co_counts, dense(z['co'], P).astype(np.float64))
    assert np.array_equal(oc.frozen().table, z['organic_argmax'])
    assert np.array_equal(bc.frozen().table, z['bandit_argmax'])
    assert np.array_equal(bc.frozen().ps.view(np.uint64), z['bandit_ps'].view(np.uint64))
    assert bc.last_product_viewed == want_meta['last_product_viewed']


def test_two_device_logs_and_mixed_host_calls_continue_each_other():
    """The carry between two rg_count_train calls, and train calls on the host followed by a device log."""
    name = 'philox_p10'
    meta, cols = gu.load(name)
    z = np.load(os.path.join(gu.GOLDEN, f'counts_{name}.npz'))
    P = 10
    u = cols['u']
    k = int(np.searchsorted(u, u[int(len(u) * 0.4)], side='left'))
    first = {c: v[:k] for c, v in cols.items() if len(v) == len(u)}
    second = {c: v[k:] for c, v in cols.items() if len(v) == len(u)}
    oc, bc = agents(P)
    for part in (first, second):
        dl = fixture_device_log(part, P)
        oc.train_from_log(dl)
        bc.train_from_log(dl)
    assert np.array_equal(oc._co.dev.cpu().numpy(), dense(z['co'], P))
    assert np.array_equal(bc._pulls.dev.cpu().numpy(), dense(z['pulls'], P))
    assert np.array_equal(bc._clicks.dev.cpu().numpy(), dense(z['clicks'], P))
    # host train_from_log on the first part (the None row lands in the host table), the device on the second
    from make_golden_ope import log_frame
    oc, bc = agents(P)
    oc.train_from_log(log_frame(first))
    bc.train_from_log(log_frame(first))
    oc.train_from_log(fixture_device_log(second, P))
    bc.train_from_log(fixture_device_log(second, P))
    assert np.array_equal(oc.co_counts, dense(z['co'], P).astype(np.float64))
    assert np.array_equal(bc.pulls_a, dense(z['pulls'], P).astype(np.float64))
    assert np.array_equal(bc.clicks_a, dense(z['clicks'], P).astype(np.float64))
    assert np.array_equal(bc.frozen().table, z['bandit_argmax'])
    assert np.array_equal(bc.frozen().ps.view(np.uint64), z['bandit_ps'].view(np.uint64))


def _nonzero(t):
    flat = t.flatten()
    idx = flat.nonzero().flatten()
    return idx.cpu().numpy(), flat[idx].cpu().numpy()


def _host_cells(table):
    r, c, v = table.coo()
    return r * table.P + c, v


def _train_both_ways(sim, P):
    dl = sim.device_log()
    cols = sim.log_columns()
    oc_d, bc_d = agents(P)
    oc_d.train_from_log(dl)
    bc_d.train_from_log(dl)
    oc_h, bc_h = agents(P)
    oc_h.train_from_log(cols)
    bc_h.train_from_log(cols)
    for dev_t, host_t, what in ((oc_d._co, oc_h._co, 'co_counts'), (bc_d._pulls, bc_h._pulls, 'pulls'),
                                (bc_d._clicks, bc_h._clicks, 'clicks')):
        gk, gv = _nonzero(dev_t.dev)
        wk, wv = _host_cells(host_t)
        assert np.array_equal(gk, wk) and np.array_equal(gv, wv), what
    assert bc_d.last_product_viewed == bc_h.last_product_viewed
    assert np.array_equal(oc_d.frozen().table, oc_h.frozen().table)
    assert np.array_equal(bc_d.frozen().table, bc_h.frozen().table)
    assert np.array_equal(bc_d.frozen().ps.view(np.uint64), bc_h.frozen().ps.view(np.uint64))
    # a second device run: identical bytes
    oc_2, bc_2 = agents(P)
    oc_2.train_from_log(dl)
    bc_2.train_from_log(dl)
    assert torch.equal(oc_2._co.dev, oc_d._co.dev) and torch.equal(bc_2._pulls.dev, bc_d._pulls.dev)
    assert torch.equal(bc_2._clicks.dev, bc_d._clicks.dev)
    return dl


@pytest.mark.parametrize('P', [10, 1000, 10000])
def test_device_equals_host_form_on_simulator_logs(P):
    """~2 10^5 users, sigma_omega = 0: hot cells under heavy contention, users of many chunks."""
    n = 200000
    cfg = Configuration({**env_1_args, 'random_seed': 11, 'num_products': P, 'K': 5, 'sigma_omega': 0.0})
    sim = Simulator(cfg, n, device=DEV)
    sim.reset_users(0, n)
    sim.run()
    dl = _train_both_ways(sim, P)
    lens = (dl.offsets[1:] - dl.offsets[:-1])
    assert int(lens.max().item()) > 64 * 4          # long users occurred
    sim.close()


def test_device_equals_host_form_with_organic_only_users():
    P, n, n_org = 1000, 20000, 5000
    cfg = Configuration({**env_1_args, 'random_seed': 5, 'num_products': P, 'K': 5, 'sigma_omega': 0.0})
    sim = Simulator(cfg, n, device=DEV)
    sim.reset_users(0, n, organic_only_below=n_org)
    sim.run()
    dl = _train_both_ways(sim, P)
    code = dl.rows[:int(dl.offsets[n_org].item()), 2]
    assert not bool(((code & _abi.RG_EV_BANDIT) != 0).any())          # the first users are organic-only
    sim.close()


def test_overflow_paths():
    """One synthetic user whose single session has 1 500 views of 700 distinct products: more than the 64-entry session list
    (the pairwise form) and, with 490 000 cells, far more than the block's LDS table holds (straight to global memory); beside it
    a session of 64 distinct products exactly (the list's last slot) and one of 65."""
    P = 1000
    rng = np.random.RandomState(1)
    u, is_b, idx = [], [], []

    def user(uid, sessions):
        for views in sessions:
            u.extend([uid] * (len(views) + 2))
            is_b.extend([False] * len(views) + [True, True])
            idx.extend(list(views) + [int(rng.randint(P)), int(rng.randint(P))])
    user(0, [rng.randint(0, P, size=5)])
    user(1, [np.r_[rng.permutation(P)[:700], rng.permutation(P)[:700], rng.permutation(P)[:100]], rng.randint(0, P, size=3)])
    user(2, [rng.permutation(P)[:64], np.r_[rng.permutation(P)[:65], rng.permutation(P)[:65]]])
    user(3, [rng.randint(0, P, size=130)])
    u, is_b, idx = np.asarray(u, dtype=np.int64), np.asarray(is_b), np.asarray(idx, dtype=np.int64)
    click = is_b & (rng.rand(len(u)) < 0.4)
    v, a = np.where(is_b, 0, idx), np.where(is_b, idx, 0)
    dl = ct.columns_to_device_log(u, is_b, v, a, click, P, torch.device(DEV))
    oc_d, bc_d = agents(P)
    oc_d.train_from_log(dl)
    bc_d.train_from_log(dl)
    oc_h, bc_h = agents(P)
    oc_h._co.add(*ct.organic_updates(u, is_b, v, P))
    log = dict(t=np.zeros(len(u), dtype=np.float32), u=u.astype(np.int32), is_bandit=is_b, v=v.astype(np.int32), a=a.astype(np.int32),
               c=np.where(is_b, click, np.nan).astype(np.float32), ps=np.where(is_b, 1.0 / P, np.nan))
    bc_h.train_from_log(log)
    assert np.array_equal(oc_d.co_counts, oc_h.co_counts)
    assert oc_d.co_counts.sum() == 5 ** 2 + 1500 ** 2 + 3 ** 2 + 64 ** 2 + 130 ** 2 + 130 ** 2
    assert np.array_equal(bc_d.pulls_a, bc_h.pulls_a) and np.array_equal(bc_d.clicks_a, bc_h.clicks_a)


@pytest.mark.parametrize('which', [0, 1])
def test_test_agent_device_training_equals_the_per_user_host_path(which):
    env = recogym.make('reco-gym-v1')
    env.init_gym({**recogym.env_1_args, 'random_seed': 42, 'num_products': 10})
    agent = agents(10)[which]
    got = recogym.test_agent(env, agent, 150, 100)
    want = recogym.test_agent(env, HostOnly(agents(10)[which]), 150, 100)
    assert got == want
    got = recogym.test_agent(env, agents(10)[which], 80, 60, num_organic_offline_users=20)
    want = recogym.test_agent(env, HostOnly(agents(10)[which]), 80, 60, num_organic_offline_users=20)
    assert got == want


def test_log_under_trained_bandit_count_carries_the_float64_ps():
    env = recogym.make('reco-gym-v1')
    env.init_gym({**recogym.env_1_args, 'random_seed': 42, 'num_products': 10})
    _, bc = agents(10)
    cnt, sim = env.simulate(400, None)
    bc.train_from_log(sim.device_log())
    sim.close()
    fz = bc.frozen()
    ctr = bc.ctr
    assert np.array_equal(fz.ps, ctr[np.arange(10), ctr.argmax(axis=1)])
    assert (fz.ps.astype(np.float32).astype(np.float64) != fz.ps).any()          # not float32 numbers
    df = env.generate_logs(300, bc)
    b = df[df['z'] == 'bandit']
    # every logged ps is the float64 CTR of (last view, action), bit for bit
    lpv = df['v'].astype('Float64').ffill().to_numpy(dtype=np.float64)[(df['z'] == 'bandit').to_numpy()].astype(np.int64)
    act = b['a'].to_numpy(dtype=np.int64)
    assert np.array_equal(act, fz.table[lpv])
    assert np.array_equal(b['ps'].to_numpy(dtype=np.float64).view(np.uint64), fz.ps[lpv].view(np.uint64))
    # and the per-user path with the Python act logs the same rows
    want = env.generate_logs(40, HostOnly(bc))
    got = df[df['u'] < 40]
    assert np.array_equal(got['a'].to_numpy(dtype=np.float64, na_value=-1), want['a'].to_numpy(dtype=np.float64, na_value=-1))
    assert np.array_equal(got['ps'].to_numpy(dtype=np.float64), want['ps'].to_numpy(dtype=np.float64), equal_nan=True)


def test_snips_of_trained_organic_count_on_a_device_log_equals_the_host_loop():
    P = 10
    cfg = Configuration({**env_1_args, 'random_seed': 9, 'num_products': P, 'K': 5})
    sim = Simulator(cfg, 600, device=DEV)
    sim.reset_users(0, 600)
    sim.run()
    dl = sim.device_log()
    oc, _ = agents(P, with_ps_all=True)
    oc.train_from_log(dl)
    assert ev.ope_policy_of(oc) is not None
    c_dev, r_dev = ev.evaluate_SNIPS(oc, dl)
    df = rows_to_dataframe(sim.rows(), P)
    c_host, r_host = ev._host_snips(oc, df)
    assert np.array_equal(r_dev.cpu().numpy(), np.asarray(r_host, dtype=np.float64))
    assert np.array_equal(c_dev.cpu().numpy(), np.asarray(c_host, dtype=np.float64))
    sim.close()


def test_error_paths():
    lib = _abi.load()
    # a table that does not fit
    oc, _ = agents(100000)
    dl = ct.columns_to_device_log(np.zeros(2, dtype=np.int64), np.array([False, True]), np.array([1, 0]), np.array([0, 2]),
                                  np.array([False, False]), 100000, torch.device(DEV))
    with pytest.raises(MemoryError, match='GiB'):
        oc.train_from_log(dl)
    # a user whose first row is a bandit row: refused before any table is touched
    P = 10
    u = np.array([0, 0, 1, 1], dtype=np.int64)
    is_b = np.array([False, True, True, True])
    dl = ct.columns_to_device_log(u, is_b, np.array([3, 0, 0, 0]), np.array([0, 1, 2, 3]), np.zeros(4, dtype=bool), P, torch.device(DEV))
    oc, bc = agents(P)
    with pytest.raises(_abi.RecoGymHipError, match='bandit row'):
        oc.train_from_log(dl)
    with pytest.raises(_abi.RecoGymHipError, match='bandit row'):
        bc.train_from_log(dl)
    assert not oc._co.dev.any() and not bc._pulls.dev.any()
    # the log's product count and the agent's differ
    with pytest.raises(ValueError):
        agents(11)[0].train_from_log(dl)
    # P out of range, a workspace too small
    tabs = _abi.RgCountTables(num_products=0x20000000, reserved=0, co_counts=oc._co.dev.data_ptr(), pulls=None, clicks=None)
    carry = torch.zeros(4, dtype=torch.int64, device=DEV)
    ws = torch.zeros(lib.rg_count_workspace_bytes(), dtype=torch.uint8, device=DEV)
    rc = lib.rg_count_train(C.byref(tabs), dl.rows.data_ptr(), dl.offsets.data_ptr(), 2, carry.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert rc == -1 and b'num_products' in lib.rg_last_error()
    tabs.num_products = P
    rc = lib.rg_count_train(C.byref(tabs), dl.rows.data_ptr(), dl.offsets.data_ptr(), 2, carry.data_ptr(), ws.data_ptr(), 8, None)
    assert rc == -3 and b'workspace' in lib.rg_last_error()
