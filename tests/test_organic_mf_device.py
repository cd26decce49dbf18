"""OrganicMFSquare's device training: rg_omf_pairs against the host enumeration, rg_omf_steps on placed pair lists against the
NumPy restatement (both instantiations), the device route end to end against the reference's fixtures, the trained agent in the
device step loop, inside EpsilonGreedy and under the off-policy estimators, and the logs the entry point refuses."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from device_util import HostOnly, assert_frames_equal, make_env
import organic_mf_util as ou
import recogym_amd as recogym
from recogym_amd import _abi
from recogym_amd import evaluate_agent as ev
from recogym_amd.agents import EpsilonGreedy, OrganicMFSquare, epsilon_greedy_args, organic_mf_square_args
from recogym_amd.agents import count_tables as ct
from recogym_amd.agents.organic_mf import log_pairs
from recogym_amd.envs.configuration import Configuration
from recogym_amd.envs.reco_env_v1 import rows_to_dataframe

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAMES = ou.fixtures()
LR = 0.01


def config(meta, **over):
    return Configuration({**organic_mf_square_args, 'num_products': meta['num_products'], 'embed_dim': meta['embed_dim'],
                          'mini_batch_size': meta['mini_batch_size'], **over})


def device_log(lc, P):
    return ct.columns_to_device_log(lc['u'].astype(np.int64), lc['is_bandit'], lc['v'].astype(np.int64), lc['a'].astype(np.int64),
                                    np.nan_to_num(lc['c']) != 0, P, torch.device(DEV))


def pairs_on_device(dl, P, n_org, first_call, mb, pending):
    """rg_omf_pairs -> (return code, pairs, step_offsets (n_steps + 2), n_calls, the raw output words)."""
    lib = _abi.load()
    n_rows, n_users = int(dl.rows.shape[0]), int(dl.offsets.numel()) - 1
    pend = np.asarray(pending, dtype=np.int32).reshape(-1, 2)
    d_pend = torch.from_numpy(pend).to(DEV)
    pairs = torch.full((len(pend) + n_rows + 1, 2), -7, dtype=torch.int32, device=DEV)
    cap = (first_call % mb + n_rows) // mb + 2
    offs = torch.full((cap,), -7, dtype=torch.int64, device=DEV)
    out = torch.zeros(8, dtype=torch.int64, device=DEV)
    need = lib.rg_omf_pairs_workspace_bytes(n_rows, len(pend))
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=DEV)
    rc = lib.rg_omf_pairs(dl.rows.data_ptr(), dl.offsets.data_ptr(), n_users, n_org, n_rows, P, first_call, mb,
                          d_pend.data_ptr() if len(pend) else None, len(pend), pairs.data_ptr(), len(pend) + n_rows, offs.data_ptr(), cap,
                          out.data_ptr(), ws.data_ptr(), need, None)
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    if rc != 0:
        return rc, pairs.cpu().numpy(), offs.cpu().numpy(), 0, res
    return rc, pairs[:int(res[3])].cpu().numpy(), offs[:int(res[2]) + 2].cpu().numpy(), int(res[1]), res


def steps_on_device(arrays, steps, lr, force_global=0):
    """rg_omf_steps on the six float64 arrays and a list of per-step pair lists -> (the six arrays after, the output words)."""
    lib = _abi.load()
    P, E = arrays[0].shape
    state = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(DEV) for x in arrays]
    flat = np.asarray([p for s in steps for p in s], dtype=np.int32).reshape(-1, 2)
    off = np.cumsum([0] + [len(s) for s in steps]).astype(np.int64)
    d_pairs, d_off = torch.from_numpy(flat).to(DEV), torch.from_numpy(off).to(DEV)
    out = torch.full((4,), -1, dtype=torch.int64, device=DEV)
    need = lib.rg_omf_steps_workspace_bytes(P, E)
    ws = torch.empty(need // 8, dtype=torch.int64, device=DEV)
    model = _abi.RgOmfModel(P, E, *[x.data_ptr() for x in state])
    _abi.check(lib.rg_omf_steps(C.byref(model), lr, ou.ALPHA, ou.EPS, d_pairs.data_ptr() if len(flat) else None, len(flat), d_off.data_ptr(),
                                len(steps), force_global, out.data_ptr(), ws.data_ptr(), need, None), 'rg_omf_steps')
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in state], out.cpu().numpy()


# ---- 1. the pair list --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_pairs_equal_the_host_enumeration(name):
    meta, cols = ou.load(name)
    P, mb, n_org = meta['num_products'], meta['mini_batch_size'], meta['n_organic']
    lc = ou.log_columns(cols)
    dl = device_log(lc, P)
    n_calls = log_pairs(lc['u'], lc['is_bandit'], lc['v'], n_org, 0, mb)[2]
    pend = [(1, 2), (2, 2), (0, 3)]
    for first_call, pending in ((0, []), (mb - 1, pend), ((-n_calls) % mb, pend), (5 * mb + 3, [])):   # a trigger on the first / last call
        want = log_pairs(lc['u'], lc['is_bandit'], lc['v'], n_org, first_call, mb, pending, P)
        got = pairs_on_device(dl, P, n_org, first_call, mb, pending)
        again = pairs_on_device(dl, P, n_org, first_call, mb, pending)
        assert got[0] == 0 and got[4][0] == 0
        assert np.array_equal(got[1], want[0]) and np.array_equal(got[2], want[1]) and got[3] == want[2] == n_calls
        assert got[4][4] == want[1][-1] - want[1][-2]                                   # the pending tail
        assert np.array_equal(got[1], again[1]) and np.array_equal(got[2], again[2]) and np.array_equal(got[4], again[4])
    if meta['n_users2']:        # the second log continues the first: its pending pairs in front, the call count carried on
        p1, o1, c1 = log_pairs(lc['u'], lc['is_bandit'], lc['v'], n_org, 0, mb)
        lc2 = ou.log_columns(cols, 'log2_')
        carried = p1[o1[-2]:o1[-1]]
        assert c1 % mb != 0 and len(carried)
        want = log_pairs(lc2['u'], lc2['is_bandit'], lc2['v'], 0, c1, mb, carried, P)
        got = pairs_on_device(device_log(lc2, P), P, 0, c1, mb, carried)
        assert np.array_equal(got[1], want[0]) and np.array_equal(got[2], want[1]) and got[3] == want[2]


def test_pairs_with_trailing_organic_rows_and_many_blocks():
    """Users that lose their last bandit row (their last views belong to no call), and a log long enough for several scan blocks."""
    meta, cols = ou.load('organic_mf_p10_s01_org')
    lc = ou.log_columns(cols)
    u, is_b = lc['u'], lc['is_bandit']
    last = np.flatnonzero(np.r_[u[1:] != u[:-1], True])
    drop = np.zeros(len(u), dtype=bool)
    drop[last[meta['n_organic']::3]] = True
    cut = {k: x[~drop] for k, x in lc.items()}
    assert len(cut['u']) > 2048 + 64                       # more than one scan block
    want = log_pairs(cut['u'], cut['is_bandit'], cut['v'], meta['n_organic'], 7, 32, [(4, 4)], 10)
    got = pairs_on_device(device_log(cut, 10), 10, meta['n_organic'], 7, 32, [(4, 4)])
    assert got[0] == 0 and np.array_equal(got[1], want[0]) and np.array_equal(got[2], want[1]) and got[3] == want[2]


# ---- 2. the step kernel on placed pair lists -------------------------------------------------------------------------------------------
def placed_steps(P, seed):
    r = np.random.RandomState(seed)
    full = lambda n: [tuple(x) for x in r.randint(0, P, size=(n, 2))]              # noqa: E731
    one = (int(r.randint(P)), int(r.randint(P)))
    i = int(r.randint(P))
    return [full(50), [], full(37), [one] * 200, [(i, int(j)) for j in r.randint(0, P, size=30)], full(3)]


def lds_split(E):
    lds_max, p_max = C.c_uint32(0), C.c_uint32(0)
    assert _abi.load().rg_omf_limits(E, C.byref(lds_max), C.byref(p_max)) == 0
    return lds_max.value


PLACED = [(3, 1, 0), (3, 5, 1), (10, 5, 0), (10, 5, 1), (65, 8, 0), (65, 5, 1), (65, 1, 0), ('split', 5, 0), ('split+1', 5, 0)]


@pytest.mark.parametrize('P,E,force_global', PLACED)
def test_steps_on_placed_pairs_equal_the_numpy_restatement(P, E, force_global):
    natural_global = P == 'split+1'
    P = lds_split(E) + (1 if natural_global else 0) if isinstance(P, str) else P
    r = np.random.RandomState(P * 100 + E)
    emb, w, b = r.standard_normal((P, E)) * 0.5, r.standard_normal((P, E)) * 0.5, r.standard_normal(P) * 0.1
    sq = [np.abs(r.standard_normal(x.shape)) * 1e-3 for x in (emb, w, b)]              # averages that have a past
    steps = placed_steps(P, 5 + E)
    model = ou.NumpyModel(emb, w, b, sq)
    before = [x.copy() for x in model.arrays()]
    for s in steps:
        model.step(s, LR)
    got, out = steps_on_device(before, steps, LR, force_global)
    again, out2 = steps_on_device(before, steps, LR, force_global)
    assert list(out) == [0, 5, 1, sum(len(s) for s in steps)]                            # taken, skipped as empty, pairs consumed
    dev = max(float(np.abs(x - y).max()) for x, y in zip(got, model.arrays()))
    print(f'P={P} E={E} {"global" if force_global or natural_global else "LDS"}: |kernel - NumPy| = {dev:.3e}')
    assert dev <= ou.TOL_KERNEL_VS_NUMPY
    assert ou.MEASURED_KERNEL_VS_NUMPY * 1000 <= ou.TOL_F64_VS_REFERENCE               # the two bounds add up to one on the reference
    for x, y in zip(got, again):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))                      # two runs, the same bits
    assert np.array_equal(out, out2)
    # a row of emb no step saw keeps its value while its average decays; an empty step leaves the averages untouched
    a1, _ = steps_on_device(before, steps[:1], LR, force_global)
    a2, o2 = steps_on_device(before, steps[:2], LR, force_global)
    assert list(o2[:3]) == [0, 1, 1]
    for x, y in zip(a1, a2):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    if not force_global and not natural_global:                                          # the two instantiations: one body, the same bits
        g, _ = steps_on_device(before, steps, LR, 1)
        assert max(float(np.abs(x - y).max()) for x, y in zip(got, g)) <= ou.TOL_KERNEL_VS_NUMPY


def test_steps_refuse_a_bad_list_and_leave_the_model():
    r = np.random.RandomState(3)
    arrays = [r.standard_normal((10, 5)), r.standard_normal((10, 5)), r.standard_normal(10)] + [np.zeros((10, 5)), np.zeros((10, 5)), np.zeros(10)]
    for force_global in (0, 1):
        got, out = steps_on_device(arrays, [[(1, 2), (3, 10)], [(0, 0)]], LR, force_global)        # j = P
        assert out[0] == 2 and list(out[1:]) == [0, 0, 0]
        for x, y in zip(got, arrays):
            assert np.array_equal(x, y)


# ---- 3. end to end -------------------------------------------------------------------------------------------------------------------
class Spy(OrganicMFSquare):
    def train_from_log(self, log, num_organic_users=0):
        Spy.seen.append(type(log).__name__)
        return super().train_from_log(log, num_organic_users)


@pytest.mark.parametrize('name', ['organic_mf_p10_s01_org', 'organic_mf_p40_e8', 'organic_mf_p10_mb4'])
def test_device_route_end_to_end_against_the_reference(name, monkeypatch):
    meta, cols = ou.load(name)
    P = meta['num_products']
    env = make_env(meta['env_args'])
    cnt, sim = env.simulate(meta['n_users'], None, meta['n_organic'])
    lc, want_lc = sim.log_columns(), ou.log_columns(cols)
    for k in ('u', 'is_bandit', 'v', 'a'):
        assert np.array_equal(np.asarray(lc[k]).astype(np.int64), want_lc[k].astype(np.int64)), k           # the fixture's log, from its seed
    agent = OrganicMFSquare(config(meta, device_training=True), cols['emb0'], cols['w0'], cols['b0'])
    assert agent.device_route() and agent.accepts_device_log
    agent.train_from_log(sim.device_log(), meta['n_organic'])
    sim.close()
    assert agent.curr_step == meta['calls']
    assert agent.last_device_stats['steps'] == meta['steps'] - meta['empty_steps'] and agent.last_device_stats['empty_steps'] == meta['empty_steps']
    keys = ('emb', 'w', 'b', 'sq_emb', 'sq_w', 'sq_b')
    state = [x.cpu().numpy() for x in agent._dev['state']]
    dev = max(float(np.abs(x - cols[k]).max()) for x, k in zip(state, keys))
    print(f'{name}: device route vs reference {dev:.3e}')
    assert dev <= ou.TOL_F64_VS_REFERENCE + ou.TOL_KERNEL_VS_NUMPY
    for p, x, sq in zip(agent._params(), state[:3], state[3:]):                          # the float32 roundings, in the modules and the optimiser
        assert np.array_equal(p.detach().numpy(), x.astype(np.float32))
        assert np.array_equal(agent.optimizer.state[p]['square_avg'].numpy(), sq.astype(np.float32))
    assert np.array_equal(agent.frozen().table, cols['table'])                           # the reference's act at every product
    # the host route's agent (the reference's bits) and this one log the same rows: in the device loop, inside EpsilonGreedy
    host = OrganicMFSquare(config(meta), cols['emb0'], cols['w0'], cols['b0'])
    host.train_from_log(want_lc, meta['n_organic'])
    assert agent.device_policy()['policy'] == _abi.RG_POLICY_LAST_VIEW_TABLE
    assert_frames_equal(env.generate_logs(50, agent), env.generate_logs(50, HostOnly(host)))
    eg_cfg = Configuration({**epsilon_greedy_args, 'epsilon': 0.3, 'random_seed': 11, 'num_products': P})
    eg = EpsilonGreedy(eg_cfg, agent)
    assert eg.device_policy()['policy'] == _abi.RG_POLICY_LAST_VIEW_TABLE and eg.device_policy()['epsilon_greedy'] is not None
    assert_frames_equal(env.generate_logs(50, eg), env.generate_logs(50, HostOnly(EpsilonGreedy(eg_cfg, host))))
    if name != 'organic_mf_p10_s01_org':
        return
    # test_agent hands the device log over and gives what the host route gives
    Spy.seen = []
    args = (meta['n_users'], 60)
    got = recogym.test_agent(env, Spy(config(meta, device_training=True), cols['emb0'], cols['w0'], cols['b0']), *args,
                             num_organic_offline_users=meta['n_organic'])
    want = recogym.test_agent(env, Spy(config(meta), cols['emb0'], cols['w0'], cols['b0']), *args, num_organic_offline_users=meta['n_organic'])
    assert Spy.seen == ['DeviceLog', 'dict'] and got == want
    # a second device log continues the first; the host route continues the device route
    two = OrganicMFSquare(config(meta, device_training=True), cols['emb0'], cols['w0'], cols['b0'])
    u = want_lc['u']
    starts = np.flatnonzero(np.r_[True, u[1:] != u[:-1]])
    for cut in starts[len(starts) // 2:]:              # a user boundary inside a mini-batch, with pairs pending across it
        _, o, c = log_pairs(u[:cut], want_lc['is_bandit'][:cut], want_lc['v'][:cut], meta['n_organic'], 0, meta['mini_batch_size'])
        if c % meta['mini_batch_size'] and o[-1] > o[-2]:
            break
    cut = int(cut)
    assert meta['n_organic'] < len(np.unique(u[:cut])) and cut < len(u)
    first, second = ({k: x[:cut] for k, x in want_lc.items()}, {k: x[cut:] for k, x in want_lc.items()})
    two.train_from_log(device_log(first, P), meta['n_organic'])
    assert two.curr_step % two.batch != 0 and two.train_data
    two.train_from_log(device_log(second, P), 0)
    assert two.curr_step == meta['calls']
    for x, y in zip(two._dev['state'], agent._dev['state']):
        assert torch.equal(x, y)                                                          # the same steps on the same pairs: the same bits
    mixed = OrganicMFSquare(config(meta, device_training=True), cols['emb0'], cols['w0'], cols['b0'])
    mixed.train_from_log(device_log(first, P), meta['n_organic'])
    mixed.config.device_training = False
    mixed.train_from_log(second, 0)                                                       # float32 from here on, from the roundings
    assert mixed.curr_step == meta['calls'] and np.array_equal(mixed.frozen().table, cols['table'])
    assert max(float(np.abs(p.detach().numpy() - cols[k]).max()) for p, k in zip(mixed._params(), keys)) <= ou.TOL_F64_VS_REFERENCE + ou.TOL_KERNEL_VS_NUMPY
    mixed.config.device_training = True
    mixed.train_from_log(device_log(second, P), 0)                                        # and back: the state is re-read from the modules
    assert mixed.curr_step == meta['calls'] + len(np.flatnonzero(second['is_bandit']))


def test_evaluate_ips_replays_the_trained_agent_on_the_device(monkeypatch):
    meta, cols = ou.load('organic_mf_p10_s01')
    env = make_env(meta['env_args'])
    agent = OrganicMFSquare(config(meta, with_ps_all=True), cols['emb'], cols['w'], cols['b'])
    assert ev.ope_policy_of(agent)['kind'] == _abi.RG_POLICY_LAST_VIEW_TABLE
    cnt, sim = env.simulate(300, None)
    df = rows_to_dataframe(sim.rows(), meta['num_products'])
    ips_dev = ev.evaluate_IPS(agent, sim.device_log()).cpu().numpy()
    c_dev, r_dev = ev.evaluate_SNIPS(agent, sim.device_log())
    sim.close()
    monkeypatch.setattr(ev, '_device_present', lambda: False)
    ips_host = np.asarray(ev.evaluate_IPS(agent, df), dtype=np.float64)
    assert len(ips_host) > 1000 and np.array_equal(ips_dev, ips_host) and ips_host.max() > 0
    assert np.array_equal(r_dev.cpu().numpy(), np.asarray(ev.evaluate_SNIPS(agent, df)[1], dtype=np.float64))


# ---- 4. what is refused --------------------------------------------------------------------------------------------------------------
def test_bad_logs_are_refused_and_leave_the_model():
    meta, cols = ou.load('organic_mf_p10_s0')
    lc = ou.log_columns(cols)
    agent = OrganicMFSquare(config(meta, device_training=True), cols['emb0'], cols['w0'], cols['b0'])
    agent.train_data = [(1, 2)]
    agent.curr_step = 5
    before = [x.copy() for x in agent._arrays32()]
    bad_v = {k: x.copy() for k, x in lc.items()}
    bad_v['v'][np.flatnonzero(~lc['is_bandit'])[40]] = 10                               # a product = P
    first_b = {k: x.copy() for k, x in lc.items()}
    start = np.flatnonzero(np.r_[True, lc['u'][1:] != lc['u'][:-1]])[3]
    first_b['is_bandit'][start] = True                                                    # a user that opens with a bandit row
    for bad in (bad_v, first_b):
        dl = device_log(bad, 10)
        rc, pairs, offs, _, res = pairs_on_device(dl, 10, 0, 0, 32, [])
        assert rc == -1 and (pairs == -7).all() and (offs == -7).all() and list(res[1:]) == [0] * 7     # RG_EINVAL, nothing written
        with pytest.raises(_abi.RecoGymHipError, match='RG_EINVAL'):
            agent.train_from_log(dl, 0)
        assert agent.curr_step == 5 and agent.train_data == [(1, 2)] and agent._dev is None
        for x, y in zip(agent._arrays32(), before):
            assert np.array_equal(x, y)


def test_a_product_count_beyond_the_cap_trains_on_the_host_after_one_warning():
    P = 2049
    cfg = Configuration({**organic_mf_square_args, 'num_products': P, 'embed_dim': 2, 'mini_batch_size': 2, 'device_training': True})
    agent = OrganicMFSquare(cfg)
    with pytest.warns(RuntimeWarning, match='caps'):
        assert not agent.device_route()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert not agent.accepts_device_log                                               # once
        u = np.array([0, 0, 0, 0, 1, 1, 1])
        is_b = np.array([0, 0, 1, 1, 0, 0, 1], dtype=bool)
        v = np.array([5, 2048, 0, 0, 7, 5, 0])
        w0 = agent.output_layer.weight.detach().numpy().copy()
        agent.train_from_log(dict(u=u.astype(np.int32), is_bandit=is_b, v=v, a=np.zeros(7, dtype=np.int64), c=np.where(is_b, 0.0, np.nan),
                                  ps=np.where(is_b, 1.0 / P, np.nan), t=np.arange(7, dtype=np.float32)), 0)
    assert agent.curr_step == 3 and agent._dev is None and not np.array_equal(agent.output_layer.weight.detach().numpy(), w0)
