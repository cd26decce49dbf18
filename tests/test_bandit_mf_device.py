"""BanditMFSquare's device training: rg_bmf_samples against log_triples, rg_bmf_steps on placed triple lists against the NumPy
restatement (both instantiations), the device route end to end against the reference's fixtures, the trained agent in the device
step loop and inside EpsilonGreedy, and what the entry points refuse."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from device_util import HostOnly, frame_key, make_env
import bandit_mf_util as bu
import recogym_amd as recogym
from recogym_amd import _abi
from recogym_amd.agents import BanditMFSquareAgent, EpsilonGreedy, bandit_mf_square_args, epsilon_greedy_args
from recogym_amd.agents import count_tables as ct
from recogym_amd.agents.bandit_mf import log_triples
from recogym_amd.envs.configuration import Configuration

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAMES = bu.fixtures()
LR = 0.01
PEND = [(1, 2, 0), (2, 2, 1), (0, 3, 0)]


def config(meta, **over):
    return Configuration({**bandit_mf_square_args, 'num_products': meta['num_products'], 'embed_dim': meta['embed_dim'],
                          'mini_batch_size': meta['mini_batch_size'], 'learning_rate': meta['learning_rate'], **over})


def device_log(lc, P):
    return ct.columns_to_device_log(np.asarray(lc['u']).astype(np.int64), np.asarray(lc['is_bandit'], dtype=bool), np.asarray(lc['v']).astype(np.int64),
                                    np.asarray(lc['a']).astype(np.int64), np.nan_to_num(np.asarray(lc['c'], dtype=np.float64)) != 0, P,
                                    torch.device(DEV))


def triples_of(lc, n_org, first_call, mb, pending=None, P=None):
    return log_triples(lc['u'], lc['is_bandit'], lc['v'], lc['a'], lc['c'], n_org, first_call, mb, pending, P)


def samples_on_device(dl, P, n_org, first_call, mb, pending):
    """rg_bmf_samples -> (return code, triples, step_offsets (n_steps + 2), n_calls, last_view, the raw output words)."""
    lib = _abi.load()
    n_rows, n_users = int(dl.rows.shape[0]), int(dl.offsets.numel()) - 1
    pend = np.asarray(pending, dtype=np.int32).reshape(-1, 3)
    d_pend = torch.from_numpy(pend).to(DEV)
    triples = torch.full((len(pend) + n_rows + 1, 3), -7, dtype=torch.int32, device=DEV)
    cap = (first_call % mb + n_rows) // mb + 2
    offs = torch.full((cap,), -7, dtype=torch.int64, device=DEV)
    out = torch.zeros(8, dtype=torch.int64, device=DEV)
    need = lib.rg_bmf_samples_workspace_bytes(n_rows, len(pend))
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=DEV)
    rc = lib.rg_bmf_samples(dl.rows.data_ptr(), dl.offsets.data_ptr(), n_users, n_org, n_rows, P, first_call, mb,
                            d_pend.data_ptr() if len(pend) else None, len(pend), triples.data_ptr(), len(pend) + n_rows, offs.data_ptr(), cap,
                            out.data_ptr(), ws.data_ptr(), need, None)
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    if rc != 0:
        return rc, triples.cpu().numpy(), offs.cpu().numpy(), 0, -1, res
    assert (triples[int(res[3]):] == -7).all()                                      # nothing behind the list
    return rc, triples[:int(res[3])].cpu().numpy(), offs[:int(res[2]) + 2].cpu().numpy(), int(res[1]), int(res[5]), res


def assert_samples(got, want):
    assert got[0] == 0 and got[5][0] == 0
    assert np.array_equal(got[1], want[0]) and np.array_equal(got[2], want[1]) and got[3:5] == want[2:]
    assert got[5][4] == want[1][-1] - want[1][-2]                                   # the pending tail


def steps_on_device(arrays, steps, lr, force_global=0, offsets=None):
    """rg_bmf_steps on the four float64 arrays and a list of per-step triple lists -> (the four arrays after, the output words)."""
    lib = _abi.load()
    P, E = arrays[0].shape
    state = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(DEV) for x in arrays]
    flat = np.asarray([t for s in steps for t in s], dtype=np.int32).reshape(-1, 3)
    off = np.cumsum([0] + [len(s) for s in steps]).astype(np.int64) if offsets is None else np.asarray(offsets, dtype=np.int64)
    d_triples, d_off = torch.from_numpy(flat).to(DEV), torch.from_numpy(off).to(DEV)
    out = torch.full((4,), -1, dtype=torch.int64, device=DEV)
    need = lib.rg_bmf_steps_workspace_bytes(P, E)
    ws = torch.empty(need // 8, dtype=torch.int64, device=DEV)
    model = _abi.RgBmfModel(P, E, *[x.data_ptr() for x in state])
    _abi.check(lib.rg_bmf_steps(C.byref(model), lr, bu.ALPHA, bu.EPS, d_triples.data_ptr() if len(flat) else None, len(flat), d_off.data_ptr(),
                                len(off) - 1, force_global, out.data_ptr(), ws.data_ptr(), need, None), 'rg_bmf_steps')
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in state], out.cpu().numpy()


def limits(E):
    lds_max, p_max, step_max = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    assert _abi.load().rg_bmf_limits(E, C.byref(lds_max), C.byref(p_max), C.byref(step_max)) == 0
    return lds_max.value, p_max.value, step_max.value


# ---- 1. the triple list -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_samples_equal_log_triples(name):
    meta, cols = bu.load(name)
    P, mb, n_org = meta['num_products'], meta['mini_batch_size'], meta['n_organic']
    lc = bu.log_columns(cols)
    dl = device_log(lc, P)
    n_calls = triples_of(lc, n_org, 0, mb)[2]
    for first_call, pending in ((0, []), (mb - 1, PEND), ((-n_calls) % mb, PEND), (5 * mb + 3, [])):   # a trigger on the first / last call
        want = triples_of(lc, n_org, first_call, mb, pending, P)
        got = samples_on_device(dl, P, n_org, first_call, mb, pending)
        again = samples_on_device(dl, P, n_org, first_call, mb, pending)
        assert_samples(got, want)
        assert got[3] == n_calls
        assert np.array_equal(got[1], again[1]) and np.array_equal(got[2], again[2]) and np.array_equal(got[5], again[5])   # the same bytes
    if meta['n_users2']:        # the second log continues the first: its pending triples in front, the call count carried on
        t1, o1, c1, _ = triples_of(lc, n_org, 0, mb)
        lc2 = bu.log_columns(cols, 'log2_')
        carried = t1[o1[-2]:o1[-1]]
        assert c1 % mb != 0 and len(carried)
        assert_samples(samples_on_device(device_log(lc2, P), P, 0, c1, mb, carried), triples_of(lc2, 0, c1, mb, carried, P))


def test_samples_of_a_long_log_with_long_users():
    """More rows than one scan block holds (2048 + the 64 of a chunk), users longer than the 64 rows of a chunk, organic-only users."""
    P = 23
    lc = bu.synthetic_log(5, 260, 7, P, long_users=((2, 100), (40, 131), (41, 64), (42, 65), (259, 300)))
    assert len(lc['u']) > 2112 + 64
    dl = device_log(lc, P)
    for first_call, mb, pending in ((7, 32, [(4, 4, 1)]), (0, 4, []), (3, 257, PEND)):
        assert_samples(samples_on_device(dl, P, 7, first_call, mb, pending), triples_of(lc, 7, first_call, mb, pending, P))


# ---- 2. the step kernel on placed triple lists ----------------------------------------------------------------------------------------
def placed_steps(P, seed, cap):
    r = np.random.RandomState(seed)
    full = lambda n: [(int(l), int(a), int(c)) for l, a, c in zip(r.randint(0, P, n), r.randint(0, P, n), r.randint(0, 2, n))]      # noqa: E731
    one = (int(r.randint(P)), int(r.randint(P)), 1)
    a = int(r.randint(P))
    same = [(int(x), int(x), int(c)) for x, c in zip(r.randint(0, P, 20), r.randint(0, 2, 20))]                                      # l == a
    return [full(50), [], [one] * 200, [(int(l), a, int(c)) for l, c in zip(r.randint(0, P, 30), r.randint(0, 2, 30))], same,
            [(l, x, 1) for l, x, _ in full(25)], [(l, x, 0) for l, x, _ in full(25)], full(cap), full(3)]


PLACED = [(3, 1, 0, 1.0), (3, 5, 1, 1.0), (10, 5, 0, 1.0), (10, 5, 1, 1.0), (65, 8, 0, 1.0), (65, 5, 1, 1.0), (65, 1, 0, 1.0),
          ('split', 5, 0, 1.0), ('split+1', 5, 0, 1.0), ('split', 8, 0, 1.0), ('split+1', 8, 0, 1.0), (10, 5, 0, 8.0), (10, 5, 1, 8.0)]


@pytest.mark.parametrize('P,E,force_global,scale', PLACED)
def test_steps_on_placed_triples_equal_the_numpy_restatement(P, E, force_global, scale):
    natural_global = P == 'split+1'
    lds_max, _, cap = limits(E)
    P = lds_max + (1 if natural_global else 0) if isinstance(P, str) else P
    r = np.random.RandomState(P * 100 + E)
    ep, eu = r.standard_normal((P, E)) * 0.5 * scale, r.standard_normal((P, E)) * 0.5 * scale
    sq = [np.abs(r.standard_normal(x.shape)) * 1e-3 for x in (ep, eu)]                   # averages that have a past
    steps = placed_steps(P, 5 + E, cap)
    if scale != 1.0:        # a saturated sigmoid: |z| around 40 occurs, and everything stays finite
        z = np.abs(np.einsum('se,se->s', ep[[t[1] for t in steps[0]]], eu[[t[0] for t in steps[0]]]))
        assert 30 < z.max() < 700
    model = bu.NumpyModel(ep, eu, sq)
    before = [x.copy() for x in model.arrays()]
    for s in steps:
        model.step(s, LR)
    got, out = steps_on_device(before, steps, LR, force_global)
    again, out2 = steps_on_device(before, steps, LR, force_global)
    assert list(out) == [0, len(steps) - 1, 1, sum(len(s) for s in steps)]                 # taken, skipped as empty, samples consumed
    assert all(np.isfinite(x).all() for x in got)
    dev = max(float(np.abs(x - y).max()) for x, y in zip(got, model.arrays()))
    print(f'P={P} E={E} scale={scale} {"global" if force_global or natural_global else "LDS"}: |kernel - NumPy| = {dev:.3e}')
    assert dev <= bu.TOL_KERNEL_VS_NUMPY
    assert bu.MEASURED_KERNEL_VS_NUMPY * 1000 <= bu.TOL_F64_VS_REFERENCE                 # the two bounds add up to one on the reference
    for x, y in zip(got, again):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))                        # two runs, the same bits
    assert np.array_equal(out, out2)
    # a row no step touched keeps its value while its average decays; an empty step leaves the averages untouched
    a1, _ = steps_on_device(before, steps[:1], LR, force_global)
    a2, o2 = steps_on_device(before, steps[:2], LR, force_global)
    assert list(o2[:3]) == [0, 1, 1]
    for x, y in zip(a1, a2):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    untouched = np.setdiff1d(np.arange(P), [t[1] for t in steps[0]])
    if len(untouched):
        assert np.array_equal(a1[0][untouched], before[0][untouched]) and np.array_equal(a1[2][untouched], bu.ALPHA * before[2][untouched])
    if not force_global and not natural_global:                                            # the two instantiations: one body
        g, _ = steps_on_device(before, steps, LR, 1)
        assert max(float(np.abs(x - y).max()) for x, y in zip(got, g)) <= bu.TOL_KERNEL_VS_NUMPY


def test_steps_refuse_a_bad_list_and_leave_the_model():
    r = np.random.RandomState(3)
    arrays = [r.standard_normal((10, 5)), r.standard_normal((10, 5)), np.abs(r.standard_normal((10, 5))), np.abs(r.standard_normal((10, 5)))]
    cap = limits(5)[2]
    good = [(1, 2, 0), (3, 4, 1)]
    bad = [([good + [(3, 10, 0)], [(0, 0, 1)]], None, 2),                                  # a = P
           ([good + [(10, 3, 0)], [(0, 0, 1)]], None, 2),                                  # l = P
           ([good + [(3, 4, 2)], [(0, 0, 1)]], None, 64),                                  # reward 2
           ([good, [(0, 0, 1)] * (cap + 1)], None, 128),                                   # a step of cap + 1
           ([good, good], [0, 3, 2], 4),                                                   # descending offsets
           ([good, good], [0, 2, 5], 4)]                                                   # offsets that leave the list
    for force_global in (0, 1):
        for steps, offsets, bit in bad:
            got, out = steps_on_device(arrays, steps, LR, force_global, offsets)
            assert out[0] == bit and list(out[1:]) == [0, 0, 0], (steps, offsets)
            for x, y in zip(got, arrays):
                assert np.array_equal(x, y)
        got, out = steps_on_device(arrays, [good, [(0, 0, 1)] * cap], LR, force_global)      # the cap itself is inside
        assert list(out) == [0, 2, 0, 2 + cap]


# ---- 3. end to end -------------------------------------------------------------------------------------------------------------------
class Spy(BanditMFSquareAgent):
    def train_from_log(self, log, num_organic_users=0):
        Spy.seen.append(type(log).__name__)
        return super().train_from_log(log, num_organic_users)


def assert_logs_row_for_row(got, want, ps_tol):
    """The same rows; `ps` (the winning logit) within the tolerance, everything else equal."""
    assert len(got) == len(want) > 0
    gk, wk = frame_key(got), frame_key(want)                                               # t, u, v, a, c, ps, is_bandit
    for i in (0, 1, 2, 3, 4, 6):
        assert np.array_equal(gk[i], wk[i], equal_nan=True), i
    assert np.array_equal(np.isnan(gk[5]), np.isnan(wk[5])) and np.nanmax(np.abs(gk[5] - wk[5])) <= ps_tol


@pytest.mark.parametrize('name', ['bandit_mf_dev_p10_s01_org', 'bandit_mf_dev_p40_e8', 'bandit_mf_dev_p10_mb4'])
def test_device_route_end_to_end_against_the_reference(name):
    meta, cols = bu.load(name)
    P, E, mb = meta['num_products'], meta['embed_dim'], meta['mini_batch_size']
    tol = bu.TOL_F64_VS_REFERENCE + bu.TOL_KERNEL_VS_NUMPY
    env = make_env(meta['env_args'])
    cnt, sim = env.simulate(meta['n_users'], None, meta['n_organic'])
    lc, want_lc = sim.log_columns(), bu.log_columns(cols)
    for k in ('u', 'is_bandit', 'v', 'a'):
        assert np.array_equal(np.asarray(lc[k]).astype(np.int64), want_lc[k].astype(np.int64)), k           # the fixture's log, from its seed
    agent = BanditMFSquareAgent(config(meta, device_training=True), cols['ep0'], cols['eu0'])
    assert agent.device_route() and agent.accepts_device_log
    agent.train_from_log(sim.device_log(), meta['n_organic'])
    sim.close()
    assert agent.curr_step == meta['calls'] and agent.last_product_viewed == meta['last_product_viewed']
    assert agent.last_device_stats['steps'] == meta['steps'] - meta['empty_steps'] and agent.last_device_stats['empty_steps'] == meta['empty_steps']
    state = [x.cpu().numpy() for x in agent._dev['state']]
    dev = max(float(np.abs(x - cols[k]).max()) for x, k in zip(state, bu.KEYS))
    print(f'{name}: device route vs reference {dev:.3e}')
    assert dev <= tol
    for p, x, sq in zip(agent._params(), state[:2], state[2:]):                            # the float32 roundings, in the modules and the optimiser
        assert np.array_equal(p.detach().numpy(), x.astype(np.float32))
        assert np.array_equal(agent.optimizer.state[p]['square_avg'].numpy(), sq.astype(np.float32))
    assert np.array_equal(agent.frozen().table, cols['table'])                             # the reference's act at every product
    # the host route's agent (the reference's bits where torch's CPU kernels are the fixtures': tests/test_bandit_mf_host.py) and this one log the same rows: in the device loop, inside EpsilonGreedy
    host = BanditMFSquareAgent(config(meta), cols['ep0'], cols['eu0'])
    host.train_from_log(want_lc, meta['n_organic'])
    assert host.train_data == agent.train_data and host.curr_step == agent.curr_step
    ps_tol = 2 * E * meta['weight_magnitude'] * tol            # `ps` is the winning logit: E products of two weights, each within tol
    assert agent.device_policy()['policy'] == _abi.RG_POLICY_LAST_VIEW_TABLE
    assert_logs_row_for_row(env.generate_logs(50, agent), env.generate_logs(50, HostOnly(host)), ps_tol)
    eg_cfg = Configuration({**epsilon_greedy_args, 'epsilon': 0.3, 'random_seed': 11, 'num_products': P})
    assert_logs_row_for_row(env.generate_logs(50, EpsilonGreedy(eg_cfg, agent)), env.generate_logs(50, HostOnly(EpsilonGreedy(eg_cfg, host))), ps_tol)
    if name != 'bandit_mf_dev_p10_s01_org':
        return
    # test_agent hands the device log over and gives what the host route gives
    Spy.seen = []
    args = (meta['n_users'], 60)
    got = recogym.test_agent(env, Spy(config(meta, device_training=True), cols['ep0'], cols['eu0']), *args,
                             num_organic_offline_users=meta['n_organic'])
    want = recogym.test_agent(env, Spy(config(meta), cols['ep0'], cols['eu0']), *args, num_organic_offline_users=meta['n_organic'])
    assert Spy.seen == ['DeviceLog', 'dict'] and got == want
    # route switching: a second device log continues the first; the host route continues the device route, and back
    u = want_lc['u']
    starts = np.flatnonzero(np.r_[True, u[1:] != u[:-1]])
    for cut in starts[len(starts) // 2:]:              # a user boundary inside a mini-batch, with samples pending across it
        _, o, c, _ = triples_of({k: x[:cut] for k, x in want_lc.items()}, meta['n_organic'], 0, mb)
        if c % mb and o[-1] > o[-2]:
            break
    cut = int(cut)
    assert meta['n_organic'] < len(np.unique(u[:cut])) and cut < len(u)
    first, second = ({k: x[:cut] for k, x in want_lc.items()}, {k: x[cut:] for k, x in want_lc.items()})
    two = BanditMFSquareAgent(config(meta, device_training=True), cols['ep0'], cols['eu0'])
    two.train_from_log(device_log(first, P), meta['n_organic'])
    assert two.curr_step % two.batch != 0 and len(two.train_data[0])
    two.train_from_log(device_log(second, P), 0)
    assert two.curr_step == meta['calls'] and two.last_product_viewed == meta['last_product_viewed']
    for x, y in zip(two._dev['state'], agent._dev['state']):
        assert torch.equal(x, y)                                                            # the same steps on the same triples: the same bits
    mixed = BanditMFSquareAgent(config(meta, device_training=True), cols['ep0'], cols['eu0'])
    mixed.train_from_log(device_log(first, P), meta['n_organic'])
    mixed.config.device_training = False
    mixed.train_from_log(device_log(second, P), 0)                                          # float32 from here on; the DeviceLog is converted
    assert mixed.curr_step == meta['calls'] and np.array_equal(mixed.frozen().table, cols['table'])
    assert max(float(np.abs(x - cols[k]).max()) for x, k in zip(mixed._arrays32(), bu.KEYS)) <= tol
    mixed.config.device_training = True
    mixed.train_from_log(second, 0)                                                         # and back: the state is re-read from the modules
    assert mixed.curr_step == meta['calls'] + len(np.flatnonzero(second['is_bandit']))
    other = BanditMFSquareAgent(config(meta), cols['ep0'], cols['eu0'])                           # host first, then the device
    other.train_from_log(first, meta['n_organic'])
    assert other._dev is None and len(other.train_data[0]) == o[-1] - o[-2]
    other.config.device_training = True
    other.train_from_log(device_log(second, P), 0)
    assert other.curr_step == meta['calls'] and np.array_equal(other.frozen().table, cols['table'])
    assert max(float(np.abs(x - cols[k]).max()) for x, k in zip(other._arrays32(), bu.KEYS)) <= tol


def test_two_log_fixture_continues_bit_for_bit():
    """The two-log fixture: the boundary falls inside a mini-batch; two device calls equal one call's chain on the joined list."""
    meta, cols = bu.load('bandit_mf_dev_p10_two')
    P, mb = meta['num_products'], meta['mini_batch_size']
    lc1, lc2 = bu.log_columns(cols), bu.log_columns(cols, 'log2_')
    agent = BanditMFSquareAgent(config(meta, device_training=True), cols['ep0'], cols['eu0'])
    agent.train_from_log(device_log(lc1, P), 0)
    assert agent.curr_step % mb != 0 and len(agent.train_data[0]) > 0
    agent.train_from_log(device_log(lc2, P), 0)
    assert agent.curr_step == meta['calls'] and agent.last_product_viewed == meta['last_product_viewed']
    state = [x.cpu().numpy() for x in agent._dev['state']]
    assert max(float(np.abs(x - cols[k]).max()) for x, k in zip(state, bu.KEYS)) <= bu.TOL_F64_VS_REFERENCE + bu.TOL_KERNEL_VS_NUMPY
    assert np.array_equal(agent.frozen().table, cols['table'])
    # one chain over both logs' steps: the same bits
    t1, o1, c1, _ = triples_of(lc1, 0, 0, mb)
    t2, o2, _, _ = triples_of(lc2, 0, c1, mb, t1[o1[-2]:o1[-1]])
    steps = [t1[o1[s]:o1[s + 1]].tolist() for s in range(len(o1) - 2)] + [t2[o2[s]:o2[s + 1]].tolist() for s in range(len(o2) - 2)]
    first = [np.asarray(x, dtype=np.float32).astype(np.float64) for x in (cols['ep0'], cols['eu0'])]
    # (the write-back between the two calls re-reads nothing: the float64 state goes on)
    joined, _ = steps_on_device(first + [np.zeros_like(x) for x in first], steps, meta['learning_rate'])
    for x, y in zip(state, joined):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))


# ---- 4. what is refused --------------------------------------------------------------------------------------------------------------
def test_bad_logs_are_refused_and_leave_the_model():
    meta, cols = bu.load('bandit_mf_dev_p10_s0')
    lc = bu.log_columns(cols)
    agent = BanditMFSquareAgent(config(meta, device_training=True), cols['ep0'], cols['eu0'])
    agent.train_data = ([1], [2], [1])
    agent.curr_step = 5
    agent.last_product_viewed = 4
    before = [x.copy() for x in agent._arrays32()]
    bad_v = {k: x.copy() for k, x in lc.items()}
    bad_v['v'][np.flatnonzero(~lc['is_bandit'])[40]] = 10                                 # a view = P
    bad_a = {k: x.copy() for k, x in lc.items()}
    bad_a['a'][np.flatnonzero(lc['is_bandit'])[40]] = 10                                  # an action = P
    first_b = {k: x.copy() for k, x in lc.items()}
    start = np.flatnonzero(np.r_[True, lc['u'][1:] != lc['u'][:-1]])[3]
    first_b['is_bandit'][start] = True                                                      # a user that opens with a bandit row
    for bad, n_org in ((bad_v, 0), (bad_a, 0), (first_b, 0), (lc, 2)):                      # (lc, 2): an organic-only user with a bandit row
        dl = device_log(bad, 10)
        rc, triples, offs, _, _, res = samples_on_device(dl, 10, n_org, 0, 32, [])
        assert rc == -1 and (triples == -7).all() and (offs == -7).all() and list(res[1:]) == [0] * 7     # RG_EINVAL, nothing written
        with pytest.raises(_abi.RecoGymHipError, match='RG_EINVAL'):
            agent.train_from_log(dl, n_org)
        assert agent.curr_step == 5 and agent.train_data == ([1], [2], [1]) and agent._dev is None and agent.last_product_viewed == 4
        for x, y in zip(agent._arrays32(), before):
            assert np.array_equal(x, y)


@pytest.mark.parametrize('over', [dict(num_products=16385, embed_dim=2, mini_batch_size=2), dict(num_products=12, embed_dim=65, mini_batch_size=2),
                                  dict(num_products=12, embed_dim=2, mini_batch_size=258)])
def test_beyond_a_cap_trains_on_the_host_after_one_warning(over):
    cfg = Configuration({**bandit_mf_square_args, **over, 'device_training': True})
    agent = BanditMFSquareAgent(cfg)
    with pytest.warns(RuntimeWarning, match='caps'):
        assert not agent.device_route()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert not agent.accepts_device_log                                                 # once
        u = np.array([0, 0, 0, 0, 1, 1, 1])
        is_b = np.array([0, 0, 1, 1, 0, 0, 1], dtype=bool)
        v = np.array([5, 11, 0, 0, 7, 5, 0])
        a = np.array([0, 0, 3, 11, 0, 0, 2])
        w0 = agent.product_embedding.weight.detach().numpy().copy()
        agent.train_from_log(dict(u=u.astype(np.int32), is_bandit=is_b, v=v, a=a, c=np.where(is_b, 1.0, np.nan),
                                  ps=np.where(is_b, 0.1, np.nan), t=np.arange(7, dtype=np.float32)), 0)
    assert agent.curr_step == 3 and agent._dev is None and agent.last_product_viewed == 5
    if over['mini_batch_size'] == 2:                           # calls 1 and 3 store a sample, call 2 steps on the first
        assert agent.train_data == ([5], [2], [1.0]) and not np.array_equal(agent.product_embedding.weight.detach().numpy(), w0)
    else:
        assert agent.train_data == ([11, 11, 5], [3, 11, 2], [1.0, 1.0, 1.0])


def test_the_cap_itself_is_inside():
    assert limits(5) == (245, 16384, 256) and limits(64)[0] >= 1
    agent = BanditMFSquareAgent(Configuration({**bandit_mf_square_args, 'num_products': 12, 'mini_batch_size': 257, 'device_training': True}))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert agent.device_route()
