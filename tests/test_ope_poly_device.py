"""Off-policy replay of the likelihood agent on the device (rg_ope_replay_poly, recogym_amd/csrc/rg_ope_poly.hip) against the
reference's own numbers (tests/golden/poly_p10_ope.npz and the poly_* logs, whose self-evaluation is exactly 1), the host loop
(LogregPolyFrozenAgent.act through evaluate_agent._host_snips), the host act on hand-made histories, decisions placed round
expit's steps, and itself.  Every ratio is compared bit for bit; the head words of the workspace prove which path an act took.
Needs a real MI355X."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import torch
from scipy.special import expit

import golden_util as gu
from make_golden_ope import log_frame
from recogym_amd import _abi
from recogym_amd import evaluate_agent as ev
from recogym_amd.agents import OrganicUserEventCounterAgent, RandomAgent
from recogym_amd.agents.logreg_poly import LogregPolyFrozenAgent, expit_steps, poly_decisions, poly_rule
from recogym_amd.envs.configuration import Configuration
from recogym_amd.envs.reco_env_v1 import env_1_args
from recogym_amd.sim import DeviceLog, Simulator
from test_logreg_poly_device import MERGE, TABLE, UNRESOLVED, constant_agent, placements
from test_ope_sums_order import documented_sums

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
W_CAP = 4096                     # this unit's wave cap (rg_ope_poly.hip: kPlMaxWaves), part of the bits of d_sums
O, B = False, True


@pytest.fixture(scope='module')
def th():
    return expit_steps()


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), np.nonzero(got != want)[0][:8]


def agent_of(P, wf, wa, wk, b):
    return LogregPolyFrozenAgent(Configuration({'num_products': P, 'random_seed': 7, 'with_ps_all': True}),
                                 np.r_[wf, wa, np.asarray(wk).reshape(-1)][None, :], [b])


def random_agent(P, scale, seed):
    rng = np.random.RandomState(seed)
    return agent_of(P, rng.randn(P) * scale, rng.randn(P) * scale / P, rng.randn(P, P) * scale, float(rng.randn()))


def with_ps_all(ag):
    return agent_of(ag.config.num_products, ag.wf, ag.wa, ag.wk, ag.b)


def replay(ag, dl, n_users=None):
    """-> (ratio, clicks, sums, stats) as host arrays; every user of the log unless n_users says otherwise."""
    st = {}
    out = ev.ope_replay(ag, dl, n_users=int(dl.offsets.numel()) - 1 if n_users is None else n_users, stats=st)
    assert out is not None and st['error'] == 0
    r, c, sums = out
    return r.cpu().numpy(), c.cpu().numpy(), sums.cpu().numpy(), st


def plus_one_user(dl):
    """The log with one more (highest, hence unevaluated) user of one organic row: what the estimators expect of a device log."""
    last = torch.zeros((1, 4), dtype=torch.int32, device=dl.rows.device)
    last[0, 0] = int(dl.offsets.numel()) - 1
    ps = dl.ps if dl.ps is None or isinstance(dl.ps, float) else torch.cat([dl.ps, torch.full((1,), float('nan'), dtype=torch.float64, device=dl.ps.device)])
    return DeviceLog(torch.cat([dl.rows, last]), torch.cat([dl.offsets, dl.offsets[-1:] + 1]), ps, dl.first_user, dl.num_products, None)


# ---- 1. the reference's numbers ------------------------------------------------------------------------------------------------
def test_device_equals_the_reference_numbers():
    want = np.load(f'{gu.GOLDEN}/poly_p10_ope.npz')
    _, cols = gu.load('philox_p10')
    df = log_frame(cols)
    ag = LogregPolyFrozenAgent(Configuration({'num_products': 10, 'random_seed': 7, 'with_ps_all': True}), want['poly_coef'],
                               want['poly_intercept'])
    pol = ev.ope_checked_policy_of(ag)
    dl = ev._frame_to_device(df, pol, torch.device(DEV))
    assert dl is not None and int(dl.offsets.numel()) - 1 == 309 and int((dl.offsets[1:] - dl.offsets[:-1]).max()) == 821
    assert ev.ope_replay(ag, dl, n_users=309) is not None            # (the policy found through the agent's hook)
    r, c, sums, st = replay(ag, dl)
    same(r, want['snips_ratio'])
    assert r.size == 22744 and np.count_nonzero(r) == 2317
    same(c, want['snips_c'])
    same(c * r, want['ips'])
    print(st)
    assert st['acts'] == 1616 and st['unresolved'] == 0 and st['table'] == 0 and not st['overflow']
    assert sums[0] == 22744.0
    # ... through the estimators: a DataFrame (lists) and a DeviceLog (tensors)
    rewards, ratio = ev.evaluate_SNIPS(ag, df)
    assert isinstance(ratio, list) and isinstance(rewards, list)
    same(ratio, want['snips_ratio'])
    same(rewards, want['snips_c'])
    ips = ev.evaluate_IPS(ag, df)
    assert isinstance(ips, list)
    same(ips, want['ips'])
    c_t, r_t = ev.evaluate_SNIPS(ag, plus_one_user(dl))
    assert torch.is_tensor(r_t) and r_t.is_cuda
    same(r_t.cpu().numpy(), want['snips_ratio'])
    same(c_t.cpu().numpy(), want['snips_c'])
    same(ev.evaluate_IPS(ag, plus_one_user(dl)).cpu().numpy(), want['ips'])


# ---- 2. self-evaluation of the reference's own logs ----------------------------------------------------------------------------
@pytest.mark.parametrize('name,rows,acts,table,lower', [('poly_p10', 6606, 497, 0, 0), ('poly_p40', 6592, 502, 8, 0),
                                                        ('poly_p10_sigma0', 6605, 497, 0, 0), ('poly_p10_ips', 6552, 509, 0, 0),
                                                        ('poly_p10_shifted', 2898, 214, 214, 13)])
def test_self_evaluation_of_reference_logged_fixtures(name, rows, acts, table, lower):
    """The agent that wrote the log evaluates it: every ratio exactly 1.  The shifted fixture proves the table zone and the merge
    (all its acts on the table, 13 of them won by a lower index than the first maximal decision)."""
    meta, cols = gu.load(name)
    P = meta['env_args']['num_products']
    ag = LogregPolyFrozenAgent(Configuration({'num_products': P, 'with_ps_all': True}), cols['poly_coef'], cols['poly_intercept'])
    df = log_frame(cols)
    dl = ev._frame_to_device(df, ev.ope_checked_policy_of(ag), torch.device(DEV))
    r, c, sums, st = replay(ag, dl)
    print(name, st)
    assert r.size == rows and bool((r == 1.0).all())
    assert sums[0] == rows and sums[2] == rows and sums[1] == c.sum()
    assert (st['acts'], st['table'], st['lower'], st['unresolved']) == (acts, table, lower, 0)
    rewards, ratio = ev.evaluate_SNIPS(ag, df)
    assert len(ratio) == rows and all(x == 1.0 for x in ratio)


# ---- 3. simulator logs against the host loop ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sim_log(P, sigma, n=300, seed=11, K=5):
    cfg = Configuration({**env_1_args, 'random_seed': seed, 'num_products': P, 'K': K, 'sigma_omega': sigma})
    sim = Simulator(cfg, n, device=DEV)
    sim.reset_users(0, n)
    sim.run()
    dl = sim.device_log()
    df = ev._device_log_to_frame(dl)
    sim.close()
    return dl, df


@pytest.mark.parametrize('large', [False, True])
@pytest.mark.parametrize('sigma', [0.0, 0.1])
@pytest.mark.parametrize('P', [10, 65, 130])
def test_device_equals_host_loop_on_simulator_logs(P, sigma, large):
    """Dense random models at two scales: decisions of order 1, and a scale raised until the head reports acts on the step table."""
    dl, df = sim_log(P, sigma)
    n_eval = int(dl.offsets.numel()) - 2
    if not large:
        ag = random_agent(P, 0.3, seed=P)
        r, c, sums, st = replay(ag, dl, n_eval)
    else:
        for scale in (2.0, 4.0, 8.0, 16.0, 32.0):
            ag = random_agent(P, scale, seed=P + 1)
            r, c, sums, st = replay(ag, dl, n_eval)
            if st['table'] > 0:
                break
        assert st['table'] > 0, st
    print(P, sigma, large, st)
    rewards, want = ev._host_snips(ag, df)
    same(r, want)
    same(c, np.asarray(rewards, dtype=np.float64))
    assert 0 < np.count_nonzero(r) < r.size and (large or st['unresolved'] == 0)
    # the sums in the skeleton's documented order at this unit's W
    total = int(dl.offsets[n_eval].item())
    code = dl.rows[:total, 2].cpu().numpy().view(np.uint32)
    is_b = (code & _abi.RG_EV_BANDIT) != 0
    ratio = np.zeros(total)
    ratio[is_b] = r
    click = ((code & _abi.RG_EV_CLICK) != 0).astype(np.float64)
    want_sums = documented_sums(ratio, click, is_b, dl.offsets[:n_eval + 1].cpu().numpy(), W_CAP)
    assert sums.tobytes() == want_sums.tobytes(), ([x.hex() for x in sums], [x.hex() for x in want_sums])
    assert st['acts'] == int((is_b[1:] & ~is_b[:-1]).sum())


# ---- 4. history shapes: hand-made logs against the host act ---------------------------------------------------------------------
def build(users, ag, ps=0.25):
    """users: per user a list of tokens, ('o', product) or 'b' -> (DeviceLog, expected ratio per bandit row, acts).  The host walks
    the rows as the reference's loop does (views kept across sessions, reset per user; act_on at a bandit row whose history
    changed) and writes the logged action itself: the host's action and another one, alternating — so the expected ratios are
    1 / ps and 0, and a device action that differs from the host's shows on every row."""
    P = ag.config.num_products
    raw, offsets, want, acts, flip = [], [0], [], 0, 0
    for u, toks in enumerate(users):
        views = np.zeros(P, dtype=np.int64)
        dirty, a_host = True, None
        for t, tok in enumerate(toks):
            if tok == 'b':
                if dirty:
                    prods = np.flatnonzero(views)
                    a_host = ag.act_on(prods, views[prods])
                    acts += 1
                    dirty = False
                a = a_host if flip % 2 == 0 else (a_host + 1 + flip % (P - 1)) % P
                flip += 1
                want.append((1.0 if a == a_host else 0.0) / ps)
                raw.append((u, t, a | _abi.RG_EV_BANDIT | (_abi.RG_EV_CLICK if flip % 3 == 0 else 0), 0))
            else:
                views[tok[1]] += 1
                dirty = True
                raw.append((u, t, tok[1], 0))
        offsets.append(len(raw))
    rows = torch.from_numpy(np.array(raw, dtype=np.uint32).reshape(-1, 4).view(np.int32)).to(DEV)
    return DeviceLog(rows, torch.tensor(offsets, dtype=torch.int64, device=DEV), float(ps), 0, P, None), np.array(want), acts


def check(users, ag, what):
    dl, want, acts = build(users, ag)
    r, _, sums, st = replay(ag, dl)
    print(what, st)
    assert st['unresolved'] == 0, (what, st)                         # (an unresolved act is the host's to decide: none here)
    same(r, want)
    assert st['acts'] == acts and sums[0] == want.size and 0 < np.count_nonzero(r) < r.size, (what, st, acts)
    return st


def distinct(n, P, seed):
    return [('o', int(p)) for p in np.random.RandomState(seed).permutation(P)[:n]]


@pytest.mark.parametrize('scale', [0.02, 1.0])
def test_history_sizes_round_the_tier_boundaries(scale):
    """1, 63, 64, 65: the 64-entry chunks the list's insert and the act's prefix walk in; 255, 256, 257: the 256 entries the act
    caches in LDS (kPolyHist; beyond it reads the list); 511, 512, 513: the 512 entries of the LDS list (kPlLds; beyond: the
    per-wave global list, entered while the user is replayed).  Every user acts once per size on the way up (bandit rows at two
    earlier sizes) and twice at its final size."""
    P = 600
    ag = random_agent(P, scale, seed=3)
    users = []
    for n in (1, 63, 64, 65, 255, 256, 257, 511, 512, 513):
        v = distinct(n, P, seed=n)
        toks = v[:n // 2] + (['b'] if n // 2 else []) + v[n // 2:n - 1] + (['b'] if n - 1 > n // 2 else []) + v[n - 1:] + ['b', 'b']
        users.append(toks)
    st = check(users, ag, f'sizes at scale {scale}')
    assert st['rows_read'] >= 513 + 512 + 511


def test_counts_chunk_positions_and_sessions():
    P = 600
    ag = random_agent(P, 0.02, seed=4)
    v = distinct(200, P, seed=9)
    users = [
        [('o', 7)] * 300 + ['b'] + [('o', 9)] + ['b', 'b'],                       # a product viewed 300 times
        v[:63] + ['b'] + v[63:70] + ['b'],                                       # the act at lane 63 of the first chunk
        v[:64] + ['b'] + v[64:70] + ['b'],                                       # the act at lane 0 of the second chunk
        v[:30] + ['b', 'b', 'b'] + v[30:40] + ['b'] + v[40:45] + ['b', 'b'],     # acts in the middle of a chunk, reused by the rows after
        (v[:3] + ['b']) * 32,                                                    # 128 = 64 k rows (the same three products again and again)
        (v[:3] + ['b']) * 32 + ['b'],                                            # 129 = 64 k + 1 rows: the last chunk holds one reused act
        [('o', 5), 'b', 'b', 'b', 'b', 'b'],                                     # one act, five rows
        [('o', 11), 'b', ('o', 12), 'b', ('o', 11), 'b'],                        # views persist across sessions (and 11 counts twice)
        [('o', 12), 'b'],                                                        # ... and are reset at the next user
        [('o', 3)],                                                              # organic rows only
        [],                                                                      # a user without rows
        [('o', 599), 'b'],
    ]
    assert len(users[4]) == 128 and len(users[5]) == 129
    check(users, ag, 'shapes')


@pytest.mark.parametrize('P', [2, 65, 130, 300])
def test_action_counts_round_the_lane_and_stride_edges(P):
    """P = 2: 62 lanes beyond P; 65 and 130: one action past a 64-block; 300: beyond poly_scan's 256-action stride."""
    rng = np.random.RandomState(P)
    users = []
    for _ in range(12):
        toks = [('o', int(rng.randint(P)))]
        for _ in range(rng.randint(3, 40)):
            toks.append('b' if rng.rand() < 0.5 else ('o', int(rng.randint(P))))
        users.append(toks)
    for scale in (0.05, 0.5):
        check(users, random_agent(P, scale, seed=P + 7), f'P = {P} at scale {scale}')


# ---- 5. the three zones, placed ---------------------------------------------------------------------------------------------------
def test_placed_table_acts_with_a_lower_index_winning(th):
    """test_placed_decisions' recipe: with wf = wa = 0, b = 0 the user that viewed product p once decides on wk[:, p] exactly.  All
    placements that the device resolves, one user each; the logged actions are the placement's expected action and the first
    maximal decision's index."""
    P = 65
    cases = [c for c in placements(P, th) if not c[3] & UNRESOLVED]
    assert len(cases) <= P and sum(1 for c in cases if c[3] & MERGE) >= 3
    wk = np.zeros((P, P))
    raw, offsets, want = [], [0], []
    for p, (name, z, want_a, want_fl) in enumerate(cases):
        wk[:, p] = z
        host = int(np.argmax(expit(z)))
        assert host == want_a and poly_rule(z, th) == (want_a, want_fl), name
        raw.append((p, 0, p, 0))
        for t, a in enumerate((want_a, int(np.argmax(z)), (want_a + 1) % P)):
            raw.append((p, 1 + t, a | _abi.RG_EV_BANDIT, 0))
            want.append(1.0 / 0.5 if a == host else 0.0)
        offsets.append(len(raw))
    ag = agent_of(P, np.zeros(P), np.zeros(P), wk, 0.0)
    for p, (_, z, _, _) in enumerate(cases):
        assert np.array_equal(poly_decisions([p], [1], ag.wf, ag.wa, ag.wk, ag.b), z)
    dl = DeviceLog(torch.from_numpy(np.array(raw, dtype=np.uint32).view(np.int32)).to(DEV),
                   torch.tensor(offsets, dtype=torch.int64, device=DEV), 0.5, 0, P, None)
    r, _, _, st = replay(ag, dl)
    print(st)
    same(r, want)
    assert st['acts'] == len(cases) and st['unresolved'] == 0
    assert st['table'] == sum(1 for c in cases if c[3] & TABLE) > 0 and st['lower'] == sum(1 for c in cases if c[3] & MERGE) > 0


def one_act_users(n, P=10):
    """n users of one organic and one bandit row (action 2, 1 alternating), ps = 1 / P."""
    raw = np.zeros((2 * n, 4), dtype=np.uint32)
    raw[:, 0] = np.repeat(np.arange(n), 2)
    raw[1::2, 1] = 1
    raw[0::2, 2] = np.arange(n) % P
    raw[1::2, 2] = np.where(np.arange(n) % 2 == 0, 2, 1).astype(np.uint32) | _abi.RG_EV_BANDIT
    return DeviceLog(torch.from_numpy(raw.view(np.int32)).to(DEV), torch.arange(0, 2 * n + 1, 2, dtype=torch.int64, device=DEV),
                     1.0 / P, 0, P, None)


def test_an_unresolved_act_the_host_confirms_stands():
    ag = with_ps_all(constant_agent(25.0, 25.0 + 2.0 ** -12))     # inside W, but expit tells them apart: the host acts 2 too
    dl, df = sim_log(10, 0.1)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        r, c, _, st = replay(ag, dl, int(dl.offsets.numel()) - 2)
        got = ev.evaluate_SNIPS(ag, dl)
    print(st)
    assert st['unresolved'] == st['acts'] > 0 and not st['overflow']
    _, want = ev._host_snips(ag, df)
    same(r, want)
    assert torch.is_tensor(got[1])
    same(got[1].cpu().numpy(), want)
    assert 0 < np.count_nonzero(r) < r.size


def test_a_refuted_act_sends_the_estimators_to_the_host_loop():
    z2 = next(z for z in (25.0 + 2.0 ** -e for e in range(20, 46)) if expit(z) == expit(25.0))      # scipy merges them: the host acts 1
    ag = with_ps_all(constant_agent(25.0, z2))
    dl, df = sim_log(10, 0.1)
    with pytest.warns(RuntimeWarning, match='host loop') as rec:
        assert ev.ope_replay(ag, dl) is None
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    with pytest.warns(RuntimeWarning, match='host loop'):
        rewards, ratio = ev.evaluate_SNIPS(ag, dl)
    want_c, want_r = ev._host_snips(ag, df)
    assert isinstance(ratio, list)
    same(ratio, want_r)
    same(rewards, want_c)
    a = df['a'][df['z'] == 'bandit'].to_numpy(dtype=np.float64)[:len(ratio)]
    assert np.array_equal(np.asarray(ratio) != 0, a == 1)           # the reference's action: the lower index of the merged pair


def test_more_unresolved_acts_than_the_list_holds():
    """4 200 users of one act each under the model whose every act is unresolved (and which the host would confirm): the list of
    4 096 overflows, so the replay is given up exactly as for a refuted act; with 4 000 users it stands."""
    ag = with_ps_all(constant_agent(25.0, 25.0 + 2.0 ** -12))
    small = one_act_users(4000)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        r, _, _, st = replay(ag, small)
    assert st['unresolved'] == st['acts'] == 4000 and not st['overflow']
    same(r, np.where(np.arange(4000) % 2 == 0, 10.0, 0.0))
    dl = plus_one_user(one_act_users(4200))
    st = {}
    with pytest.warns(RuntimeWarning, match='host loop') as rec:
        assert ev.ope_replay(ag, dl, stats=st) is None
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    assert st['unresolved'] == 4200 and st['overflow']
    with pytest.warns(RuntimeWarning, match='host loop'):
        rewards, ratio = ev.evaluate_SNIPS(ag, dl)
    same(ratio, np.where(np.arange(4200) % 2 == 0, 10.0, 0.0))
    assert isinstance(ratio, list) and not any(rewards)


# ---- 6. determinism ----------------------------------------------------------------------------------------------------------------
def test_two_replays_and_both_ways_in_give_the_same_bits():
    P, n = 65, 300
    ag = random_agent(P, 0.3, seed=5)
    cfg = Configuration({**env_1_args, 'random_seed': 3, 'num_products': P, 'K': 5})
    sim = Simulator(cfg, n, device=DEV)
    sim.reset_users(0, n)
    sim.run()
    dl = sim.device_log()
    r1, c1, s1 = ev.ope_replay(ag, dl)
    r2, c2, s2 = ev.ope_replay(ag, dl)
    assert torch.equal(r1, r2) and torch.equal(c1, c2) and s1.cpu().numpy().tobytes() == s2.cpu().numpy().tobytes()
    c_sim, r_sim = ev.evaluate_SNIPS(ag, sim)
    c_dl, r_dl = ev.evaluate_SNIPS(ag, dl)
    assert torch.equal(r_sim, r_dl) and torch.equal(c_sim, c_dl) and torch.equal(r_sim, r1)
    assert torch.equal(ev.evaluate_IPS(ag, sim), c1 * r1)
    sim.close()


# ---- 7. ABI errors -------------------------------------------------------------------------------------------------------------------
def test_abi_errors():
    """Every call is well-formed apart from the one argument under test; all are refused before anything is written."""
    lib = _abi.load()
    dev = torch.device(DEV)
    P = 4
    z = torch.zeros(P * P, dtype=torch.float64, device=dev)
    steps = torch.from_numpy(expit_steps()).to(dev)
    raw = np.zeros((4, 4), dtype=np.uint32)
    raw[:, 1] = [0, 1, 2, 3]
    raw[:, 2] = [1, 2 | _abi.RG_EV_BANDIT, 0 | _abi.RG_EV_BANDIT | _abi.RG_EV_CLICK, 3]
    rows = torch.from_numpy(raw.view(np.int32)).to(dev)
    offsets = torch.tensor([0, 3], dtype=torch.int64, device=dev)
    ratio = torch.full((4,), -7.0, dtype=torch.float64, device=dev)
    sums = torch.full((3,), -7.0, dtype=torch.float64, device=dev)

    def model(**over):
        kw = dict(num_products=P, n_steps=int(steps.numel()), wf=z.data_ptr(), wa=z.data_ptr(), wk_t=z.data_ptr(), th=steps.data_ptr(),
                  intercept=0.0)
        kw.update(over)
        return _abi.RgOpePoly(**kw)

    need = lib.rg_ope_poly_workspace_bytes(C.byref(model()), 1, 3)
    assert need >= 256 + 4096 * 12
    assert lib.rg_ope_poly_workspace_bytes(C.byref(model()), 1, 600) > need          # the per-wave global lists
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)

    def call(m, **over):
        a = dict(rows=rows.data_ptr(), offsets=offsets.data_ptr(), n_users=1, max_rows=3, mode=_abi.RG_OPE_PS_CONST, ps=None,
                 ps_const=0.25, ratio=ratio.data_ptr(), click=None, sums=sums.data_ptr(), ws=ws.data_ptr(), ws_bytes=need)
        a.update(over)
        with torch.cuda.device(dev):
            rc = lib.rg_ope_replay_poly(C.byref(m) if m is not None else None, a['rows'], a['offsets'], a['n_users'], a['max_rows'],
                                        a['mode'], a['ps'], a['ps_const'], a['ratio'], a['click'], a['sums'], a['ws'], a['ws_bytes'],
                                        None)
        return rc, lib.rg_last_error()

    einval = [('null model', None, {}),
              ('null wf', model(wf=None), {}), ('null wa', model(wa=None), {}), ('null wk_t', model(wk_t=None), {}),
              ('null th', model(th=None), {}), ('n_steps == 0', model(n_steps=0), {}), ('n_steps > 1024', model(n_steps=1025), {}),
              ('num_products == 0', model(num_products=0), {}),
              ('null rows', model(), dict(rows=None)), ('null offsets', model(), dict(offsets=None)),
              ('null ratio', model(), dict(ratio=None)), ('null sums', model(), dict(sums=None)),
              ('null workspace', model(), dict(ws=None)),
              ('null ps array', model(), dict(mode=_abi.RG_OPE_PS_ARRAY, ps=None)), ('bad ps mode', model(), dict(mode=3)),
              ('rows not 16-byte aligned', model(), dict(rows=rows.data_ptr() + 8)),
              ('an action >= P', model(num_products=2), {}),
              ('a product >= P', model(num_products=3), dict(offsets=torch.tensor([3, 4], dtype=torch.int64, device=dev).data_ptr())),
              ('more rows than max_user_rows', model(), dict(max_rows=2)),
              ('a user that opens with a bandit row', model(), dict(offsets=torch.tensor([1, 3], dtype=torch.int64, device=dev).data_ptr()))]
    for what, m, over in einval:
        rc, msg = call(m, **over)
        assert rc == -1 and b'rg_ope_replay_poly' in msg, (what, rc, msg)
    assert b'bandit' in msg
    rc, msg = call(model(), ws_bytes=need - 1)
    assert rc == -3 and b'rg_ope_replay_poly' in msg and b'workspace' in msg, (rc, msg)
    assert lib.rg_ope_poly_workspace_bytes(None, 1, 3) == 0 and b'null' in lib.rg_last_error()
    torch.cuda.synchronize()
    assert bool((ratio == -7.0).all()) and bool((sums == -7.0).all())      # nothing was written by any refused call
    # ... and the well-formed call, in all three ps modes: an all-zero model acts 0 — the clicked row's action
    ps64 = torch.tensor([float('nan'), 0.5, 0.125], dtype=torch.float64, device=dev)
    rows_ps = rows.clone()
    rows_ps[:, 3] = torch.tensor([0.0, 0.25, 0.0625, 0.0], dtype=torch.float32).view(torch.int32).to(dev)
    for over, ps in ((dict(), 0.25), (dict(mode=_abi.RG_OPE_PS_ARRAY, ps=ps64.data_ptr()), 0.125),
                     (dict(mode=_abi.RG_OPE_PS_ROW, rows=rows_ps.data_ptr()), 0.0625)):
        ratio.fill_(-7.0)
        rc, msg = call(model(), **over)
        assert rc == 0, msg
        torch.cuda.synchronize()
        assert ratio.cpu().tolist() == [-7.0, 0.0, 1.0 / ps, -7.0]
        assert sums.cpu().tolist() == [2.0, 1.0 / ps, 1.0 / ps]
        # error, acts, table, lower index, unresolved, overflow, wk_t rows read
        assert ws[:64].view(torch.int64).cpu().tolist() == [0, 1, 0, 0, 0, 0, 1, 0]


# ---- 8. the A/B tables -----------------------------------------------------------------------------------------------------------------
def test_verify_agents_tables_equal_the_host_loops(monkeypatch):
    """verify_agents_SNIPS / _IPS over a device log, the likelihood agent among RandomAgent and the organic count agent, against the
    same functions on the host loop (the log as a DataFrame, the device hidden).  The tables hold means and standard errors of
    n < 2^15 non-negative float64 terms, summed by torch on one side and by NumPy on the other: each sum is within n 2^-53 relative
    of the exact one whatever its order, so the entries agree to 2^15 2^-52 < 1e-11 of the largest entry of their row."""
    P = 10
    dl, df = sim_log(P, 0.1)
    cfg = dict(num_products=P, random_seed=5, with_ps_all=True)
    agents = {'random': RandomAgent(Configuration(cfg)),
              'count': OrganicUserEventCounterAgent(Configuration({**cfg, 'weight_history_function': None, 'select_randomly': False,
                                                                   'exploit_explore': True, 'epsilon': 0.0, 'reverse_pop': False})),
              'likelihood': random_agent(P, 0.3, seed=P)}
    assert int(((dl.rows[:, 2] & _abi.RG_EV_BANDIT) != 0).sum()) < 2 ** 15
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        got = [ev.verify_agents_SNIPS(dl, agents), ev.verify_agents_IPS(dl, agents)]
        ratios = {k: ev.evaluate_SNIPS(a, dl)[1] for k, a in agents.items()}
    monkeypatch.setattr(ev, '_device_present', lambda: False)
    for k, a in agents.items():                                     # the rows behind the tables: exactly the host loop's
        assert torch.is_tensor(ratios[k])
        same(ratios[k].cpu().numpy(), ev.evaluate_SNIPS(a, df)[1])
    want = [ev.verify_agents_SNIPS(df, agents), ev.verify_agents_IPS(df, agents)]
    for g, w in zip(got, want):
        assert list(g['Agent']) == list(w['Agent']) == ['random', 'count', 'likelihood']
        gv, wv = g[['0.025', '0.500', '0.975']].to_numpy(dtype=np.float64), w[['0.025', '0.500', '0.975']].to_numpy(dtype=np.float64)
        print(gv, wv)
        assert np.all(np.abs(gv - wv) <= 1e-11 * np.abs(wv).max(axis=1, keepdims=True)) and np.all(wv[:, 1] > 0)
