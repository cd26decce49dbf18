"""Shared by the device tests of the two model replays (rg_ope_replay_nn, rg_ope_replay_bayes): agents on seeded random models,
hand-made logs with the host's act as the expectation, and the properties every replay result is held to."""
import functools

import numpy as np
import torch
from scipy.special import expit

from recogym_amd import _abi
from recogym_amd import evaluate_agent as ev
from recogym_amd.agents.bayesian_poly_vb import BayesianVBFrozenAgent
from recogym_amd.agents.nn_ips import NnIpsFrozenAgent
from recogym_amd.envs.configuration import Configuration
from recogym_amd.envs.reco_env_v1 import env_1_args
from recogym_amd.sim import DeviceLog, Simulator
from test_ope_sums_order import documented_sums

DEV = 'cuda:0'
W_CAP = {'nn': 2048, 'bayes': 3072}      # the units' wave caps (kOnMaxWaves, kObMaxWaves): part of the bits of d_sums
UNRESOLVED_SHARE = 0.05                  # above it a comparison with the host loop would compare the host with itself


def cfg(P, **kw):
    return Configuration({'num_products': P, 'random_seed': 7, 'with_ps_all': True, 'device_replay': True, **kw})


def nn_state(P, H, seed, scale=1.0):
    rng = np.random.RandomState(seed)
    f = lambda *shape: (rng.standard_normal(shape) * scale).astype(np.float32)     # noqa: E731
    return dict(w1=f(H, P), b1=f(H), w2=f(H, H), b2=f(H), w3=f(P, H), b3=f(P))


def nn_agent(P, H, seed, scale=1.0, **kw):
    return NnIpsFrozenAgent(cfg(P, **kw), nn_state(P, H, seed, scale))


def bayes_agent(P, S, seed, scale=1.0, **kw):
    return BayesianVBFrozenAgent(cfg(P, **kw), np.random.RandomState(seed).standard_normal((S, P * P)) * scale)


def unit_of(ag):
    return 'nn' if isinstance(ag, NnIpsFrozenAgent) else 'bayes'


def bayes_sparse_act(ag, prods, cnts):
    """BayesianAgentVB's act from the viewed products alone: the reference's means, the terms of the viewed products only (its
    np.kron(X, eye(P)) is a (P, P^2) float64 array: 1.1 GB per act at P = 520).  Another summation order than BLAS's, which the
    device's margin covers: a test that uses it asserts that the device resolved every act."""
    lam_t = ag.lam_t
    z = (np.asarray(cnts, dtype=np.float64)[:, None, None] * lam_t[np.asarray(prods, dtype=np.int64)]).sum(axis=0)
    return int(np.argmax(expit(z).mean(axis=1)))


def host_action(ag, prods, cnts):
    """The frozen agent's action on a history (distinct products ascending, counts)."""
    if unit_of(ag) == 'nn':
        return ag.act_on(prods, cnts)[0]
    return bayes_sparse_act(ag, prods, cnts) if ag.config.num_products > 130 else ag.act_on(prods, cnts)


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), np.nonzero(got != want)[0][:8]


def replay(ag, dl, n_users=None, **kw):
    """-> (ratio, clicks, sums, stats) as host arrays; every user of the log unless n_users says otherwise."""
    st = {}
    out = ev.ope_replay(ag, dl, n_users=int(dl.offsets.numel()) - 1 if n_users is None else n_users, stats=st, **kw)
    assert out is not None and st['error'] == 0, st
    r, c, sums = out
    return r.cpu().numpy(), c.cpu().numpy(), sums.cpu().numpy(), st


def plus_one_user(dl):
    """The log with one more (highest, hence unevaluated) user of one organic row: what the estimators expect of a device log."""
    last = torch.zeros((1, 4), dtype=torch.int32, device=dl.rows.device)
    last[0, 0] = int(dl.offsets.numel()) - 1
    ps = dl.ps if dl.ps is None or isinstance(dl.ps, float) else torch.cat([dl.ps, torch.full((1,), float('nan'), dtype=torch.float64, device=dl.ps.device)])
    return DeviceLog(torch.cat([dl.rows, last]), torch.cat([dl.offsets, dl.offsets[-1:] + 1]), ps, dl.first_user, dl.num_products, None)


@functools.lru_cache(maxsize=None)
def sim_log(P, sigma, n=300, seed=11, K=5):
    """A log of n users by the uniform logger (RandomAgent's policy) -> (DeviceLog, the same log as a DataFrame)."""
    c = Configuration({**env_1_args, 'random_seed': seed, 'num_products': P, 'K': K, 'sigma_omega': sigma})
    sim = Simulator(c, n, device=DEV)
    sim.reset_users(0, n)
    sim.run()
    dl = sim.device_log()
    df = ev._device_log_to_frame(dl)
    sim.close()
    return dl, df


def walk(dl, n_eval):
    """A numpy walk of the log's first n_eval users -> (is_bandit per row, click per row as float64, offsets, acts): an act is a
    bandit row whose history changed since the user's previous act — the row after an organic row (every user opens with one)."""
    offsets = dl.offsets[:n_eval + 1].cpu().numpy()
    total = int(offsets[-1])
    code = dl.rows[:total, 2].cpu().numpy().view(np.uint32)
    is_b = (code & _abi.RG_EV_BANDIT) != 0
    return is_b, ((code & _abi.RG_EV_CLICK) != 0).astype(np.float64), offsets, int((is_b[1:] & ~is_b[:-1]).sum())


def check_result(ag, dl, n_eval, r, sums, st, what=''):
    """What every replay result is held to: the acts are the walk's, few of them unresolved, the sums the documented order's at
    the unit's W."""
    is_b, click, offsets, acts = walk(dl, n_eval)
    print(what, st)
    assert st['acts'] == acts, (what, st, acts)
    assert st['unresolved'] <= UNRESOLVED_SHARE * max(acts, 1) and not st['overflow'], (what, st)
    ratio = np.zeros(is_b.size)
    ratio[is_b] = r
    want = documented_sums(ratio, click, is_b, offsets, W_CAP[unit_of(ag)])
    assert sums.tobytes() == want.tobytes(), (what, [x.hex() for x in sums], [x.hex() for x in want])


def build(users, ag, ps=0.25):
    """users: per user a list of tokens, ('o', product), ('o', product, times) or 'b' -> (DeviceLog, expected ratio per bandit row,
    acts).  The host walks the rows as the reference's loop does (views kept across sessions, reset per user; the act at a bandit
    row whose history changed) and writes the logged action itself: the host's action and another one, alternating — so the expected
    ratios are 1 / ps and 0, and a device action that differs from the host's shows on every row."""
    P = ag.config.num_products
    raw, offsets, want, acts, flip = [], [0], [], 0, 0
    for u, toks in enumerate(users):
        views = np.zeros(P, dtype=np.int64)
        dirty, a_host, t = True, None, 0
        for tok in toks:
            if tok == 'b':
                if dirty:
                    prods = np.flatnonzero(views)
                    a_host = host_action(ag, prods, views[prods])
                    acts += 1
                    dirty = False
                a = a_host if flip % 2 == 0 else (a_host + 1 + flip % (P - 1)) % P
                flip += 1
                want.append((1.0 if a == a_host else 0.0) / ps)
                raw.append((u, t, a | _abi.RG_EV_BANDIT | (_abi.RG_EV_CLICK if flip % 3 == 0 else 0), 0))
                t += 1
            else:
                for _ in range(tok[2] if len(tok) > 2 else 1):
                    views[tok[1]] += 1
                    raw.append((u, t, tok[1], 0))
                    t += 1
                dirty = True
        offsets.append(len(raw))
    rows = torch.from_numpy(np.array(raw, dtype=np.uint32).reshape(-1, 4).view(np.int32)).to(DEV)
    return DeviceLog(rows, torch.tensor(offsets, dtype=torch.int64, device=DEV), float(ps), 0, P, None), np.array(want), acts


def check(users, ag, what, all_resolved=False):
    """A hand-made log against the host's act.  At most UNRESOLVED_SHARE of the acts are the host's to confirm (the replay is None
    where it refutes one); all_resolved: none is."""
    dl, want, acts = build(users, ag)
    r, _, sums, st = replay(ag, dl)
    print(what, st)
    assert st['unresolved'] <= (0 if all_resolved else UNRESOLVED_SHARE * acts) and not st['overflow'], (what, st)
    same(r, want)
    assert st['acts'] == acts and sums[0] == want.size and 0 < np.count_nonzero(r) < r.size, (what, st, acts)
    return st


def distinct(n, P, seed):
    return [('o', int(p)) for p in np.random.RandomState(seed).permutation(P)[:n]]


def tier_users(P):
    """A user per history size round kPolyHist = 256 (the entries the acts cache in LDS) and the 512 entries of the LDS list (beyond:
    the per-wave global list, entered while the user is replayed): it acts at two sizes on the way up and twice at its final size;
    its first product is viewed three times."""
    users = []
    for n in (255, 256, 257, 511, 512, 513):
        v = distinct(n, P, seed=n)
        v[0] = (*v[0], 3)
        users.append(v[:n // 2] + ['b'] + v[n // 2:n - 1] + ['b'] + v[n - 1:] + ['b', 'b'])
    return users


def geometry_users(P):
    """Chunk geometry: bandit rows at lanes 0 and 63, a bandit run that continues into the next 64-row chunk with no organic row
    between, users of more than 128 rows, a user with organic rows only and one with none."""
    v = distinct(min(P, 200), P, seed=9)
    m = len(v)
    return [
        (v * 2)[:63] + ['b'] + v[:7] + ['b'],                                    # the act at lane 63 of the first chunk
        (v * 2)[:64] + ['b'] + v[:6] + ['b'],                                    # the act at lane 0 of the second chunk
        (v * 2)[:60] + ['b'] * 10 + v[:2] + ['b'],                               # one act whose run crosses into the next chunk
        (v * 2)[:30] + ['b', 'b', 'b'] + v[:10] + ['b'] + v[:5] + ['b', 'b'],    # acts in the middle of a chunk, reused by the rows after
        (v[:3] + ['b']) * 32,                                                    # 128 = 64 k rows
        (v[:3] + ['b']) * 32 + ['b'],                                            # 129 rows: the last chunk holds one reused act
        (v[:2] + ['b']) * 60,                                                    # 180 rows, three chunks
        [v[0], 'b', 'b', 'b', 'b', 'b'],                                         # one act, five rows
        [v[1 % m], 'b', v[2 % m], 'b', v[1 % m], 'b'],                           # views persist across sessions (and one counts twice)
        [v[2 % m], 'b'],                                                         # ... and are reset at the next user
        [v[0]],                                                                  # organic rows only
        [],                                                                      # a user without rows
        [('o', P - 1), 'b'],
    ]


def random_users(P, seed, n=12):
    rng = np.random.RandomState(seed)
    users = []
    for _ in range(n):
        toks = [('o', int(rng.randint(P)))]
        for _ in range(rng.randint(3, 40)):
            toks.append('b' if rng.rand() < 0.5 else ('o', int(rng.randint(P))))
        users.append(toks)
    return users


def one_act_users(n, P=10):
    """n users of one organic and one bandit row (action 0, 1 alternating), ps = 1 / P."""
    raw = np.zeros((2 * n, 4), dtype=np.uint32)
    raw[:, 0] = np.repeat(np.arange(n), 2)
    raw[1::2, 1] = 1
    raw[0::2, 2] = np.arange(n) % P
    raw[1::2, 2] = (np.arange(n) % 2).astype(np.uint32) | _abi.RG_EV_BANDIT
    return DeviceLog(torch.from_numpy(raw.view(np.int32)).to(DEV), torch.arange(0, 2 * n + 1, 2, dtype=torch.int64, device=DEV),
                     1.0 / P, 0, P, None)


def table(values, snips_ratio=None):
    """A row of verify_agents_IPS / _SNIPS / _recall_at_k from per-row values on the device: the estimators' own reductions
    (evaluate_agent._two_pass_std on a device tensor) -> (0.025, 0.500, 0.975)."""
    ee = torch.as_tensor(np.asarray(values, dtype=np.float64)).to(DEV)
    mean, std, n = ev._two_pass_std(ee)
    if snips_ratio is not None:
        mean = float((ee.sum() / torch.as_tensor(np.asarray(snips_ratio, dtype=np.float64)).to(DEV).sum()).item())
    se = std / np.sqrt(n)
    return mean - 2 * se, mean, mean + 2 * se


# ---- the scenarios both units run (the test files name the models) ---------------------------------------------------------------
def estimators_equal_the_host_loop(ag, df):
    """A DataFrame through ope_replay and the estimators: a result, no warning, the walk's acts, the host loop's numbers."""
    import warnings
    pol = ev.ope_checked_policy_of(ag)
    assert pol is not None and ev.ope_policy_of(ag) is None
    dl = ev._frame_to_device(df, pol, torch.device(DEV))
    n_eval = int(dl.offsets.numel()) - 1
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        r, c, sums, st = replay(ag, dl)
        ips = ev.evaluate_IPS(ag, df)
        rewards, ratio = ev.evaluate_SNIPS(ag, df)
    check_result(ag, dl, n_eval, r, sums, st)
    want_c, want_r = ev._host_snips(ag, df)
    same(r, want_r)
    same(ratio, want_r)
    same(rewards, np.asarray(want_c, dtype=np.float64))
    same(ips, ev._host_ips(ag, df))
    assert isinstance(ips, list) and isinstance(ratio, list) and np.count_nonzero(r) > 0
    return r, st


def sim_log_equals_the_host_loop(ag, sigma):
    dl, df = sim_log(ag.config.num_products, sigma)
    n_eval = int(dl.offsets.numel()) - 2
    r, c, sums, st = replay(ag, dl, n_eval)
    check_result(ag, dl, n_eval, r, sums, st, f'sigma {sigma}')
    rewards, want = ev._host_snips(ag, df)
    same(r, want)
    same(c, np.asarray(rewards, dtype=np.float64))
    assert 0 < np.count_nonzero(r) < r.size
    ips = ev.evaluate_IPS(ag, dl)
    assert torch.is_tensor(ips)
    same(ips.cpu().numpy(), ev._host_ips(ag, df))


def tie_stands(ag):
    """Every act of the tie model is unresolved and listed; the host confirms action 0 and the replay stands."""
    import warnings
    dl, df = sim_log(ag.config.num_products, 0.1)
    n_eval = int(dl.offsets.numel()) - 2
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        r, c, _, st = replay(ag, dl, n_eval)
        got = ev.evaluate_SNIPS(ag, dl)
    print(st)
    assert st['unresolved'] == st['acts'] == walk(dl, n_eval)[3] > 0 and not st['overflow']
    _, want = ev._host_snips(ag, df)
    same(r, want)
    assert torch.is_tensor(got[1])
    same(got[1].cpu().numpy(), want)
    a = df['a'][df['z'] == 'bandit'].to_numpy(dtype=np.float64)[:r.size]
    assert np.array_equal(r != 0, a == 0) and 0 < np.count_nonzero(r) < r.size


def refuted_takes_the_host_loop(ag, monkeypatch, host_act_name):
    """The host act disagrees with a listed act: one RuntimeWarning, no replay, the estimator equal to the host loop."""
    import pytest
    from recogym_amd import sim as sim_module
    dl, df = sim_log(ag.config.num_products, 0.1)
    monkeypatch.setattr(sim_module, host_act_name, lambda views, *a: 1)
    with pytest.warns(RuntimeWarning, match='host loop') as rec:
        assert ev.ope_replay(ag, dl) is None
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    assert 'likelihood' not in str(rec[0].message)
    with pytest.warns(RuntimeWarning, match='host loop'):
        ips = ev.evaluate_IPS(ag, dl)
    assert isinstance(ips, list)
    same(ips, ev._host_ips(ag, df))


def overflow_takes_the_host_loop(ag):
    """More one-act users under the tie model than the list holds: given up as a refuted act is; one fewer than the cap + 1 stands."""
    import warnings
    import pytest
    cap = _abi.OPE_POLY_LIST_CAP
    small = one_act_users(cap)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        r, _, _, st = replay(ag, small)
    assert st['unresolved'] == st['acts'] == cap and not st['overflow']
    same(r, np.where(np.arange(cap) % 2 == 0, 10.0, 0.0))
    dl = plus_one_user(one_act_users(cap + 104))
    st = {}
    with pytest.warns(RuntimeWarning, match='host loop') as rec:
        assert ev.ope_replay(ag, dl, stats=st) is None
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    assert st['unresolved'] == cap + 104 and st['overflow']
    with pytest.warns(RuntimeWarning, match='host loop'):
        rewards, ratio = ev.evaluate_SNIPS(ag, dl)
    same(ratio, np.where(np.arange(cap + 104) % 2 == 0, 10.0, 0.0))
    assert isinstance(ratio, list) and not any(rewards)


def shard(dl, lo, hi):
    """Users lo .. hi - 1 of a device log as a log of its own."""
    b, e = int(dl.offsets[lo].item()), int(dl.offsets[hi].item())
    ps = dl.ps if dl.ps is None or isinstance(dl.ps, float) else dl.ps[b:e].contiguous()
    return DeviceLog(dl.rows[b:e].contiguous(), (dl.offsets[lo:hi + 1] - b).contiguous(), ps, dl.first_user + lo, dl.num_products, None)


def determinism_and_both_ways_in(ag):
    dl, df = sim_log(ag.config.num_products, 0.1)
    n = int(dl.offsets.numel()) - 1
    r1, c1, s1 = ev.ope_replay(ag, dl, n_users=n)
    r2, c2, s2 = ev.ope_replay(ag, dl, n_users=n)
    assert torch.equal(r1, r2) and torch.equal(c1, c2) and s1.cpu().numpy().tobytes() == s2.cpu().numpy().tobytes()
    # a DataFrame and the DeviceLog built from it (users 0 .. max(u) - 1 on both sides)
    rewards, ratio = ev.evaluate_SNIPS(ag, df)
    c_dl, r_dl = ev.evaluate_SNIPS(ag, dl)
    assert isinstance(ratio, list) and torch.is_tensor(r_dl)
    same(ratio, r_dl.cpu().numpy())
    same(rewards, c_dl.cpu().numpy())
    assert torch.equal(r_dl, r1[:r_dl.numel()])
    # one run of n users against two shards
    k = n // 3
    ra, _, _ = ev.ope_replay(ag, shard(dl, 0, k), n_users=k)
    rb, _, _ = ev.ope_replay(ag, shard(dl, k, n), n_users=n - k)
    assert torch.equal(torch.cat([ra, rb]), r1)


def eg_form(ag, epsilon, pure_new, seed=9):
    """ope_replay under an EpsilonGreedy entry against a host restatement: the frozen agent's act_on of the views so far, the
    wrapper's addressed coin and explore_table's probability."""
    from recogym_amd import rng
    from recogym_amd.agents.epsilon_greedy import explore_table
    P = ag.config.num_products
    dl, _ = sim_log(P, 0.1)
    n_eval = int(dl.offsets.numel()) - 2
    pol = dict(ev.ope_checked_policy_of(ag), epsilon_greedy=dict(epsilon=epsilon, seed=seed, pure_new=pure_new))
    out = {}
    r, _, sums, st = replay(ag, dl, n_eval, pol=pol, eg_out=out)
    greedy, h0 = out['greedy'].cpu().numpy(), out['h0'].cpu().numpy()
    is_b, _, offsets, acts = walk(dl, n_eval)
    assert st['acts'] == acts and st['unresolved'] <= UNRESOLVED_SHARE * acts
    raw = dl.rows[:int(offsets[-1])].cpu().numpy().view(np.uint32)
    ps = 1.0 / P if isinstance(dl.ps, float) else None
    ps64 = None if ps is not None else dl.ps.cpu().numpy()
    prob, thr = explore_table(P, pure_new)[1], epsilon / (epsilon + (1.0 - epsilon))
    want_r, want_greedy, want_h0 = [], [], []
    for u in range(n_eval):
        views, g = np.zeros(P, dtype=np.int64), None
        for i in range(int(offsets[u]), int(offsets[u + 1])):
            idx = int(raw[i, 2] & _abi.RG_EV_INDEX_MASK)
            if not raw[i, 2] & _abi.RG_EV_BANDIT:
                views[idx] += 1
                g = None
                continue
            if g is None:
                g = host_action(ag, np.flatnonzero(views), views[np.flatnonzero(views)])
            explore = not (thr <= rng.policy_uniforms(seed, int(raw[i, 0]), int(raw[i, 1]))[1])
            pi = epsilon * (0.0 if pure_new and idx == g else prob) if explore else (1.0 - epsilon) * (1.0 if idx == g else 0.0)
            want_r.append(pi / (ps if ps is not None else ps64[i]))
            want_greedy.append(0 if explore else 1)
            want_h0.append(g)
    same(r, want_r)
    assert np.array_equal(greedy, np.array(want_greedy, dtype=np.uint8)) and np.array_equal(h0, np.array(want_h0, dtype=np.int32))
    if epsilon == 0.0:
        plain, _, plain_sums, _ = replay(ag, dl, n_eval)
        same(r, plain)
        assert bool((greedy == 1).all()) and sums.tobytes() == plain_sums.tobytes()
    else:
        assert 0 < int((greedy == 0).sum()) < greedy.size


def recall_and_tables(agents, monkeypatch):
    """evaluate_recall_at_k for k = 1, 5, P and the three verify_agents tables over a device log against the host loops: the rows
    bit for bit, the tables as the estimators' own reductions of the host loops' rows give them."""
    import warnings
    P = next(iter(agents.values())).config.num_products
    dl, df = sim_log(P, 0.1)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        hits = {(name, k): ev.evaluate_recall_at_k(ag, dl, k=k) for name, ag in agents.items() for k in (1, 5, P)}
        got = dict(ips=ev.verify_agents_IPS(dl, agents), snips=ev.verify_agents_SNIPS(dl, agents),
                   recall=ev.verify_agents_recall_at_k(dl, agents, k=5))
    monkeypatch.setattr(ev, '_device_present', lambda: False)
    for frame in got.values():
        assert list(frame['Agent']) == list(agents)
    for i, (name, ag) in enumerate(agents.items()):
        for k in (1, 5, P):
            want = ev._host_recall(ag, df, k)
            assert torch.is_tensor(hits[name, k]) and hits[name, k].cpu().tolist() == want and len(want) > 0, (name, k)
            assert k < P or all(want)
        rewards, ratio = ev._host_snips(ag, df)
        ips = np.asarray(ev._host_ips(ag, df), dtype=np.float64)
        want = dict(ips=table(ips), snips=table(np.asarray(rewards, dtype=np.float64) * np.asarray(ratio), snips_ratio=ratio),
                    recall=table(ev._host_recall(ag, df, 5)))
        for what, frame in got.items():
            row = tuple(float(frame[q][i]) for q in ('0.025', '0.500', '0.975'))
            assert bits(row).tolist() == bits(want[what]).tolist(), (name, what, row, want[what])
