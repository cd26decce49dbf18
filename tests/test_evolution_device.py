"""The exploration study on the device: rg_evolution_stats against the reference's EpsilonGreedy logs and NumPy,
rg_count_train_online against the NumPy form on synthetic logs, evaluate_agent's device route against the fixtures recorded from
the reference's own evaluate_agent (tests/make_golden_evolution.py) and against the host route, and the error paths.  Every
comparison is exact integer equality."""
import ctypes as C

import numpy as np
import pytest
import torch

import eg_util as eu
import golden_util as gu
import recogym_amd as recogym
from recogym_amd import _abi
from recogym_amd import evaluate_agent as ev
from recogym_amd.agents import BanditCount, EpsilonGreedy, OrganicCount, bandit_count_args, epsilon_greedy_args, organic_count_args
from recogym_amd.agents import count_tables as ct
from recogym_amd.constants import EvolutionCase, TrainingApproach
from recogym_amd.envs.configuration import Configuration

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EVO = gu.fixtures('evo_')


# ----------------------------------------------------------------------------------------------------------
# rg_evolution_stats
# ----------------------------------------------------------------------------------------------------------
def eg_device_log(cols, P):
    is_b = cols['z'] == 1
    return ct.columns_to_device_log(cols['u'].astype(np.int64), is_b, np.where(is_b, 0, cols['v']).astype(np.int64),
                                    np.where(is_b, cols['a'], 0).astype(np.int64), is_b & (cols['c'] == 1), P, torch.device(DEV),
                                    t=cols['t'])


@pytest.mark.parametrize('name', eu.LOG_FIXTURES)
def test_stats_equal_the_reference_greedy_column_and_numpy(name):
    meta, cols, P = eu.load(name)
    eg = dict(epsilon=meta['eg_args']['epsilon'], seed=meta['eg_args']['random_seed'])
    is_b = cols['z'] == 1
    dl = eg_device_log(cols, P)
    counts, clicks, explored = ev.evolution_stats_device(dl, eg)
    want = ev.evolution_stats(cols['u'], cols['t'], is_b, np.where(is_b, cols['a'], 0), cols['c'] == 1, P, greedy=cols['greedy'])
    assert np.array_equal(explored.cpu().numpy() != 0, is_b & (cols['greedy'] == 0))         # the fixture's `greedy`, inverted
    assert np.array_equal(counts.cpu().numpy(), want[0]) and counts[:2].sum().item() == is_b.sum()
    assert np.array_equal(clicks.cpu().numpy(), want[1])
    # a second run: the same bytes, and the sums are ADDED to the arrays handed in
    counts2, clicks2, explored2 = ev.evolution_stats_device(dl, eg, counts=counts.clone(), action_clicks=clicks.clone())
    assert torch.equal(counts2, 2 * counts) and torch.equal(clicks2, 2 * clicks) and torch.equal(explored2, explored)
    # no wrapper: no act is greedy, none explored
    counts0, clicks0, explored0 = ev.evolution_stats_device(dl, None)
    assert counts0.cpu().tolist() == [int(want[0][0]), int(want[0][1]), 0, 0]
    assert torch.equal(clicks0, clicks) and not explored0.any()


def test_stats_skip_phantom_rows_and_empty_users():
    u = np.array([3, 3, 3, 5, 5, 9, 9, 9])
    is_b = np.array([0, 1, 1, 0, 1, 0, 0, 1], dtype=bool)
    a = np.array([0, 2, 1, 0, 2, 0, 0, 0])
    click = np.array([0, 1, 0, 0, 1, 0, 0, 1], dtype=bool)
    phantom = np.array([0, 0, 1, 0, 0, 0, 0, 1], dtype=bool)
    dl = ct.columns_to_device_log(u, is_b, np.zeros(8, dtype=np.int64), a, click, 3, torch.device(DEV), t=np.arange(8), phantom=phantom)
    counts, clicks, explored = ev.evolution_stats_device(dl, dict(epsilon=0.0, seed=1))
    assert counts.cpu().tolist() == [2, 0, 2, 0] and clicks.cpu().tolist() == [0, 0, 2] and not explored.any()
    counts, clicks, explored = ev.evolution_stats_device(dl, dict(epsilon=1.0, seed=1))
    assert counts.cpu().tolist() == [2, 0, 0, 0] and explored.cpu().tolist() == [0, 1, 0, 0, 1, 0, 0, 0]


# ----------------------------------------------------------------------------------------------------------
# rg_count_train_online against the NumPy form
# ----------------------------------------------------------------------------------------------------------
def synthetic_log(P, seed, n_users=300, clean=False):
    """Columns of a log of about `n_users` users: users without a bandit row, users of 64, 65 and 129 rows (chunk boundaries),
    at P > 64 a session of more than 64 distinct products, phantom-flagged last rows and trailing organic rows.  `clean`: every
    user ends in a bandit row that is no phantom row (the log rg_count_train reads the same way)."""
    r = np.random.RandomState(seed)
    u, is_b, idx, click, phantom = [], [], [], [], []
    for uid in range(n_users):
        n = {5: 64, 6: 65, 7: 129}.get(uid, int(r.randint(1, 24)))
        zb = r.random_sample(n) < 0.45
        zb[0] = False
        if uid == 8 and P > 64:
            n = 100
            zb = np.zeros(n, dtype=bool)
            zb[80] = zb[99] = True
        if uid % 11 == 3 and not clean:
            zb[:] = False                                   # an organic-only user
        ph = np.zeros(n, dtype=bool)
        if clean:
            zb[-1] = True
            if n == 1:
                n, zb, ph = 2, np.array([False, True]), np.zeros(2, dtype=bool)
        elif zb[-1] and uid % 3:
            ph[-1] = True                                   # (the others end in trailing organic rows or a plain bandit row)
        ix = r.randint(0, P, size=n)
        if uid == 8 and P > 64:
            ix[:80] = r.permutation(P)[:80]
        u += [uid + 1000] * n
        is_b += zb.tolist()
        idx += ix.tolist()
        click += (zb & (r.random_sample(n) < 0.3)).tolist()
        phantom += ph.tolist()
    u, is_b, idx = np.array(u, dtype=np.int64), np.array(is_b, dtype=bool), np.array(idx, dtype=np.int64)
    return dict(u=u, is_b=is_b, v=np.where(is_b, 0, idx), a=np.where(is_b, idx, 0), click=np.array(click, dtype=bool),
                phantom=np.array(phantom, dtype=bool))


def to_device(log, P):
    return ct.columns_to_device_log(log['u'], log['is_b'], log['v'], log['a'], log['click'], P, torch.device(DEV), phantom=log['phantom'])


def column_dict(log):
    n = len(log['u'])
    return dict(u=log['u'].astype(np.int32), is_bandit=log['is_b'], v=log['v'], a=log['a'], c=np.where(log['is_b'], log['click'], np.nan),
                ps=np.full(n, np.nan), phantom=log['phantom'])


def masks(log):
    """name -> mask (one entry per row, or None)."""
    r = np.random.RandomState(5)
    n = len(log['u'])
    counted = log['is_b'] & ~log['phantom']
    nth = np.zeros(n, dtype=bool)
    nth[np.flatnonzero(counted)[6::7]] = True
    after_bandit = np.r_[False, log['is_b'][:-1] & (log['u'][1:] == log['u'][:-1])]
    early = np.arange(n) < n // 3
    users = log['u'] - log['u'].min()
    return {'null': None, 'zeros': np.zeros(n, dtype=bool), 'ones': np.ones(n, dtype=bool), 'every_7th': nth, 'random_5pct': r.random_sample(n) < 0.05,
            # the first counted rows have empty sessions: last_product_viewed stays None over several rows
            'none_rows': np.where(early, after_bandit, True),
            # no counted row over more than 200 consecutive users: last_product_viewed crosses the stretch
            'gap_200_users': (users < 40) | (users >= 250)}


def host_train(log, P, mask, carry=None, agents=None):
    oc, bc = agents or (OrganicCount(Configuration({**organic_count_args, 'num_products': P})),
                        BanditCount(Configuration({**bandit_count_args, 'num_products': P})))
    if agents is None:
        bc.last_product_viewed = carry
    oc.train_online_from_log(column_dict(log), mask)
    bc.train_online_from_log(column_dict(log), mask)
    return oc, bc


def device_train(dl, P, mask, carry=None, tables=None):
    dev = torch.device(DEV)
    co, pulls, clicks = tables or [torch.zeros((P, P), dtype=torch.int64, device=dev) for _ in range(3)]
    m = None if mask is None else torch.from_numpy(mask).to(dev)
    new_carry, stats = ct.count_train_online(dl, P, co=co, pulls=pulls, clicks=clicks, carry=carry, mask=m)
    return (co, pulls, clicks), new_carry, stats


def assert_same(tables, carry, oc, bc, what):
    assert np.array_equal(tables[0].cpu().numpy(), oc.co_counts.astype(np.int64)), f'{what}: co_counts'
    assert np.array_equal(tables[1].cpu().numpy(), bc.pulls_a.astype(np.int64)), f'{what}: pulls'
    assert np.array_equal(tables[2].cpu().numpy(), bc.clicks_a.astype(np.int64)), f'{what}: clicks'
    assert carry == bc.last_product_viewed, f'{what}: carry'


@pytest.mark.parametrize('P', [2, 10, 257])
def test_online_training_equals_numpy_under_every_mask(P):
    log = synthetic_log(P, seed=P)
    dl = to_device(log, P)
    assert (~log['is_b'][np.r_[log['u'][1:] != log['u'][:-1], True]]).any() and log['phantom'].any()
    for name, mask in masks(log).items():
        for carry in (None, 1):
            tables, new_carry, stats = device_train(dl, P, mask, carry)
            oc, bc = host_train(log, P, mask, carry)
            assert_same(tables, new_carry, oc, bc, f'{name} carry {carry}')
            if name == 'zeros':
                assert not any(t.any() for t in tables) and new_carry == carry and stats['updates'] == 0
            if name == 'none_rows' and carry is None:
                counted = ct.counted_rows(log['is_b'], log['phantom'], mask)
                ix = ct.online_bandit_updates(log['u'], log['is_b'], log['v'], log['a'], log['click'], P, counted, None)[0]
                assert (ix < 0).sum() >= 3                        # several rows met None
    if P == 257:
        s = np.flatnonzero(log['u'] == 1008)
        assert len(np.unique(log['v'][s[:80]])) > 64              # the pairwise form ran


def test_two_logs_chained_through_the_carry_equal_one_log():
    P = 10
    a, b = synthetic_log(P, seed=21, n_users=120), synthetic_log(P, seed=22, n_users=90)
    b['u'] = b['u'] + 1000
    both = {k: np.concatenate([a[k], b[k]]) for k in a}
    for name in ('null', 'random_5pct', 'every_7th'):
        ma, mb = masks(a)[name], masks(b)[name]
        tables, carry, _ = device_train(to_device(a, P), P, ma)
        tables, carry, _ = device_train(to_device(b, P), P, mb, carry, tables)
        whole, carry_whole, _ = device_train(to_device(both, P), P, None if ma is None else np.concatenate([ma, mb]))
        assert all(torch.equal(x, y) for x, y in zip(tables, whole)) and carry == carry_whole, name
        oc, bc = host_train(a, P, ma)
        oc, bc = host_train(b, P, mb, agents=(oc, bc))
        assert_same(tables, carry, oc, bc, name)


@pytest.mark.parametrize('P', [10, 257])
def test_null_mask_on_a_clean_log_equals_rg_count_train(P):
    log = synthetic_log(P, seed=40 + P, clean=True)
    assert not log['phantom'].any() and log['is_b'][np.r_[log['u'][1:] != log['u'][:-1], True]].all()
    dl = to_device(log, P)
    for carry in (None, 1):
        tables, new_carry, _ = device_train(dl, P, None, carry)
        want = [torch.zeros((P, P), dtype=torch.int64, device=DEV) for _ in range(3)]
        want_carry, _ = ct.count_train(dl, P, co=want[0], pulls=want[1], clicks=want[2], carry=carry)
        assert all(torch.equal(x, y) for x, y in zip(tables, want)) and new_carry == want_carry


# ----------------------------------------------------------------------------------------------------------
# evaluate_agent
# ----------------------------------------------------------------------------------------------------------
def study(meta):
    P = meta['env_args']['num_products']
    env = recogym.make('reco-gym-v1')
    env.init_gym(dict(meta['env_args']))
    if meta['agent'] == 'oc':
        agent = OrganicCount(Configuration({**organic_count_args, 'num_products': P}))
    else:
        agent = BanditCount(Configuration({**bandit_count_args, 'num_products': P}))
    if meta['eg_args'] is not None:
        agent = EpsilonGreedy(Configuration({**epsilon_greedy_args, **meta['eg_args'], 'num_products': P}), agent)
    return env, agent, (meta['n_init'], meta['n_step_users'], meta['num_steps'], TrainingApproach[meta['approach']], meta['window'])


def final_tables(meta, cols):
    P = meta['env_args']['num_products']
    out = {}
    for tab in ('co_counts', 'pulls_a', 'clicks_a'):
        if tab in cols:
            out[tab] = cols[tab][-1]
        elif tab + '_coo' in cols:
            coo = cols[tab + '_coo']
            coo = coo[coo[:, 0] == meta['num_steps']]
            out[tab] = np.zeros((P, P), dtype=np.int64)
            out[tab][coo[:, 1], coo[:, 2]] = coo[:, 3]
    return out


def assert_study(rewards, last, meta, cols, what):
    for key, col in ((EvolutionCase.SUCCESS, 'success'), (EvolutionCase.SUCCESS_GREEDY, 'success_greedy'),
                     (EvolutionCase.FAILURE, 'failure'), (EvolutionCase.FAILURE_GREEDY, 'failure_greedy')):
        assert rewards[key] == cols[col].tolist(), f'{what}: {col}'
    assert [rewards[EvolutionCase.ACTIONS][a] for a in range(meta['env_args']['num_products'])] == cols['actions'].tolist(), what
    inner = last.agent if isinstance(last, EpsilonGreedy) else last
    for tab, value in final_tables(meta, cols).items():
        assert np.array_equal(getattr(inner, tab), value.astype(np.float64)), f'{what}: {tab}'
    lpv = inner.last_product_viewed
    assert (-1 if lpv is None else lpv) == cols['lpv'][-1], f'{what}: last_product_viewed'


@pytest.mark.parametrize('name', EVO)
def test_device_route_reproduces_the_reference(name):
    meta, cols = gu.load(name)
    env, agent, args = study(meta)
    assert ev._device_route(env, agent)
    rewards, last = ev.evolve(env, agent, *args)
    assert_study(rewards, last, meta, cols, name)
    inner = last.agent if isinstance(last, EpsilonGreedy) else last
    assert all(t.dev is not None for t in ([inner._co] if meta['agent'] == 'oc' else [inner._pulls, inner._clicks]))   # trained where the log is
    env.close()


def test_host_route_equals_the_device_route_and_the_reference():
    name = 'evo_bc_slide_explore3'
    meta, cols = gu.load(name)
    env, agent, args = study(meta)
    rewards, last = ev.evolve(env, agent, *args, route='host')
    assert_study(rewards, last, meta, cols, name + ' (host)')
    env2, agent2, _ = study(meta)
    assert recogym.evaluate_agent(env2, agent2, *args) == rewards            # the public call, on the device route
    env.close()
    env2.close()


# ----------------------------------------------------------------------------------------------------------
# argument errors: nothing is written
# ----------------------------------------------------------------------------------------------------------
def _raw_online(tabs, dl, n_users, carry, ws, ws_bytes):
    lib = _abi.load()
    stream = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    return lib.rg_count_train_online(C.byref(tabs), dl.rows.data_ptr(), dl.offsets.data_ptr(), n_users, None, carry.data_ptr(),
                                     ws.data_ptr(), ws_bytes, stream)


def test_errors_write_nothing():
    lib = _abi.load()
    P = 4
    dev = torch.device(DEV)
    good = dict(u=np.array([1, 1, 2, 2, 2]), is_b=np.array([0, 1, 0, 0, 1], dtype=bool), v=np.array([1, 0, 2, 3, 0]),
                a=np.array([0, 2, 0, 0, 3]), click=np.array([0, 1, 0, 0, 0], dtype=bool), phantom=np.zeros(5, dtype=bool))
    first_bandit = dict(good, is_b=np.array([0, 1, 1, 0, 1], dtype=bool))             # user 2 opens with a bandit row
    too_large = dict(good, v=np.array([1, 0, 2, 4, 0]))                               # a view of product P
    tables = [torch.full((P, P), 7, dtype=torch.int64, device=dev) for _ in range(3)]
    tabs = _abi.RgCountTables(num_products=P, reserved=0, co_counts=tables[0].data_ptr(), pulls=tables[1].data_ptr(), clicks=tables[2].data_ptr())
    need = lib.rg_count_online_workspace_bytes(P, 2)
    ws = torch.zeros(need // 8 + 1, dtype=torch.int64, device=dev)
    carry = torch.tensor([2], dtype=torch.int64, device=dev)
    counts = torch.full((4,), 5, dtype=torch.int64, device=dev)
    clicks = torch.full((P,), 5, dtype=torch.int64, device=dev)

    def untouched():
        torch.cuda.synchronize()
        return all((t == 7).all().item() for t in tables) and carry.item() == 2 and (counts == 5).all().item() and (clicks == 5).all().item()

    for bad, what in ((first_bandit, 'opens with a bandit row'), (too_large, '>= num_products')):
        dl = to_device(bad, P)
        assert _raw_online(tabs, dl, 2, carry, ws, need) == -1 and what in lib.rg_last_error().decode()          # RG_EINVAL
        with pytest.raises(_abi.RecoGymHipError, match='RG_EINVAL'):
            ev.evolution_stats_device(dl, dict(epsilon=0.3, seed=1), counts=counts, action_clicks=clicks)
        assert what in lib.rg_last_error().decode() and untouched()
    dl = to_device(good, P)
    half = _abi.RgCountTables(num_products=P, reserved=0, co_counts=None, pulls=tables[1].data_ptr(), clicks=None)
    assert _raw_online(half, dl, 2, carry, ws, need) == -1 and 'come together' in lib.rg_last_error().decode() and untouched()
    assert _raw_online(tabs, dl, 2, carry, ws, need - 8) == -3 and untouched()                                   # RG_ENOMEM
    for eps in (-0.1, 1.5, float('nan')):
        with pytest.raises(_abi.RecoGymHipError, match='RG_EINVAL.*epsilon'):
            ev.evolution_stats_device(dl, dict(epsilon=eps, seed=1), counts=counts, action_clicks=clicks)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    short = lib.rg_evolution_workspace_bytes(P) - 8
    assert lib.rg_evolution_stats(None, dl.rows.data_ptr(), dl.offsets.data_ptr(), 2, P, None, counts.data_ptr(), clicks.data_ptr(),
                                  ws.data_ptr(), short, stream) == -3
    assert untouched()
    # and the same log, valid, is counted
    assert _raw_online(tabs, dl, 2, carry, ws, need) == 0
    torch.cuda.synchronize()
    assert carry.item() == 3 and tables[0].sum().item() == 7 * P * P + 1 + 4 and tables[1].sum().item() == 7 * P * P + 2


def test_exploration_approach_over_a_plain_agent_raises_key_error():
    meta, cols = gu.load('evo_oc_plain')
    env, agent, args = study(meta)
    with pytest.raises(KeyError, match='greedy'):
        ev.evolve(env, agent, args[0], args[1], 1, TrainingApproach.ALL_EXPLORATION_DATA, 10000)
    env.close()


# ----------------------------------------------------------------------------------------------------------
# the two gather_* wrappers
# ----------------------------------------------------------------------------------------------------------
def test_gather_exploration_stats_is_evaluate_agent_per_epsilon():
    from recogym_amd.constants import AgentStats
    meta, _ = gu.load('evo_oc_all')
    env_args = dict(meta['env_args'])
    env = recogym.make('reco-gym-v1')
    env.init_gym(env_args)
    init = recogym.build_agent_init('Organic', OrganicCount, {**organic_count_args})
    extra = {'random_seed': 77}
    stats = recogym.gather_exploration_stats(env, env_args, extra, init, TrainingApproach.ALL_EXPLORATION_DATA, num_initial_train_users=5,
                                             num_step_users=6, epsilons=(0.0, 0.3), num_evolution_steps=2)
    assert list(stats) == ['Organic'] and list(stats['Organic']) == ['0.00', '0.30']
    for eps in (0.0, 0.3):
        env2 = recogym.make('reco-gym-v1')
        env2.init_gym({**env_args, **extra})
        agent = EpsilonGreedy(Configuration({**epsilon_greedy_args, **env_args, **extra, 'epsilon': eps}),
                              OrganicCount(Configuration({**organic_count_args, **env_args, **extra})))
        want = recogym.evaluate_agent(env2, agent, 5, 6, 2, TrainingApproach.ALL_EXPLORATION_DATA)
        assert stats['Organic'][ev.format_epsilon(eps)] == want
        env2.close()
    zero = stats['Organic']['0.00']
    assert zero[EvolutionCase.SUCCESS] == zero[EvolutionCase.SUCCESS_GREEDY] and zero[EvolutionCase.FAILURE] == zero[EvolutionCase.FAILURE_GREEDY]
    # gather_agent_stats: test_agent per sample size
    got = recogym.gather_agent_stats(env, env_args, extra, init, user_samples=(5, 9), num_online_users=8, num_organic_offline_users=2)
    assert got[AgentStats.SAMPLES] == (5, 9) and list(got[AgentStats.AGENTS]) == ['Organic']
    env3 = recogym.make('reco-gym-v1')
    env3.init_gym({**env_args, **extra})
    for k, n in enumerate((5, 9)):
        q500, q025, q975 = recogym.test_agent(env3, OrganicCount(Configuration({**organic_count_args, **env_args, **extra})), n, 8, 2)
        row = got[AgentStats.AGENTS]['Organic']
        assert (row[AgentStats.Q0_500][k], row[AgentStats.Q0_025][k], row[AgentStats.Q0_975][k]) == (q500, q025, q975)
    env.close()
    env3.close()


# ----------------------------------------------------------------------------------------------------------
# many users: the scan across tiles of 2 048 users, and the grid-stride loops (more users than waves)
# ----------------------------------------------------------------------------------------------------------
TILE = 2048          # kOnlTile of rg_evolve.hip


def many_short_users(n_users=140_000, P=10, seed=9):
    """Users of one row (organic), two rows (organic, bandit) or three (organic, bandit, bandit), mostly two: n_users / 2 048
    = 69 tiles of the user scan, more than the 64 one pass of its middle kernel takes, and 27 users per wave."""
    r = np.random.RandomState(seed)
    n = r.choice([1, 2, 3], size=n_users, p=[0.1, 0.8, 0.1])
    u = np.repeat(np.arange(n_users, dtype=np.int64) + 7, n)
    first = np.r_[True, u[1:] != u[:-1]]
    is_b = ~first
    idx = r.randint(0, P, size=len(u)).astype(np.int64)
    return dict(u=u, is_b=is_b, v=np.where(is_b, 0, idx), a=np.where(is_b, idx, 0), click=is_b & (r.random_sample(len(u)) < 0.3),
                phantom=is_b & np.r_[first[1:], True] & (r.random_sample(len(u)) < 0.2))


def test_online_training_across_tiles_of_the_user_scan():
    P = 10
    log = many_short_users(P=P)
    users = log['u'] - log['u'].min()
    n_users = int(users.max()) + 1
    assert n_users > 64 * TILE + TILE
    dl = to_device(log, P)
    # counted rows more than a whole tile apart, in the first tile, past tile 64 and in the last one; then two denser masks
    picked = np.array([5, TILE + 952, 4 * TILE + 808, 66 * TILE + 7, n_users - 3])
    with_session = log['is_b'] & ~log['phantom'] & np.r_[False, ~log['is_b'][:-1]]
    far = np.isin(users, picked) & with_session
    tiles = np.unique(users[far] // TILE)
    assert len(tiles) >= 4 and np.diff(tiles).max() >= 62 and (np.diff(tiles) >= 2).sum() >= 2 and tiles[-1] == (n_users - 1) // TILE
    r = np.random.RandomState(3)
    sparse = (users % 4099 == 17) | (r.random_sample(len(users)) < 0.0002)
    for name, mask in (('far', far), ('sparse', sparse), ('random_5pct', r.random_sample(len(users)) < 0.05), ('null', None)):
        for carry in (None, 3):
            tables, new_carry, _ = device_train(dl, P, mask, carry)
            oc, bc = host_train(log, P, mask, carry)
            assert_same(tables, new_carry, oc, bc, f'{name} carry {carry}')
    # under `far` every counted row but the first takes its ix from a counted row in an earlier tile
    ix = ct.online_bandit_updates(log['u'], log['is_b'], log['v'], log['a'], log['click'], P, ct.counted_rows(log['is_b'], log['phantom'], far), None)[0]
    assert (ix < 0).sum() == 1 and len(ix) >= 4


def test_stats_over_more_users_than_waves():
    P = 600                                                        # the global-memory histogram
    log = many_short_users(n_users=30_000, P=P, seed=11)
    dl = ct.columns_to_device_log(log['u'], log['is_b'], log['v'], log['a'], log['click'], P, torch.device(DEV),
                                  t=np.arange(len(log['u'])) % 3, phantom=log['phantom'])
    act = log['is_b'] & ~log['phantom']
    for eps, greedy in ((0.0, act), (1.0, np.zeros(len(act), dtype=bool))):
        counts, clicks, explored = ev.evolution_stats_device(dl, dict(epsilon=eps, seed=5))
        want = ev.evolution_stats(log['u'], None, log['is_b'], log['a'], log['click'], P, phantom=log['phantom'], greedy=greedy)
        assert np.array_equal(counts.cpu().numpy(), want[0]) and np.array_equal(clicks.cpu().numpy(), want[1])
        assert np.array_equal(explored.cpu().numpy() != 0, want[2])


def test_a_carry_beyond_the_tables_is_refused():
    P = 4
    log = dict(u=np.array([1, 1]), is_b=np.array([0, 1], dtype=bool), v=np.array([1, 0]), a=np.array([0, 2]),
               click=np.array([0, 1], dtype=bool), phantom=np.zeros(2, dtype=bool))
    dl = to_device(log, P)
    tables = [torch.zeros((P, P), dtype=torch.int64, device=DEV) for _ in range(3)]
    for carry in (P, P + 100):
        with pytest.raises(_abi.RecoGymHipError, match='RG_EINVAL.*d_carry'):
            device_train(dl, P, None, carry, tables)
        assert not any(t.any() for t in tables)
    _, new_carry, _ = device_train(dl, P, None, P - 1, tables)
    assert new_carry == 1 and tables[1][P - 1, 2].item() == 1 and tables[0].sum().item() == 1      # OrganicCount needs no carry
