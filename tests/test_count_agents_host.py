"""OrganicCount / BanditCount on the host against the reference's own classes (tests/golden/counts_*.npz, written by
tests/make_golden_counts.py): `train` call by call through the package's _train_from_dataframe, and the vectorised
train_from_log.  Every comparison is exact; BanditCount's `ps` is compared bit for bit."""
import json
import os

import numpy as np
import pytest

import golden_util as gu
from make_golden_counts import LOGS
from make_golden_ope import log_frame
from recogym_amd.agents import BanditCount, OrganicCount, bandit_count_args, organic_count_args
from recogym_amd.bench_agents import _train_from_dataframe
from recogym_amd.envs.configuration import Configuration
from recogym_amd.envs.context import DefaultContext
from recogym_amd.envs.observation import Observation
from recogym_amd.envs.session import OrganicSessions


def golden(name):
    z = np.load(os.path.join(gu.GOLDEN, f'counts_{name}.npz'))
    return json.loads(str(z['meta'])), z


def dense(coo, P):
    out = np.zeros((P, P))
    out[coo[0], coo[1]] = coo[2]
    return out


def agents(P, with_ps_all=False):
    return (OrganicCount(Configuration({**organic_count_args, 'num_products': P, 'with_ps_all': with_ps_all})),
            BanditCount(Configuration({**bandit_count_args, 'num_products': P, 'with_ps_all': with_ps_all})))


def check(oc, bc, name):
    meta, want = golden(name)
    P = meta['num_products']
    if oc is not None:
        co = oc.co_counts
        assert co.dtype == np.float64 and np.array_equal(co, dense(want['co'], P)), 'co_counts'
        assert np.array_equal(oc.frozen().table, want['organic_argmax']), 'organic argmax'
    if bc is not None:
        assert np.array_equal(bc.pulls_a, dense(want['pulls'], P)), 'pulls_a'
        assert np.array_equal(bc.clicks_a, dense(want['clicks'], P)), 'clicks_a'
        assert np.array_equal(bc.ctr, (dense(want['clicks'], P) + 1) / (dense(want['pulls'], P) + 2)), 'ctr'
        fz = bc.frozen()
        assert np.array_equal(fz.table, want['bandit_argmax']), 'bandit argmax'
        assert fz.ps.dtype == np.float64 and np.array_equal(fz.ps.view(np.uint64), want['bandit_ps'].view(np.uint64)), 'ps bits'
        assert bc.last_product_viewed == meta['last_product_viewed']


def test_names_and_argument_tables():
    import recogym_amd.agents as ag
    for n in ('OrganicCount', 'organic_count_args', 'BanditCount', 'bandit_count_args'):
        assert hasattr(ag, n)
    meta, _ = golden(LOGS[0])
    assert organic_count_args == meta['organic_args'] and bandit_count_args == meta['bandit_args']
    oc, bc = agents(10)
    assert oc.needs_training and bc.needs_training
    assert OrganicCount().config.num_products == 10 and BanditCount().config.num_products == 10


@pytest.mark.parametrize('name', LOGS)
def test_train_call_by_call_equals_reference(name):
    meta, cols = gu.load(name)
    oc, bc = agents(meta['env_args']['num_products'])
    df = log_frame(cols)
    _train_from_dataframe(oc, df)
    _train_from_dataframe(bc, df)
    check(oc, bc, name)


@pytest.mark.parametrize('name', LOGS)
def test_train_from_log_equals_reference(name):
    meta, cols = gu.load(name)
    oc, bc = agents(meta['env_args']['num_products'])
    df = log_frame(cols)
    oc.train_from_log(df)
    bc.train_from_log(df)
    check(oc, bc, name)


def test_fixtures_cover_the_hard_cases():
    """Organic-only users, argmax ties and all-zero rows, and the None row in every log."""
    _, cols = gu.load('philox_p10')
    u, z = cols['u'], cols['z']
    assert any(not z[u == i].any() for i in np.unique(u)[:10])
    meta, want = golden('philox_p1000_k20')
    assert meta['organic_rows_tied'] == 824
    assert (np.bincount(want['co'][0], minlength=1000) == 0).any()           # products never viewed: an all-zero row
    for name in LOGS:
        meta, want = golden(name)
        P = meta['num_products']
        pulls = dense(want['pulls'], P)
        assert (pulls.min(axis=1) >= 1).sum() >= 1, name                        # one whole row was raised by pulls_a[None, a] += 1


def _split_at_user(df, frac):
    users = df['u'].to_numpy()
    cut_user = users[int(len(users) * frac)]
    k = int(np.searchsorted(users, cut_user, side='left'))
    return df.iloc[:k].reset_index(drop=True), df.iloc[k:].reset_index(drop=True)


@pytest.mark.parametrize('name', ['philox_p10', 'philox_p1000_k20', 'mt_config1'])
def test_two_logs_and_mixed_calls_equal_one_pass(name):
    """The carried last_product_viewed, and the None row applied once only."""
    meta, cols = gu.load(name)
    P = meta['env_args']['num_products']
    df = log_frame(cols)
    first, second = _split_at_user(df, 0.4)
    assert len(first) and len(second)
    oc, bc = agents(P)
    for part in (first, second):
        oc.train_from_log(part)
        bc.train_from_log(part)
    check(oc, bc, name)
    oc, bc = agents(P)
    _train_from_dataframe(oc, first)            # train calls, then a whole log
    _train_from_dataframe(bc, first)
    oc.train_from_log(second)
    bc.train_from_log(second)
    check(oc, bc, name)
    oc, bc = agents(P)
    oc.train_from_log(first)                    # and the other way round
    bc.train_from_log(first)
    _train_from_dataframe(oc, second)
    _train_from_dataframe(bc, second)
    check(oc, bc, name)


def test_log_columns_dict_is_accepted():
    meta, cols = gu.load('philox_p10_sigma0')
    is_b = cols['z'] == 1
    log = dict(t=cols['t'].astype(np.float32), u=cols['u'].astype(np.int32), is_bandit=is_b,
               v=np.where(is_b, 0, cols['v']).astype(np.int32), a=np.where(is_b, cols['a'], 0).astype(np.int32),
               c=np.where(is_b, cols['c'], np.nan).astype(np.float32), ps=np.where(is_b, cols['ps'], np.nan))
    oc, bc = agents(meta['env_args']['num_products'])
    oc.train_from_log(log)
    bc.train_from_log(log)
    check(oc, bc, 'philox_p10_sigma0')


def _obs(last_view):
    s = OrganicSessions()
    s.next(DefaultContext(3, 7), last_view)
    return Observation(DefaultContext(4, 7), s)


@pytest.mark.parametrize('name', LOGS)
def test_act_equals_reference(name):
    meta, cols = gu.load(name)
    P = meta['env_args']['num_products']
    _, want = golden(name)
    for with_ps_all in (False, True):
        oc, bc = agents(P, with_ps_all)
        df = log_frame(cols)
        oc.train_from_log(df)
        bc.train_from_log(df)
        for l, oa, ops, oarg, ba, bps in want['acts']:
            ao, ab = oc.act(_obs(int(l)), 0, False), bc.act(_obs(int(l)), 0, False)
            assert sorted(ao) == sorted(ab) == ['a', 'ps', 'ps-a', 't', 'u']
            assert (ao['t'], ao['u']) == (4, 7)
            assert ao['a'] == int(oa) and ao['ps'] == ops == 1.0
            assert ab['a'] == int(ba) and np.float64(ab['ps']).view(np.uint64) == np.float64(bps).view(np.uint64)
            for d, a in ((ao, int(oa)), (ab, int(ba))):
                if with_ps_all:
                    assert d['ps-a'].shape == (P,) and d['ps-a'][a] == 1.0 and d['ps-a'].sum() == 1.0
                else:
                    assert d['ps-a'] == ()
        # an observation without a session keeps the last view
        assert oc.act(Observation(DefaultContext(5, 7), OrganicSessions()), 0, False)['a'] == int(want['acts'][-1][1])
        assert (oc.ope_policy() is not None) == with_ps_all and (oc.device_policy() is None) == with_ps_all


def test_save_load_round_trip(tmp_path):
    meta, cols = gu.load('philox_p10')
    _, bc = agents(10)
    bc.train_from_log(log_frame(cols))
    loc = str(tmp_path) + os.sep
    bc.save(loc)
    assert sorted(os.listdir(tmp_path)) == ['clicks_a.npy', 'pulls_a.npy']
    assert np.load(loc + 'pulls_a.npy').dtype == np.float64
    _, other = agents(10)
    other.load(loc)
    assert np.array_equal(other.pulls_a, bc.pulls_a) and np.array_equal(other.clicks_a, bc.clicks_a)
    assert np.array_equal(other.frozen().table, bc.frozen().table)
    assert np.array_equal(other.frozen().ps, bc.frozen().ps)


def test_frozen_table_is_rebuilt_only_after_training():
    meta, cols = gu.load('philox_p10')
    oc, bc = agents(10)
    df = log_frame(cols)
    oc.train_from_log(df)
    bc.train_from_log(df)
    fo, fb = oc.frozen(), bc.frozen()
    oc.act(_obs(1), 0, False)
    bc.act(_obs(1), 0, False)
    assert oc.frozen() is fo and bc.frozen() is fb
    oc.train(_obs(2), None, None, True)
    bc.train(_obs(2), {'a': 3}, 1, False)
    assert oc.frozen() is not fo and bc.frozen() is not fb


def test_sparse_host_tables_keep_large_catalogues_cheap():
    """P = 10^4: training touches a few cells; the dense 0.8 GB array is only built when asked for."""
    P = 10000
    oc, bc = agents(P)
    rng = np.random.RandomState(0)
    n = 4000
    u = np.repeat(np.arange(n // 8), 8)
    is_b = np.tile(np.array([0, 0, 1, 1, 0, 1, 0, 1], dtype=bool), n // 8)
    idx = rng.randint(0, P, size=n)
    log = dict(t=np.tile(np.arange(8), n // 8).astype(np.float32), u=u.astype(np.int32), is_bandit=is_b,
               v=np.where(is_b, 0, idx).astype(np.int32), a=np.where(is_b, idx, 0).astype(np.int32),
               c=np.where(is_b, rng.rand(n) < 0.3, np.nan).astype(np.float32), ps=np.where(is_b, 1.0 / P, np.nan))
    oc.train_from_log(log)
    bc.train_from_log(log)
    r, c, v = oc._co.coo()
    assert v.sum() == (n // 8) * (4 + 1 + 1)                     # sessions of 2, 1 and 1 views
    pr, pc, pv = bc._pulls.coo()
    assert pv.sum() == is_b.sum() + (P - 1)                       # every bandit row once, the None row P times
    assert oc.frozen().table.shape == (P,) and bc.frozen().ps.shape == (P,)


def test_table_too_large_is_an_error():
    oc, _ = agents(100000)
    with pytest.raises(MemoryError, match='GiB'):
        oc.co_counts
