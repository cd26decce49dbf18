"""Self-check of tests/history_model.py on the CPU: with room for every product and no presets the capped model IS the oracle
(its own generate_logs, bit for bit, ps included), and the capacity references are well posed (most users meet their row's
capacity) — so that the GPU tests that hold the device against the model hold it against the oracle's arithmetic."""
import numpy as np
import pytest

import history_model as hm
from recogym_amd import _abi

COLS = ('u', 't', 'z', 'v', 'a', 'c', 'phantom')


def assert_same_rows(got, want):
    assert len(got) == len(want)
    for k in COLS:
        assert np.array_equal(got[k].astype(np.int64), want[k].astype(np.int64)), k
    assert np.array_equal(got['ps'], want['ps'], equal_nan=True)               # the same float64, not merely close


@pytest.mark.parametrize('sigma_omega', [0.0, 0.1])
def test_uncapped_model_is_the_oracle(sigma_omega):
    from oracle import oracle as orc
    n = 256
    cfg = hm.config(hm.P_CAP, 7102, sigma_omega)
    env = orc.OracleEnv(cfg, rng_mode=orc.RNG_PHILOX, **hm.POL)
    want = env.generate_logs(n)
    rows, dropped, users_dropped, final = hm.capped_model(cfg, n, keep=hm.P_CAP)
    assert_same_rows(rows, want)
    assert dropped == users_dropped == 0
    assert hm.counters_of(rows, n) == env.counters()
    # the final histories are the distinct products of each user's organic rows, with their multiplicities
    org = want[want['z'] == 0]
    for user in (0, 17, n - 1):
        prods, counts = np.unique(org['v'][org['u'] == user], return_counts=True)
        assert np.array_equal(final[user][0], prods) and np.array_equal(final[user][1], counts)


def test_uncapped_logreg_model_is_the_oracle():
    """the second act: the dyadic model's exact scores, against the oracle's CSR-ordered sums"""
    from oracle import oracle as orc
    n, P = 96, 200                          # (the oracle scores every class against every product: a small table)
    cfg = hm.config(P, 7102, 0.1)
    lr = hm.dyadic_logreg(P)
    pol = dict(policy=_abi.RG_POLICY_LOGREG_FROZEN, policy_seed=0)
    want = orc.OracleEnv(cfg, rng_mode=orc.RNG_PHILOX, logreg=lr, **pol).generate_logs(n)
    rows = hm.capped_model(cfg, n, keep=P, pol=pol, logreg=lr)[0]
    assert_same_rows(rows, want)
    assert len(np.unique(rows['a'][rows['z'] == 1])) > 20                      # (the act follows the history)


def test_capacity_table():
    assert {c: hm.hist_cap_of(c) for c in hm.HIST_CAP_TABLE} == hm.HIST_CAP_TABLE


def test_capped_model_drops_views_and_then_acts_on_the_kept_counts():
    """keep = 15 on the capacity shape: users overflow, no final history exceeds keep, a history that started full still holds
    exactly its preset products, and every logged action is a kept product (the policy never sees a dropped view)."""
    ref = hm.capacity_reference(0.0, 15)
    assert ref.keep == 15 and ref.users_dropped >= ref.n // 4 and ref.dropped >= 1000
    assert all((ref.nd == k).sum() > 100 for k in ref.classes)
    assert max(len(f[0]) for f in ref.final) == 15
    rows = ref.rows
    for user in np.flatnonzero(ref.nd == 15)[:20]:
        assert np.array_equal(ref.final[user][0], ref.prod[user, :15])
        acts = rows['a'][(rows['u'] == user) & (rows['z'] == 1)]
        assert np.isin(acts, ref.prod[user, :15]).all()
        views = rows['v'][(rows['u'] == user) & (rows['z'] == 0)]
        assert ref.final[user][1].sum() == ref.cnt[user, :15].sum() + np.isin(views, ref.prod[user, :15]).sum()
