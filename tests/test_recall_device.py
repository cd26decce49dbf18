"""recall@k on the device (rg_ope_recall_hits, recogym_amd/csrc/rg_ope_recall.hip; rg_ope_recall_logreg, the ranking instantiation
of rg_ope_logreg.hip's kernel) against the reference's own numbers (tests/golden/ope_*.npz: `{key}__recall`, k = 5) and against the
host loop, whose hits every comparison here equals exactly.  Needs a real MI355X."""
import json
import warnings

import numpy as np
import pandas as pd
import pytest
import torch

import eg_models_util as mu
import golden_util as gu
from make_golden_ope import LOGS, OUC_VARIANTS, log_frame
from recogym_amd import _abi
from recogym_amd import evaluate_agent as ev
from recogym_amd.agents import (BanditCount, LastViewTableAgent, OrganicUserEventCounterAgent, RandomAgent, bandit_count_args)
from recogym_amd.agents.logreg_frozen import LogregFrozenAgent
from recogym_amd.envs.configuration import Configuration
from recogym_amd.envs.reco_env_v1 import env_1_args, rows_to_dataframe
from recogym_amd.sim import Simulator
from test_ope_logreg_host import frozen

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def host_only(monkeypatch):
    monkeypatch.setattr(ev, '_device_present', lambda: False)


def sim_log(P, n, seed=7):
    cfg = Configuration({**env_1_args, 'random_seed': seed, 'num_products': P, 'K': 5})
    sim = Simulator(cfg, n, device=DEV)
    sim.reset_users(0, n)
    sim.run()
    return sim


def replay(agent, dl, k, **kw):
    """recall_replay, which must have taken the device route without a warning -> (hits as a list, counts as a list)."""
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        out = ev.recall_replay(agent, dl, k, **kw)
    assert out is not None, 'the device route was left out'
    hit, counts = out
    assert hit.dtype == torch.uint8 and counts.dtype == torch.int64
    hit, counts = hit.cpu().numpy().tolist(), counts.cpu().numpy().tolist()
    assert counts == [len(hit), sum(hit)]
    return hit, counts


# ---- 5. the reference's own numbers ----------------------------------------------------------------------------------------
def golden_agent(key, P, cols):
    if key == 'random':
        return RandomAgent(Configuration({'num_products': P, 'random_seed': 5, 'with_ps_all': True}))
    return LastViewTableAgent.from_bandit_mf(Configuration({'num_products': P, 'with_ps_all': True}),
                                             cols['bmf_product_embedding'], cols['bmf_user_embedding'])


@pytest.mark.parametrize('name', LOGS)
def test_device_equals_reference_fixture(name):
    meta, cols = gu.load(name)
    P = meta['env_args']['num_products']
    want = np.load(f'{gu.GOLDEN}/ope_{name}.npz')
    df = log_frame(cols)
    keys = [key for key in json.loads(str(want['meta']))['agents'] if key in ('random', 'bmf')]
    assert keys
    for key in keys:
        ag = golden_agent(key, P, cols)
        assert ev._recall_device_or_none(ag, df, 5) is not None                   # DataFrame in, device route
        got = ev.evaluate_recall_at_k(ag, df, k=5)
        assert isinstance(got, list) and all(type(h) is int for h in got)
        assert got == want[f'{key}__recall'].astype(np.int64).tolist(), key


# ---- 6. the boundaries of the counting rule ---------------------------------------------------------------------------------
O, B, BC = 0, 1, 2            # organic, bandit without a click, bandit with a click


def boundary_users():
    """One list of row kinds per user.  Every user opens with an organic row; the last one (max u) is not evaluated."""
    rng = np.random.RandomState(17)

    def filler(n):
        return [O] + [int(x) for x in rng.choice([O, B, BC], size=n - 1, p=[0.5, 0.35, 0.15])]
    u63 = filler(63)
    u64 = filler(64)
    u64[63] = B                                      # the user's last row at chunk position 63: no successor
    u65 = filler(65)
    u65[63], u65[64] = B, O                          # position 63 of a chunk, the organic successor opens the next chunk
    u129 = filler(129)
    u129[61:66] = [B, B, BC, B, O]                   # bandit after bandit, a click, then position 63 -> 64 across the chunks
    u129[126:129] = [BC, O, B]                       # a clicked bandit row before an organic row; the user ends on a bandit row
    return [[O],                                     # 1 row
            [O, B],                                  # 2 rows, ending unclicked: the next row of the log is the next user's organic row
            u63, u64, u65, u129,
            [O, B, O, BC, O, B, B],                  # the last evaluated user ends on a bandit row: the last row the kernel may read
            [O, B, O]]                               # max(u): not evaluated


def boundary_frame(P):
    rng = np.random.RandomState(23)
    rows = []
    for uid, kinds in enumerate(boundary_users()):
        for t, kind in enumerate(kinds):
            rows.append((uid, t, kind != O, int(rng.randint(P)), kind == BC))
    is_b = np.array([r[2] for r in rows], dtype=bool)
    idx = [r[3] for r in rows]
    return pd.DataFrame({'t': np.array([r[1] for r in rows], dtype=np.float32), 'u': [r[0] for r in rows],
                         'z': np.where(is_b, 'bandit', 'organic').astype(object),
                         'v': pd.array([None if b else i for b, i in zip(is_b, idx)], dtype=pd.UInt16Dtype()),
                         'a': pd.array([i if b else None for b, i in zip(is_b, idx)], dtype=pd.UInt16Dtype()),
                         'c': np.array([float(r[4]) if r[2] else np.nan for r in rows], dtype=np.float32),
                         'ps': np.where(is_b, 1.0 / P, np.nan)})


@pytest.mark.parametrize('k', [1, 5, 10])
def test_boundaries_of_the_counting_rule(k):
    P = 10
    users = boundary_users()
    assert [len(u) for u in users[:6]] == [1, 2, 63, 64, 65, 129]
    df = boundary_frame(P)
    ag = LastViewTableAgent(Configuration({'num_products': P, 'with_ps_all': True}), np.random.RandomState(3).randint(0, P, size=P))
    counted = sum(1 for kinds in users[:-1] for i in range(len(kinds) - 1) if kinds[i] == B and kinds[i + 1] == O)
    dl = ev._frame_to_device(df, ev.ope_policy_of(ag), torch.device(DEV))
    hit, counts = replay(ag, dl, k, n_users=len(users) - 1)
    want = ev._host_recall(ag, df, k)
    assert len(want) == counted == counts[0]
    assert hit == want
    assert 0 < sum(want) and (k == 10 or sum(want) < len(want))
    assert ev._recall_device_or_none(ag, df, k) is not None
    assert ev.evaluate_recall_at_k(ag, df, k=k) == want


# ---- 7. every one-hot route against the host loop ----------------------------------------------------------------------------
def one_hot_targets(dl):
    P = 10
    meta, cols, _ = mu.load('model_eg_ope_poly')
    eg = dict(epsilon=0.3, random_seed=7)
    bc = BanditCount(Configuration({**bandit_count_args, 'num_products': P, 'with_ps_all': True}))
    bc.train_from_log(dl)

    def table():
        return LastViewTableAgent(Configuration({'num_products': P, 'with_ps_all': True}), np.random.RandomState(3).randint(0, P, size=P))
    out = {'logreg': frozen(P, with_ps_all=True), 'poly': mu.inner_agent(meta, cols, P, with_ps_all=True), 'bandit_count': bc}
    for pn in (True, False):
        out[f'eg_logreg_{pn}'] = mu.wrap(frozen(P, with_ps_all=True), P, dict(eg, epsilon_pure_new=pn), with_ps_all=True)
        out[f'eg_table_{pn}'] = mu.wrap(table(), P, dict(eg, epsilon_pure_new=pn), with_ps_all=True)
    return out


ONE_HOT = ('logreg', 'poly', 'bandit_count', 'eg_logreg_True', 'eg_logreg_False', 'eg_table_True', 'eg_table_False')


@pytest.fixture(scope='module')
def p10_log():
    sim = sim_log(10, 300)
    dl = sim.device_log()
    yield dl, rows_to_dataframe(sim.rows(), 10), one_hot_targets(dl)
    sim.close()


@pytest.mark.parametrize('which', ONE_HOT)
def test_one_hot_routes_equal_the_host_loop(which, p10_log, monkeypatch):
    dl, df, targets = p10_log
    ag = targets[which]
    hit, counts = replay(ag, dl, 5)
    want = ev._host_recall(ag, df, 5)
    assert hit == want and 0 < sum(want) < len(want)
    got = ev.evaluate_recall_at_k(ag, dl, k=5)
    assert got.dtype == torch.int64 and got.is_cuda and got.cpu().numpy().tolist() == want
    on_frame = ev.verify_agents_recall_at_k(df, {which: ag}, k=5)                  # DataFrame in, device route
    on_log = ev.verify_agents_recall_at_k(dl, {which: ag}, k=5)
    host_only(monkeypatch)
    host = ev.verify_agents_recall_at_k(df, {which: ag}, k=5)
    assert on_frame.equals(host)
    for col in ('0.025', '0.500', '0.975'):
        a, b = float(on_log[col][0]), float(host[col][0])
        print(which, col, a, b)
        assert abs(a - b) <= 1e-12 * abs(b)


# ---- 10. determinism ---------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bytes(p10_log):
    dl, _, targets = p10_log
    first = ev.recall_replay(targets['logreg'], dl, 5)
    second = ev.recall_replay(targets['logreg'], dl, 5)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1]) and int(first[1][0].item()) > 0


# ---- 8. the ranking form -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', [10, 65, 130])
def test_ranking_form_equals_the_host_loop(P):
    sim = sim_log(P, 120, seed=11)
    dl, df = sim.device_log(), rows_to_dataframe(sim.rows(), P)
    ag = frozen(P, with_ps_all=True, select_randomly=True)
    for k in sorted({1, 5, P // 2, P - 1, P}):       # (P // 2 and P - 1: verdicts deep in the ranking, where most rows hit)
        stats = {}
        hit, counts = replay(ag, dl, k, stats=stats)
        want = ev._host_recall(ag, df, k)
        print(P, k, stats, counts)
        assert hit == want and len(want) > 0
        assert stats['unresolved'] == 0 and not stats['overflow'] and stats['error'] == 0 and stats['acts'] > 0
        assert sum(want) == len(want) if k == P else (k > 5 or sum(want) < len(want))
    sim.close()


# ---- 9. the margin's list ------------------------------------------------------------------------------------------------------
def twin_model(P=10):
    """Classes 2 and 7 are the same class twice (equal coef rows and intercepts) and outweigh the others: their probabilities
    tie at the top on every act, and k = 1 must take NumPy's pick of the two."""
    rng = np.random.RandomState(5)
    coef, intercept = 0.1 * rng.randn(P, P), 0.1 * rng.randn(P)
    coef[7], intercept[7] = coef[2], intercept[2]
    intercept[[2, 7]] += 3.0
    return LogregFrozenAgent(Configuration({'num_products': P, 'random_seed': 3, 'with_ps_all': True, 'select_randomly': True}),
                             coef, intercept, np.arange(P))


def five_pairs_model(P=10):
    rng = np.random.RandomState(6)
    coef, intercept = 0.5 * rng.randn(P, P), 0.5 * rng.randn(P)
    coef[5:], intercept[5:] = coef[:5], intercept[:5]
    return LogregFrozenAgent(Configuration({'num_products': P, 'random_seed': 3, 'with_ps_all': True, 'select_randomly': True}),
                             coef, intercept, np.arange(P))


def test_rows_inside_the_margin_are_listed_and_confirmed_on_the_host(p10_log, monkeypatch):
    dl, df, _ = p10_log
    ag = twin_model()
    want = ev._host_recall(ag, df, 1)
    stats = {}
    hit, counts = replay(ag, dl, 1, stats=stats)
    print(stats, counts)
    assert 1 < stats['unresolved'] <= _abi.OPE_RECALL_LIST_CAP and not stats['overflow']
    assert hit == want and sum(want) < len(want)
    # five classes twice, k = 5: the fifth place is one of a pair's two on every act — hits, misses and listed rows all occur
    pairs = five_pairs_model()
    want5 = ev._host_recall(pairs, df, 5)
    hit5, _ = replay(pairs, dl, 5, stats=stats)
    print(stats, len(want5), sum(want5))
    assert 1 < stats['unresolved'] < len(want5) and hit5 == want5 and 0 < sum(want5) < len(want5)
    # a list too short for them (the capacity is the call's parameter): one warning, then the host loop's result
    def runtime_warnings(caught):
        return [w for w in caught if issubclass(w.category, RuntimeWarning)]
    with pytest.warns(RuntimeWarning) as caught:
        assert ev.recall_replay(ag, dl, 1, list_cap=1) is None
    assert len(runtime_warnings(caught)) == 1
    monkeypatch.setattr(_abi, 'OPE_RECALL_LIST_CAP', 1)
    with pytest.warns(RuntimeWarning) as caught:
        got = ev.evaluate_recall_at_k(ag, df, k=1)
    assert len(runtime_warnings(caught)) == 1 and got == want


# ---- 11. no form: the host loop ------------------------------------------------------------------------------------------------
def test_count_vector_agents_take_the_host_loop(p10_log, monkeypatch):
    dl, df, _ = p10_log
    small = df[df['u'] <= 60].reset_index(drop=True)
    ouc = OrganicUserEventCounterAgent(Configuration({'num_products': 10, 'random_seed': 11, 'weight_history_function': None,
                                                      'with_ps_all': True, **OUC_VARIANTS[0]}))
    wrapped = mu.wrap(OrganicUserEventCounterAgent(Configuration({'num_products': 10, 'random_seed': 11, 'weight_history_function': None,
                                                                  'with_ps_all': True, **OUC_VARIANTS[0]})),
                      10, dict(epsilon=0.3, random_seed=7), with_ps_all=True)
    for ag in (ouc, wrapped):
        assert ev.recall_replay(ag, dl, 5) is None
        assert ev._recall_device_or_none(ag, small, 5) is None
        got = ev.evaluate_recall_at_k(ag, small, k=5)
        assert isinstance(got, list) and got == ev._host_recall(ag, small, 5) and len(got) > 0
