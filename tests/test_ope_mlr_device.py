"""Off-policy replay of PyTorchMLRAgent on the device (rg_ope_replay_mlr / rg_ope_replay_mlr_eg, recogym_amd/csrc/rg_ope_mlr.hip)
against the host loop of the same call (PyTorchMLRFrozenAgent.act through evaluate_agent._host_ips / _host_snips / _host_recall),
the host act on hand-made histories, and itself.  Every ratio, click and IPS term is compared bit for bit, the sums with the
documented order of the unit's wave cap bit for bit (as tests/test_ope_nn_device.py holds d_sums); the head words of the workspace
prove that the device took the acts.  Needs a real MI355X."""
import warnings

import numpy as np
import pytest
import torch

import golden_util as gu
import mlr_util as fx
import ope_models_util as mu
from make_golden_ope import log_frame
from test_ope_sums_order import documented_sums
from recogym_amd import _abi
from recogym_amd import evaluate_agent as ev
from recogym_amd.agents.pytorch_mlr import PyTorchMLRFrozenAgent
from recogym_amd.sim import DeviceLog

pytestmark = pytest.mark.gpu
DEV = mu.DEV
W_CAP = 2048                # kOmMaxWaves: part of the bits of d_sums


def mlr_agent(P, seed, scale=1.0):
    return PyTorchMLRFrozenAgent(mu.cfg(P), (np.random.RandomState(seed).standard_normal((P, P)) * scale).astype(np.float32))


def fixture_agent(name):
    meta, cols = gu.load(name)
    return PyTorchMLRFrozenAgent(mu.cfg(meta['env_args']['num_products']), fx.fixture_weight(meta, cols))


def tie_agent(P=10):
    """Rows 0 and 5 of W are equal and lead the rest on every history: every act is an exact tie, the device lists it with action
    0, and the host's first maximum is action 0."""
    W = np.full((P, P), -5.0, dtype=np.float32)
    W[0] = W[5] = 1.0
    return PyTorchMLRFrozenAgent(mu.cfg(P), W)


def check_result(dl, n_eval, r, sums, st, what='', max_unresolved=None):
    """The acts are the walk's, the sums the documented order's at the unit's W."""
    is_b, click, offsets, acts = mu.walk(dl, n_eval)
    print(what, st)
    assert st['acts'] == acts and not st['overflow'], (what, st, acts)
    if max_unresolved is not None:
        assert st['unresolved'] <= max_unresolved, (what, st)
    ratio = np.zeros(is_b.size)
    ratio[is_b] = r
    want = documented_sums(ratio, click, is_b, offsets, W_CAP)
    assert sums.tobytes() == want.tobytes(), (what, [x.hex() for x in sums], [x.hex() for x in want])


# ---- 1. the estimators on the fixtures' training logs ---------------------------------------------------------------------------
@pytest.mark.parametrize('target', ['mlr_p10_a05', 'mlr_p10_ties'])
@pytest.mark.parametrize('log', ['mlr_p10_a05', 'mlr_p10_a1'])
def test_the_estimators_equal_the_host_loop_on_the_training_logs(target, log):
    """evaluate_IPS / evaluate_SNIPS of a fixture's agent over a fixture's training log (the uniform logger's): a result, no warning,
    the walk's acts, the host loop's ratios, clicks and IPS terms bit for bit.  Under mlr_p10_ties every act is listed and the host
    confirms each."""
    ag, df = fixture_agent(target), log_frame(fx.training_log(log))
    pol = ev.ope_checked_policy_of(ag)
    assert pol is not None and pol['kind'] == _abi.RG_POLICY_MLR and ev.ope_policy_of(ag) is None
    dl = ev._frame_to_device(df, pol, torch.device(DEV))
    n_eval = int(dl.offsets.numel()) - 1
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        r, c, sums, st = mu.replay(ag, dl)
        ips = ev.evaluate_IPS(ag, df)
        rewards, ratio = ev.evaluate_SNIPS(ag, df)
    ties = target == 'mlr_p10_ties'
    check_result(dl, n_eval, r, sums, st, f'{target} on {log}', None if ties else st['acts'] // 100)
    assert st['acts'] > 100 and st['rows_read'] >= st['acts'] and (st['unresolved'] == st['acts']) == ties
    want_c, want_r = ev._host_snips(ag, df)
    mu.same(r, want_r)
    mu.same(ratio, want_r)
    mu.same(rewards, np.asarray(want_c, dtype=np.float64))
    mu.same(ips, ev._host_ips(ag, df))
    assert isinstance(ips, list) and isinstance(ratio, list) and 0 < np.count_nonzero(r) < r.size


def test_the_replay_is_opt_in():
    ag = fixture_agent('mlr_p10_a05')
    off = PyTorchMLRFrozenAgent(mu.cfg(10, device_replay=False), ag.W)
    dl, _ = mu.sim_log(10, 0.1)
    assert ev.ope_checked_policy_of(off) is None and ev.ope_replay(off, dl) is None


@pytest.mark.parametrize('sigma', [0.0, 0.1])
def test_simulator_logs_equal_the_host_loop(sigma):
    ag = mlr_agent(10, seed=3)
    dl, df = mu.sim_log(10, sigma)
    n_eval = int(dl.offsets.numel()) - 2
    r, c, sums, st = mu.replay(ag, dl, n_eval)
    check_result(dl, n_eval, r, sums, st, f'sigma {sigma}', st['acts'] // 20)
    rewards, want = ev._host_snips(ag, df)
    mu.same(r, want)
    mu.same(c, np.asarray(rewards, dtype=np.float64))
    assert 0 < np.count_nonzero(r) < r.size
    ips = ev.evaluate_IPS(ag, dl)
    assert torch.is_tensor(ips)
    mu.same(ips.cpu().numpy(), ev._host_ips(ag, df))


# ---- 2. hand-made logs ------------------------------------------------------------------------------------------------------------
def build(users, ag, ps=0.25):
    """ope_models_util.build with this agent's host act: per user a list of tokens, ('o', product), ('o', product, times) or 'b' ->
    (DeviceLog, expected ratio per bandit row, acts); the logged action alternates between the host's and another one."""
    P = ag.config.num_products
    raw, offsets, want, acts, flip = [], [0], [], 0, 0
    for u, toks in enumerate(users):
        views = np.zeros(P, dtype=np.int64)
        dirty, a_host, t = True, None, 0
        for tok in toks:
            if tok == 'b':
                if dirty:
                    prods = np.flatnonzero(views)
                    a_host = ag.act_on(prods, views[prods])[0]
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
    dl, want, acts = build(users, ag)
    r, _, sums, st = mu.replay(ag, dl)
    print(what, st)
    assert st['unresolved'] <= (0 if all_resolved else mu.UNRESOLVED_SHARE * acts) and not st['overflow'], (what, st)
    mu.same(r, want)
    assert st['acts'] == acts and sums[0] == want.size and 0 < np.count_nonzero(r) < r.size, (what, st, acts)
    return st


def test_a_user_longer_than_the_lds_list_takes_the_global_scratch():
    """Users of 255 ... 513 distinct products at P = 520: past kPolyHist = 256 the act reads the list itself, past the 512 entries
    of the LDS list the history moves to the per-wave global list."""
    st = check(mu.tier_users(520), mlr_agent(520, seed=3, scale=0.1), 'tiers', all_resolved=True)
    assert st['rows_read'] >= 513 + 512 + 511


def test_chunk_geometry():
    ag = mlr_agent(65, seed=4, scale=0.3)
    users = mu.geometry_users(65)
    check(users, ag, 'geometry')
    dl, _, _ = build(users, ag)
    r, c, sums, st = mu.replay(ag, dl, n_users=0)
    assert r.size == 0 and sums.tolist() == [0.0, 0.0, 0.0] and st['acts'] == 0


@pytest.mark.parametrize('P', [63, 64, 65, 78, 79, 129])
def test_lane_and_stride_edges(P):
    """(The table is staged in LDS up to P = 78 and read from global memory from 79 on; from P = 68 the kernel needs the LDS opt-in.)"""
    check(mu.random_users(P, seed=P), mlr_agent(P, seed=P, scale=0.3), f'P = {P}')


@pytest.mark.parametrize('n_users', [1, 37, 300])
def test_user_counts(n_users):
    ag = mlr_agent(10, seed=3)
    dl, _ = mu.sim_log(10, 0.1)
    full, _, _, _ = mu.replay(ag, dl, 300)
    r, c, sums, st = mu.replay(ag, dl, n_users)
    check_result(dl, n_users, r, sums, st, f'{n_users} users')
    mu.same(r, full[:r.size])
    assert r.size > 0 and (n_users < 300 or r.size == full.size)


# ---- 3. the unresolved protocol ---------------------------------------------------------------------------------------------------
def test_an_exact_tie_is_listed_and_the_host_confirms_action_0():
    mu.tie_stands(tie_agent())


def test_a_refuted_act_sends_the_estimators_to_the_host_loop(monkeypatch):
    mu.refuted_takes_the_host_loop(tie_agent(), monkeypatch, 'mlr_host_act')


def test_more_unresolved_acts_than_the_list_holds():
    mu.overflow_takes_the_host_loop(tie_agent())


# ---- 4. determinism, recall@k and the tables --------------------------------------------------------------------------------------
def test_two_replays_both_ways_in_and_two_shards_give_the_same_bits():
    mu.determinism_and_both_ways_in(mlr_agent(10, seed=3))


def test_recall_and_the_tables_equal_the_host_loops(monkeypatch):
    """evaluate_recall_at_k (rg_ope_recall_hits over the host-built one-hot sets; the act of every row from rg_ope_replay_mlr_eg with
    epsilon = 0) and the three verify_agents tables, with the two fixture agents as targets."""
    mu.recall_and_tables({'mlr': fixture_agent('mlr_p10_a05'), 'ties': fixture_agent('mlr_p10_ties')}, monkeypatch)


def test_out_of_range_models_are_refused():
    import ctypes as C
    lib = _abi.load()
    wt = torch.zeros(100, dtype=torch.float64, device=DEV)
    dl, _ = mu.sim_log(10, 0.1)
    n = int(dl.offsets.numel()) - 1
    longest = int((dl.offsets[1:] - dl.offsets[:-1]).max().item())

    def call(model, need=None):
        need = lib.rg_ope_mlr_workspace_bytes(C.byref(model), n, longest) if need is None else need
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=DEV)
        ratio = torch.empty(int(dl.offsets[-1]), dtype=torch.float64, device=DEV)
        sums = torch.empty(3, dtype=torch.float64, device=DEV)
        return lib.rg_ope_replay_mlr(C.byref(model), dl.rows.data_ptr(), dl.offsets.data_ptr(), n, longest, _abi.RG_OPE_PS_CONST, None, 0.1,
                                     ratio.data_ptr(), None, sums.data_ptr(), ws.data_ptr(), need, None)
    assert lib.rg_ope_mlr_workspace_bytes(None, n, longest) == 0
    need = lib.rg_ope_mlr_workspace_bytes(C.byref(_abi.RgOpeMlr(10, wt.data_ptr())), n, longest)
    assert need > 0
    assert call(_abi.RgOpeMlr(10, None), need) == -1 and b'null wt' in lib.rg_last_error()
    assert call(_abi.RgOpeMlr(0, wt.data_ptr()), need) == -1 and b'num_products' in lib.rg_last_error()
    assert call(_abi.RgOpeMlr(4001, wt.data_ptr()), need) == -1 and b'num_products' in lib.rg_last_error()
    wt[5] = float('nan')
    assert call(_abi.RgOpeMlr(10, wt.data_ptr())) == -1 and b'finite' in lib.rg_last_error()
    wt[5] = 0.0
    assert call(_abi.RgOpeMlr(10, wt.data_ptr())) == 0
    # the EG entry serves the wrapper that never explores (recall@k's way to the act of every row) and no other
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    ratio = torch.empty(int(dl.offsets[-1]), dtype=torch.float64, device=DEV)
    sums = torch.empty(3, dtype=torch.float64, device=DEV)
    model = _abi.RgOpeMlr(10, wt.data_ptr())
    for eps, want in ((0.3, -1), (0.0, 0)):
        eg = _abi.RgOpeEg(epsilon=eps, seed=1, pure_new=0, reserved=0, prob_explore=0.1)
        rc = lib.rg_ope_replay_mlr_eg(C.byref(model), C.byref(eg), dl.rows.data_ptr(), dl.offsets.data_ptr(), n, longest, _abi.RG_OPE_PS_CONST,
                                      None, 0.1, ratio.data_ptr(), None, sums.data_ptr(), None, None, ws.data_ptr(), need, None)
        assert rc == want and (rc == 0 or b'epsilon' in lib.rg_last_error()), (eps, rc, lib.rg_last_error())
