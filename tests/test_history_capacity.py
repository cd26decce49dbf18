"""The capacity contract of the per-user view history (include/recogym_hip.h: RG_CNT_HIST_OVERFLOW; DESIGN.md §3, data layout) on every run
form, against tests/history_model.py: rows of hist_cap entries keep hist_cap - 1 distinct products, a view of a new product
beyond that is dropped — row and view total unchanged, the overflow counter + 1 PER DROPPED VIEW, the policy acting on the kept
counts from then on — and the organic row is logged either way.

P = 2 000, K = 20, 512 users whose histories are preset (rg_sim_debug_set_history) at 0, keep - 2, keep - 1 and keep distinct
products: two thirds of the users drop views, some 5 000 in all.  Every insertion implementation has its own "row is full" branch
(history_add's register path and its line-at-a-time path, history_tail_add behind k_walk2's two line forms, solo_hist_add, the
repack's row copy), so every run form is held to the same model: every row, the counters, hist_overflow == the model's dropped
views EXACTLY, and — where slot == user index survives the run — the act on the final history (rg_sim_debug_ouc_acts) for
eight uniforms per user.  A path that drops without counting, counts without dropping, raises the total on a dropped view or
miscounts at the hand-over between the LDS line and the row fails here; nothing else in the suite makes the counter non-zero."""
import numpy as np
import pytest
import torch

import adversarial_util as au
import golden_util as gu
import history_model as hm
from recogym_amd import _abi
from test_hip_parity import assert_sweeps_of, assert_walk_pipe

pytestmark = pytest.mark.gpu

COLS = ('u', 't', 'z', 'v', 'a', 'c', 'ps')
SWITCHES = ('RECOGYM_DRAW', 'RECOGYM_BF16', 'RECOGYM_WALK', 'RECOGYM_WALK_HANDOVER', 'RECOGYM_WALK_HIST', 'RECOGYM_PIPE', 'RECOGYM_PIPE_MIN',
            'RECOGYM_XH', 'RECOGYM_XH_WAVES', 'RECOGYM_SLICES', 'RECOGYM_SWEEP_LDS', 'RECOGYM_TAIL', 'RECOGYM_RUN_AHEAD', 'RECOGYM_REPACK',
            'RECOGYM_REPACK_MIN', 'RECOGYM_CACHE', 'RECOGYM_LOGREG')

# form -> the switches the existing tests of the form use
FORM_ENV = {
    # sigma_omega = 0
    'walk2': {},                                                              # run_walk: k_walk2 (+ k_walk_solo for the last users)
    'walk2_line64': {},                                                       # the same with the walk_line64 option set
    'pipe': {'RECOGYM_PIPE_MIN': '256'},                                      # run_walk_pipe
    'solo': {'RECOGYM_WALK_HANDOVER': '64'},                                  # k_walk_solo emits most events
    'k_walk': {'RECOGYM_WALK': '1'},
    'lockstep': {'RECOGYM_WALK': '0', 'RECOGYM_TAIL': '0'},                   # k_draw_cached + k_advance to the end
    'tail': {'RECOGYM_WALK': '0'},                                            # ... handed over to k_tail at the first poll
    'repack': {'RECOGYM_WALK': '0', 'RECOGYM_TAIL': '0', 'RECOGYM_REPACK_MIN': '1', 'RECOGYM_REPACK': '3'},
    # sigma_omega = 0.1
    'rounds32': {'RECOGYM_RUN_AHEAD': '32', 'RECOGYM_TAIL': '0'},
    'rounds0': {'RECOGYM_RUN_AHEAD': '0', 'RECOGYM_TAIL': '0'},
    'lds': {'RECOGYM_SLICES': '1', 'RECOGYM_SWEEP_LDS': '1', 'RECOGYM_TAIL': '0'},        # k_draw_tp + k_pick
    'lds_scratch': {'RECOGYM_SLICES': '1', 'RECOGYM_SWEEP_LDS': '0', 'RECOGYM_TAIL': '0'},  # the fused sweep, prefixes in scratch
    'f64': {'RECOGYM_DRAW': 'f64', 'RECOGYM_TAIL': '0'},
    'drift_tail': {},                                                         # the rounds handed over to k_tail
}
# forms whose propensities the existing tests hold to 0.0 (tests/test_walk_line_layout.py); 1e-12 elsewhere
PS_EXACT = ('walk2', 'walk2_line64', 'pipe', 'solo')


def assert_form(led, form, drifts):
    """the launch ledger proves the form, the way the existing test of the form does"""
    if form in ('walk2', 'walk2_line64', 'solo'):
        assert led['walk2'] >= 1 and led['sweep_xh'] == led['walk'] == led['advance'] == led['advance_run'] == led['tail'] == 0, led
        assert form != 'solo' or led['walk_solo'] == 1, led
        assert led['walk_line64'] == (1 if form == 'walk2_line64' else 0), led
    elif form == 'pipe':
        assert_walk_pipe(led)
    elif form == 'k_walk':
        assert led['walk'] > 0 and led['walk2'] == led['walk_solo'] == led['draw_cached'] == led['advance'] == 0, led
    elif form in ('lockstep', 'tail', 'repack'):
        if drifts:      # (the boundary cases' rounds are 'rounds32')
            raise AssertionError(form)
        assert led['draw_cached'] > 0 and led['advance'] > 0 and led['walk'] == led['walk2'] == led['advance_run'] == 0, led
        assert (led['repack'] > 0) == (form == 'repack') and (led['tail'] > 0) == (form == 'tail'), led
    else:
        assert drifts and led['walk'] == led['walk2'] == led['draw_cached'] == 0, led
        assert (led['tail'] > 0) == (form == 'drift_tail'), led
        if form == 'rounds0':
            assert led['advance'] > 0 and led['advance_run'] == 0, led
        else:
            assert led['advance_run'] > 0 and led['advance'] == 0, led
        if form == 'lds':
            au.assert_draws_by(led, 'draw_tp')
            assert led['pick'] == led['draw_tp'] and led['search'] == 0 and led['sweep_lds_kernel'] == 1, led
        elif form == 'lds_scratch':
            au.assert_draws_by(led, 'draw16_fused')
            assert led['pick'] == led['search'] == 0, led
        elif form == 'f64':
            assert_sweeps_of(led, 'f64')


def set_form(form, monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in FORM_ENV[form].items():
        monkeypatch.setenv(k, v)


def assert_well_posed(ref):
    """on the model alone: a shape that stops overflowing fails instead of passing vacuously"""
    assert all((ref.nd == k).sum() > 100 for k in ref.classes)
    assert ref.users_dropped >= ref.n // 4 and ref.dropped >= 1000, (ref.users_dropped, ref.dropped)


def probe_uniforms(n):
    """eight uniforms per user spread over [0, 1): one in every eighth"""
    return (np.arange(8)[None, :] + np.random.RandomState(8).random_sample((n, 8))) / 8.0


def run_form(ref, form, monkeypatch, probe=True):
    """The run of `ref`'s population in `form` -> rows, counters, ledger, and the acts of the final histories on probe_uniforms
    ((n, 8) actions and propensities; None without the probe)."""
    from recogym_amd.sim import Simulator
    set_form(form, monkeypatch)
    n, dev = ref.n, 'cuda:0'
    sim = Simulator(ref.cfg, n, device=dev, p_click=False, **ref.pol)
    assert sim.get_option('hist_cap') == ref.hist_cap == ref.keep + 1
    if form == 'walk2_line64':
        sim.set_option('walk_line64', 1)
    sim.reset_users(0, n)
    d_nd, d_p, d_c = (torch.from_numpy(np.array(x).view(np.int32)).to(dev) for x in (ref.nd, ref.prod, ref.cnt))      # (copies: the reference's arrays are read-only)
    _abi.check(sim.lib.rg_sim_debug_set_history(sim._h, d_nd.data_ptr(), d_p.data_ptr(), d_c.data_ptr(), ref.stride, sim._stream()),
               'debug_set_history')
    sim.run()
    rows, cnt, led = sim.rows(), sim.counters(), au.ledger(sim)
    led['walk_line64'] = sim.get_option('walk_line64')
    acts = None
    if probe:
        u = probe_uniforms(n)
        got_a, got_ps = np.zeros((n, 8), dtype=np.int64), np.zeros((n, 8))
        d_a = torch.zeros(n, dtype=torch.int32, device=dev)
        d_ps = torch.zeros(n, dtype=torch.float64, device=dev)
        d_fl = torch.zeros(n, dtype=torch.uint8, device=dev)
        for j in range(8):
            d_u = torch.from_numpy(np.ascontiguousarray(u[:, j])).to(dev)
            _abi.check(sim.lib.rg_sim_debug_ouc_acts(sim._h, d_u.data_ptr(), d_a.data_ptr(), d_ps.data_ptr(), d_fl.data_ptr(), sim._stream()),
                       'debug_ouc_acts')
            torch.cuda.synchronize()
            got_a[:, j], got_ps[:, j] = d_a.cpu().numpy(), d_ps.cpu().numpy()
        acts = got_a, got_ps
    sim.close()
    return rows, cnt, led, acts


def assert_run_is_the_models(ref, form, rows, cnt, acts, what):
    print(f"{what}: hist_overflow {cnt['hist_overflow']} (model {ref.dropped}), rows {len(rows)} (model {len(ref.rows)})")
    gu.assert_rows_equal(rows, {k: ref.rows[k] for k in COLS}, ps_rtol=0.0 if form in PS_EXACT else 1e-12, what=what)
    assert (rows['phantom'] == ref.rows['phantom']).all()
    oc = ref.counters
    assert (cnt['organic'], cnt['bandit'], cnt['clicks'], cnt['phantom']) == (oc['organic'], oc['bandit'], oc['clicks'], oc['phantom'])
    assert cnt['live'] == 0 and cnt['log_dropped'] == 0
    assert cnt['hist_overflow'] == ref.dropped, (cnt['hist_overflow'], ref.dropped)
    if acts is not None:
        # the histories the run left behind: the act on them is the model's act on its final kept counts
        u = probe_uniforms(ref.n)
        P = ref.cfg.num_products
        for user in range(ref.n):
            views = np.zeros(P)
            views[ref.final[user][0]] = ref.final[user][1]
            for j in range(8):
                a, ps = hm.ouc_act(views, u[user, j])
                assert acts[0][user, j] == a, (what, user, j, int(acts[0][user, j]), a, len(ref.final[user][0]))
                assert abs(acts[1][user, j] - ps) <= 1e-15 * ps, (what, user, j, acts[1][user, j], ps)


def test_capacity_table():
    """ouc_history_cap -> hist_cap as the library reports it (read-only option), once"""
    from recogym_amd.sim import Simulator
    for cap, hist_cap in hm.HIST_CAP_TABLE.items():
        sim = Simulator(hm.config(hm.P_CAP, 7102), 64, device='cuda:0', **dict(hm.POL, ouc=dict(gu.OUC_DEFAULTS, history_cap=cap)))
        assert sim.get_option('hist_cap') == hist_cap == hm.hist_cap_of(cap), cap
        sim.close()


# history_cap 15: the 64-bit line (no compact line below hist_cap 32) and history_add's register path; 31: the compact line exactly
# full; 47: a tail behind the line, history_add's line-at-a-time path; 0: the default 255, where the solo kernel's LDS history meets
# its own limit
CAPPED_WALK_CASES = [('walk2', 15), ('walk2', 31), ('walk2', 47), ('walk2_line64', 31), ('pipe', 31), ('pipe', 47), ('solo', 47), ('solo', 0),
                     ('k_walk', 15), ('k_walk', 47), ('lockstep', 15), ('lockstep', 47), ('tail', 15), ('tail', 47),
                     ('repack', 15), ('repack', 47)]


@pytest.mark.parametrize('form,history_cap', CAPPED_WALK_CASES)
def test_full_rows_drop_and_count_views_at_sigma_omega_zero(form, history_cap, monkeypatch):
    ref = hm.capacity_reference(0.0, history_cap)
    assert_well_posed(ref)
    rows, cnt, led, acts = run_form(ref, form, monkeypatch, probe=form != 'repack')      # (the repack moves users to other slots)
    assert_form(led, form, False)
    assert_run_is_the_models(ref, form, rows, cnt, acts, f'{form}, history_cap {history_cap}')


@pytest.mark.parametrize('history_cap', [15, 31])
@pytest.mark.parametrize('form', ['rounds32', 'rounds0', 'lds', 'lds_scratch', 'f64', 'drift_tail'])
def test_full_rows_drop_and_count_views_with_drifting_omega(form, history_cap, monkeypatch):
    ref = hm.capacity_reference(0.1, history_cap)
    assert_well_posed(ref)
    rows, cnt, led, acts = run_form(ref, form, monkeypatch)
    assert_form(led, form, True)
    assert_run_is_the_models(ref, form, rows, cnt, acts, f'{form}, history_cap {history_cap}')


@pytest.mark.parametrize('form', ['lockstep', 'tail', 'rounds32', 'k_walk', 'solo'])
def test_histories_grow_through_the_line_boundaries_without_a_cap(form, monkeypatch):
    """The default capacity and presets of 14 .. 49 distinct products: history_add's switch from registers to lines (15 -> 16), its
    line loads at the multiples of 16, the walk kernels' lines filling up, on purpose and not by luck.  Nothing is dropped."""
    drifts = form == 'rounds32'
    ref = hm.boundary_reference(0.1 if drifts else 0.0)
    assert all((ref.nd == k).sum() >= 30 for k in hm.BOUNDARY_ND0) and ref.dropped == 0
    assert 49 < max(len(f[0]) for f in ref.final) < ref.keep
    rows, cnt, led, acts = run_form(ref, form, monkeypatch)
    assert_form(led, form, drifts)
    assert_run_is_the_models(ref, form, rows, cnt, acts, f'boundaries, {form}')
    assert cnt['hist_overflow'] == 0


@pytest.mark.parametrize('form', ['lockstep', 'rounds32', 'rounds0'])
def test_frozen_logreg_on_full_rows(form, monkeypatch):
    """The frozen LogReg on rows of 15 products (history_model.dyadic_logreg: exact scores, no ties).  A dropped view marks the cached
    act stale without changing the history: the act computed again must be the same action, which the rows show."""
    drifts = form != 'lockstep'
    ref = hm.logreg_reference(0.1 if drifts else 0.0)
    assert_well_posed(ref)
    rows, cnt, led, _ = run_form(ref, form, monkeypatch, probe=False)
    assert led['walk'] == led['walk2'] == led['tail'] == 0, led
    if form == 'rounds32':
        assert led['advance_run'] > 0 and led['advance'] == 0, led
    else:
        assert led['advance'] > 0 and led['advance_run'] == 0, led
    assert led['logreg_screen'] + led['logreg_acts'] > 0 and cnt['lr_acts'] > 0, led
    assert_run_is_the_models(ref, form, rows, cnt, None, f'frozen LogReg, {form}')


class CappedCounterAgent:
    """the OrganicUserEventCounter policy on rows of 15 products"""

    def device_policy(self):
        return dict(hm.POL, ouc=dict(gu.OUC_DEFAULTS, history_cap=15))


def retry_setup(monkeypatch):
    """-> env, the oracle's uncapped log of 512 users, the list of policies make_simulator is called with"""
    import recogym_amd as recogym
    from oracle import oracle as orc
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    n = hm.N_CAP
    cfg = hm.config(hm.P_CAP, 7102)
    want = orc.OracleEnv(cfg, rng_mode=orc.RNG_PHILOX, **hm.POL).generate_logs(n)
    org = want[want['z'] == 0]
    pairs = np.unique(np.stack([org['u'].astype(np.int64), org['v'].astype(np.int64)], axis=1), axis=0)
    assert (np.bincount(pairs[:, 0]) > 15).sum() >= 10             # users that view more than 15 products: the first run overflows
    env = recogym.make('reco-gym-v1')
    env.init_gym({**recogym.env_1_args, 'random_seed': 7102, 'num_products': hm.P_CAP, 'K': hm.K, 'sigma_omega': 0.0})
    calls = []
    real = env.make_simulator

    def counting(*args, **kwargs):
        calls.append(kwargs.get('policy'))
        return real(*args, **kwargs)
    monkeypatch.setattr(env, 'make_simulator', counting)
    return env, want, calls


def test_simulate_runs_again_with_longer_rows_after_an_overflow(monkeypatch):
    env, want, calls = retry_setup(monkeypatch)
    cnt, sim = env.simulate(hm.N_CAP, CappedCounterAgent())
    rows = sim.rows()
    hist_cap = sim.get_option('hist_cap')
    sim.close()
    assert len(calls) == 2 and calls[0]['ouc']['history_cap'] == 15 and calls[1]['ouc']['history_cap'] == 511, calls
    assert hist_cap == 512 and cnt['hist_overflow'] == 0 and cnt['log_dropped'] == 0 and cnt['live'] == 0
    gu.assert_rows_equal(rows, {k: want[k] for k in COLS}, ps_rtol=1e-12, what='simulate after the retry')
    assert (rows['phantom'] == want['phantom']).all()


def test_generate_logs_runs_again_with_longer_rows_after_an_overflow(monkeypatch):
    from test_env_dropin import assert_frames_match, frame_to_cols
    env, want, calls = retry_setup(monkeypatch)
    df = env.generate_logs(hm.N_CAP, CappedCounterAgent())
    assert len(calls) == 2 and calls[1]['ouc']['history_cap'] == 511, calls
    assert_frames_match(frame_to_cols(df), {k: want[k] for k in COLS}, 1e-12)
