"""The frozen LogReg act kernels (k_logreg_screen + k_logreg_decide, k_logreg_acts, the float64 walk logreg_act_wave) on placed
histories and class edges, through rg_sim_debug_logreg_acts: every builder of tests/logreg_frozen_util.py at class counts whose
ranges are ragged, empty, exactly one 512-class batch and longer; the benchmark's 10^4 classes; the fp32 form at its block borders;
padded models; whole runs (select and the dirty flag); the hook's refusals.  The tests marked gpu need a real MI355X; the unmarked
ones hold the reference and the builders' well-posedness on the CPU."""
import ctypes as C
import warnings

import numpy as np
import pytest

import adversarial_util as au
import golden_util as gu
import logreg_frozen_util as lu
from recogym_amd import _abi
from recogym_amd.envs.configuration import Configuration
from recogym_amd.envs.reco_env_v1 import env_1_args
from recogym_amd.envs.static_params import make_rg_config

gpu = pytest.mark.gpu
FP16_C = (8, 16, 56, 64, 72, 520, 4096, 4104)
FP32_C = (1, 2, 63, 64, 65, 255, 256, 257, 300)
FP32_NDS = (1, 32, 33)
FROZEN = _abi.RG_POLICY_LOGREG_FROZEN
EINVAL, ESTATE = -1, -4                       # RG_EINVAL, RG_ESTATE


def fp32_builders(C):
    out = [lu.clear_winners(C, nds=FP32_NDS), lu.all_zero(C)]
    if C > 1:
        out += [lu.exact_ties(C, nds=FP32_NDS), lu.fp32_band_pairs(C)]
    return out


def bench_builders():
    """classes = c % P as the benchmark-size case is stated, and (c + 1) % P beside it: there no class index is its own action, so
    the winners planted below P tell a class index from an action too.  The cross-batch list overflow at ranges of 1 256 classes."""
    out = []
    for shift in (0, 1):
        kw = dict(P=128, bench=True, shift=shift)
        out += [lu.clear_winners(10000, **kw), lu.exact_ties(10000, **kw), lu.band_edge_pairs(10000, **kw)]
    return out + [lu.stream_cases(10000, P=128, bench=True)]


# ------------------------------------------------------------------------------------------------
# on the CPU: the reference and the builders
# ------------------------------------------------------------------------------------------------
def test_reference_is_sklearn_predict():
    """lu.reference against sklearn.linear_model.LogisticRegression.predict on a CSR row (scipy's csr_matvecs order), for 300 random
    models and histories with hidden classes — and lu.exact_decision agrees wherever the float64 margin is not a rounding."""
    from scipy import sparse
    from sklearn.linear_model import LogisticRegression
    rng = np.random.RandomState(9)
    for trial in range(300):
        P, n_cls = int(rng.randint(4, 40)), int(rng.randint(3, 12))
        n_cls = min(n_cls, P - 1)
        classes = np.sort(rng.choice(P, n_cls, replace=False)).astype(np.int64)
        lr = LogisticRegression()
        lr.coef_, lr.intercept_, lr.classes_ = rng.standard_normal((n_cls, P)) * 10.0 ** rng.uniform(-3, 3), rng.standard_normal(n_cls), classes
        if trial % 5 == 0:                       # a duplicated class: the first maximum
            lr.coef_[-1], lr.intercept_[-1] = lr.coef_[0], lr.intercept_[0]
        nd = int(rng.randint(1, P + 1))
        prod = np.sort(rng.choice(P, nd, replace=False))
        cnt = np.where(rng.rand(nd) < 0.5, 1, rng.randint(1, 5000, nd))
        x = np.zeros(P)
        x[prod] = cnt
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            want = int(lr.predict(sparse.csr_matrix(x.reshape(1, P)))[0])
        coef_t = np.ascontiguousarray(lr.coef_.T)
        c, a = lu.reference(coef_t, lr.intercept_, classes, prod, cnt)
        assert a == want == classes[c], (trial, a, want)
        s = np.sort(lu.scores64(coef_t, lr.intercept_, prod, cnt))
        if s[-1] - s[-2] > 1e-9 * np.abs(s).max() or s[-1] == s[-2]:
            assert lu.exact_decision(coef_t, lr.intercept_, prod, cnt) == c


def assert_well_posed(case, C, hist_entries=lu.HIST_ENTRIES):
    n = len(case.nd)
    assert 0 < n <= 2048 and case.prod.shape == case.cnt.shape and case.prod.shape[1] <= hist_entries
    assert case.coef_t.shape[1] == C == len(case.classes) == len(case.intercept)
    assert (case.classes[case.want_c] == case.want_a).all()
    assert np.abs(case.coef_t).max() < 6.0e4                 # (the Simulator attaches the fp16 copy below that)
    print(C, case.label, case.proof)


@pytest.mark.parametrize('n_classes', FP16_C)
def test_fp16_builders_are_what_they_claim(n_classes):
    """Every builder asserts its own proof while it builds (the float64 gaps, the bit-identical columns, the emulated inversions,
    the exact-arithmetic agreement); here: the shapes, the class maps and what the set as a whole covers."""
    cases = lu.fp16_builders(n_classes)
    for case in cases:
        assert_well_posed(case, n_classes)
        if not case.label.startswith(('all_zero', 'order')):
            assert (case.classes != np.arange(n_classes)).all() and case.proof['products_0_and_last']
            assert set(case.proof['nds']) == (set(lu.NDS) | {lu.HIST_ENTRIES}) - ({1} if case.label == 'band_edge' else set())
            assert case.cnt.max() >= 1000 and (case.cnt[case.cnt > 0] == 1).any()
    labels = {c.label for c in cases}
    assert {'clear', 'ties', 'near_ties', 'band_edge', 'all_zero', 'order'} <= labels
    assert ('overflow' in labels) == ('overflow_climb' in labels) == (n_classes >= 520) and ('order_walk' in labels) == (n_classes >= 72)
    assert ('overflow_stream' in labels) == (n_classes > 4096)           # a range longer than one 512-class batch
    edge = [c for c in cases if c.label == 'band_edge'][0]
    assert 0.75 < edge.proof['min_ratio'] <= edge.proof['max_ratio'] < 1.0
    clear = [c for c in cases if c.label == 'clear'][0]
    assert set(lu.winner_positions(n_classes)) == set(clear.want_c.tolist())
    RC = lu.range_len(n_classes)
    assert {0, n_classes - 1, min(7, n_classes - 1)} <= set(clear.want_c.tolist())
    if n_classes > RC:
        assert {RC - 1, RC} <= set(clear.want_c.tolist())
    if RC > 512:
        assert {511, 512} <= set(clear.want_c.tolist())      # inside a multi-batch range


def test_bench_and_fp32_builders_are_what_they_claim():
    for case in bench_builders():
        assert_well_posed(case, 10000)
        assert lu.range_len(10000) == 1256 and (np.array_equal(case.classes, np.arange(10000) % 128) or
                                                np.array_equal(case.classes, (np.arange(10000) + 1) % 128))
    for n_classes in FP32_C:
        for case in fp32_builders(n_classes):
            assert_well_posed(case, n_classes)
        if n_classes > 1:
            reached = lu.fp32_band_pairs(n_classes).proof['reached']
            for nd, (lo, hi) in reached.items():
                assert lu.FP32_REACHED[nd] / 2 < lo <= hi < 1.0 and abs(hi - lu.FP32_REACHED[nd]) < 0.01, (nd, lo, hi)


# ------------------------------------------------------------------------------------------------
# through the hook
# ------------------------------------------------------------------------------------------------
def make_sim(case, n, fp16=True, sigma_omega=0.0, **kw):
    from recogym_amd.sim import Simulator
    P = case.coef_t.shape[0]
    cfg = Configuration({**env_1_args, 'random_seed': 5, 'num_products': P, 'K': 2, 'sigma_omega': sigma_omega})
    logreg = dict(coef_t=case.coef_t, intercept=case.intercept, classes=case.classes)
    if not fp16:
        logreg['fp16'] = False
    kw.setdefault('log_capacity', 0)
    return Simulator(cfg, n, device='cuda:0', policy=FROZEN, policy_seed=0, logreg=logreg, **kw)


def hook_acts(case, fp16=True):
    """One Simulator, one reset_users, one rg_sim_debug_set_history, one hook call -> (actions, counter differences, ledger
    differences)."""
    n = len(case.nd)
    sim = make_sim(case, n, fp16)
    assert hasattr(sim, 'logreg16') == fp16
    sim.reset_users(0, n)
    sim.debug_set_history(case.nd, case.prod, case.cnt)
    c0, l0 = sim.counters(), au.ledger(sim)
    act = sim.debug_logreg_acts()
    c1, l1 = sim.counters(), au.ledger(sim)
    sim.close()
    return act, {k: c1[k] - c0[k] for k in ('lr_acts', 'lr_rows', 'lr_exact')}, {k: l1[k] - l0[k] for k in ('logreg_screen', 'logreg_acts', 'logreg_sample')}


def assert_case(case, fp16, want_a=None):
    act, cnt, led = hook_acts(case, fp16)
    want_a = case.want_a if want_a is None else want_a
    exact = case.exact16 if fp16 else case.exact32
    print(case.label, len(case.nd), cnt, led, 'wrong', int((act != want_a).sum()))
    bad = np.flatnonzero(act != want_a)
    assert not len(bad), (case.label, bad[:8], act[bad[:8]], want_a[bad[:8]], case.nd[bad[:8]])
    assert cnt['lr_acts'] == len(case.nd) and cnt['lr_rows'] == int(case.nd.sum())
    # the path: a clear winner is certified by the screen (no float64), every tie, near tie, band-edge pair and overflow takes
    # float64 — by construction (bit-identical columns; in one range nine of them are nine candidates: the walk)
    assert cnt['lr_exact'] == int(exact.sum()), (case.label, cnt, int(exact.sum()))
    assert (led['logreg_screen'] > 0, led['logreg_acts'] > 0) == ((True, False) if fp16 else (False, True)) and led['logreg_sample'] == 0, led


@gpu
@pytest.mark.parametrize('n_classes', FP16_C)
def test_fp16_form_on_every_builder(n_classes):
    """C = 8, 16: one range and seven empty ones; 56, 64: seven / eight ranges of 8; 72: a ragged range 4 and three empty; 520: a
    last range of 16; 4096: exactly one batch per range; 4104: a second batch of one lane."""
    for case in lu.fp16_builders(n_classes):
        assert_case(case, True)


@gpu
def test_fp16_form_at_the_benchmark_class_count():
    """C = 10 000: ranges of 1 256 classes, batches of 512, 512 and 232; P = 128 with classes = c % P keeps the model small."""
    for case in bench_builders():
        assert_case(case, True)


@gpu
@pytest.mark.parametrize('n_classes', FP32_C)
def test_fp32_form_on_every_builder(n_classes):
    """k_logreg_acts (fp16=False: no padding) at its blocks of 256 classes and waves of 64; nd = 33 takes the float64 walk (lr_exact).
    The band-edge pairs reach 0.2475, 0.396 and 0.905 of the band at nd = 1, 2, 32 (lu.FP32_REACHED, measured against the NumPy
    emulation): every pair is above half of that."""
    for case in fp32_builders(n_classes):
        if len(case.nd):
            assert_case(case, False)


@gpu
@pytest.mark.parametrize('n_classes', [13, 700])
def test_padded_models(n_classes):
    """A model whose class count is no multiple of 8, given to the Simulator with defaults: it pads with copies of the last class.
    Winners: class 0 (certified) and the last class (an exact tie with its copies: float64, the same action)."""
    from recogym_amd.sim import Simulator
    case = lu.clear_winners(n_classes, nds=(1, 9, 33))
    n = len(case.nd)
    assert {0, n_classes - 1} <= set(case.want_c.tolist())
    sim = make_sim(case, n)
    assert hasattr(sim, 'logreg16') and sim.logreg[2].numel() == (n_classes + 7) // 8 * 8
    sim.reset_users(0, n)
    sim.debug_set_history(case.nd, case.prod, case.cnt)
    act = sim.debug_logreg_acts()
    cnt, led = sim.counters(), au.ledger(sim)
    sim.close()
    assert np.array_equal(act, case.want_a)
    assert cnt['lr_exact'] == int((case.want_c == n_classes - 1).sum()) and led['logreg_screen'] > 0 and led['logreg_acts'] == 0


# ------------------------------------------------------------------------------------------------
# whole runs: k_logreg_select and the dirty flag
# ------------------------------------------------------------------------------------------------
@gpu
def test_run_at_4104_classes_matches_the_oracle():
    """P = C = 4 104: ranges of 520 classes, a second batch of one lane in every range.  Duplicated and almost duplicated classes as
    in the config-5-scale test, some of them across the batch border."""
    from oracle import oracle as orc
    from test_hip_parity import run_sim
    P = n_cls = 4104
    rng = np.random.RandomState(15)
    coef_t = rng.standard_normal((P, n_cls)) * 0.1
    intercept = rng.standard_normal(n_cls) * 0.1
    for a, b in ((10, 3000), (511, 512), (519, 520), (77, 4103)):
        coef_t[:, b] = coef_t[:, a]; intercept[b] = intercept[a]
    for a, b in ((20, 2000), (1031, 1032)):
        coef_t[:, b] = coef_t[:, a]; intercept[b] = intercept[a] + 1e-9
    intercept[[10, 3000, 511, 512, 519, 520, 77, 4103, 20, 2000, 1031, 1032]] += 0.6
    pol = dict(policy=FROZEN, policy_seed=0, logreg=dict(coef_t=coef_t, intercept=intercept, classes=np.arange(n_cls, dtype=np.int32)))
    cfg = Configuration({**env_1_args, 'random_seed': 56, 'num_products': P, 'K': 10})
    want = orc.OracleEnv(cfg, rng_mode=orc.RNG_PHILOX, **pol).generate_logs(100)
    rows, cnt, led = run_sim(cfg, 100, with_ledger=True, **pol)
    assert led['logreg_screen'] > 0 and led['logreg_acts'] == 0 and led['logreg_sample'] == 0, led
    gu.assert_rows_equal(rows, {k: want[k] for k in ('u', 't', 'z', 'v', 'a', 'c', 'ps', 'p_click')}, ps_rtol=1e-12, what='logreg 4104 classes')
    used = set(np.unique(rows['a'][rows['z'] == 1]).tolist())
    assert used & {10, 511, 519, 77} and used & {2000, 1032} and not used & {3000, 512, 520, 4103}
    assert cnt['lr_acts'] > 250 and cnt['lr_exact'] > 0 and cnt['hist_overflow'] == 0


@gpu
def test_run_from_placed_band_edge_histories():
    """600 users at C = 72 start a run from placed band-edge histories (rg_sim_debug_set_history, then run).  The check comes from
    the log itself: the action of every bandit and phantom row is the reference's on the placed history plus the user's views
    logged so far."""
    case = lu.band_edge_pairs(72, nds=(1, 2, 7, 8, 9, 11, 12, 13, 16, 33))
    n = 600
    pick = np.arange(n) % len(case.nd)
    nd, prod, cnt = case.nd[pick], case.prod[pick], case.cnt[pick]
    sim = make_sim(case, n, sigma_omega=0.1, log_capacity=None)
    sim.reset_users(0, n)
    sim.debug_set_history(nd, prod, cnt)
    sim.run()
    rows, counters, led = sim.rows(), sim.counters(), au.ledger(sim)
    sim.close()
    assert counters['hist_overflow'] == 0 and counters['live'] == 0 and counters['log_dropped'] == 0
    assert led['logreg_screen'] > 0 and led['logreg_acts'] == 0
    P = case.coef_t.shape[0]
    checked = first = 0
    for u in range(n):
        mine = rows[rows['u'] == u]
        assert (np.diff(mine['t'].astype(np.int64)) > 0).all()
        x = np.zeros(P, dtype=np.int64)
        x[prod[u, :nd[u]]] = cnt[u, :nd[u]]
        seen = False
        for r in mine:
            if r['z'] == 0:
                x[r['v']] += 1
            else:
                p = np.flatnonzero(x)
                assert r['a'] == lu.reference(case.coef_t, case.intercept, case.classes, p, x[p])[1], (u, int(r['t']))
                checked += 1
                first += not seen and r['a'] == case.want_a[pick[u]]
                seen = True
        assert np.count_nonzero(x) <= lu.HIST_ENTRIES
    print('rows checked', checked, 'users whose first act is the placed band-edge decision', first, counters)
    assert checked > 10000 and first > 50 and counters['lr_exact'] > 0


# ------------------------------------------------------------------------------------------------
# the hook's refusals
# ------------------------------------------------------------------------------------------------
@gpu
def test_refusals():
    import torch
    from recogym_amd.sim import Simulator
    lib = _abi.load()
    case = lu.exact_ties(16, nds=(1, 9))
    n = len(case.nd)
    out = torch.zeros(n, dtype=torch.int32, device='cuda:0')
    assert lib.rg_sim_debug_logreg_acts(None, out.data_ptr(), None) == EINVAL
    cfg = Configuration({**env_1_args, 'random_seed': 5, 'num_products': case.coef_t.shape[0], 'K': 2})
    # another policy
    sim = Simulator(cfg, n, device='cuda:0', log_capacity=0)
    sim.reset_users(0, n)
    assert lib.rg_sim_debug_logreg_acts(sim._h, out.data_ptr(), None) == ESTATE and b'RG_POLICY_LOGREG_FROZEN' in lib.rg_last_error()
    sim.close()
    # the sampling form (a class per product)
    P = 12
    rng = np.random.RandomState(1)
    sim = Simulator(Configuration({**env_1_args, 'random_seed': 5, 'num_products': P, 'K': 2}), n, device='cuda:0', policy=FROZEN, policy_seed=1,
                    logreg=dict(coef_t=rng.standard_normal((P, P)), intercept=np.zeros(P), classes=np.arange(P), select_randomly=True), log_capacity=0)
    sim.reset_users(0, n)
    assert lib.rg_sim_debug_logreg_acts(sim._h, out.data_ptr(), None) == EINVAL and b'lr_select_randomly' in lib.rg_last_error()
    sim.close()
    # no model
    rc = make_rg_config(cfg, 5, FROZEN, 0)
    need = lib.rg_sim_workspace_bytes(C.byref(rc), n)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda:0')
    h = C.c_void_p()
    assert lib.rg_sim_create(C.byref(h), C.byref(rc), n, ws.data_ptr(), need) == 0
    assert lib.rg_sim_debug_logreg_acts(h, out.data_ptr(), None) == ESTATE and b'rg_sim_set_logreg' in lib.rg_last_error()
    lib.rg_sim_destroy(h)
    # not right after the reset: before it, and after a step; NULL
    sim = make_sim(case, n)
    assert lib.rg_sim_debug_logreg_acts(sim._h, out.data_ptr(), None) == ESTATE and b'rg_sim_reset_users' in lib.rg_last_error()
    sim.reset_users(0, n)
    assert lib.rg_sim_debug_logreg_acts(sim._h, None, None) == EINVAL
    sim.debug_set_history(case.nd, case.prod, case.cnt)
    assert np.array_equal(sim.debug_logreg_acts(), case.want_a)
    # the hook leaves step 0's act list filled: nothing steps, runs or calls it again before the next reset
    assert lib.rg_sim_step(sim._h, None, None) == ESTATE and b'rg_sim_reset_users' in lib.rg_last_error()
    assert lib.rg_sim_run(sim._h, 1 << 16, None) == ESTATE
    assert lib.rg_sim_debug_logreg_acts(sim._h, out.data_ptr(), None) == ESTATE
    sim.reset_users(0, n)
    sim.step()
    assert lib.rg_sim_debug_logreg_acts(sim._h, out.data_ptr(), None) == ESTATE and b'rg_sim_reset_users' in lib.rg_last_error()
    sim.close()
