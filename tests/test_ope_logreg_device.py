"""Off-policy replay of the frozen LogReg policy on the device (rg_ope_replay_logreg, recogym_amd/csrc/rg_ope_logreg.hip) against
the host loop (LogregFrozenAgent.act through evaluate_agent._host_snips), the reference's own numbers
(tests/golden/ope_logreg_philox_p10.npz) and itself: the argmax form bit for bit, the softmax form to 1e-12 against NumPy (float64
sums over the classes in another order: (C + 4) 2^-52, as for the dense OrganicUserEventCounter forms) and EXACTLY 1 on logs the
device wrote under the same model."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest
import torch

from device_util import close
import golden_util as gu
from make_golden_ope import log_frame
from recogym_amd import _abi
from recogym_amd import evaluate_agent as ev
from recogym_amd.agents.logreg_frozen import LogregFrozenAgent
from recogym_amd.envs.configuration import Configuration
from recogym_amd.envs.reco_env_v1 import env_1_args, rows_to_dataframe
from recogym_amd.sim import Simulator

pytestmark = pytest.mark.gpu


def agent(P, coef, intercept, classes, select_randomly=False):
    return LogregFrozenAgent(Configuration({'num_products': P, 'random_seed': 7, 'with_ps_all': True,
                                            'select_randomly': select_randomly}), coef, intercept, classes)


def fixture_agent(cols, P, select_randomly):
    return agent(P, cols['logreg_coef'], cols['logreg_intercept'], cols['logreg_classes'], select_randomly)


def replay_frame(ag, df):
    """DataFrame -> device replay with the kernel's statistics: (ratio, clicks, sums, stats), host arrays."""
    pol = ev.ope_policy_of(ag)
    assert pol is not None and pol['kind'] == _abi.RG_POLICY_LOGREG_FROZEN
    dl = ev._frame_to_device(df, pol, torch.device('cuda:0'))
    assert dl is not None
    st = {}
    r, c, sums = ev.ope_replay(ag, dl, pol, n_users=int(dl.offsets.numel()) - 1, stats=st)
    assert st['error'] == 0
    return r.cpu().numpy(), c.cpu().numpy(), sums.cpu().numpy(), st


def make_frame(rows, P):
    """rows of (u, t, is_bandit, index, click) -> the reference's DataFrame under a uniform logger."""
    is_b = np.array([r[2] for r in rows], dtype=bool)
    idx = [int(r[3]) for r in rows]
    return pd.DataFrame({'t': np.array([r[1] for r in rows], dtype=np.float32), 'u': [r[0] for r in rows],
                         'z': np.where(is_b, 'bandit', 'organic').astype(object),
                         'v': pd.array([None if b else i for b, i in zip(is_b, idx)], dtype=pd.UInt16Dtype()),
                         'a': pd.array([i if b else None for b, i in zip(is_b, idx)], dtype=pd.UInt16Dtype()),
                         'c': np.array([float(r[4]) if r[2] else np.nan for r in rows], dtype=np.float32),
                         'ps': np.where(is_b, 1.0 / P, np.nan)})


# ---- 1. reference-logged fixtures ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,logged_softmax', [('philox_logreg', False), ('mt_logreg', False), ('hostpath_logreg_random', True)])
def test_self_evaluation_of_reference_logged_fixtures(name, logged_softmax):
    meta, cols = gu.load(name)
    P = meta['env_args']['num_products']
    df = log_frame(cols)
    ag = fixture_agent(cols, P, logged_softmax)
    assert ev.ope_policy_of(ag) is not None
    rewards, ratio = ev.evaluate_SNIPS(ag, df)                       # DataFrame in, device replay
    order = np.argsort(cols['u'], kind='stable')
    evaluated = (cols['z'][order] == 1) & (cols['u'][order] < cols['u'].max())
    assert len(ratio) == int(evaluated.sum()) > 0
    close(ratio, np.ones(len(ratio)), 1e-12 if logged_softmax else 0)
    close(rewards, cols['c'][order][evaluated], 0)
    # the same model in the other form on the same log: the host loop's numbers
    other = fixture_agent(cols, P, not logged_softmax)
    got, _, _, st = replay_frame(other, df)
    _, want = ev._host_snips(other, df)
    close(got, want, 0 if logged_softmax else 1e-12)
    assert 0 < st['acts'] <= len(want)


# ---- 2. the reference's own numbers -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['argmax', 'softmax'])
def test_device_equals_reference_numbers(form):
    want = np.load(f'{gu.GOLDEN}/ope_logreg_philox_p10.npz')
    _, cols = gu.load('philox_p10')
    ag = agent(10, want['logreg_coef'], want['logreg_intercept'], want['logreg_classes'], form == 'softmax')
    assert ev.ope_policy_of(ag) is not None
    rewards, ratio = ev.evaluate_SNIPS(ag, log_frame(cols))
    close(ratio, want[f'{form}__ratio'], 0 if form == 'argmax' else 1e-12)
    close(rewards, want[f'{form}__c'], 0)
    assert np.count_nonzero(ratio) and (form == 'softmax' or np.count_nonzero(ratio) < len(ratio))


# ---- 3. simulator logs: device log in, frame in, host loop --------------------------------------------------------------------
@pytest.mark.parametrize('select_randomly', [False, True])
def test_device_equals_host_loop_on_simulator_logs(select_randomly):
    P, n = 100, 2000
    _, m = gu.load('c5_trained_p100')
    ag = agent(P, m['logreg_coef'], m['logreg_intercept'], m['logreg_classes'], select_randomly)
    cfg = Configuration({**env_1_args, 'random_seed': 7, 'num_products': P, 'K': 5})
    sim = Simulator(cfg, n, device='cuda:0')
    sim.reset_users(0, n)
    sim.run()
    dl = sim.device_log()
    df = rows_to_dataframe(sim.rows(), P)
    st = {}
    r_dev, c_dev, sums = ev.ope_replay(ag, dl, stats=st)
    r_frame, c_frame, _, from_frame = ev._device_or_none(ag, df)
    assert from_frame and torch.equal(r_dev, r_frame) and torch.equal(c_dev, c_frame)
    df_small = df[df['u'] < 300].reset_index(drop=True)          # the host loop on the first 300 users (time budget)
    n_small = int((df_small['z'] == 'bandit').sum() - (df_small[df_small['u'] == 299]['z'] == 'bandit').sum())
    _, want = ev._host_snips(ag, df_small)
    close(r_dev[:n_small].cpu().numpy(), want, 1e-12 if select_randomly else 0)
    # acts: the bandit rows whose user had an organic row since its previous bandit row (every user opens with an organic row)
    last = int(dl.offsets[n - 1].item())
    is_b = ((dl.rows[:last, 2] & _abi.RG_EV_BANDIT) != 0).cpu().numpy()
    acts = int((is_b[1:] & ~is_b[:-1]).sum())
    assert st['error'] == 0 and st['acts'] == acts and st['rows_read'] >= acts
    if select_randomly:
        assert st['exact'] == st['acts']
    else:
        assert 0 <= st['exact'] < st['acts']
    s = sums.cpu().numpy()
    assert s[0] == r_dev.numel() == int(is_b.sum())
    ips = ev.evaluate_IPS(ag, dl)
    assert torch.equal(ips, c_dev * r_dev)


# ---- 4. class-set shapes ------------------------------------------------------------------------------------------------------
def test_class_set_shapes():
    meta, cols = gu.load('philox_logreg')
    P = meta['env_args']['num_products']
    df = log_frame(cols)
    coef, b, cls = cols['logreg_coef'], cols['logreg_intercept'], cols['logreg_classes']
    shapes = {'every second class': agent(P, coef[::2], b[::2], cls[::2]),
              'sklearn two-class form': agent(P, coef[7:8], b[7:8], np.array([3, 8])),
              'one class': agent(P, coef[5:6], b[5:6], np.array([5]))}
    assert shapes['every second class'].classes.size == 15 and shapes['sklearn two-class form'].classes.size == 2
    for key, ag in shapes.items():
        got, _, _, st = replay_frame(ag, df)
        _, want = ev._host_snips(ag, df)
        close(got, want, 0)
        assert 0 < np.count_nonzero(got) < got.size, key          # actions outside the class set get 0


# ---- 5. ties and the certificate ------------------------------------------------------------------------------------------------
def _random_frame(P, n_users, seed, max_rows=40):
    rng = np.random.RandomState(seed)
    rows = []
    for uid in range(n_users + 1):                                 # (+ the highest user, which is not evaluated)
        t = 0
        for i in range(rng.randint(4, max_rows)):
            is_b = i > 0 and rng.rand() < 0.5
            rows.append((uid, t, is_b, rng.randint(P), rng.rand() < 0.3))
            t += 1
    return make_frame(rows, P)


def test_ties_and_near_ties_go_to_the_float64_walk():
    """P = 70 products, C = 130 classes (the 64- and 128-class block edges and a ragged tail; the labels repeat, classes[c] = c % 70)."""
    P, Cn = 70, 130
    df = _random_frame(P, 50, seed=5)
    classes = np.arange(Cn) % P
    rng = np.random.RandomState(9)
    zero = agent(P, np.zeros((Cn, P)), np.zeros(Cn), classes)
    got, _, _, st = replay_frame(zero, df)
    _, want = ev._host_snips(zero, df)
    close(got, want, 0)
    a_rows = np.array(df['a'][df['z'] == 'bandit'][:got.size].astype(int))
    assert np.array_equal(got != 0, a_rows == 0)                   # always class index 0
    # exact ties across the block edges: columns 63 = 64 and 127 = 128 (and 129 = 5), the pairs often the best
    coef = rng.standard_normal((Cn, P)) * 0.1
    b = rng.standard_normal(Cn) * 0.1
    coef[63, :35] = np.abs(rng.standard_normal(35)) + 1.0
    coef[127, 35:] = np.abs(rng.standard_normal(35)) + 1.0
    for x, y in ((63, 64), (127, 128), (5, 129)):
        coef[y] = coef[x]; b[y] = b[x]
    ties = agent(P, coef, b, classes)
    got, _, _, st = replay_frame(ties, df)
    _, want = ev._host_snips(ties, df)
    close(got, want, 0)
    assert st['exact'] > 0 and np.count_nonzero(got)
    # the best two columns differ by a factor 1 +- 2^-40: beyond fp32, the later class a hair better for one pair
    coef2 = rng.standard_normal((Cn, P)) * 0.1
    w = np.abs(rng.standard_normal(P)) + 1.0
    coef2[62], coef2[65] = w * (1.0 - 2.0 ** -40), w * (1.0 + 2.0 ** -40)
    near = agent(P, coef2, b, classes)
    near.intercept[62] = near.intercept[65] = 0.0
    got, _, _, st = replay_frame(near, df)
    _, want = ev._host_snips(near, df)
    close(got, want, 0)
    assert st['exact'] > 0 and np.count_nonzero(got)


# ---- 6. history beyond the registers and beyond LDS ---------------------------------------------------------------------------
def test_long_histories():
    """Users with 400 distinct products (beyond the 64 register entries) and with 700 (beyond the 512 LDS entries: the per-wave
    global list), a user of 3 rows, a user with organic rows only, a user id without rows."""
    P = 1000
    rng = np.random.RandomState(1)
    rows = []
    for uid, n, distinct in ((0, 1500, 400), (1, 1500, 700), (2, 3, 3), (3, 5, 5), (5, 6, 6), (6, 2, 2)):
        views = rng.permutation(P)[:distinct]
        t = 0
        for i in range(n):
            if i % 2 == 0 or uid == 3:
                rows.append((uid, t, False, views[(i // 2) % len(views)], False)); t += 1
            if uid != 3 and (uid != 1 or i % 8 == 0):              # (user 1: an act per 4 views, the host loop's time)
                rows.append((uid, t, True, rng.randint(8), rng.rand() < 0.3)); t += 1
    df = make_frame(rows, P)
    assert (df['u'] == 0).sum() > 1024 and not (df['u'] == 4).any() and not ((df['u'] == 3) & (df['z'] == 'bandit')).any()
    # 1 000 classes with the labels 0 .. 7 (and logged actions among them: the ratios are not all 0)
    ag = agent(P, rng.standard_normal((P, P)) * 0.3, rng.standard_normal(P) * 0.1, np.arange(P) % 8)
    got, _, _, st = replay_frame(ag, df)
    _, want = ev._host_snips(ag, df)
    close(got, want, 0)
    assert st['rows_read'] > 700 * 100 and np.count_nonzero(got)


# ---- 7. the device's own logs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('select_randomly', [False, True])
def test_self_evaluation_of_device_logs_is_exact_and_deterministic(select_randomly):
    n, P = 20_000, 100
    _, m = gu.load('c5_trained_p100')
    ag = agent(P, m['logreg_coef'], m['logreg_intercept'], m['logreg_classes'], select_randomly)
    lr = dict(coef_t=ag.coef_t, intercept=ag.intercept, classes=ag.classes)
    if select_randomly:
        lr['select_randomly'] = True
    cfg = Configuration({**env_1_args, 'random_seed': 23, 'num_products': P, 'K': 20})
    sim = Simulator(cfg, n, device='cuda:0', policy=_abi.RG_POLICY_LOGREG_FROZEN, policy_seed=7 if select_randomly else 0, logreg=lr)
    sim.reset_users(0, n)
    sim.run()
    assert sim.counters()['hist_overflow'] == 0
    dl = sim.device_log()
    assert (dl.ps is not None) == select_randomly                  # softmax: the float64 side array; argmax: the rows' own ps = 1
    r, c, sums = ev.ope_replay(ag, dl)
    assert r.numel() > n and bool((r == 1.0).all())
    last = int(dl.offsets[n - 1].item())
    code = dl.rows[:last, 2]
    clicks = int((((code & _abi.RG_EV_BANDIT) != 0) & ((code & _abi.RG_EV_CLICK) != 0)).sum().item())
    s = sums.cpu().numpy()
    assert s[0] == r.numel() and s[1] == clicks and s[2] == r.numel()
    r2, _, sums2 = ev.ope_replay(ag, dl)
    assert torch.equal(r, r2) and np.array_equal(s.view(np.uint64), sums2.cpu().numpy().view(np.uint64))


# ---- 8. ABI errors ------------------------------------------------------------------------------------------------------------
def test_abi_errors():
    """Every call is well-formed apart from the one argument under test; all are refused before anything runs on the model."""
    lib = _abi.load()
    dev = torch.device('cuda:0')
    P = 1025                                                       # (arrays large enough for every case below)
    coef_t = torch.zeros((P, P), dtype=torch.float64, device=dev)
    b = torch.zeros(P, dtype=torch.float64, device=dev)
    cls = torch.arange(P, dtype=torch.int32, device=dev)
    swapped = cls.clone()
    swapped[1], swapped[2] = 2, 1
    c32, b32, wmax = coef_t.float(), b.float(), torch.zeros(P, dtype=torch.float32, device=dev)
    raw = np.zeros((3, 4), dtype=np.uint32)
    raw[:, 1] = [0, 1, 2]
    raw[:, 2] = [1, 2 | _abi.RG_EV_BANDIT, 0 | _abi.RG_EV_BANDIT | _abi.RG_EV_CLICK]
    rows = torch.from_numpy(raw.view(np.int32)).to(dev)
    offsets = torch.tensor([0, 3], dtype=torch.int64, device=dev)
    ratio = torch.full((3,), -7.0, dtype=torch.float64, device=dev)
    sums = torch.full((3,), -7.0, dtype=torch.float64, device=dev)

    def model(**over):
        kw = dict(num_products=4, n_classes=4, select_randomly=0, reserved=0, coef_t=coef_t.data_ptr(), intercept=b.data_ptr(),
                  classes=cls.data_ptr(), coef32_t=c32.data_ptr(), intercept32=b32.data_ptr(), wmax=wmax.data_ptr(), bmax=0.0,
                  reserved2=0)
        kw.update(over)
        return _abi.RgOpeLogreg(**kw)

    need = lib.rg_ope_logreg_workspace_bytes(C.byref(model()), 1, 3)
    assert need >= 256
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)

    def call(m, **over):
        a = dict(rows=rows.data_ptr(), offsets=offsets.data_ptr(), n_users=1, max_rows=3, mode=_abi.RG_OPE_PS_CONST, ps=None,
                 ps_const=0.25, ratio=ratio.data_ptr(), click=None, sums=sums.data_ptr(), ws=ws.data_ptr(), ws_bytes=need)
        a.update(over)
        with torch.cuda.device(dev):
            rc = lib.rg_ope_replay_logreg(C.byref(m) if m is not None else None, a['rows'], a['offsets'], a['n_users'], a['max_rows'],
                                          a['mode'], a['ps'], a['ps_const'], a['ratio'], a['click'], a['sums'], a['ws'], a['ws_bytes'],
                                          None)
        return rc, lib.rg_last_error()

    einval = [('null model', None, {}),
              ('null coef_t', model(coef_t=None), {}), ('null intercept', model(intercept=None), {}),
              ('null classes', model(classes=None), {}),
              ('null rows', model(), dict(rows=None)), ('null offsets', model(), dict(offsets=None)),
              ('null ratio', model(), dict(ratio=None)), ('null sums', model(), dict(sums=None)),
              ('null workspace', model(), dict(ws=None)),
              ('null ps array', model(), dict(mode=_abi.RG_OPE_PS_ARRAY, ps=None)),
              ('n_classes == 0', model(n_classes=0), {}), ('num_products == 0', model(num_products=0), {}),
              ('fp32 group: coef32_t only', model(intercept32=None, wmax=None), {}),
              ('fp32 group: no wmax', model(wmax=None), {}),
              ('softmax: n_classes != num_products', model(select_randomly=1, n_classes=3, coef32_t=None, intercept32=None, wmax=None), {}),
              ('softmax: P > 1024', model(select_randomly=1, num_products=1025, n_classes=1025, coef32_t=None, intercept32=None,
                                          wmax=None), {}),
              ('softmax: classes not 0 .. P-1', model(select_randomly=1, classes=swapped.data_ptr(), coef32_t=None, intercept32=None,
                                                      wmax=None), {}),
              ('an action >= P', model(num_products=2, n_classes=2), {}),
              ('more rows than max_user_rows', model(), dict(max_rows=2))]
    for what, m, over in einval:
        rc, msg = call(m, **over)
        assert rc == -1 and b'rg_ope_replay_logreg' in msg, (what, rc, msg)
    rc, msg = call(model(), ws_bytes=need - 1)
    assert rc == -3 and b'workspace' in msg, (rc, msg)
    assert lib.rg_ope_logreg_workspace_bytes(None, 1, 3) == 0 and b'null' in lib.rg_last_error()
    # a user that opens with a bandit row
    rc, msg = call(model(), offsets=torch.tensor([1, 3], dtype=torch.int64, device=dev).data_ptr())
    assert rc == -1 and b'bandit' in msg
    torch.cuda.synchronize()
    assert bool((ratio == -7.0).all()) and bool((sums == -7.0).all())      # nothing was written by any refused call
    # ... and the well-formed call: an all-zero model acts 0 — the clicked row's action
    for m in (model(), model(select_randomly=1, coef32_t=None, intercept32=None, wmax=None)):
        rc, msg = call(m)
        assert rc == 0, msg
        torch.cuda.synchronize()
        pi = [0.0, 1.0] if not m.select_randomly else [0.25, 0.25]
        assert ratio.cpu().tolist() == [-7.0, pi[0] / 0.25, pi[1] / 0.25]
        assert sums.cpu().tolist() == [2.0, pi[1] / 0.25, (pi[0] + pi[1]) / 0.25]
        assert ws[:32].view(torch.int64).cpu().tolist() == [0, 1, 1, 1]    # one act (one float64 act: the tie), one coef_t row
