"""The replay form of the likelihood agent, host side: the hook that offers it (ope_policy_checked — ope_policy stays None), the
ctypes mirror of struct rg_ope_poly against the header, the ABI version in its three places, and the host's confirmation of the
acts a replay lists as unresolved (sim.poly_replay_verify) on hand-made logs.  No device needed."""
import ctypes as C
import os
import re

import numpy as np
import torch
from scipy.special import expit

import golden_util as gu
from make_golden_ope import log_frame
from recogym_amd import _abi
from recogym_amd import agents
from recogym_amd import evaluate_agent as ev
from recogym_amd.agents.logreg_poly import LogregPolyAgent, LogregPolyFrozenAgent, logreg_poly_args, poly_decisions
from recogym_amd.envs.configuration import Configuration
from recogym_amd.sim import DeviceLog, poly_host_act, poly_replay_verify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def frozen(P=6, seed=2, **cfg):
    w = np.random.RandomState(seed).randn(1, 2 * P + P * P)
    return LogregPolyFrozenAgent(Configuration({'num_products': P, **cfg}), w, [0.5])


def test_the_hook_is_a_dict_with_the_model_under_ps_all():
    ag = frozen(with_ps_all=True)
    pol = ag.ope_policy_checked()
    assert pol['kind'] == _abi.RG_POLICY_LOGREG_POLY and pol['num_products'] == 6 and pol['policy_seed'] == 0
    lp = pol['logreg_poly']
    assert lp['wf'] is ag.wf and lp['wa'] is ag.wa and lp['wk'] is ag.wk and lp['intercept'] == 0.5
    assert ev.ope_checked_policy_of(ag)['logreg_poly']['wk'] is ag.wk
    assert not ev._draws(pol)                                      # nothing drawn: a float clock does not disqualify a log


def test_the_hook_is_none_where_only_the_host_loop_is_exact():
    assert frozen().ope_policy_checked() is None                   # no `ps-a` without with_ps_all
    assert frozen(with_ps_all=False).ope_policy_checked() is None
    hist = frozen(with_ps_all=True, weight_history_function=gu.WEIGHT_FUNCS['inverse'])
    assert hist.ope_policy_checked() is None and ev.ope_checked_policy_of(hist) is None
    # agents without the hook
    assert ev.ope_checked_policy_of(agents.RandomAgent(Configuration({'num_products': 6, 'random_seed': 1, 'with_ps_all': True}))) is None


def test_ope_policy_stays_none_and_epsilon_greedy_has_neither_form():
    ag = frozen(with_ps_all=True)
    assert ag.ope_policy() is None and ev.ope_policy_of(ag) is None
    eg = agents.EpsilonGreedy(Configuration({**agents.epsilon_greedy_args, 'num_products': 6, 'random_seed': 1, 'with_ps_all': True}), ag)
    assert eg.device_policy() is None and eg.ope_policy() is None and ev.ope_policy_of(eg) is None
    assert ev.ope_checked_policy_of(eg) is None


def test_trained_agent_delegates_to_its_built_model():
    _, cols = gu.load('poly_p10')
    train = {k[len('trainlog_'):]: v for k, v in cols.items() if k.startswith('trainlog_')}
    ag = LogregPolyAgent(Configuration({**logreg_poly_args, 'num_products': 10, 'random_seed': 7, 'with_ps_all': True}))
    ag.train_from_log(log_frame(train))
    assert ag.frozen is None
    pol = ev.ope_checked_policy_of(ag)                              # builds the model
    assert ag.frozen is not None and pol is not None and pol['kind'] == _abi.RG_POLICY_LOGREG_POLY
    want = ag.frozen.ope_policy_checked()
    for k in ('wf', 'wa', 'wk'):
        assert pol['logreg_poly'][k] is want['logreg_poly'][k]
    assert ag.ope_policy() is None and ev.ope_policy_of(ag) is None


def test_struct_layout_matches_header():
    header = open(os.path.join(ROOT, 'include', 'recogym_hip.h')).read()
    struct = header[header.index('typedef struct rg_ope_poly {'):header.index('} rg_ope_poly;')]
    fields = re.findall(r'^\s*(const\s+\w+\s*\*|uint32_t|double)\s*([a-zA-Z_0-9]+);', struct, flags=re.M)
    assert [n for _, n in fields] == [n for n, _ in _abi.RgOpePoly._fields_], fields
    size = {'uint32_t': 4}
    want_sizes = [size.get(t, 8) for t, _ in fields]                # (pointers and the double)
    assert [C.sizeof(t) for _, t in _abi.RgOpePoly._fields_] == want_sizes
    offs, at = [], 0
    for s in want_sizes:
        at = (at + s - 1) // s * s
        offs.append(at)
        at += s
    assert [getattr(_abi.RgOpePoly, n).offset for n, _ in _abi.RgOpePoly._fields_] == offs
    assert C.sizeof(_abi.RgOpePoly) == (at + 7) // 8 * 8 == 48
    for name in ('rg_ope_poly_workspace_bytes', 'rg_ope_replay_poly'):
        assert name in _abi.SYMBOLS and re.search(r'\b' + name + r'\s*\(', header)
    assert _abi.SYMBOLS['rg_ope_replay_poly'][1][1:] == _abi.SYMBOLS['rg_ope_replay_logreg'][1][1:]
    assert _abi.SYMBOLS['rg_ope_poly_workspace_bytes'][1][1:] == _abi.SYMBOLS['rg_ope_logreg_workspace_bytes'][1][1:]


def test_abi_version_is_the_same_in_its_three_places():
    header = open(os.path.join(ROOT, 'include', 'recogym_hip.h')).read()
    md = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert int(re.search(r'#define RG_ABI_VERSION (\d+)', header).group(1)) == 15
    assert _abi.RG_ABI_VERSION == 15
    assert int(re.search(r'rg_abi_version\(\) == (\d+)', md).group(1)) == 15


# ---- the confirmation step ---------------------------------------------------------------------------------------------------
def hand_log(users, P):
    """users: one list of (is_bandit, index) per user -> DeviceLog on the host."""
    raw, offsets = [], [0]
    for u, rows in enumerate(users):
        for t, (b, i) in enumerate(rows):
            raw.append((u, t, int(i) | (_abi.RG_EV_BANDIT if b else 0), 0))
        offsets.append(len(raw))
    rows = torch.from_numpy(np.array(raw, dtype=np.uint32).reshape(-1, 4).view(np.int32))
    return DeviceLog(rows, torch.tensor(offsets, dtype=torch.int64), 1.0 / P, 0, P, None)


def constant_model(z1, z2, P=10):
    """wf = wk = 0: every history decides on z[a] = a wa[a] — z[1] = z1, z[2] = z2, the rest 0 (test_logreg_poly_device.constant_agent)."""
    wa = np.zeros(P)
    wa[1], wa[2] = z1, z2 / 2.0
    assert 2.0 * wa[2] == z2
    return np.zeros(P), wa, np.zeros((P, P)), 0.0


O, B = False, True
LOG = [[(O, 3), (B, 1), (O, 4), (B, 2), (B, 2)], [(O, 5), (O, 5), (B, 0)], [(O, 1)]]


def test_confirmed_refuted_and_overflow():
    dl = hand_log(LOG, 10)
    ok = constant_model(25.0, 25.0 + 2.0 ** -12)                    # expit tells the pair apart: the host acts 2, as the device
    assert expit(25.0) < expit(25.0 + 2.0 ** -12)
    acts = np.array([[0, 1, 2], [0, 3, 2], [1, 2, 2]], dtype=np.uint32)
    assert poly_replay_verify(dl, acts, False, ok) is True
    assert poly_replay_verify(dl, acts[:0], False, ok) is True
    assert poly_replay_verify(dl, acts, True, ok) is False          # the list did not hold every act
    assert poly_replay_verify(dl, acts[:0], True, ok) is False
    z2 = next(z for z in (25.0 + 2.0 ** -e for e in range(20, 46)) if expit(z) == expit(25.0))
    merged = constant_model(25.0, z2)                               # scipy merges them: the host acts 1, the device said 2
    assert poly_replay_verify(dl, acts, False, merged) is False
    assert poly_replay_verify(dl, acts[2:], False, merged) is False
    assert poly_replay_verify(dl, np.array([[1, 2, 1]], dtype=np.uint32), False, merged) is True


def history_model(P=10):
    """Decisions that depend on the history (test_logreg_poly_device.history_agent): z[2] = 25, z[1] = 25 + 2^-16 (a sum of small
    integers g[p] over the views) — which of the two expit prefers changes with the views."""
    rng = np.random.RandomState(17)
    wa = np.zeros(P)
    wa[1], wa[2] = 25.0, 12.5
    wk = np.zeros((P, P))
    wk[1] = rng.randint(-3, 4, P) * 2.0 ** -16
    return np.zeros(P), wa, wk, 0.0


def test_the_history_of_a_listed_act_is_the_organic_rows_before_it_and_no_later_ones():
    """A user whose action changes along its views: at every bandit position the function must judge the act on exactly the
    organic rows before that position — the action of the full history, or of a shorter one, is refuted where it differs."""
    m = history_model()
    views = [3, 7, 7, 1, 9, 0, 4, 4, 8, 2, 6, 5]
    rows, want = [], []                                              # an organic row, then a bandit row, alternating
    for i, v in enumerate(views):
        rows.append((O, v))
        prods, cnts = np.unique(views[:i + 1], return_counts=True)
        a = int(np.argmax(expit(poly_decisions(prods, cnts, *m))))
        assert a == poly_host_act(views[:i + 1], m)
        want.append((len(rows), a))
        rows.append((B, a))
    assert len({a for _, a in want}) > 1, 'the model must act differently on different prefixes'
    other = [[(O, 2), (B, 0)]]
    dl = hand_log(other + [rows] + other, 10)                        # the user under test is neither first nor last
    acts = np.array([(1, pos, a) for pos, a in want], dtype=np.uint32)
    assert poly_replay_verify(dl, acts, False, m) is True
    checked = 0
    for j in range(1, len(want)):
        if want[j][1] != want[j - 1][1]:
            # the action of the history one view shorter / one view longer at this position: refuted
            assert poly_replay_verify(dl, np.array([(1, want[j][0], want[j - 1][1])], dtype=np.uint32), False, m) is False
            assert poly_replay_verify(dl, np.array([(1, want[j - 1][0], want[j][1])], dtype=np.uint32), False, m) is False
            checked += 1
    assert checked > 0
    # bandit rows before the position are no views: the same act listed at the user's later bandit row of the same session
    two = [(O, 3), (B, 9), (B, 9), (O, 7), (B, 0)]
    dl2 = hand_log([two, [(O, 0)]], 10)
    a1, a2 = poly_host_act([3], m), poly_host_act([3, 7], m)
    assert poly_replay_verify(dl2, np.array([(0, 1, a1), (0, 2, a1), (0, 4, a2)], dtype=np.uint32), False, m) is True
