"""The replay form of the likelihood agent on a time-weighted view history, host side: the hook that offers it (the count form's
dict plus `weight_history`), EpsilonGreedy's refusal of it, the ctypes mirror of struct rg_ope_poly_w against the header, the
argument checks of rg_ope_replay_poly_w (they answer before a device is looked for) and the host's confirmation of the acts a replay
lists as unresolved (sim.weighted_replay_verify) on hand-made logs.  No device needed."""
import ctypes as C
import os
import re

import numpy as np
import torch

import golden_util as gu
from recogym_amd import _abi
from recogym_amd import agents
from recogym_amd import evaluate_agent as ev
from recogym_amd.agents.logreg_poly import LogregPolyAgent, LogregPolyFrozenAgent
from recogym_amd.agents.views_history import weight_table
from recogym_amd.envs.configuration import Configuration
from recogym_amd.sim import DeviceLog, weighted_host_act, weighted_replay_verify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RG_EINVAL, RG_ENOMEM = -1, -3


def exp_t(t):
    return np.exp(-t)


def frozen(P=6, seed=2, **cfg):
    w = np.random.RandomState(seed).randn(1, 2 * P + P * P)
    return LogregPolyFrozenAgent(Configuration({'num_products': P, **cfg}), w, [0.5])


# ---- the hook --------------------------------------------------------------------------------------------------------------------
def test_the_hook_carries_the_weight_table_under_the_key():
    for fn, f32 in ((exp_t, True), (gu.WEIGHT_FUNCS['exp_0.2'], False), (gu.WEIGHT_FUNCS['inverse'], False)):
        ag = frozen(with_ps_all=True, weight_history_function=fn, device_weight_history=True)
        pol = ag.ope_policy_checked()
        assert pol is not None and pol['kind'] == _abi.RG_POLICY_LOGREG_POLY and pol['num_products'] == 6 and pol['policy_seed'] == 0
        lp = pol['logreg_poly']
        assert lp['wf'] is ag.wf and lp['wa'] is ag.wa and lp['wk'] is ag.wk and lp['intercept'] == 0.5
        table, is_f32 = weight_table(fn)
        assert lp['weight_history'] is ag.weight_history and lp['weight_history']['f32'] == is_f32 == f32
        got = lp['weight_history']['table']
        assert got.dtype == table.dtype and got.tobytes() == table.tobytes()
        assert ev.ope_checked_policy_of(ag)['logreg_poly']['weight_history'] is ag.weight_history
        assert ev._weighted(pol) and not ev._draws(pol)
        assert ag.ope_policy() is None


def test_the_hook_is_none_without_the_key_without_ps_all_and_without_a_table():
    assert frozen(with_ps_all=True, weight_history_function=exp_t).ope_policy_checked() is None            # no device_weight_history
    assert frozen(with_ps_all=True, weight_history_function=exp_t, device_weight_history=False).ope_policy_checked() is None
    assert frozen(weight_history_function=exp_t, device_weight_history=True).ope_policy_checked() is None    # no `ps-a`
    not_elementwise = frozen(with_ps_all=True, weight_history_function=lambda t: t / t.sum(), device_weight_history=True)
    assert not_elementwise.weight_history is None and not_elementwise.ope_policy_checked() is None
    # the count form is what it was: no `weight_history` key
    pol = frozen(with_ps_all=True).ope_policy_checked()
    assert 'weight_history' not in pol['logreg_poly'] and not ev._weighted(pol)


def test_the_trained_agent_delegates():
    ag = LogregPolyAgent(Configuration({**agents.logreg_poly_args, 'num_products': 6, 'with_ps_all': True, 'weight_history_function': exp_t,
                                        'device_weight_history': True}))
    ag.frozen = frozen(with_ps_all=True, weight_history_function=exp_t, device_weight_history=True)
    ag._ready = lambda: ag.frozen
    assert ag.ope_policy_checked()['logreg_poly']['weight_history'] is ag.frozen.weight_history


def test_epsilon_greedy_round_a_weighted_agent_has_no_replay_form():
    inner = frozen(with_ps_all=True, weight_history_function=exp_t, device_weight_history=True)
    eg = agents.EpsilonGreedy(Configuration({**agents.epsilon_greedy_args, 'num_products': 6, 'random_seed': 1, 'with_ps_all': True,
                                             'device_models': True}), inner)
    assert eg.ope_policy_checked() is None and eg.ope_policy() is None and ev._replay_policy_of(eg) is None
    # the same wrapper round the count form keeps its replay form
    plain = agents.EpsilonGreedy(Configuration({**agents.epsilon_greedy_args, 'num_products': 6, 'random_seed': 1, 'with_ps_all': True,
                                                'device_models': True}), frozen(with_ps_all=True))
    assert plain.ope_policy_checked() is not None
    # ... and a dict that pairs the two never reaches an entry point (returned before a device or the library is touched)
    pol = dict(inner.ope_policy_checked(), epsilon_greedy=dict(epsilon=0.1, seed=1, pure_new=True))
    assert ev._replay_target(pol, torch.device('cpu')) is None


def test_the_replay_entry_table_and_the_head():
    assert ev._REPLAY_ENTRY['poly_w', False] == ('rg_ope_poly_w_workspace_bytes', 'rg_ope_replay_poly_w')
    assert ('poly_w', True) not in ev._REPLAY_ENTRY
    assert 'poly_w' in ev._REFUTED and 'host loop' in ev._REFUTED['poly_w'] and 'host loop' in ev._CLOCK_RANGE
    assert _abi.OPE_HEADS['poly_w'] == _abi.OPE_HEADS['poly'] + ('range',)


# ---- the struct, the symbols, the version --------------------------------------------------------------------------------------------
def test_struct_layout_matches_header():
    header = open(os.path.join(ROOT, 'include', 'recogym_hip.h')).read()
    struct = header[header.index('typedef struct rg_ope_poly_w {'):header.index('} rg_ope_poly_w;')]
    fields = re.findall(r'^\s*(const\s+\w+\s*\*|uint32_t|double|rg_ope_poly)\s*([a-zA-Z_0-9]+);', struct, flags=re.M)
    assert [n for _, n in fields] == [n for n, _ in _abi.RgOpePolyW._fields_] == ['model', 'table', 'n', 'accumulate_f32'], fields
    size = {'uint32_t': 4, 'rg_ope_poly': C.sizeof(_abi.RgOpePoly)}
    want_sizes = [size.get(t, 8) for t, _ in fields]                # (the pointer)
    assert [C.sizeof(t) for _, t in _abi.RgOpePolyW._fields_] == want_sizes
    offs, at = [], 0
    for s in want_sizes:
        al = min(s, 8)
        at = (at + al - 1) // al * al
        offs.append(at)
        at += s
    assert [getattr(_abi.RgOpePolyW, n).offset for n, _ in _abi.RgOpePolyW._fields_] == offs == [0, 48, 56, 60]
    assert C.sizeof(_abi.RgOpePolyW) == (at + 7) // 8 * 8 == 64
    assert _abi.RgOpePolyW._fields_[0][1] is _abi.RgOpePoly
    for name in ('rg_ope_poly_w_workspace_bytes', 'rg_ope_replay_poly_w'):
        assert name in _abi.SYMBOLS and re.search(r'\b' + name + r'\s*\(', header)
    # rg_ope_replay_poly's arguments with d_t16 ahead of ps_mode and d_act ahead of the workspace
    plain, w = _abi.SYMBOLS['rg_ope_replay_poly'][1][1:], _abi.SYMBOLS['rg_ope_replay_poly_w'][1][1:]
    assert w == plain[:4] + [C.c_void_p] + plain[4:10] + [C.c_void_p] + plain[10:]
    assert _abi.SYMBOLS['rg_ope_poly_w_workspace_bytes'][1][1:] == _abi.SYMBOLS['rg_ope_poly_workspace_bytes'][1][1:]
    proto = header[header.index('int rg_ope_replay_poly_w('):]
    proto = proto[:proto.index(';')]
    assert proto.count(',') + 1 == len(_abi.SYMBOLS['rg_ope_replay_poly_w'][1])
    assert re.search(r'const uint16_t\* d_t16, uint32_t ps_mode', proto) and re.search(r'int32_t\* d_act, void\* d_workspace', proto)


def test_abi_version_stays_15_and_the_header_says_what_was_added():
    header = open(os.path.join(ROOT, 'include', 'recogym_hip.h')).read()
    assert int(re.search(r'#define RG_ABI_VERSION (\d+)', header).group(1)) == 15 == _abi.RG_ABI_VERSION
    assert re.search(r'v15, additive since: rg_ope_poly_w_workspace_bytes / rg_ope_replay_poly_w', header)
    assert 'rg_ope_replay_poly_w' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


# ---- the argument checks: before the device check, so they answer here ---------------------------------------------------------------
def test_validation_codes():
    lib = _abi.load()
    P = 6
    arr = (C.c_double * 64)()                                       # stands for every model array: nothing is dereferenced
    rows = (C.c_uint8 * 256)()
    base = C.addressof(rows)
    aligned = base + (-base) % 16
    ptr = C.addressof(arr)

    def model(**over):
        m = _abi.RgOpePoly(num_products=P, n_steps=4, wf=ptr, wa=ptr, wk_t=ptr, th=ptr, intercept=0.0)
        w = dict(model=m, table=ptr, n=32768, accumulate_f32=0)
        w.update(over)
        return _abi.RgOpePolyW(**w)

    def call(m, n_users=1, d_rows=aligned, t16=ptr, ws_bytes=None, max_rows=8):
        need = lib.rg_ope_poly_w_workspace_bytes(C.byref(m), n_users, max_rows) if m is not None else 0
        return lib.rg_ope_replay_poly_w(None if m is None else C.byref(m), d_rows, ptr, n_users, max_rows, t16, _abi.RG_OPE_PS_CONST, None, 0.25,
                                        ptr, None, ptr, None, ptr, need if ws_bytes is None else ws_bytes, None)

    def refused(rc, code, text):
        msg = lib.rg_last_error().decode()
        assert rc == code and text in msg, (rc, msg)

    assert lib.rg_ope_poly_w_workspace_bytes(None, 1, 8) == 0
    refused(call(None), RG_EINVAL, 'null model')
    refused(call(model(table=None)), RG_EINVAL, 'weight table')
    refused(call(model(n=0)), RG_EINVAL, 'weight table')
    refused(call(model(n=32769)), RG_EINVAL, 'weight table')
    bad = model()
    bad.model.wk_t = None
    refused(call(bad), RG_EINVAL, 'null wf / wa / wk_t / th')
    bad = model()
    bad.model.n_steps = 1025
    refused(call(bad), RG_EINVAL, 'n_steps')
    refused(call(model(), t16=None), RG_EINVAL, 'null times')
    need = lib.rg_ope_poly_w_workspace_bytes(C.byref(model()), 1, 8)
    assert need > 256 + 4096 * 12
    refused(call(model(), ws_bytes=need - 1), RG_ENOMEM, 'workspace')
    refused(call(model(), d_rows=aligned + 8), RG_EINVAL, '16-byte aligned')
    # a null d_t16 is no error of a call without users: the next check answers (every call here is refused before a device is touched)
    refused(call(model(), n_users=0, t16=None, ws_bytes=16), RG_ENOMEM, 'workspace')
    # the workspace grows with the timed list (8 bytes per row and wave) and, beyond kPolyHist = 256 products, the spill scratch
    # (max_user_rows + 1 words per wave; 104 and 208 words: both sizes are whole 256-byte units)
    small = lib.rg_ope_poly_w_workspace_bytes(C.byref(model()), 4, 103)
    assert lib.rg_ope_poly_w_workspace_bytes(C.byref(model()), 4, 207) - small == 4 * 104 * 8
    big = model()
    big.model.num_products = 300
    assert lib.rg_ope_poly_w_workspace_bytes(C.byref(big), 4, 1000) - lib.rg_ope_poly_w_workspace_bytes(C.byref(model()), 4, 1000) == 4 * 2 * 300 * 4


# ---- the confirmation step ---------------------------------------------------------------------------------------------------------
O, B = False, True


def hand_log(users, P):
    """users: one list of (is_bandit, index, clock value) per user -> (DeviceLog on the host, the clock tensor beside its rows)."""
    raw, offsets, clock = [], [0], []
    for u, rows in enumerate(users):
        for b, i, t in rows:
            raw.append((u, int(t), int(i) | (_abi.RG_EV_BANDIT if b else 0), 0))
            clock.append(float(t))
        offsets.append(len(raw))
    rows = torch.from_numpy(np.array(raw, dtype=np.uint32).reshape(-1, 4).view(np.int32))
    return DeviceLog(rows, torch.tensor(offsets, dtype=torch.int64), 1.0 / P, 0, P, None), torch.tensor(clock, dtype=torch.float64)


def test_weighted_replay_verify_confirms_refutes_and_gives_up():
    P = 10
    rng = np.random.RandomState(5)
    model = (rng.normal(0, 0.4, P), rng.normal(0, 0.05, P), rng.normal(0, 0.6, (P, P)), 0.25)
    table, f32 = weight_table(gu.WEIGHT_FUNCS['exp_0.2'])
    wh = dict(table=table, f32=f32)
    users = [[(O, 2, 0), (B, 0, 1)],
             [(O, 3, 0), (O, 7, 2), (B, 1, 3), (O, 3, 9), (B, 2, 12), (B, 2, 30)],
             [(O, 1, 0)]]
    dl, clock = hand_log(users, P)
    # the host acts: the organic rows BEFORE the position with their times, at the row's own clock value
    a3 = weighted_host_act([3, 7], [0, 2], 3, wh, model)
    a12 = weighted_host_act([3, 7, 3], [0, 2, 9], 12, wh, model)
    a30 = weighted_host_act([3, 7, 3], [0, 2, 9], 30, wh, model)
    acts = np.array([[1, 2, a3], [1, 4, a12], [1, 5, a30], [0, 1, weighted_host_act([2], [0], 1, wh, model)]], dtype=np.uint32)
    assert weighted_replay_verify(dl, clock, acts, False, wh, model) is True
    assert weighted_replay_verify(dl, clock, acts[:0], False, wh, model) is True
    # the clock beside the rows may be the rows' own event index (a log without a float clock)
    assert weighted_replay_verify(dl, dl.rows[:, 1], acts, False, wh, model) is True
    # the same log with one action changed
    for i in range(len(acts)):
        wrong = acts.copy()
        wrong[i, 2] = (wrong[i, 2] + 1) % P
        assert weighted_replay_verify(dl, clock, wrong, False, wh, model) is False
    # the list did not hold every act
    assert weighted_replay_verify(dl, clock, acts, True, wh, model) is False
    assert weighted_replay_verify(dl, clock, acts[:0], True, wh, model) is False
    # the act depends on the clock: a model whose decision follows the weight of one product
    far = clock.clone()
    far[5] = 40000.0                                                # the listed row at position 4 of user 1
    assert weighted_host_act([3, 7, 3], [0, 2, 9], 40000, wh, model) == -1
    assert weighted_replay_verify(dl, far, acts[1:2], False, wh, model) is False
    assert weighted_replay_verify(dl, far, acts[:1], False, wh, model) is True          # (another row of the user: untouched)
    view = clock.clone()
    view[1 + 1] = 40000.0                                           # a VIEW of user 1 outside the range refutes every later act
    assert weighted_replay_verify(dl, view, acts[:1], False, wh, model) is False


def test_the_act_of_a_listed_row_is_taken_at_its_own_clock_value():
    """exp(-t) in float32: a view 104 clock values back weighs exactly 0 and leaves the list — the act at that distance is the act
    on the remaining views, and the confirmation must see it so."""
    P = 10
    rng = np.random.RandomState(8)
    table, f32 = weight_table(exp_t)
    wh = dict(table=table, f32=f32)
    for seed in range(40):
        rng = np.random.RandomState(seed)
        model = (rng.normal(0, 2.0, P), rng.normal(0, 0.05, P), rng.normal(0, 3.0, (P, P)), 0.0)
        near, far = weighted_host_act([4, 6], [0, 100], 101, wh, model), weighted_host_act([4, 6], [0, 100], 110, wh, model)
        if near != far:
            break
    assert near != far and far == weighted_host_act([6], [100], 110, wh, model)
    dl, clock = hand_log([[(O, 4, 0), (O, 6, 100), (B, 0, 101), (B, 0, 110)]], P)
    assert weighted_replay_verify(dl, clock, np.array([[0, 2, near], [0, 3, far]], dtype=np.uint32), False, wh, model) is True
    assert weighted_replay_verify(dl, clock, np.array([[0, 2, far]], dtype=np.uint32), False, wh, model) is False
    assert weighted_replay_verify(dl, clock, np.array([[0, 3, near]], dtype=np.uint32), False, wh, model) is False


def test_device_clock16_truncates_inside_the_range_and_marks_the_rest():
    from recogym_amd.agents.feature_feed import device_clock16
    t = torch.tensor([0.0, 0.99, 1.0, 32767.999, 32768.0, -0.5, -1e-9, float('nan'), 40000.0, 12.7], dtype=torch.float64)
    want = np.array([0, 0, 1, 32767, 0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF, 12], dtype=np.uint16)
    assert np.array_equal(device_clock16(t).numpy().view(np.uint16), want)
    assert np.array_equal(device_clock16(t.to(torch.float32)).numpy().view(np.uint16)[[0, 2, 4, 5, 7, 8, 9]], want[[0, 2, 4, 5, 7, 8, 9]])
    i = torch.tensor([0, 5, 32767, 32768, -1, 40000], dtype=torch.int32)
    assert np.array_equal(device_clock16(i).numpy().view(np.uint16), np.array([0, 5, 32767, 0xFFFF, 0xFFFF, 0xFFFF], dtype=np.uint16))
