"""The host side of NnIpsAgent's off-policy replay (rg_ope_replay_nn): the ABI's mirrors and argument checks, the agent's opt-in hook,
the host's confirmation of listed acts (sim.replay_verify with sim.nn_host_act) on a hand-made log, and the recall forms.  No device
needed: every library call here is refused before it touches one."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
import golden_util as gu
from make_golden_ope import log_frame
from recogym_amd import _abi
from recogym_amd import evaluate_agent as ev
from recogym_amd import sim
from recogym_amd.agents.nn_ips import HIDDEN_CAP, PRODUCTS_CAP, NnIpsAgent, NnIpsFrozenAgent, nn_ips_args
from recogym_amd.envs.configuration import Configuration
from recogym_amd.sim import DeviceLog
from test_ope_args_host import ADDR, CASES, MAX_USER_ROWS, N_USERS, P, wrapper

HEADER = os.path.join(graft.ROOT, 'include', 'recogym_hip.h')
C_TYPES = {'uint32_t': C.c_uint32, 'uint64_t': C.c_uint64, 'double': C.c_double, 'float': C.c_float}


@pytest.fixture(scope='module')
def lib():
    graft.build()
    return _abi.load()


# ---- what both units' host tests share ----------------------------------------------------------------------------------------------
def header_struct(name):
    """The fields of `typedef struct NAME { ... } NAME;` in the header -> [(field, ctypes type)] (a pointer is a c_void_p)."""
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), open(HEADER).read(), flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    out = []
    for decl in filter(None, (d.strip() for d in body.split(';'))):
        m = re.fullmatch(r'(const\s+)?(\w+)\s*(\*?)\s*(\w+)', decl)
        assert m, decl
        out.append((m.group(4), C.c_void_p if m.group(3) else C_TYPES[m.group(2)]))
    return out


def check_mirror(name, mirror):
    assert [(f, t) for f, t in mirror._fields_] == header_struct(name)


def check_symbols_follow_the_poly_unit(unit, mirror):
    """After the model pointer the three entry points take what the likelihood unit's take."""
    for fmt in ('rg_ope_{}_workspace_bytes', 'rg_ope_replay_{}', 'rg_ope_replay_{}_eg'):
        res, args = _abi.SYMBOLS[fmt.format(unit)]
        want_res, want_args = _abi.SYMBOLS[fmt.format('poly')]
        assert res is want_res and args[0]._type_ is mirror and args[1:] == want_args[1:], fmt
    assert f'rg_ope_{unit}' in graft.UNITS
    one_unit = open(os.path.join(graft.ROOT, 'recogym_amd', 'csrc', 'recogym_hip.hip')).read()
    assert f'#include "rg_ope_{unit}.hip"' in one_unit


def check_abi_version(lib):
    assert '#define RG_ABI_VERSION 15\n' in open(HEADER).read() and _abi.RG_ABI_VERSION == 15 and lib.rg_abi_version() == 15


def refused(lib, unit, model, wrapped, over):
    """One malformed call (test_ope_args_host's recipe) -> (return code, rg_last_error())."""
    what = f'rg_ope_replay_{unit}' + ('_eg' if wrapped else '')
    m, eg = model, wrapper()
    need = getattr(lib, f'rg_ope_{unit}_workspace_bytes')(C.byref(m), N_USERS, MAX_USER_ROWS)
    assert need >= _abi.OPE_HEAD_BYTES + _abi.OPE_POLY_LIST_CAP * _abi.OPE_POLY_LIST_ENTRY_BYTES
    a = dict(d_rows=ADDR, d_offsets=ADDR, ps_mode=_abi.RG_OPE_PS_CONST, d_ps=None, d_ratio=ADDR, d_sums=ADDR, d_workspace=ADDR, short=0,
             eg=eg)
    a.update(over)
    rc = getattr(lib, what)(C.byref(m) if m is not None else None, *([C.byref(a['eg']) if a['eg'] is not None else None] if wrapped else []),
                            a['d_rows'], a['d_offsets'], N_USERS, MAX_USER_ROWS, a['ps_mode'], a['d_ps'], 1.0 / P, a['d_ratio'], None,
                            a['d_sums'], *([None, None] if wrapped else []), a['d_workspace'], need - a['short'], None)
    return what, rc, lib.rg_last_error().decode()


def check_shared_argument_checks(lib, unit, model):
    """ope_args_ok's refusals: test_ope_args_host's cases, with the code and — after the entry point's name — the text of the
    likelihood unit's; the wrapper's own checks on the _eg entry."""
    from test_ope_args_host import refused as poly_refused
    for case, (over, code) in CASES.items():
        _, want = poly_refused(lib, 'rg_ope_replay_poly', over)
        for wrapped in (False, True):
            what, rc, msg = refused(lib, unit, model(), wrapped, over)
            assert rc == code and msg.startswith(what + ': '), (case, what, rc, msg)
            strip = (lambda s: re.sub(r'\d+', '', s)) if case == 'workspace one byte short' else (lambda s: s)
            assert strip(msg[len(what) + 2:]) == strip(want[len('rg_ope_replay_poly: '):]), (case, msg, want)
    for over in (dict(eg=None), dict(eg=_abi.RgOpeEg(epsilon=1.5, seed=1, pure_new=0, reserved=0, prob_explore=0.1)),
                 dict(eg=_abi.RgOpeEg(epsilon=float('nan'), seed=1, pure_new=0, reserved=0, prob_explore=0.1))):
        what, rc, msg = refused(lib, unit, model(), True, over)
        assert rc == -1 and msg.startswith(what + ': '), (over, rc, msg)


def check_model_refusals(lib, unit, bad_models):
    """A null model and every malformed model: RG_EINVAL from both replay entries, 0 from the size function for the null model."""
    size_fn = getattr(lib, f'rg_ope_{unit}_workspace_bytes')
    assert size_fn(None, N_USERS, MAX_USER_ROWS) == 0 and 'null model' in lib.rg_last_error().decode()
    for what_is_wrong, m in [('null model', None)] + bad_models:
        for wrapped in (False, True):
            what = f'rg_ope_replay_{unit}' + ('_eg' if wrapped else '')
            rc = getattr(lib, what)(C.byref(m) if m is not None else None, *([C.byref(wrapper())] if wrapped else []), ADDR, ADDR, N_USERS,
                                    MAX_USER_ROWS, _abi.RG_OPE_PS_CONST, None, 1.0 / P, ADDR, None, ADDR, *([None, None] if wrapped else []),
                                    ADDR, 1 << 30, None)
            assert rc == -1 and lib.rg_last_error().decode().startswith(what + ': '), (what_is_wrong, what, rc, lib.rg_last_error())


def slot_bytes(W):
    """rg_ope_common.hpp: ope_slot_bytes — three doubles per wave, rounded up to 256 bytes."""
    return (W * 24 + 255) & ~255


def hand_log():
    """Two users on the CPU: u0 = o3 o1 B o1 B B o2 B, u1 = o0 B o3 B.  -> (DeviceLog, the acts' (user, position, views before it))."""
    O, B = 0, _abi.RG_EV_BANDIT
    toks = [[(O, 3), (O, 1), (B, 9), (O, 1), (B, 9), (B, 9), (O, 2), (B, 9)], [(O, 0), (B, 9), (O, 3), (B, 9)]]
    raw = np.array([(u, t, kind | idx, 0) for u, rows in enumerate(toks) for t, (kind, idx) in enumerate(rows)], dtype=np.uint32)
    dl = DeviceLog(torch.from_numpy(raw.view(np.int32)), torch.tensor([0, 8, 12], dtype=torch.int64), 0.1, 0, 10, None)
    return dl, [(0, 2, [3, 1]), (0, 4, [3, 1, 1]), (0, 7, [3, 1, 1, 2]), (1, 1, [0]), (1, 3, [0, 3])]


def check_replay_verify(host_act):
    """Placed acts on the hand-made log: the act at (user, position) sees the user's organic rows BEFORE that position — not the
    act's own row's later organic rows, not another user's — and is confirmed iff it is the host's; an overflowed list refutes."""
    dl, acts = hand_log()
    seen = []

    def spy(views):
        seen.append(sorted(int(v) for v in views))
        return host_act(views)
    good = np.array([(u, pos, host_act(np.array(views))) for u, pos, views in acts], dtype=np.uint32)
    assert sim.replay_verify(dl, good, False, spy) is True
    assert seen == [sorted(v) for _, _, v in acts]
    assert sim.replay_verify(dl, good[:0], False, host_act) is True
    assert sim.replay_verify(dl, good, True, host_act) is False and sim.replay_verify(dl, good[:0], True, host_act) is False
    for i in range(len(good)):
        bad = good.copy()
        bad[i, 2] = (bad[i, 2] + 1) % 10
        assert sim.replay_verify(dl, bad, False, host_act) is False
        assert sim.replay_verify(dl, bad[i:i + 1], False, host_act) is False and sim.replay_verify(dl, good[i:i + 1], False, host_act) is True


def check_recall_forms(pol):
    assert ev._recall_form(pol) == 'table' and ev._recall_form(dict(pol, epsilon_greedy=dict(epsilon=0.2, seed=1, pure_new=True))) == 'table'
    P_ = int(pol['num_products'])
    sets = ev.recall_sets(pol, [0, 2 * 3, 2 * (P_ - 1)], 1)
    assert sets.tolist() == [[0], [3], [P_ - 1]]
    eg = dict(pol, epsilon_greedy=dict(epsilon=0.2, seed=1, pure_new=True))
    assert ev.recall_sets(eg, [2 * 3], 1).tolist() == [[3]] and 3 not in ev.recall_sets(eg, [2 * 3 + 1], P_ - 1)[0].tolist()
    assert sorted(ev.recall_sets(pol, [4], P_)[0].tolist()) == list(range(P_))


# ---- the NN unit ------------------------------------------------------------------------------------------------------------------
def state(P_=10, H=6, seed=2, scale=0.5):
    rng = np.random.RandomState(seed)
    shapes = dict(w1=(H, P_), b1=(H,), w2=(H, H), b2=(H,), w3=(P_, H), b3=(P_,))
    return {k: (rng.standard_normal(s) * scale).astype(np.float32) for k, s in shapes.items()}


def model(**over):
    kw = dict(num_products=P, num_hidden=4, w1t=ADDR, b1=ADDR, w2t=ADDR, b2=ADDR, w3t=ADDR, b3=ADDR)
    kw.update(over)
    return _abi.RgOpeNn(**kw)


def test_the_mirror_matches_the_header_and_the_symbols_the_poly_unit(lib):
    check_mirror('rg_ope_nn', _abi.RgOpeNn)
    check_symbols_follow_the_poly_unit('nn', _abi.RgOpeNn)
    check_abi_version(lib)
    assert _abi.OPE_HEADS['nn'] == ('error', 'acts', 'unresolved', 'overflow', 'rows_read')
    assert ev._REPLAY_ENTRY['nn', False] == ('rg_ope_nn_workspace_bytes', 'rg_ope_replay_nn')
    assert ev._REPLAY_ENTRY['nn', True] == ('rg_ope_nn_workspace_bytes', 'rg_ope_replay_nn_eg')


def test_argument_errors(lib):
    check_shared_argument_checks(lib, 'nn', model)
    bad = [(f'null {k}', model(**{k: None})) for k in ('w1t', 'b1', 'w2t', 'b2', 'w3t', 'b3')]
    bad += [('H == 0', model(num_hidden=0)), ('H above the cap', model(num_hidden=HIDDEN_CAP + 1)), ('P == 0', model(num_products=0)),
            ('P above the cap', model(num_products=PRODUCTS_CAP + 1))]
    check_model_refusals(lib, 'nn', bad)
    # the workspace grows with the per-wave global lists, and the caps themselves are accepted by the size function
    small = lib.rg_ope_nn_workspace_bytes(C.byref(model()), 1, 3)
    assert lib.rg_ope_nn_workspace_bytes(C.byref(model()), 1, 600) == small + 4 * 2 * 600 * 4
    assert lib.rg_ope_nn_workspace_bytes(C.byref(model(num_hidden=HIDDEN_CAP, num_products=PRODUCTS_CAP)), 1, 3) == small
    # W = 2048: the slots of 10^5 users are those of 2048 waves
    assert lib.rg_ope_nn_workspace_bytes(C.byref(model()), 100000, 3) - small == slot_bytes(2048) - slot_bytes(4)


def test_the_hook_is_opt_in():
    st = state()
    on = dict(num_products=10, with_ps_all=True, device_replay=True)
    ag = NnIpsFrozenAgent(Configuration(on), st)
    pol = ag.ope_policy_checked()
    assert set(pol) == {'kind', 'num_products', 'policy_seed', 'nn_ips'} and set(pol['nn_ips']) == {'state'}
    assert (pol['kind'], pol['num_products'], pol['policy_seed']) == (_abi.RG_POLICY_NN_IPS, 10, 0)
    assert all(np.array_equal(pol['nn_ips']['state'][k], st[k]) for k in st)
    assert ag.ope_policy() is None and ag.device_policy() is None and ev.ope_policy_of(ag) is None
    assert ev.ope_checked_policy_of(ag) is not None and ev._replay_policy_of(ag)['kind'] == _abi.RG_POLICY_NN_IPS
    for off in (dict(with_ps_all=False), dict(device_replay=False), dict(weight_history_function=lambda dt: np.exp(-0.2 * dt)),
                dict(select_randomly=True)):
        assert NnIpsFrozenAgent(Configuration({**on, **off}), st).ope_policy_checked() is None, off
    for drop in ('with_ps_all', 'device_replay'):
        assert NnIpsFrozenAgent(Configuration({k: v for k, v in on.items() if k != drop}), st).ope_policy_checked() is None, drop
    bad = {k: v.copy() for k, v in st.items()}
    bad['w2'][3, 4] = np.inf
    assert NnIpsFrozenAgent(Configuration(on), bad).ope_policy_checked() is None
    assert NnIpsFrozenAgent(Configuration(on), state(H=HIDDEN_CAP + 1, scale=0.01)).ope_policy_checked() is None
    assert NnIpsFrozenAgent(Configuration(on), state(H=HIDDEN_CAP, scale=0.01)).ope_policy_checked() is not None


def test_a_trained_agent_asks_its_frozen_agent():
    cols = gu.load('nn_ips_p10')[1]
    train = {k[len('trainlog_'):]: v[cols['trainlog_u'] < 5] for k, v in cols.items() if k.startswith('trainlog_')}
    base = {**nn_ips_args, 'num_products': 10, 'random_seed': 7, 'num_epochs': 1, 'with_ps_all': True}
    for extra, want in ((dict(device_replay=True), True), ({}, False)):
        ag = NnIpsAgent(Configuration({**base, **extra}))
        ag.train_from_log(log_frame(train))
        pol = ag.ope_policy_checked()
        assert (pol is not None) == want and ag.ope_policy() is None and ag.device_policy() is None
        if want:
            assert pol['kind'] == _abi.RG_POLICY_NN_IPS and all(np.array_equal(pol['nn_ips']['state'][k], v) for k, v in ag.frozen.state().items())


def test_replay_verify_with_the_nn_host_act():
    host = NnIpsFrozenAgent(Configuration({'num_products': 10}), state(scale=2.0))
    check_replay_verify(lambda views: sim.nn_host_act(views, 10, host))
    # ... and the likelihood agent's entry is a call of it
    dl, acts = hand_log()
    rng = np.random.RandomState(4)
    m = (rng.randn(10), rng.randn(10), rng.randn(10, 10), 0.5)
    listed = np.array([(u, pos, sim.poly_host_act(np.array(views), m)) for u, pos, views in acts], dtype=np.uint32)
    assert sim.poly_replay_verify(dl, listed, False, m) is True and sim.poly_replay_verify(dl, listed, True, m) is False
    listed[2, 2] = (listed[2, 2] + 1) % 10
    assert sim.poly_replay_verify(dl, listed, False, m) is False


def test_the_recall_forms_accept_the_kind():
    check_recall_forms(NnIpsFrozenAgent(Configuration(dict(num_products=10, with_ps_all=True, device_replay=True)), state()).ope_policy_checked())
