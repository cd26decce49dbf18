"""recall@k's device form, host side: the sets table recall_sets builds against np.argpartition on the very vector the agent's
host act returns, the cap on that table, the k that leave the device route out, and the ctypes mirrors of the two new entry
points against the header.  No device needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import golden_util as gu
from make_golden_ope import log_frame
from recogym_amd import _abi
from recogym_amd import evaluate_agent as ev
from recogym_amd.agents import EpsilonGreedy, LastViewTableAgent, RandomAgent, epsilon_greedy_args
from recogym_amd.envs.configuration import Configuration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 10


def table_agent():
    return LastViewTableAgent(Configuration({'num_products': P, 'with_ps_all': True}), np.random.RandomState(3).randint(0, P, size=P))


def random_agent():
    return RandomAgent(Configuration({'num_products': P, 'random_seed': 5, 'with_ps_all': True}))


def wrapped(eps, pure_new):
    return EpsilonGreedy(Configuration({**epsilon_greedy_args, 'epsilon': eps, 'random_seed': 7, 'epsilon_pure_new': pure_new,
                                        'num_products': P, 'with_ps_all': True}), table_agent())


AGENTS = {'table': table_agent, 'random': random_agent}
AGENTS.update({f'eg{eps}{"_pure_new" if pn else ""}': (lambda eps=eps, pn=pn: wrapped(eps, pn))
               for eps in (0.0, 0.3, 1.0) for pn in (True, False)})


class Recording:
    """The agent, with the dict of its last act kept (the host loop hands on `ps-a` only)."""

    def __init__(self, agent):
        self.agent, self.last = agent, None

    def reset(self):
        self.agent.reset()

    def act(self, observation, reward, done):
        self.last = self.agent.act(observation, reward, done)
        return self.last


def key_of(name, action):
    if name == 'random':
        return 0
    if 'greedy' not in action:
        return 2 * int(action['a'])
    return 2 * int(action['a']) if action['greedy'] else 2 * int(action['h0']) + 1


@pytest.fixture(scope='module')
def frame():
    df = log_frame(gu.load('philox_p10')[1])
    return df[df['u'] <= 150].reset_index(drop=True)


@pytest.mark.parametrize('name', sorted(AGENTS))
def test_sets_equal_argpartition_on_the_acts_own_vector(name, frame):
    agent = AGENTS[name]()
    rec = Recording(agent)
    seen = {}

    def visit(uid, idx, jj, prob_policy, cols):
        seen.setdefault(key_of(name, rec.last), []).append(np.array(prob_policy))
    ev._host_loop(rec, frame, visit)                     # the host act, with the real flips
    assert seen
    if name.startswith('eg0.3'):
        assert any(key & 1 for key in seen) and any(not key & 1 for key in seen)       # both branches occurred
    keys = sorted(seen)
    for k in (1, 5, 10):
        sets = ev.recall_sets(agent, keys, k)
        assert sets.dtype == np.int32 and sets.shape == (len(keys), k)
        assert (np.diff(sets, axis=1) > 0).all()                                       # ascending within a key
        for key, row in zip(keys, sets):
            for vec in seen[key]:
                assert set(row.tolist()) == set(np.argpartition(vec, -k)[-k:].tolist()), (name, key, k)


def test_cap_refuses_an_oversized_table(monkeypatch):
    agent = table_agent()
    monkeypatch.setattr(ev, 'RECALL_TABLE_MAX', 10)
    assert ev.recall_sets(agent, [0, 2], 5) is not None                                # 10 entries: the cap itself
    assert ev.recall_sets(agent, [0, 2, 4], 5) is None
    assert ev.recall_sets(agent, list(range(0, 20, 2)), 2) is None


@pytest.mark.parametrize('k', [0, -1, P + 1, 2.5, None])
def test_k_outside_1_to_P_leaves_the_device_route_out(k):
    # (dl = None: anything that touched the log or a device would raise)
    for make in (table_agent, random_agent, lambda: wrapped(0.3, True)):
        assert ev.recall_replay(make(), None, k) is None


def test_host_loop_keeps_numpys_behaviour_outside_1_to_P(frame):
    small = frame[frame['u'] <= 20].reset_index(drop=True)
    with pytest.raises(ValueError):
        ev._host_recall(table_agent(), small, P + 1)
    quirk = ev._host_recall(table_agent(), small, 0)                                   # [-0:] is the whole vector: every view hits
    assert quirk and all(h == 1 for h in quirk)


def test_no_form_for_the_count_vector_agent():
    from recogym_amd.agents import OrganicUserEventCounterAgent
    ouc = OrganicUserEventCounterAgent(Configuration({'num_products': P, 'random_seed': 11, 'weight_history_function': None,
                                                      'with_ps_all': True, 'select_randomly': True, 'exploit_explore': True,
                                                      'epsilon': 0.0, 'reverse_pop': False}))
    assert ev._recall_form(ev.ope_policy_of(ouc)) is None
    assert ev.recall_replay(ouc, None, 5) is None


C_TYPES = {'uint64_t': C.c_uint64, 'uint32_t': C.c_uint32, 'size_t': C.c_size_t, 'int': C.c_int}


def declared(header, name):
    """-> (result ctype, [argument ctypes]) of a function as include/recogym_hip.h declares it."""
    m = re.search(r'^(\w+)\s+' + name + r'\s*\(([^;]*)\);', header, flags=re.M)
    assert m, name
    args = []
    for arg in m.group(2).split(','):
        words = arg.replace('*', ' * ').split()
        if '*' in words:
            args.append(C.POINTER(_abi.RgOpeLogreg) if 'rg_ope_logreg' in words else C.c_void_p)
        else:
            args.append(C_TYPES[words[-2]])
    return C_TYPES[m.group(1)], args


def test_ctypes_argument_lists_match_the_header():
    header = open(os.path.join(ROOT, 'include', 'recogym_hip.h')).read()
    for name in ('rg_ope_recall_hits', 'rg_ope_recall_logreg_workspace_bytes', 'rg_ope_recall_logreg'):
        assert name in _abi.SYMBOLS
        res, args = declared(header, name)
        assert _abi.SYMBOLS[name][0] is res, name
        assert _abi.SYMBOLS[name][1] == args, name
    # the parser itself, on an entry point whose mirror the existing tests hold
    assert declared(header, 'rg_ope_logreg_workspace_bytes') == _abi.SYMBOLS['rg_ope_logreg_workspace_bytes']
    for word, value in (('RG_RECALL_MISS', _abi.RG_RECALL_MISS), ('RG_RECALL_HIT', _abi.RG_RECALL_HIT),
                        ('RG_RECALL_NOT_COUNTED', _abi.RG_RECALL_NOT_COUNTED), ('RG_RECALL_UNRESOLVED', _abi.RG_RECALL_UNRESOLVED),
                        ('RG_OPE_RECALL_LIST_CAP', _abi.OPE_RECALL_LIST_CAP)):
        assert int(re.search(r'#define ' + word + r' (\d+)', header).group(1)) == value, word
    assert _abi.OPE_RECALL_HEAD[:4] == _abi.OPE_HEADS['logreg'] and _abi.OPE_RECALL_HEAD[4:] == ('unresolved', 'overflow')
