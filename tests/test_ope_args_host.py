"""The argument checks the six off-policy replay entry points share (rg_ope_common.hpp: ope_args_ok) are the same in every one of
them: the same code and, after the entry point's own name, the same text.  Every call here is malformed and returns before anything
touches a device or reads a pointer, so the test needs no GPU."""
import ctypes as C
import re

import pytest

from recogym_amd import _abi

ADDR = 0x10000              # a made-up 16-byte-aligned address: nothing reads it on these paths
P, N_USERS, MAX_USER_ROWS = 10, 1, 3


def policy():
    return _abi.RgOpePolicy(kind=_abi.RG_POLICY_RANDOM_AGENT, num_products=P, policy_seed=3, ouc_select_randomly=1, ouc_exploit_explore=1,
                            ouc_reverse_pop=0, reserved=0, ouc_epsilon=0.0, table=None)


def logreg():
    return _abi.RgOpeLogreg(num_products=P, n_classes=P, select_randomly=0, reserved=0, coef_t=ADDR, intercept=ADDR, classes=ADDR,
                            coef32_t=None, intercept32=None, wmax=None, bmax=0.0, reserved2=0)


def poly():
    return _abi.RgOpePoly(num_products=P, n_steps=4, wf=ADDR, wa=ADDR, wk_t=ADDR, th=ADDR, intercept=0.0)


def wrapper():
    return _abi.RgOpeEg(epsilon=0.1, seed=7, pure_new=1, reserved=0, prob_explore=1.0 / (P - 1))


# entry point -> (its workspace-size function, its policy or model, under the EpsilonGreedy wrapper)
ENTRY_POINTS = {
    'rg_ope_replay': ('rg_ope_workspace_bytes', policy, False),
    'rg_ope_replay_eg': ('rg_ope_eg_workspace_bytes', policy, True),
    'rg_ope_replay_logreg': ('rg_ope_logreg_workspace_bytes', logreg, False),
    'rg_ope_replay_logreg_eg': ('rg_ope_logreg_workspace_bytes', logreg, True),
    'rg_ope_replay_poly': ('rg_ope_poly_workspace_bytes', poly, False),
    'rg_ope_replay_poly_eg': ('rg_ope_poly_workspace_bytes', poly, True),
}

# one malformed argument per call -> the code it is refused with; `short`: the workspace size less that many bytes
CASES = {
    'ps_mode 3': (dict(ps_mode=3), -1),
    'ps array without d_ps': (dict(ps_mode=_abi.RG_OPE_PS_ARRAY, d_ps=None), -1),
    'null rows': (dict(d_rows=None), -1),
    'null offsets': (dict(d_offsets=None), -1),
    'null ratio': (dict(d_ratio=None), -1),
    'null sums': (dict(d_sums=None), -1),
    'null workspace': (dict(d_workspace=None), -1),
    'rows at +8 bytes': (dict(d_rows=ADDR + 8), -1),
    'workspace one byte short': (dict(short=1), -3),
}


def refused(lib, what, over):
    """One malformed call of entry point `what` -> (return code, rg_last_error())."""
    size_name, model, wrapped = ENTRY_POINTS[what]
    m, eg = model(), wrapper()
    need = getattr(lib, size_name)(C.byref(m), N_USERS, MAX_USER_ROWS)
    assert need > 0
    a = dict(d_rows=ADDR, d_offsets=ADDR, ps_mode=_abi.RG_OPE_PS_CONST, d_ps=None, d_ratio=ADDR, d_sums=ADDR, d_workspace=ADDR, short=0)
    a.update(over)
    rc = getattr(lib, what)(C.byref(m), *([C.byref(eg)] if wrapped else []), a['d_rows'], a['d_offsets'], N_USERS, MAX_USER_ROWS,
                            a['ps_mode'], a['d_ps'], 1.0 / P, a['d_ratio'], None, a['d_sums'], *([None, None] if wrapped else []),
                            a['d_workspace'], need - a['short'], None)
    return rc, lib.rg_last_error().decode()


@pytest.mark.parametrize('case', list(CASES))
def test_shared_argument_checks_are_the_same_in_every_entry_point(case):
    lib = _abi.load()
    over, code = CASES[case]
    assert _abi.RG_ERRORS[code] == ('RG_ENOMEM' if case == 'workspace one byte short' else 'RG_EINVAL')
    texts = set()
    for what in ENTRY_POINTS:
        rc, msg = refused(lib, what, over)
        assert rc == code, (what, rc, msg)
        assert msg.startswith(what + ': '), msg
        text = msg[len(what) + 2:]
        # (the two byte counts of the short-workspace text differ per unit)
        texts.add(re.sub(r'\d+', '', text) if case == 'workspace one byte short' else text)
    assert len(texts) == 1 and texts.pop(), texts
