"""The host side of BayesianAgentVB's off-policy replay (rg_ope_replay_bayes): the ABI's mirrors and argument checks, the agent's
opt-in hook, the host's confirmation of listed acts (sim.replay_verify with sim.bayes_host_act) on a hand-made log, and the recall
forms.  No device needed: every library call here is refused before it touches one."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as graft
import golden_util as gu
import test_ope_nn_host as th
from make_golden_ope import log_frame
from recogym_amd import _abi
from recogym_amd import evaluate_agent as ev
from recogym_amd import sim
from recogym_amd.agents.bayesian_poly_vb import MODEL_BYTES_CAP, BayesianAgentVB, BayesianVBFrozenAgent, bayesian_poly_args
from recogym_amd.envs.configuration import Configuration
from test_ope_args_host import ADDR, P


@pytest.fixture(scope='module')
def lib():
    graft.build()
    return _abi.load()


def model(**over):
    kw = dict(num_products=P, num_samples=3, lam_t=ADDR)
    kw.update(over)
    return _abi.RgOpeBayes(**kw)


def test_the_mirror_matches_the_header_and_the_symbols_the_poly_unit(lib):
    th.check_mirror('rg_ope_bayes', _abi.RgOpeBayes)
    th.check_symbols_follow_the_poly_unit('bayes', _abi.RgOpeBayes)
    th.check_abi_version(lib)
    assert _abi.OPE_HEADS['bayes'] == ('error', 'acts', 'saturated', 'unresolved', 'overflow', 'rows_read')
    assert ev._REPLAY_ENTRY['bayes', False] == ('rg_ope_bayes_workspace_bytes', 'rg_ope_replay_bayes')
    assert ev._REPLAY_ENTRY['bayes', True] == ('rg_ope_bayes_workspace_bytes', 'rg_ope_replay_bayes_eg')


def test_argument_errors(lib):
    th.check_shared_argument_checks(lib, 'bayes', model)
    bad = [('null lam_t', model(lam_t=None)), ('S == 0', model(num_samples=0)), ('P == 0', model(num_products=0)),
           ('P above the index mask', model(num_products=_abi.RG_EV_INDEX_MASK + 1)),
           ('a model of one double beyond 2 GiB', model(num_products=4096, num_samples=17)),
           ('P P alone beyond 2 GiB', model(num_products=1 << 20, num_samples=1))]
    assert 4096 * 4096 * 16 * 8 == MODEL_BYTES_CAP
    th.check_model_refusals(lib, 'bayes', bad)
    small = lib.rg_ope_bayes_workspace_bytes(C.byref(model()), 1, 3)
    assert lib.rg_ope_bayes_workspace_bytes(C.byref(model()), 1, 600) == small + 4 * 2 * 600 * 4
    # W = 3072: the slots of 10^5 users are those of 3072 waves
    assert lib.rg_ope_bayes_workspace_bytes(C.byref(model()), 100000, 3) - small == th.slot_bytes(3072) - th.slot_bytes(4)


def test_the_hook_is_opt_in():
    lam = np.random.RandomState(3).randn(5, 16)
    on = dict(num_products=4, with_ps_all=True, device_replay=True)
    ag = BayesianVBFrozenAgent(Configuration(on), lam)
    pol = ag.ope_policy_checked()
    assert set(pol) == {'kind', 'num_products', 'policy_seed', 'bayes_vb'} and set(pol['bayes_vb']) == {'lam'}
    assert (pol['kind'], pol['num_products'], pol['policy_seed']) == (_abi.RG_POLICY_BAYES_VB, 4, 0) and pol['bayes_vb']['lam'] is ag.Lambda
    assert ag.ope_policy() is None and ag.device_policy() is None and ev.ope_policy_of(ag) is None
    assert ev.ope_checked_policy_of(ag) is not None and ev._replay_policy_of(ag)['kind'] == _abi.RG_POLICY_BAYES_VB
    for off in (dict(with_ps_all=False), dict(device_replay=False), dict(weight_history_function=lambda dt: np.exp(-0.1 * dt))):
        assert BayesianVBFrozenAgent(Configuration({**on, **off}), lam).ope_policy_checked() is None, off
    for drop in ('with_ps_all', 'device_replay'):
        assert BayesianVBFrozenAgent(Configuration({k: v for k, v in on.items() if k != drop}), lam).ope_policy_checked() is None, drop
    bad = lam.copy()
    bad[2, 5] = np.nan
    assert BayesianVBFrozenAgent(Configuration(on), bad).ope_policy_checked() is None


def test_a_trained_agent_asks_its_frozen_agent():
    _, cols = gu.load('bayes_p4')
    log = log_frame({k[len('trainlog_'):]: v[cols['trainlog_u'] < 8] for k, v in cols.items() if k.startswith('trainlog_')})
    base = {**bayesian_poly_args, 'num_products': 4, 'random_seed': 3, 'num_samples': 17, 'with_ps_all': True}
    for extra, want in ((dict(device_replay=True), True), ({}, False)):
        ag = BayesianAgentVB(Configuration({**base, **extra}))
        ag.train_from_log(log)
        pol = ag.ope_policy_checked()
        assert (pol is not None) == want and ag.ope_policy() is None and ag.device_policy() is None
        if want:
            assert pol['kind'] == _abi.RG_POLICY_BAYES_VB and pol['bayes_vb']['lam'] is ag.frozen.Lambda and ag.frozen.Lambda.shape == (17, 16)


def test_replay_verify_with_the_bayes_host_act():
    lam = np.random.RandomState(6).randn(7, 100)
    th.check_replay_verify(lambda views: sim.bayes_host_act(views, 10, lam))


def test_the_recall_forms_accept_the_kind():
    lam = np.random.RandomState(3).randn(5, 100)
    th.check_recall_forms(BayesianVBFrozenAgent(Configuration(dict(num_products=10, with_ps_all=True, device_replay=True)), lam).ope_policy_checked())
