"""Shared by the tests of EpsilonGreedy round NnIpsAgent and BayesianAgentVB: the fixtures of tests/make_golden_eg_nn_bayes.py
(tests/golden/nn_eg_*.npz, bayes_eg_*.npz) and this package's frozen agents and wrappers rebuilt from them."""
import numpy as np

import bayes_util as bu
import golden_util as gu
import nn_ips_util as nu
from recogym_amd.agents import EpsilonGreedy, epsilon_greedy_args
from recogym_amd.agents.bayesian_poly_vb import BayesianVBFrozenAgent
from recogym_amd.agents.nn_ips import UNRESOLVED, NnIpsFrozenAgent
from recogym_amd.envs.configuration import Configuration

NN_FIXTURES = ['nn_eg_p10', 'nn_eg_p10_not_pure_new', 'nn_eg_p10_sigma0', 'nn_eg_p40']
BAYES_FIXTURES = ['bayes_eg_p4', 'bayes_eg_p10_s120', 'bayes_eg_p10_s120_not_pure_new']
LOG_FIXTURES = NN_FIXTURES + BAYES_FIXTURES
OPE_FIXTURES = ['nn_eg_ope', 'bayes_eg_ope']


def load(name):
    meta, cols = gu.load(name)
    return meta, cols, meta.get('num_products') or meta['env_args']['num_products']


def model_of(meta, cols):
    """The fixture's model: the six arrays of the net it names (inner = 'nn') or the posterior draws of the fixture it names."""
    if meta['inner'] == 'nn':
        return nu.fixture_state(meta, cols)
    return bu.fixture_lambda(meta, cols)


def inner_agent(meta, cols, P, with_ps_all=False, **cfg):
    """This package's frozen agent with the fixture's model (the reference's own agent acted with it); with_ps_all brings the replay
    key `device_replay` with it, as a caller of the checked replay sets both."""
    extra = {'device_replay': True} if with_ps_all else {}
    config = Configuration({'num_products': P, 'with_ps_all': with_ps_all, **extra, **cfg})
    if meta['inner'] == 'nn':
        return NnIpsFrozenAgent(config, model_of(meta, cols))
    return BayesianVBFrozenAgent(config, model_of(meta, cols))


def wrap(inner, P, eg_args, with_ps_all=False, device_models=True, **over):
    extra = {} if device_models is None else {'device_models': device_models}      # (None: the key is absent)
    return EpsilonGreedy(Configuration({**epsilon_greedy_args, **eg_args, 'num_products': P, 'with_ps_all': with_ps_all, **extra, **over}),
                         inner)


def wrapper(meta, cols, P, with_ps_all=False, device_models=True, **over):
    return wrap(inner_agent(meta, cols, P, with_ps_all), P, meta['eg_args'], with_ps_all, device_models, **over)


def greedy_actions(cols):
    """The inner agent's action on every row (-1 on organic rows): the logged one on a greedy act, `h0` on an explored one."""
    return np.where(cols['z'] == 1, np.where(cols['greedy'] == 1, cols['a'], cols['h0']), -1)


def greedy_cols(cols):
    """The fixture's columns with `a` replaced by the greedy action: the log the unwrapped agent's rule is restated over."""
    return dict(cols, a=np.where(cols['z'] == 1, greedy_actions(cols), cols['a']).astype(cols['a'].dtype))


def nn_row_bounds(meta, cols, P):
    """nn_ps_bound of the act that serves each row (0 on organic rows), and which rows an unresolved act serves."""
    bound, unresolved = np.zeros(len(cols['u'])), np.zeros(len(cols['u']), dtype=bool)
    for act in nu.rule_over_log(greedy_cols(cols), P, model_of(meta, cols)):
        bound[act['rows']] = act['bound']
        unresolved[act['rows']] = bool(act['flags'] & UNRESOLVED)
    return bound, unresolved
