"""Shared by the tests of EpsilonGreedy round the two model agents: the fixtures of tests/make_golden_eg_models.py
(tests/golden/model_eg_*.npz) and this package's frozen agents and wrappers rebuilt from them."""
import golden_util as gu
from recogym_amd.agents import EpsilonGreedy, LogregFrozenAgent, LogregPolyFrozenAgent, epsilon_greedy_args
from recogym_amd.envs.configuration import Configuration

LOG_FIXTURES = [n for n in gu.fixtures('model_eg_') if not n.startswith('model_eg_ope_')]
OPE_FIXTURES = gu.fixtures('model_eg_ope_')


def load(name):
    meta, cols = gu.load(name)
    return meta, cols, meta.get('num_products') or meta['env_args']['num_products']


def inner_agent(meta, cols, P, with_ps_all=False, **cfg):
    """This package's frozen agent with the fixture's fitted arrays (the reference trained them)."""
    config = Configuration({'num_products': P, 'with_ps_all': with_ps_all, **cfg})
    if meta['inner'] == 'poly':
        return LogregPolyFrozenAgent(config, cols['poly_coef'], cols['poly_intercept'])
    return LogregFrozenAgent(config, cols['coef'], cols['intercept'], cols['classes'])


def wrap(inner, P, eg_args, with_ps_all=False, device_models=True, **over):
    extra = {} if device_models is None else {'device_models': device_models}      # (None: the key is absent)
    return EpsilonGreedy(Configuration({**epsilon_greedy_args, **eg_args, 'num_products': P, 'with_ps_all': with_ps_all, **extra, **over}),
                         inner)


def wrapper(meta, cols, P, with_ps_all=False, device_models=True, **over):
    return wrap(inner_agent(meta, cols, P, with_ps_all), P, meta['eg_args'], with_ps_all, device_models, **over)
