"""EpsilonGreedy — reference: recogym/agents/epsilon_greedy.py.

`EpsilonGreedy(config, agent)` wraps any agent: with probability epsilon the act explores — a uniform action among the others
(`epsilon_pure_new`: the greedy action excluded), or with `epsilon_select_worse` proportionally to 1 - `ps-a` of the inner
act — and logs the mixed propensity; the act also reports `greedy` and, on the explored branch, `h0` (the greedy action).

The reference draws from a RandomState of its own.  Here the two draws are addressed like every other draw of the package
(include/recogym_rng.h): the policy block of (the wrapper's random_seed, user, t), words 0,1 the explore flip, words 2,3 the
explore action through NumPy's own cumsum / searchsorted.  Over an inner agent with a device form (RandomAgent,
OrganicUserEventCounterAgent, the last-view tables of OrganicCount / BanditCount / BanditMFSquare) the wrapper runs inside the
device step loop (`device_policy()`: the inner dict plus `epsilon_greedy=`), and with `with_ps_all` over a RandomAgent or a
last-view table it has a replay form for the off-policy estimators (`ope_policy()`).

Over the two model agents — the frozen LogReg argmax (LogregFrozenAgent / LogregMulticlassIpsAgent without select_randomly) and
the likelihood agent (LogregPolyFrozenAgent / LogregPolyAgent) — the same device forms exist and are opt-in: the wrapper's
configuration key `device_models` (read with getattr, default False; not one of `epsilon_greedy_args`, whose keys are the
reference's).  The rows and ratios are the same bits on either route; the key chooses where they are computed.  With it,
`device_policy()` returns the model's dict plus `epsilon_greedy=`, `ope_policy()` the LogReg argmax replay dict and
`ope_policy_checked()` the likelihood agent's checked dict (the host confirms the acts the device cannot resolve), each plus
`epsilon_greedy=`.

NnIpsAgent (argmax form) and BayesianAgentVB take the same key: `device_policy()` returns their dict plus `epsilon_greedy=`
(rg_sim_set_epsilon_greedy_model_ps: a greedy NnIpsAgent row logs (1 - epsilon) * prob[a]) and `ope_policy_checked()` their checked
replay dict (rg_ope_replay_nn_eg / rg_ope_replay_bayes_eg), where the inner agent carries with_ps_all and `device_replay`.  The acts
either device rule lists as unresolved are the GREEDY ones, and generate_logs / ope_replay confirm them on the host as they do
without the wrapper.
"""
import numpy as np

from .. import _abi, rng
from .abstract import Agent

epsilon_greedy_args = {
    'epsilon': 0.01,
    'random_seed': np.random.randint(2 ** 31 - 1),
    # Select an action that is different from the one the inner agent would have taken.
    'epsilon_pure_new': True,
    # Explore proportionally to 1 - `ps-a` of the inner act (host path only).
    'epsilon_select_worse': False,
    'with_ps_all': False,
}

_DEVICE_INNER = (_abi.RG_POLICY_RANDOM_AGENT, _abi.RG_POLICY_ORGANIC_USER_COUNT, _abi.RG_POLICY_LAST_VIEW_TABLE)
_REPLAY_INNER = (_abi.RG_POLICY_RANDOM_AGENT, _abi.RG_POLICY_LAST_VIEW_TABLE)
# with `device_models`: the agents whose act is a model's, computed once per change of the view history (its action is greedy, ps = 1)
_MODEL_INNER = (_abi.RG_POLICY_LOGREG_FROZEN, _abi.RG_POLICY_LOGREG_POLY, _abi.RG_POLICY_NN_IPS, _abi.RG_POLICY_BAYES_VB)
# ... whose replay lists the greedy acts the device cannot resolve, for the host's confirmation (ope_policy_checked)
_CHECKED_INNER = (_abi.RG_POLICY_LOGREG_POLY, _abi.RG_POLICY_NN_IPS, _abi.RG_POLICY_BAYES_VB)
# what the wrapper passes on to the inner agent only where that agent has it (test_agent asks with hasattr / getattr)
_DELEGATED = ('train_from_log', 'train_online_from_log', 'accepts_device_log', 'needs_training')


def explore_table(num_products, pure_new):
    """-> (cdf, prob): what RandomState.choice compares its uniform with for the explore draw, by NumPy itself — cdf = cumsum(p) /
    last over the n non-zero entries of product_probas (n = P - 1 with pure_new: the zero at the greedy action adds 0.0 to the
    running sum and only shifts the indices behind it) — and prob = 1.0 / n, the value of every such entry."""
    n = int(num_products) - 1 if pure_new else int(num_products)
    ones = np.ones(n)
    p = ones / np.sum(ones)
    cdf = p.cumsum()
    cdf /= cdf[-1]
    return cdf, float(p[0])


class EpsilonGreedy(Agent):
    def __init__(self, config, agent):
        super().__init__(config)
        self.agent = agent

    def __getattr__(self, name):
        agent = self.__dict__.get('agent')
        if name in _DELEGATED and agent is not None:
            return getattr(agent, name)
        raise AttributeError(name)

    @property
    def batch_safe(self):
        # the wrapper's own draws are addressed by (user, t): copies of it are as safe as copies of the inner agent
        from ..envs.reco_env_v1 import batch_safe
        return batch_safe(self.agent)

    def train(self, observation, action, reward, done=False):
        self.agent.train(observation, action, reward, done)

    def reset(self):
        self.agent.reset()

    def _num_products(self):
        return int(getattr(self.config, 'num_products', None) or self.agent.config.num_products)

    def _overlay(self):
        c = self.config
        return dict(epsilon=float(c.epsilon), seed=int(c.random_seed), pure_new=bool(c.epsilon_pure_new))

    def device_policy(self):
        """The inner agent's device policy plus `epsilon_greedy=dict(epsilon, seed, pure_new)`; None where the inner agent has no
        device form of the kinds the overlay serves (the model kinds — LogReg argmax, likelihood agent, NnIpsAgent, BayesianAgentVB —
        only with `device_models`, and never a sampling LogReg), with epsilon_select_worse and with with_ps_all."""
        c = self.config
        if getattr(c, 'epsilon_select_worse', False) or getattr(c, 'with_ps_all', False):
            return None
        from ..envs.reco_env_v1 import device_policy_of
        pol = device_policy_of(self.agent)
        if pol is None or pol.get('epsilon_greedy') is not None:
            return None
        if pol.get('policy') in _MODEL_INNER:
            # opt-in; a sampling LogReg's act is a sampled action with a propensity of its own: host path
            if not getattr(c, 'device_models', False) or (pol.get('logreg') or {}).get('select_randomly'):
                return None
            if (pol.get('logreg_poly') or {}).get('weight_history') is not None:      # a time-weighted likelihood agent: host path
                return None
        elif pol.get('policy') not in _DEVICE_INNER:
            return None
        if self._num_products() < 2 and c.epsilon_pure_new:
            return None
        pol = {k: v for k, v in pol.items() if k != 'ps_all'}        # (`ps-a` is () without the wrapper's with_ps_all)
        return dict(pol, epsilon_greedy=self._overlay())

    def ope_policy(self):
        """The replay form of `ps-a` (evaluate_agent.evaluate_IPS on the device) under with_ps_all: the inner agent's replay
        policy — RandomAgent, a last-view table or, with `device_models`, the LogReg argmax; the others' `h0` is their SAMPLED
        action — plus `epsilon_greedy=`."""
        c = self.config
        if getattr(c, 'epsilon_select_worse', False) or not getattr(c, 'with_ps_all', False):
            return None
        from ..evaluate_agent import ope_policy_of
        if type(self.agent).__module__.split('.')[0] != __name__.split('.')[0]:
            return None                     # a reference agent object inside: its greedy action comes from its own MT stream
        pol = ope_policy_of(self.agent)
        if pol is None or pol.get('epsilon_greedy') is not None:
            return None
        if pol.get('kind') == _abi.RG_POLICY_LOGREG_FROZEN:
            # opt-in (`device_models`): the argmax form only — exact as the device leaves it (rg_ope_replay_logreg_eg)
            if not getattr(c, 'device_models', False) or (pol.get('logreg') or {}).get('select_randomly'):
                return None
        elif pol.get('kind') not in _REPLAY_INNER:
            return None
        if int(pol['num_products']) < 2 and c.epsilon_pure_new:
            return None
        if pol['kind'] == _abi.RG_POLICY_RANDOM_AGENT:
            pol = dict(pol, policy_seed=self.agent.config.random_seed)      # the greedy action is the inner agent's own draw
        return dict(pol, epsilon_greedy=self._overlay())

    def ope_policy_checked(self):
        """With `device_models` and with_ps_all on the wrapper and the inner agent: the checked replay dict of the likelihood agent,
        NnIpsAgent or BayesianAgentVB (rg_ope_replay_poly_eg / _nn_eg / _bayes_eg; the host confirms the greedy acts the device lists
        as unresolved) plus `epsilon_greedy=`.  None wherever the inner agent's own ope_policy_checked() is (the last two: without
        their key `device_replay`)."""
        c = self.config
        if getattr(c, 'epsilon_select_worse', False) or not getattr(c, 'with_ps_all', False) or not getattr(c, 'device_models', False):
            return None
        if type(self.agent).__module__.split('.')[0] != __name__.split('.')[0]:
            return None
        from ..evaluate_agent import ope_checked_policy_of
        pol = ope_checked_policy_of(self.agent)
        if pol is None or pol.get('kind') not in _CHECKED_INNER or pol.get('epsilon_greedy') is not None:
            return None
        if (pol.get('logreg_poly') or {}).get('weight_history') is not None:          # a time-weighted likelihood agent: host loop
            return None
        if int(pol['num_products']) < 2 and c.epsilon_pure_new:
            return None
        return dict(pol, epsilon_greedy=self._overlay())

    def act(self, observation, reward, done):
        c = self.config
        greedy_action = self.agent.act(observation, reward, done)
        ctx = observation.context()
        _, u0, u1 = rng.policy_uniforms(c.random_seed, *(ctx.draw_key() if hasattr(ctx, 'draw_key') else (ctx.user(), ctx.time())))
        eps = c.epsilon
        # rng.choice([True, False], p=[eps, 1 - eps]): True iff the normalised cdf's first entry exceeds u0
        if not (eps / (eps + (1.0 - eps)) <= u0):
            P = self._num_products()
            if getattr(c, 'epsilon_select_worse', False):
                product_probas = 1.0 - greedy_action['ps-a']
            else:
                product_probas = np.ones(P)
            if c.epsilon_pure_new:
                product_probas[greedy_action['a']] = 0.0
            product_probas = product_probas / np.sum(product_probas)
            cdf = product_probas.cumsum()
            cdf /= cdf[-1]
            epsilon_action = int(cdf.searchsorted(u1, side='right'))
            return {
                **Agent.act(self, observation, reward, done),
                'a': epsilon_action,
                'ps': eps * product_probas[epsilon_action],
                'ps-a': eps * product_probas if getattr(c, 'with_ps_all', False) else (),
                'greedy': False,
                'h0': greedy_action['a'],
            }
        return {
            **greedy_action,
            'greedy': True,
            'ps': (1.0 - eps) * greedy_action['ps'],
            'ps-a': (1.0 - eps) * greedy_action['ps-a'] if getattr(c, 'with_ps_all', False) else (),
        }
