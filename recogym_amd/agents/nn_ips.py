"""NnIpsAgent — reference: recogym/agents/nn_ips.py.

A three-layer perceptron over the user's view counts, trained by full-batch SGD on a clipped IPS loss (nn_ips.py:28-41, 74-94):

    h1 = sigmoid(W1 x + b1);  h2 = sigmoid(W2 h1 + b2);  prob = softmax(W3 h2 + b3);  a = argmax prob;  ps = prob[a]

— the one argmax agent whose logged propensity is a model output, not 1.

Training (`NnIpsAgent`): `train` / `train_from_log` / the model built at the first act are LogregMulticlassIpsAgent's; `build()` is
the reference's recipe on torch: the same `nn.Sequential`, initialised from torch's global generator in the same order, the same
loss — its `nn.Threshold(M, M)` replaces every ratio that is not above M by M, i.e. it clips from BELOW as written; reproduced —
with the deltas negated and broadcast over the products, `optim.SGD`, `num_epochs` full-batch steps.  (With the default M = 111
every ratio prob / ps is below M, the clipped loss is constant and the net keeps its initial weights; an M below the ratios trains.)

Inference (`NnIpsFrozenAgent`, a plain Agent that holds the net as a member): `act` on the host is torch's fp32 forward on the
dense float32 counts, the reference's arithmetic.  Torch adds in BLAS's order with vectorised exp / sigmoid, so no device kernel
can be held to its bits.  The device (RG_POLICY_NN_IPS, rg_nn_common.hpp) computes the net in float64 on the fp32
weights widened, in one stated order with an exponential made of IEEE operations only, which `nn_forward` restates to the bit,
and decides by the margin W (`nn_margin`): an act is resolved when the best logit leads every other by more than 2 W (`nn_rule`).
An act the rule cannot resolve is listed and recomputed here (`Simulator.poly_verify`, the likelihood agent's protocol).
`nn_ps_bound` is the proven relative distance of the device's ps from torch's fp32 prob[a].
"""
import math

import numpy as np

from .. import _abi, rng
from ..envs.configuration import Configuration
from .abstract import Agent
from .logreg_ips import LogregMulticlassIpsAgent

# The reference's keys and defaults (its nn_ips_args).
nn_ips_args = {
    'num_products': 10,
    'number_of_flips': 1,
    'random_seed': np.random.randint(2 ** 31 - 1),

    # Select a Product randomly with the the probability predicted by Neural Network with IPS.
    'select_randomly': False,

    'M': 111,
    'learning_rate': 0.01,
    'num_epochs': 100,
    'num_hidden': 20,
    'lambda_val': 0.01,
    'with_ps_all': False,
}

UNRESOLVED = 2              # flag bit (RG_NN_UNRESOLVED)
HIDDEN_CAP = 1024           # kNnHidden
PRODUCTS_CAP = 4000         # kNnProducts
COUNT_CAP = 1 << 24         # a larger view count is not an fp32 value: torch's input differs from the device's

_LN2_HI, _LN2_LO = 6.93147180369123816490e-01, 1.90821492927058770002e-10          # fdlibm's split of ln 2
_TAYLOR = [1.0 / math.factorial(i) for i in range(14)]       # correctly rounded quotients: the kernel's constants


def nn_exp(x):
    """The device's exponential (rg_nn_common.hpp: nn_exp) to the bit: x clamped to [-700, 700], k = rint(x log2 e), r = x - k ln2 in
    two pieces, the Taylor polynomial of degree 13 by Horner (multiply, then add), scaled by 2^k.  IEEE operations only."""
    x = np.minimum(np.maximum(np.asarray(x, dtype=np.float64), -700.0), 700.0)
    k = np.rint(x * 1.4426950408889634)
    r = x - k * _LN2_HI
    r = r - k * _LN2_LO
    p = np.full_like(r, _TAYLOR[13])
    for i in range(12, -1, -1):
        p = p * r + _TAYLOR[i]
    return np.ldexp(p, k.astype(np.int32))


def nn_sigmoid(z):
    return 1.0 / (1.0 + nn_exp(-np.asarray(z, dtype=np.float64)))


def nn_abs_row_sums(wt, b):
    """max over the columns of (sum over the rows, ascending, of |wt|) + |b|, one add per term (rg_sim_set_nn_ips: the same bits)."""
    r = np.zeros(wt.shape[1], dtype=np.float64)
    for row in wt:
        r = r + np.abs(row)
    return np.float64((r + np.abs(b)).max())


class NnModel:
    """The net as the device takes it: the six fp32 arrays widened to float64, the matrices transposed ([viewed product][hidden],
    [hidden][hidden], [hidden][product]), and the absolute row sums A2, A3 of the margin."""

    def __init__(self, state):
        f = {k: np.asarray(state[k], dtype=np.float32) for k in ('w1', 'b1', 'w2', 'b2', 'w3', 'b3')}
        self.H, self.P = f['w1'].shape
        assert f['w2'].shape == (self.H, self.H) and f['w3'].shape == (self.P, self.H), {k: v.shape for k, v in f.items()}
        assert f['b1'].shape == f['b2'].shape == (self.H,) and f['b3'].shape == (self.P,)
        self.w1t, self.w2t, self.w3t = (np.ascontiguousarray(f[k].T, dtype=np.float64) for k in ('w1', 'w2', 'w3'))
        self.b1, self.b2, self.b3 = (np.ascontiguousarray(f[k], dtype=np.float64) for k in ('b1', 'b2', 'b3'))
        self.A2, self.A3 = nn_abs_row_sums(self.w2t, self.b2), nn_abs_row_sums(self.w3t, self.b3)

    def arrays(self):
        return self.w1t, self.b1, self.w2t, self.b2, self.w3t, self.b3

    def finite(self):
        return all(np.isfinite(x).all() for x in self.arrays())


def nn_forward(prods, cnts, m):
    """The device's act on a history (`prods` the distinct viewed products ascending, `cnts` their counts) in the contract's order,
    to the bit -> (z (P,), ps, action, M1): float64, multiply then add, index ascending, bias last; the softmax sum per lane over
    a = lane, lane + 64, ..., then folded over the lanes as the xor butterfly adds them."""
    s, a = np.zeros(m.H, dtype=np.float64), np.zeros(m.H, dtype=np.float64)
    for p, c in zip(np.asarray(prods, dtype=np.int64), np.asarray(cnts, dtype=np.float64)):
        t = c * m.w1t[p]
        s = s + t
        a = a + np.abs(t)
    M1 = np.float64((a + np.abs(m.b1)).max())
    h1 = nn_sigmoid(s + m.b1)
    s = np.zeros(m.H, dtype=np.float64)
    for j in range(m.H):
        s = s + m.w2t[j] * h1[j]
    h2 = nn_sigmoid(s + m.b2)
    z = np.zeros(m.P, dtype=np.float64)
    for k in range(m.H):
        z = z + m.w3t[k] * h2[k]
    z = z + m.b3
    action = int(np.argmax(z))
    e = np.zeros(-(-m.P // 64) * 64, dtype=np.float64)
    e[:m.P] = nn_exp(z - z[action])
    lanes = np.zeros(64, dtype=np.float64)
    for row in e.reshape(-1, 64):
        lanes = lanes + row
    o = 32
    while o:
        lanes = lanes[:o] + lanes[o:2 * o]
        o >>= 1
    return z, np.float64(e[action] / lanes[0]), action, M1


def nn_logit_bound(n, M1, H, A2, A3):
    """E3: the bound on |z_device[a] - z_torch[a]| for any one logit, any summation order of torch's, fused or not.
    IEEE operations only."""
    hu = np.ldexp(np.float64(int(H) + 5), -24)
    E1 = np.ldexp(np.float64(int(n) + 5), -24) * np.float64(M1)
    d1 = E1 * np.float64(0.25) + np.ldexp(np.float64(1.0), -21)
    E2 = np.float64(A2) * (hu + d1)
    d2 = E2 * np.float64(0.25) + np.ldexp(np.float64(1.0), -21)
    return np.float64(A3) * (hu + d2)


def nn_margin(n, M1, H, A2, A3):
    """W = E3 + 2^-20: the logit bound plus half the gap (2^-19) below which torch's fp32 softmax can tie or reorder two distinct
    logits.  The device computes the same bits."""
    return nn_logit_bound(n, M1, H, A2, A3) + np.ldexp(np.float64(1.0), -20)


def nn_rule(prods, cnts, m):
    """The device's decision (numpy restatement of nn_act) -> (action, flags, z, ps)."""
    z, ps, action, M1 = nn_forward(prods, cnts, m)
    W = nn_margin(len(prods), M1, m.H, m.A2, m.A3)
    others = np.delete(z, action)
    gap = z[action] - others.max() if len(others) else np.float64(np.inf)
    big = len(cnts) > 0 and int(np.max(cnts)) > COUNT_CAP
    resolved = bool(gap > 2.0 * W) and not big
    return action, (0 if resolved else UNRESOLVED), z, ps


def nn_ps_bound(n, M1, H, A2, A3, P):
    """The proven bound on |ps_device / ps_torch - 1|: both logit sets within E3 of each other move ln ps by at most
    2 E3; torch's fp32 arithmetic adds (ln P + P + 24) 2^-24: ln P its subtraction of the maximum, 16 its two exps (4 ulp allowed
    each), P its sum, 3 its division (or reciprocal and product), 5 spare for second-order terms and the device's own roundings."""
    t = 2.0 * float(nn_logit_bound(n, M1, H, A2, A3)) + (math.log(max(int(P), 1)) + int(P) + 24.0) * 2.0 ** -24
    return math.expm1(t) if t < 700.0 else math.inf


def make_net(num_products, num_hidden):
    """The reference's nn.Sequential (nn_ips.py:53-60), initialised from torch's global generator in the same order."""
    from torch import nn
    return nn.Sequential(nn.Linear(num_products, num_hidden), nn.Sigmoid(), nn.Linear(num_hidden, num_hidden), nn.Sigmoid(),
                         nn.Linear(num_hidden, num_products), nn.Softmax(dim=1))


def net_state(net):
    """The six arrays of a net built by make_net (or the reference's NeuralNet.model) as float32 numpy arrays."""
    lin = [net[0], net[2], net[4]]
    out = {}
    for i, layer in enumerate(lin, 1):
        out[f'w{i}'] = layer.weight.detach().cpu().numpy().astype(np.float32).copy()
        out[f'b{i}'] = layer.bias.detach().cpu().numpy().astype(np.float32).copy()
    return out


def torch_forward(net, views):
    """torch's fp32 forward on the dense float32 counts -> prob (P,) float32 numpy."""
    import torch
    x = torch.from_numpy(np.asarray(views, dtype=np.float32).reshape(1, -1))
    with torch.no_grad():
        return net(x)[0, :].numpy()


class NnIpsFrozenAgent(Agent):
    def __init__(self, config, state):
        """state: dict(w1 (H, P), b1 (H,), w2 (H, H), b2 (H,), w3 (P, H), b3 (P,)) as torch's nn.Linear stores them (float32)."""
        import torch
        super().__init__(config)
        self.model = NnModel(state)
        assert self.model.P == int(config.num_products), (self.model.P, config.num_products)
        self.select_randomly = bool(getattr(config, 'select_randomly', False))
        self.net = make_net(self.model.P, self.model.H)
        with torch.no_grad():
            for i, layer in enumerate((self.net[0], self.net[2], self.net[4]), 1):
                layer.weight.copy_(torch.from_numpy(np.asarray(state[f'w{i}'], dtype=np.float32)))
                layer.bias.copy_(torch.from_numpy(np.asarray(state[f'b{i}'], dtype=np.float32)))
        # weight_history_function (ViewsFeaturesProvider with history): time-weighted features, on the host path only
        self.history = None
        if getattr(config, 'weight_history_function', None) is not None:
            from .views_history import ViewsHistory
            self.history = ViewsHistory(self.model.P, config.weight_history_function, is_sparse=False)
        self.reset()

    def state(self):
        return net_state(self.net)

    def device_policy(self):
        """None under with_ps_all (no `ps-a` on the device), with a weight function, with select_randomly (a sampled act), with a
        net beyond the kernel's caps or one that is not finite."""
        if getattr(self.config, 'with_ps_all', False) or self.history is not None or self.select_randomly:
            return None
        if self.model.H > HIDDEN_CAP or self.model.P > PRODUCTS_CAP or not self.model.finite():
            return None
        return dict(policy=_abi.RG_POLICY_NN_IPS, policy_seed=0, ouc=None, nn_ips=dict(state=self.state()))

    def ope_policy(self):
        return None

    def ope_policy_checked(self):
        """The replay form of the argmax act (rg_ope_replay_nn; `ps-a` is one-hot at the act), which lists the acts its margin cannot
        resolve for the host's confirmation (evaluate_agent.ope_replay, sim.replay_verify).  Opt-in: the configuration key
        `device_replay`.  None — the host loop — without it, without with_ps_all, with a weight function, with select_randomly
        (its `ps-a` is torch's fp32 softmax: no device value equals it), with a net beyond the kernel's caps or one that is not
        finite."""
        c = self.config
        if not getattr(c, 'with_ps_all', False) or not getattr(c, 'device_replay', False) or self.history is not None or self.select_randomly:
            return None
        if self.model.H > HIDDEN_CAP or self.model.P > PRODUCTS_CAP or not self.model.finite():
            return None
        return dict(kind=_abi.RG_POLICY_NN_IPS, num_products=int(c.num_products), policy_seed=0, nn_ips=dict(state=self.state()))

    def reset(self):
        self.views = np.zeros(self.config.num_products, dtype=np.int64)
        if getattr(self, 'history', None) is not None:
            self.history.reset()

    def act_on(self, prods, cnts):
        """(action, ps) on a history given as (distinct products, counts): torch's forward on the dense float32 counts."""
        x = np.zeros(self.config.num_products, dtype=np.float32)
        x[np.asarray(prods, dtype=np.int64)] = np.asarray(cnts)
        prob = torch_forward(self.net, x)
        a = int(np.argmax(prob))
        return a, float(prob[a])

    def act(self, observation, reward, done):
        for session in observation.sessions():
            self.views[int(session['v'])] += 1
        if self.history is not None:
            self.history.observe(observation)
            x = np.asarray(self.history.features(observation.context().time()), dtype=np.float32)
        else:
            x = self.views
        prob = torch_forward(self.net, x)
        with_all = getattr(self.config, 'with_ps_all', False)
        if self.select_randomly:
            # nn_ips.py:113-122 draws from its own RandomState; here one addressed policy uniform, as LogregFrozenAgent.act does
            ctx = observation.context()
            key = ctx.draw_key() if hasattr(ctx, 'draw_key') else (ctx.user(), ctx.time())
            _, _, u1 = rng.policy_uniforms(self.config.random_seed, *key)
            cdf = prob.astype(np.float64).cumsum()
            cdf /= cdf[-1]
            a = min(int(cdf.searchsorted(u1, side='right')), len(cdf) - 1)
            ps_all = prob if with_all else ()
        else:
            a = int(np.argmax(prob))
            ps_all = ()
            if with_all:                                      # nn_ips.py:125-127: a one-hot vector over the products
                ps_all = np.zeros(self.config.num_products)
                ps_all[a] = 1.0
        return {**super().act(observation, reward, done), 'a': a, 'ps': float(prob[a]), 'ps-a': ps_all}


class NnIpsAgent(LogregMulticlassIpsAgent):
    """`train` / `train_from_log` / the model built at the first act: LogregMulticlassIpsAgent's; `build()` is this agent's."""

    def __init__(self, config=Configuration(nn_ips_args)):
        super().__init__(config)

    def ope_policy_checked(self):
        return self._ready().ope_policy_checked()

    def build(self):
        """nn_ips.py:74-94."""
        import torch
        from torch import nn, optim
        feats, actions, deltas, pss = self._training_set()
        c = self.config
        P = int(c.num_products)
        X = np.asarray(feats.todense(), dtype=np.float64) if hasattr(feats, 'todense') else np.asarray(feats, dtype=np.float64)
        net = make_net(P, int(c.num_hidden))
        clipping = nn.Threshold(c.M, c.M)
        optimizer = optim.SGD(net.parameters(), lr=c.learning_rate)
        deltas = np.asarray(deltas)[:, np.newaxis] * np.ones((1, P))
        pss = np.asarray(pss)[:, np.newaxis] * np.ones((1, P))
        for _ in range(int(c.num_epochs)):
            optimizer.zero_grad()
            hx, h0, d = net(torch.Tensor(X)), torch.Tensor(pss), torch.Tensor(-1.0 * deltas)
            u = clipping(hx / h0) * d
            loss = torch.mean(u) + c.lambda_val * torch.sqrt(torch.var(u) / d.shape[0])
            loss.backward()
            optimizer.step()
        self.frozen = NnIpsFrozenAgent(c, net_state(net))
        return self.frozen
