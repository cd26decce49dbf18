"""PyTorchMLRAgent — reference: recogym/agents/pytorch_mlr.py.

A P x P multinomial logistic regression over the user's view counts, trained on a (clipped / logged / variance-penalised) IPS
estimate of the reward of the clicked rows; with `alpha` > 0 the objective is mixed with an (IPS-weighted) click likelihood of a
binomial model that shares the weight.  Training is a full-batch L-BFGS; the model then acts by

    a = argmax(x W^T)  in fp32,  ps = 1,  `ps-a` the one-hot vector at a (whatever with_ps_all says).

Training (`PyTorchMLRAgent`): `train` / `train_from_log` / the model built at the first act are LogregMulticlassIpsAgent's; `build()`
is the reference's recipe on torch (pytorch_mlr.py:119-259): the same two modules, initialised from torch's global generator in the
same order, the same closure, 200 optimiser steps with max_ls = 20.  The reference vendors a third-party L-BFGS of which one path
is live — the full-batch step with the weak-Wolfe line search and interpolation.  `WolfeLBFGS` below restates that path (curvature
update with rejection, two-loop recursion, bracketing, two-point quadratic interpolation, t = 0 on failure) so that it issues the
same torch operations in the same order: the trained weight equals the reference's bit for bit (tests/test_mlr_host.py).  No
prints, no progress bar.

Inference (`PyTorchMLRFrozenAgent`): `act` on the host is the reference's arithmetic, an fp32 dot per action in BLAS's order: no
device kernel can be held to its bits.  The device (RG_POLICY_MLR, rg_mlr_common.hpp) computes the scores in float64
on the fp32 weights widened, in one stated order, which `mlr_forward` restates to the bit, and decides by the margin E
(`mlr_margin`): an act is resolved when the best score leads the second best by more than 2 E (`mlr_rule`).  An act the rule
cannot resolve is listed and recomputed here (`Simulator.poly_verify`, the likelihood agent's protocol).
"""
import numpy as np

from .. import _abi
from ..envs.configuration import Configuration
from .abstract import Agent
from .logreg_ips import LogregMulticlassIpsAgent

# The reference's keys and defaults (its pytorch_mlr_args).
pytorch_mlr_args = {
    'n_epochs': 30,
    'learning_rate': 0.01,
    'random_seed': np.random.randint(2 ** 31 - 1),
    'logIPS': False,
    'variance_penalisation_strength': .0,
    'clip_weights': False,
    'alpha': .0,
    'll_IPS': True,
}

UNRESOLVED = 2              # flag bit (RG_MLR_UNRESOLVED)
PRODUCTS_CAP = 4000         # kMlrProducts
COUNT_CAP = 1 << 24         # a larger view count is not an fp32 value: the reference's input differs from the device's
M1_CAP = 2.0 ** 126         # below it no partial sum of an fp32 dot can overflow

MAX_EPOCH, MAX_LS = 200, 20        # pytorch_mlr.py:229, 236


# ------------------------------------------------------------------------------------------------
# the act contract
# ------------------------------------------------------------------------------------------------
def mlr_table(W):
    """W (P, P) float32 [action][viewed product] -> the device's table: float64, [viewed product][action]."""
    W = np.asarray(W, dtype=np.float32)
    assert W.ndim == 2 and W.shape[0] == W.shape[1], W.shape
    return np.ascontiguousarray(W.T, dtype=np.float64)


def mlr_forward(prods, cnts, wt):
    """The device's scores on a history (`prods` the distinct viewed products ascending, `cnts` their counts) in the contract's
    order, to the bit -> (z (P,), action, M1): float64, multiply then add, the viewed products ascending; the lowest index among
    the maxima."""
    P = wt.shape[0]
    z, m = np.zeros(P, dtype=np.float64), np.zeros(P, dtype=np.float64)
    for p, c in zip(np.asarray(prods, dtype=np.int64), np.asarray(cnts, dtype=np.float64)):
        t = c * wt[p]
        z = z + t
        m = m + np.abs(t)
    return z, int(np.argmax(z)), np.float64(m.max())


def mlr_margin(n, M1):
    """E = (n + 5) 2^-24 M1: the bound on |z_device[a] - z_reference[a]| for any one score, any summation order of the reference's
    fp32 dot, fused or not.  IEEE operations only; the device computes the same bits."""
    return np.ldexp(np.float64(int(n) + 5), -24) * np.float64(M1)


def mlr_rule(prods, cnts, wt):
    """The device's decision (numpy restatement of mlr_act) -> (action, flags, z)."""
    z, action, M1 = mlr_forward(prods, cnts, wt)
    others = np.delete(z, action)
    gap = z[action] - others.max() if len(others) else np.float64(np.inf)
    big = len(cnts) > 0 and int(np.max(cnts)) > COUNT_CAP
    resolved = len(cnts) > 0 and bool(gap > 2.0 * mlr_margin(len(prods), M1)) and bool(M1 < M1_CAP) and not big
    return action, (0 if resolved else UNRESOLVED), z


def host_act(views, W):
    """The reference's arithmetic (pytorch_mlr.py:30-32, 70-72) on the dense view counts."""
    P = W.shape[0]
    return int(np.argmax(np.asarray(views).astype(np.float32).reshape(1, P).dot(W.T).reshape(P)))


# ------------------------------------------------------------------------------------------------
# the frozen agent
# ------------------------------------------------------------------------------------------------
class PyTorchMLRFrozenAgent(Agent):
    def __init__(self, config, W):
        """W: (P, P) float32, [action][viewed product], as the reference's model.weight stores it."""
        super().__init__(config)
        self.W = np.ascontiguousarray(W, dtype=np.float32)
        assert self.W.shape == (int(config.num_products),) * 2, (self.W.shape, config.num_products)
        # weight_history_function (ViewsFeaturesProvider with history): time-weighted features, on the host path only
        self.history = None
        if getattr(config, 'weight_history_function', None) is not None:
            from .views_history import ViewsHistory
            self.history = ViewsHistory(int(config.num_products), config.weight_history_function, is_sparse=False)
        self.reset()

    def state(self):
        return dict(W=self.W.copy())

    def _device_form(self):
        return self.history is None and self.W.shape[0] <= PRODUCTS_CAP and bool(np.isfinite(self.W).all())

    def ps_all_from_log(self, df):
        """`ps-a` of every bandit row of a log this agent produced: the one-hot vector at the row's action (the device log carries
        none; the reference emits it whatever with_ps_all says); None on organic rows.  One lookup in a table of the P one-hot rows
        (the rows of an action share their vector, as the uniform logger's rows share theirs: envs/reco_env_v1.rows_to_dataframe)."""
        P = int(self.config.num_products)
        lut = np.empty(P + 1, dtype=object)
        for a, row in enumerate(np.eye(P)):
            lut[a] = row
        lut[P] = None
        is_b = (df['z'] == 'bandit').to_numpy()
        a_col = df['a'].to_numpy(dtype=np.float64, na_value=0.0).astype(np.int64)
        return lut[np.where(is_b, a_col, P)]

    def device_policy(self):
        """None with a weight function, with a table beyond the kernel's cap or one that is not finite."""
        if not self._device_form():
            return None
        return dict(policy=_abi.RG_POLICY_MLR, policy_seed=0, ouc=None, mlr=dict(state=self.state()), ps_all=self.ps_all_from_log)

    def ope_policy(self):
        return None

    def ope_policy_checked(self):
        """The replay form of the act (rg_ope_replay_mlr; `ps-a` is one-hot at the act), which lists the acts its margin cannot
        resolve for the host's confirmation (evaluate_agent.ope_replay, sim.replay_verify).  Opt-in: the configuration key
        `device_replay`.  None — the host loop — without it, with a weight function, with a table beyond the kernel's cap or one
        that is not finite."""
        c = self.config
        if not getattr(c, 'device_replay', False) or not self._device_form():
            return None
        return dict(kind=_abi.RG_POLICY_MLR, num_products=int(c.num_products), policy_seed=0, mlr=dict(state=self.state()))

    def reset(self):
        self.views = np.zeros(self.config.num_products, dtype=np.int64)
        if getattr(self, 'history', None) is not None:
            self.history.reset()

    def act_on(self, prods, cnts):
        """(action, ps) on a history given as (distinct products, counts): the reference's arithmetic on the dense float32 counts."""
        x = np.zeros(self.config.num_products, dtype=np.float32)
        x[np.asarray(prods, dtype=np.int64)] = np.asarray(cnts)
        return host_act(x, self.W), 1.0

    def act(self, observation, reward, done):
        for session in observation.sessions():
            self.views[int(session['v'])] += 1
        if self.history is not None:
            self.history.observe(observation)
            x = np.asarray(self.history.features(observation.context().time()))
        else:
            x = self.views
        a = host_act(x, self.W)
        ps_all = np.zeros(self.config.num_products)
        ps_all[a] = 1.0
        return {**super().act(observation, reward, done), 'a': a, 'ps': 1.0, 'ps-a': ps_all}


# ------------------------------------------------------------------------------------------------
# training
# ------------------------------------------------------------------------------------------------
def _finite(v):
    import torch
    return not torch.isnan(v).any() and not torch.isinf(v)


def _quadratic_min(x1, f1, g1, x2, f2):
    """The minimiser of the parabola through (x1, f1) with slope g1 and (x2, f2), clamped to [min(x1, x2), max(x1, x2)]: float64."""
    x1, f1, g1, x2, f2 = (np.float64(v) for v in (x1, f1, g1, x2, f2))
    with np.errstate(all='ignore'):
        if x1 == 0:
            sol = -g1 * x2 ** 2 / (2 * (f2 - f1 - g1 * x2))
        else:
            a = -(f1 - f2 - g1 * (x1 - x2)) / (x1 - x2) ** 2
            sol = x1 - g1 / (2 * a)
    return np.minimum(np.maximum(np.minimum(x1, x2), sol), np.maximum(x1, x2))


def _next_length(t, lo, hi, F_lo, g_lo, F_hi):
    """The next trial step length of the bracketing search.  [lo, hi] brackets a weak-Wolfe point (hi None: no upper bound yet);
    F_lo / g_lo: objective and slope along the direction at lo, F_hi: objective at hi.  Without an upper bound the length doubles;
    with one whose objective is finite the parabola's minimiser is taken, kept at least a fifth of the bracket above lo and at
    most half the bracket's WIDTH (not its midpoint: the reference's safeguard, kept for its bits); otherwise the midpoint."""
    if hi is None:
        return 2 * t
    if not _finite(F_hi):
        return (lo + hi) / 2.0
    width = hi - lo
    t = _quadratic_min(lo, F_lo.item(), g_lo.item(), hi, F_hi.item())
    if t < lo + 0.2 * width:
        t = lo + 0.2 * width
    elif t > width / 2.0:
        t = width / 2.0
    return width / 2.0 if t <= 0 else t


class WolfeLBFGS:
    """Full-batch L-BFGS with a weak-Wolfe bracketing line search: 10 curvature pairs, first trial length 1, sufficient decrease
    1e-4, curvature 0.9, pairs with y.s <= 1e-2 s.Bs rejected.  Flat float32 vectors throughout.  The torch operations that touch
    the parameters, the gradients and the pairs are issued in the order of the reference optimiser's one live path, which is what
    makes the trained weight the reference's to the bit; the bookkeeping round them is this class's own: a pair's step s, its
    B s = -t g and s.Bs are formed when the step is taken (one place), not when the next gradient arrives."""
    PAIRS, REJECT, DECREASE, CURVATURE = 10, 1e-2, 1e-4, 0.9

    def __init__(self, params):
        self.params = list(params)
        self.steps = 0
        self.scale = 1                        # the initial inverse-Hessian scale: y.s / y.y of the newest pair
        self.S, self.Y = [], []               # steps s = t d, gradient differences y
        self.last = None                      # (gradient at the last iterate, s, s.Bs) of the last step, None after a failed search

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    def _gradient(self):
        import torch
        return torch.cat([torch.zeros_like(p.data).view(-1) if p.grad is None else p.grad.data.view(-1) for p in self.params], 0)

    def _move(self, length, direction):
        at = 0
        for p in self.params:
            n = p.numel()
            p.data.add_(direction[at:at + n].view_as(p.data), alpha=length)
            at += n

    def _remember(self, grad):
        """The curvature pair of the last step, kept where y.s > 1e-2 s.Bs."""
        if self.last is None:
            return
        g_prev, s, sBs = self.last
        y = grad.sub(g_prev)
        ys = y.dot(s)
        if ys > self.REJECT * sBs:
            self.S, self.Y = (self.S + [s])[-self.PAIRS:], (self.Y + [y])[-self.PAIRS:]
            self.scale = ys / y.dot(y)

    def _direction(self, q):
        """The two-loop recursion on q = -gradient (overwritten)."""
        import torch
        pairs = list(zip(self.S, self.Y))
        rho = [1. / y.dot(s) for s, y in pairs]
        coef = []
        for (s, y), r in zip(reversed(pairs), reversed(rho)):
            a = s.dot(q) * r
            q.add_(y, alpha=float(-a))
            coef.append(a)
        d = torch.mul(q, self.scale)
        for (s, y), r, a in zip(pairs, rho, reversed(coef)):
            b = y.dot(d) * r
            d.add_(s, alpha=float(a - b))
        return d

    def _search(self, closure, F_0, slope, d, max_ls):
        """The parameters move along d until the weak Wolfe conditions hold -> (objective there, length); after max_ls trials they
        are back at the iterate, with its objective and gradient evaluated once more, and the length is 0."""
        import torch
        t = t_at = 1                          # the trial length; the length the parameters stand at
        lo, hi = 0, None
        F_lo, g_lo, F_hi = F_0, slope, torch.tensor(np.nan, dtype=torch.float)
        self._move(t, d)
        F = closure()
        for _ in range(max_ls):
            if F > F_0 + self.DECREASE * t * slope:        # no sufficient decrease: an upper bound
                hi, F_hi = t, F
            else:
                F.backward()
                g = self._gradient().dot(d)
                if not g < self.CURVATURE * slope:         # the slope has flattened: done
                    return F, t
                lo, F_lo, g_lo = t, F, g                   # still steep: a lower bound
            t_at, t = t, _next_length(t, lo, hi, F_lo, g_lo, F_hi)
            self._move(t - t_at, d)
            F = closure()
        self._move(-t, d)                                  # (the trial after the last test is not tested: the reference's count)
        F = closure()
        F.backward()
        return F, 0

    def step(self, closure, current_loss, max_ls):
        """One step from the gradients the last backward left -> the objective at the new iterate (with its graph)."""
        grad = self._gradient()
        if self.steps:
            self._remember(grad)
        self.steps += 1
        d = self._direction(-grad)
        F, t = self._search(closure, current_loss, grad.dot(d), d, max_ls)
        if t == 0:
            self.last = None
        else:
            s, Bs = d.mul(t), grad.mul(-t)
            self.last = (grad, s, s.dot(Bs))
        return F


def make_models(P):
    """The reference's two modules (pytorch_mlr.py:86-117): the multinomial one owns a (P, P) weight (kaiming_uniform_, a = sqrt 5)
    and a one-element bias (uniform in +-1 / sqrt(fan_in)), drawn from torch's global generator in this order; the binomial one
    shares both."""
    import torch
    from torch.nn import functional as F

    class Multinomial(torch.nn.Module):
        def __init__(self, input_dim, output_dim):
            super().__init__()
            self.weight = torch.nn.Parameter(torch.Tensor(output_dim, input_dim))
            torch.nn.init.kaiming_uniform_(self.weight, a=np.sqrt(5))
            self.bias = torch.nn.Parameter(torch.Tensor(1))
            fan_in, _ = torch.nn.init._calculate_fan_in_and_fan_out(self.weight)
            bound = 1 / np.sqrt(fan_in)
            torch.nn.init.uniform_(self.bias, -bound, bound)

        def forward(self, x):
            return F.linear(x, self.weight)

    class Binomial(torch.nn.Module):
        def __init__(self, multinomial):
            super().__init__()
            self.weight = multinomial.weight
            self.bias = multinomial.bias

        def forward(self, x, a):
            return torch.sigmoid((x * self.weight[a, :]).sum(dim=1) + self.bias)

    multinomial = Multinomial(P, P)
    return multinomial, Binomial(multinomial)


class PyTorchMLRAgent(LogregMulticlassIpsAgent):
    """`train` / `train_from_log` / the model built at the first act: LogregMulticlassIpsAgent's; `build()` is this agent's."""

    def __init__(self, config=Configuration(pytorch_mlr_args)):
        super().__init__(config)

    def ope_policy_checked(self):
        return self._ready().ope_policy_checked()

    def build(self):
        """pytorch_mlr.py:119-259."""
        import torch
        from torch.nn import functional as F
        feats, actions, deltas, pss = self._training_set()
        c = self.config
        X = np.asarray(feats.todense()) if hasattr(feats, 'todense') else np.asarray(feats)
        A, y, pss = np.asarray(actions), np.asarray(deltas), np.asarray(pss)
        P = X.shape[1]
        multinomial, binomial = make_models(P)

        # the clipping constant: a number, or the ratio of the 90th and 10th percentile of the clicked propensities (POEM)
        M = np.inf
        if type(c.clip_weights) != bool:
            M = c.clip_weights
        elif c.clip_weights:
            M = np.percentile(pss[y != 0], 90) / np.percentile(pss[y != 0], 10)

        # the clicked rows for the multinomial part, all rows for the binomial part
        X1 = torch.Tensor(X[y != 0])
        A1 = torch.LongTensor(A[y != 0])
        w1 = torch.Tensor(pss[y != 0] ** -1)
        N1 = X1.shape[0]
        X = torch.Tensor(X)
        A = torch.LongTensor(A)
        w = torch.Tensor(pss ** -1)
        y = torch.Tensor(y)
        bce = torch.nn.BCELoss(reduction='none')
        opt = WolfeLBFGS(multinomial.parameters())

        def closure():
            opt.zero_grad()
            if c.alpha < 1.0:
                p_a = F.softmax(multinomial(X1), dim=1)
                p_a = torch.gather(p_a, 1, A1.unsqueeze(1))
                p_a = p_a.reshape(-1)
                reward = torch.clamp(p_a * w1, max=M)                         # the (clipped) IPS estimate of the reward
                log_reward = torch.log(torch.clamp(p_a, min=1e-10)) * w1
                loss = -reward
                log_loss = -log_reward
                if c.variance_penalisation_strength:
                    avg = torch.mean(loss)
                    var = torch.sqrt(torch.sum((loss - avg) ** 2) / (N1 - 1) / N1)
                    if c.logIPS:
                        loss = log_loss.mean() + c.variance_penalisation_strength * var
                    else:
                        loss = loss.mean() + c.variance_penalisation_strength * var
                else:
                    loss = log_loss.mean() if c.logIPS else loss.mean()
            if .0 < c.alpha:
                nll = bce(binomial(X, A), y)
                if c.ll_IPS:
                    nll = nll * w
                nll = nll.mean()
            if c.alpha == .0:
                pass
            elif c.alpha == 1.0:
                loss = nll
            else:
                loss = (1.0 - c.alpha) * loss + c.alpha * nll
            return loss

        obj = closure()
        for _ in range(MAX_EPOCH):
            obj = opt.step(closure, obj, MAX_LS)
        self.frozen = PyTorchMLRFrozenAgent(c, multinomial.weight.detach().numpy().astype(np.float32).copy())
        return self.frozen
