"""BayesianAgentVB — reference: recogym/agents/bayesian_poly_vb.py.

A Bayesian logistic regression of the click on kron(view counts, one-hot action), fitted by variational Bayes (Ormerod & Wand,
Algorithm 6: 200 fixed-point iterations), and S = 1000 draws `Lambda` (S, P^2) from the fitted posterior.  Its act averages the
click probability over the draws and takes the best action: `argmax(expit(matmul(kron(X, eye(P)), Lambda.T)).mean(1))`, `ps = 1`
(bayesian_poly_vb.py:71-91).

Training (`BayesianAgentVB`): `train` / `train_from_log` / the model built at the first act are LogregMulticlassIpsAgent's;
`build()` is the reference's recipe (bayesian_poly_vb.py:30-41, 93-107) with two deviations: the two random draws
(`rand(N)` for zeta, then `multivariate_normal.rvs`) come, in the reference's order, from the agent's own
`np.random.RandomState(config.random_seed)` instead of NumPy's global stream; and the number of draws is the key `num_samples`
(default 1000, the reference's constant).  The reference's two N x N intermediates are not formed: `Psi.T @ diag(JJ)` is a column
scaling (every entry of a product with a diagonal matrix has one non-zero term: the same values), and
`diag(Psi B Psi.T)` is the row-wise sum of `(Psi B) * Psi` (the same terms in another order than BLAS adds them: the bits differ,
by a few units of the last place of zeta per iteration).

Inference (`BayesianVBFrozenAgent`): `act` on the host is the reference's expression itself.  Its matmul adds the non-zero
terms in BLAS's order, so the value of `action_proba` is not a function of the inputs alone, and no device kernel can be held to
it bit for bit.  The device (RG_POLICY_BAYES_VB, rg_bayes_common.hpp) computes

    z[a][s] = 0;  for p viewed, ascending: z[a][s] += count[p] lam_t[p][a][s]        (`bayes_decisions`: bit for bit)
    q[a] = (sum_s 1 / (1 + exp(-z[a][s]))) / S

and decides by a margin W (`bayes_margin`) that bounds the distance of q[a] from the reference's mean in ANY summation order,
with a second exact zone where means saturate at 1.0 (`bayes_rule`).  An act the rule cannot resolve is listed and recomputed
here (`Simulator.poly_verify`, the likelihood agent's protocol).
"""
import numpy as np

from .. import _abi
from ..envs.configuration import Configuration
from .abstract import Agent
from .logreg_ips import LogregMulticlassIpsAgent

# The reference's keys and defaults (its bayesian_poly_args) and `num_samples`.
bayesian_poly_args = {
    'num_products': 10,
    'random_seed': np.random.randint(2 ** 31 - 1),

    'poly_degree': 2,
    'max_iter': 5000,
    'aa': 1.,
    'bb': 1.,
    'with_ps_all': False,
    'num_samples': 1000,            # posterior draws (the reference's constant)
}

ZSAT = 40.0                 # a decision from here up has expit exactly 1.0 on both sides (RG_BAYES_ZSAT; expit saturates at 36.74)
SATURATED, UNRESOLVED = 1, 2        # flag bits (RG_BAYES_SATURATED, RG_BAYES_UNRESOLVED)
MODEL_BYTES_CAP = 1 << 31   # P P S 8 bytes of transposed model at most (kBayesModelBytes: what one raw buffer resource spans)
VB_ITERATIONS = 200


def JJ(zeta):
    return 1. / (2. * zeta) * (1. / (1 + np.exp(-zeta)) - 0.5)


def bayesian_logistic(Psi, y, mu_beta, Sigma_beta, rng, iterations=VB_ITERATIONS):
    """bayesian_poly_vb.py:35-41 without its N x N intermediates (module docstring); zeta starts from rng.rand(N)."""
    from numpy.linalg import inv
    zeta = rng.rand(Psi.shape[0])
    for _ in range(iterations):
        q_Sigma = inv(inv(Sigma_beta) + 2 * np.matmul(Psi.T * JJ(zeta)[np.newaxis, :], Psi))
        q_mu = np.matmul(q_Sigma, (np.matmul(Psi.T, y - 0.5) + np.matmul(inv(Sigma_beta), mu_beta)))
        zeta = np.sqrt(np.einsum('ij,ij->i', np.matmul(Psi, q_Sigma + np.matmul(q_mu, q_mu.T)), Psi))
    return q_mu, q_Sigma


def bayes_transpose(Lambda, num_products):
    """Lambda (S, P^2), column p P + a -> lam_t (P, P, S) [viewed product][action][sample], contiguous."""
    P = int(num_products)
    Lambda = np.asarray(Lambda, dtype=np.float64)
    assert Lambda.ndim == 2 and Lambda.shape[1] == P * P, (Lambda.shape, P)
    return np.ascontiguousarray(Lambda.T.reshape(P, P, Lambda.shape[0]))


def bayes_decisions(prods, cnts, lam_t):
    """The (P, S) decisions of one act in the contract's order: `prods` the distinct viewed products ascending, `cnts` their
    counts; s = s + c lam_t[p], multiply then add, float64."""
    z = np.zeros(lam_t.shape[1:], dtype=np.float64)
    for p, c in zip(np.asarray(prods, dtype=np.int64), np.asarray(cnts, dtype=np.float64)):
        z = z + c * lam_t[p]
    return z


def bayes_abs_sum(prods, cnts, lam_t):
    """M = max over (a, s) of sum_j |c_j lam_t[p_j][a][s]|, the sum in the contract's order (the kernel accumulates it beside the
    decisions: the same bits)."""
    m = np.zeros(lam_t.shape[1:], dtype=np.float64)
    for p, c in zip(np.asarray(prods, dtype=np.int64), np.asarray(cnts, dtype=np.float64)):
        m = m + np.abs(c * lam_t[p])
    return np.float64(m.max()) if m.size else np.float64(0.0)


def bayes_z_bound(n, M):
    """ez = (2 n + 4) 2^-53 M >= 2 gamma_n M: the distance of a decision as the device adds it from the same n products added in
    any other order, fused or not.  IEEE operations only."""
    return np.ldexp(np.float64(2 * int(n) + 4), -53) * np.float64(M)


def bayes_margin(n, M, S):
    """W = ez / 4 + (2 S + 44) 2^-53: the bound on |q_device[a] - q_reference[a]| for any one action, any summation order of the
    reference, valid whenever ez < 1 (DESIGN.md 4h has the five terms).  IEEE operations only: the device computes the same bits."""
    return bayes_z_bound(n, M) * np.float64(0.25) + np.ldexp(np.float64(2 * int(S) + 44), -53)


def bayes_means(z):
    """q[a] in the device's order: per lane the sum of expit over s = lane, lane + 64, ..., then the xor butterfly over the 64
    lanes, divided by S.  (expit here is scipy's, the device's is 1 / (1 + exp(-z)) with its own exp: the two q differ by what W's
    third and fourth term cover, a few units of 2^-53 — z, M, W and the saturated set are the device's to the bit.)"""
    from scipy.special import expit
    P, S = z.shape
    e = np.zeros((P, -(-S // 64) * 64), dtype=np.float64)
    e[:, :S] = expit(z)
    e = e.reshape(P, -1, 64)
    lanes = np.zeros((P, 64), dtype=np.float64)
    for k in range(e.shape[1]):
        lanes = lanes + e[:, k, :]
    o = 32
    while o:
        lanes = lanes[:, :o] + lanes[:, o:2 * o]
        o >>= 1
    return lanes[:, 0] / np.float64(S)


def bayes_rule(z, n, M):
    """The device's decision (numpy restatement of bayes_act) on the (P, S) decisions z of a history of n distinct products whose
    absolute sums peak at M -> (action, flags)."""
    if n == 0:
        return 0, 0
    P, S = z.shape
    q = bayes_means(z)
    a_star = int(np.argmax(q))
    W = bayes_margin(n, M, S)
    if bayes_z_bound(n, M) >= 1.0:
        return a_star, UNRESOLVED
    sat = np.flatnonzero(z.min(axis=1) >= ZSAT)
    if len(sat):
        a_c = int(sat[0])
        return a_c, SATURATED | (UNRESOLVED if bool(np.any(np.float64(1.0) - q[:a_c] <= W)) else 0)
    others = np.delete(q, a_star)
    return a_star, (UNRESOLVED if bool(np.any(q[a_star] - others <= 2.0 * W)) else 0)


def reference_act(X, Lambda):
    """The reference's expression (bayesian_poly_vb.py:73-78) on the (1, P) features X -> (action, action_proba)."""
    from scipy.special import expit
    P = X.shape[1]
    A = np.eye(P)
    XA = np.kron(X, A)
    action_proba = expit(np.matmul(XA, Lambda.T)).mean(1)
    return int(np.argmax(action_proba)), action_proba


class BayesianVBFrozenAgent(Agent):
    def __init__(self, config, Lambda):
        """Lambda (S, P^2): the posterior draws, column p P + a the weight of (viewed product p, action a)."""
        super().__init__(config)
        P = int(config.num_products)
        self.Lambda = np.ascontiguousarray(Lambda, dtype=np.float64)
        assert self.Lambda.ndim == 2 and self.Lambda.shape[1] == P * P and self.Lambda.shape[0] >= 1, (self.Lambda.shape, P)
        # weight_history_function (ViewsFeaturesProvider with history): time-weighted features, on the host path only
        self.history = None
        if getattr(config, 'weight_history_function', None) is not None:
            from .views_history import ViewsHistory
            self.history = ViewsHistory(P, config.weight_history_function, is_sparse=False)
        self._lam_t = None
        self.reset()

    @property
    def lam_t(self):
        if self._lam_t is None:
            self._lam_t = bayes_transpose(self.Lambda, self.config.num_products)
        return self._lam_t

    def device_policy(self):
        """None under with_ps_all (no `ps-a` on the device), with a weight function, with a model beyond MODEL_BYTES_CAP or one
        that is not finite."""
        if getattr(self.config, 'with_ps_all', False) or self.history is not None:
            return None
        if self.Lambda.size * 8 > MODEL_BYTES_CAP or not np.isfinite(self.Lambda).all():
            return None
        return dict(policy=_abi.RG_POLICY_BAYES_VB, policy_seed=0, ouc=None, bayes_vb=dict(lam=self.Lambda))

    def ope_policy(self):
        return None

    def ope_policy_checked(self):
        """The replay form of the act (rg_ope_replay_bayes; `ps-a` is one-hot at the act), which lists the acts its margin cannot
        resolve for the host's confirmation (evaluate_agent.ope_replay, sim.replay_verify).  Opt-in: the configuration key
        `device_replay`.  None — the host loop — without it, without with_ps_all, with a weight function, with a model beyond
        MODEL_BYTES_CAP or one that is not finite."""
        c = self.config
        if not getattr(c, 'with_ps_all', False) or not getattr(c, 'device_replay', False) or self.history is not None:
            return None
        if self.Lambda.size * 8 > MODEL_BYTES_CAP or not np.isfinite(self.Lambda).all():
            return None
        return dict(kind=_abi.RG_POLICY_BAYES_VB, num_products=int(c.num_products), policy_seed=0, bayes_vb=dict(lam=self.Lambda))

    def reset(self):
        self.views = np.zeros((1, self.config.num_products), dtype=np.int16)     # the reference's dense int16 counts
        if getattr(self, 'history', None) is not None:
            self.history.reset()

    def act_on(self, prods, cnts):
        """The action on a history given as (distinct products, counts): the reference's expression on the dense counts."""
        X = np.zeros((1, self.config.num_products), dtype=np.int16)
        X[0, np.asarray(prods, dtype=np.int64)] = np.asarray(cnts)
        return reference_act(X, self.Lambda)[0]

    def act(self, observation, reward, done):
        for session in observation.sessions():
            self.views[0, int(session['v'])] += 1
        if self.history is not None:
            self.history.observe(observation)
            X = self.history.features(observation.context().time()).reshape(1, self.config.num_products)
        else:
            X = self.views
        a = reference_act(X, self.Lambda)[0]
        ps_all = ()
        if getattr(self.config, 'with_ps_all', False):       # bayesian_poly_vb.py:79-83: a one-hot vector over the products
            ps_all = np.zeros(self.config.num_products)
            ps_all[a] = 1.0
        return {**super().act(observation, reward, done), 'a': a, 'ps': 1.0, 'ps-a': ps_all}


class BayesianAgentVB(LogregMulticlassIpsAgent):
    """`train` / `train_from_log` / the model built at the first act: LogregMulticlassIpsAgent's; `build()` is this agent's."""

    def __init__(self, config=Configuration(bayesian_poly_args)):
        super().__init__(config)
        self.q_mu = self.q_Sigma = None

    def ope_policy_checked(self):
        return self._ready().ope_policy_checked()

    def build(self):
        """bayesian_poly_vb.py:93-107."""
        from scipy.stats import multivariate_normal
        feats, actions, deltas, pss = self._training_set()
        c = self.config
        X = np.asarray(feats.todense(), dtype=np.float64) if hasattr(feats, 'todense') else np.asarray(feats, dtype=np.float64)
        N, P = X.shape
        A = np.zeros((N, P), dtype=np.float32)               # to_categorical(actions, P)
        A[np.arange(N), np.asarray(actions, dtype=np.int64)] = 1.0
        XA = (X[:, :, np.newaxis] * A[:, np.newaxis, :]).reshape(N, P * P)        # row n = kron(X[n], A[n])
        y = np.asarray(deltas)
        aa, bb = getattr(c, 'aa', 1.), getattr(c, 'bb', 1.)
        Sigma = np.kron(aa * np.eye(P) + bb, aa * np.eye(P) + bb)
        rng = np.random.RandomState(c.random_seed)
        self.q_mu, self.q_Sigma = bayesian_logistic(XA, y.reshape((N, 1)), mu_beta=-6 * np.ones((P ** 2, 1)), Sigma_beta=Sigma, rng=rng)
        S = int(getattr(c, 'num_samples', 1000))
        Lambda = multivariate_normal.rvs(self.q_mu.reshape(P ** 2), self.q_Sigma, S, random_state=rng)
        self.frozen = BayesianVBFrozenAgent(c, np.asarray(Lambda, dtype=np.float64).reshape(S, P ** 2))
        return self.frozen
