"""LogregPolyAgent, the likelihood agent — reference: recogym/agents/logreg_poly.py.

A BINARY logistic regression on polynomial features of (view counts, action): the click model P(c = 1 | views, a).  Its act
scores every action and takes `argmax(predict_proba[:, 1])`, `ps = 1` (logreg_poly.py:143-167).

Training (`LogregPolyAgent`): `train` collects rows like the reference's ModelBuilder, `train_from_log` takes a whole log;
`build()` is the reference's recipe (logreg_poly.py:169-194): `train_data_from_log` -> the design matrix of the transform's
"sliding" branch, one row per bandit row [view counts | the action's index at column P + a | counts at columns 2P + aP + p]
(`poly_design_matrix`, array operations) -> sklearn's LogisticRegression(solver, max_iter, random_state), with the `with_ips`
weights and the clipping line that uses `deltas / pss` whatever the numerator is.  The model is built at the first act.

Inference (`LogregPolyFrozenAgent`): two facts of the reference are reproduced, not fixed.

1. The act's feature rows are NOT the training rows' layout.  `SparsePolynomialFeatures.transform` gets one feature row and all P
   actions and lays out `np.kron(data, ones(P))` in slices of n (the number of distinct viewed products) per action, so the cross
   term of action a for the j-th viewed product is weighted by `data[(a n + j) // P]`; and the action block stores the action's
   INDEX as its value.  With w = coef_[0], wf = w[:P], wa = w[P:2P], wk = w[2P:].reshape(P, P), b = intercept_[0], in float64,
   multiply then add, in this order (`poly_decisions`; sklearn's decision_function bit for bit):

       s = 0;  for p viewed, ascending: s += count[p] wf[p];   s += a wa[a]
       for j, p in enumerate(viewed, ascending): s += count_of_viewed[(a n + j) // P] wk[a, p];   z[a] = s + b

2. The action is the first maximum of `expit(z)`, and expit merges distinct decisions: it is exactly 1.0 from z = 36.7368...
   upwards and moves in steps of 2^-53 below that, so among confident decisions the LOWER INDEX wins, not the larger z.  The
   device decides that with the host's table of expit's top steps (`expit_steps`, built with scipy's expit itself) and, below
   the table, with the margin `poly_margin` inside which two decisions MAY round to one expit value; an act with a lower-index
   decision inside that margin is reported as unresolved and recomputed here (`Simulator.poly_verify`; in an off-policy
   replay, `sim.poly_replay_verify`).

`act` on the host is (1), scipy.special.expit, first maximum — the reference's act bit for bit.
"""
import warnings

import numpy as np

from .. import _abi
from ..envs.configuration import Configuration
from .abstract import Agent
from .logreg_ips import LogregMulticlassIpsAgent

# The reference's keys and defaults (its logreg_poly_args), grouped by what reads them.
logreg_poly_args = dict(
    num_products=10,
    random_seed=np.random.randint(2 ** 31 - 1),
    poly_degree=2,                  # kept for the reference's callers; the features are of degree 2 whatever it says
    # the fit: sklearn's LogisticRegression(solver, max_iter, random_state = random_seed)
    solver='lbfgs',
    max_iter=5000,
    # sample weights of the fit.  with_ips = False: none.  True: 1 / ps per bandit row, or click / ps under
    # ips_numerator_is_delta; ips_with_clipping replaces them by min(click / ps, ips_clipping_value)
    with_ips=False,
    ips_numerator_is_delta=False,
    ips_with_clipping=False,
    ips_clipping_value=10,
    with_ps_all=False,              # act() also returns the one-hot `ps-a` vector
)

EXPIT_STEPS = 1024          # steps of expit below 1.0 the table resolves (8 KB: the device keeps it in LDS)
LOG2E = 1.4426950408889634
POLY_FLOOR = -700.0         # a best decision below this is outside the margin's proof: unresolved whenever a lower index exists


def expit_steps(n_steps=EXPIT_STEPS):
    """th[k] = the smallest double z with scipy.special.expit(z) >= 1 - k 2^-53, k = 0 .. n_steps - 1, by bisection on the doubles
    (positive doubles are ordered like their bit patterns) with expit itself.  Asserts at every step that expit(th[k]) meets its
    target and the double below it does not, and that th never increases.  (It is not STRICTLY decreasing: scipy's expit is
    1 / (1 + exp(-z)), whose denominator moves in steps of 2^-52 up here, so it takes every second value only and thresholds
    coincide in pairs — th[1] == th[0]; a step nothing maps to is harmless: the step of a decision is the NUMBER of thresholds
    above it.)  The ONE assumption the table's users make beyond that: expit is monotone (non-decreasing) — then two decisions
    with the same number of thresholds above them have the same expit (doubles in [0.5, 1) are 2^-53 apart, and both values lie
    in [1 - k 2^-53, 1 - (k - 1) 2^-53)), two with different numbers have different ones, every z >= th[0] has 1.0 and every
    z < th[n_steps - 1] something smaller than all of those."""
    from scipy.special import expit
    k = np.arange(n_steps, dtype=np.float64)
    target = 1.0 - k * 2.0 ** -53                               # exact
    lo = np.full(n_steps, np.float64(20.0)).view(np.int64)      # expit(20) = 1 - 2e-9: below every target
    hi = np.full(n_steps, np.float64(40.0)).view(np.int64)      # expit(40) = 1.0
    assert (expit(lo.view(np.float64)) < target).all() and (expit(hi.view(np.float64)) >= target).all()
    while (hi - lo > 1).any():
        mid = lo + (hi - lo) // 2
        ge = expit(mid.view(np.float64)) >= target
        hi = np.where(ge, mid, hi)
        lo = np.where(ge, lo, mid)
    th = hi.view(np.float64).copy()
    assert (expit(th) >= target).all() and (expit(np.nextafter(th, -np.inf)) < target).all()
    assert (np.diff(th) <= 0).all() and th[-1] < th[0], 'the thresholds must not increase'
    return th


def poly_margin(z):
    """W(z*) = 2^-49 (1 + 2^m), m = ceil(z* log2 e) + 1: an upper bound of 8 2^-52 (1 + exp(z*)) made of IEEE operations only (the
    device computes the same bits).  Two decisions further apart than W have distinct expit values."""
    m = np.ceil(np.float64(z) * LOG2E) + 1.0
    m = min(max(m, -1100.0), 1023.0) if m == m else -1100.0
    return np.float64(2.0 ** -49) * (np.float64(1.0) + np.ldexp(np.float64(1.0), int(m)))


def poly_split(coef, intercept, num_products):
    """sklearn's coef_ (1, 2P + P^2) / intercept_ (1,) -> (wf, wa, wk (P, P) [action][viewed product], b)."""
    P = int(num_products)
    w = np.asarray(coef, dtype=np.float64).reshape(-1)
    assert w.shape == (2 * P + P * P,), (w.shape, P)
    b = float(np.asarray(intercept, dtype=np.float64).reshape(-1)[0])
    return (np.ascontiguousarray(w[:P]), np.ascontiguousarray(w[P:2 * P]), np.ascontiguousarray(w[2 * P:].reshape(P, P)), b)


def poly_decisions(prods, cnts, wf, wa, wk, b):
    """The P decisions of one act: `prods` the distinct viewed products ascending, `cnts` their values (view counts, or the weighted
    float features), in the contract's order (module docstring, 1)."""
    P = len(wf)
    prods = np.asarray(prods, dtype=np.int64)
    cnts = np.asarray(cnts, dtype=np.float64)
    n = len(prods)
    s = np.float64(0.0)
    for p, c in zip(prods, cnts):
        s = s + c * wf[p]
    a = np.arange(P, dtype=np.int64)
    z = s + a.astype(np.float64) * wa
    for j, p in enumerate(prods):
        z = z + cnts[(a * n + j) // P] * wk[:, p]
    return z + np.float64(b)


def poly_rule(z, th):
    """The device's decision on the decisions z (numpy restatement of k_poly_acts) -> (action, flags): bit 0 decided on the step
    table, bit 1 unresolved, bit 2 a lower index than the first maximal decision won."""
    K = len(th)
    steps = K - np.searchsorted(th[::-1], z, side='right')      # thresholds above z
    a_star = int(np.argmax(z))
    smin = int(steps.min())
    if smin < K:
        a = int(np.argmax(steps == smin))
        return a, 1 | (4 if a != a_star else 0)
    if z[a_star] < POLY_FLOOR:                                  # expit is subnormal or 0 down here: outside W's proof
        return a_star, (2 if a_star > 0 else 0)
    g = z[a_star] - z[:a_star]
    return a_star, (2 if bool(np.any((g > 0.0) & (g <= poly_margin(z[a_star])))) else 0)


def poly_design_matrix(features, actions, num_products):
    """The training design matrix — the "sliding" branch of the reference's transform (logreg_poly.py:30-119: every sample's own
    feature row and action): CSR (n, 2P + P^2) float64 with sorted indices, row i = [features[i] | i's action index stored at
    column P + a_i (an explicit 0 for action 0) | features[i] again at columns 2P + a_i P + p]."""
    from scipy import sparse
    P = int(num_products)
    feats = sparse.csr_matrix(features)
    feats.sort_indices()
    actions = np.asarray(actions, dtype=np.int64)
    n = len(actions)
    assert feats.shape == (n, P)
    lens = np.diff(feats.indptr).astype(np.int64)
    indptr = np.concatenate([[0], np.cumsum(2 * lens + 1)]).astype(np.int64)
    row = np.repeat(np.arange(n, dtype=np.int64), lens)
    within = np.arange(feats.nnz, dtype=np.int64) - np.repeat(feats.indptr[:-1].astype(np.int64), lens)
    pos_f = indptr[:-1][row] + within
    pos_a = indptr[:-1] + lens
    pos_k = pos_f + lens[row] + 1
    indices = np.empty(indptr[-1], dtype=np.int64)
    data = np.empty(indptr[-1], dtype=np.float64)
    idx = feats.indices.astype(np.int64)
    indices[pos_f] = idx
    data[pos_f] = feats.data
    indices[pos_a] = P + actions
    data[pos_a] = actions
    indices[pos_k] = 2 * P + actions[row] * P + idx
    data[pos_k] = feats.data
    return sparse.csr_matrix((data, indices, indptr), shape=(n, 2 * P + P * P))


class LogregPolyFrozenAgent(Agent):
    def __init__(self, config, coef, intercept):
        """coef (1, 2P + P^2) / intercept (1,) as sklearn stores the fitted binary model."""
        super().__init__(config)
        self.wf, self.wa, self.wk, self.b = poly_split(coef, intercept, config.num_products)
        # weight_history_function (ViewsFeaturesProvider with history): time-weighted float features instead of view counts.  On the
        # host path unless `device_weight_history` is set AND the function stands for a table over the int16 clock differences
        # (views_history.weight_table)
        self.history = None
        self.weight_history = None
        if getattr(config, 'weight_history_function', None) is not None:
            from .views_history import ViewsHistory, weight_table
            self.history = ViewsHistory(config.num_products, config.weight_history_function, is_sparse=True)
            if getattr(config, 'device_weight_history', False):
                tabled = weight_table(config.weight_history_function)
                if tabled is not None:
                    self.weight_history = dict(table=tabled[0], f32=tabled[1])
        self.reset()

    @classmethod
    def from_sklearn(cls, config, logreg):
        return cls(config, logreg.coef_, logreg.intercept_)

    def device_policy(self):
        if getattr(self.config, 'with_ps_all', False) or (self.history is not None and self.weight_history is None):
            return None
        model = dict(wf=self.wf, wa=self.wa, wk=self.wk, intercept=self.b)
        if self.weight_history is not None:
            model['weight_history'] = self.weight_history
        return dict(policy=_abi.RG_POLICY_LOGREG_POLY, policy_seed=0, ouc=None, logreg_poly=model)

    def ope_policy(self):
        """None: `ope_policy` is the hook of replay forms that are exact without a host step; this agent's is `ope_policy_checked`."""
        return None

    def ope_policy_checked(self):
        """The replay form of rg_ope_replay_poly, or None where only the host loop is exact (no `ps-a` without with_ps_all; the
        time-weighted features of a weight_history_function that has no device form).  With `device_weight_history` and a function
        that stands for a table the dict's `logreg_poly` carries `weight_history` (table, f32), the form of rg_ope_replay_poly_w.
        "Checked": the device lists the acts its rule cannot resolve and the caller confirms them on the host
        (sim.poly_replay_verify, sim.weighted_replay_verify) before it lets the result stand."""
        if not getattr(self.config, 'with_ps_all', False) or (self.history is not None and self.weight_history is None):
            return None
        model = dict(wf=self.wf, wa=self.wa, wk=self.wk, intercept=self.b)
        if self.weight_history is not None:
            model['weight_history'] = self.weight_history
        return dict(kind=_abi.RG_POLICY_LOGREG_POLY, num_products=int(self.config.num_products), policy_seed=0, logreg_poly=model)

    def reset(self):
        self.views = np.zeros(self.config.num_products, dtype=np.int64)
        if getattr(self, 'history', None) is not None:
            self.history.reset()

    def decisions(self, prods, cnts):
        return poly_decisions(prods, cnts, self.wf, self.wa, self.wk, self.b)

    def act_on(self, prods, cnts):
        """The action on a history: expit of the decisions, first maximum."""
        from scipy.special import expit
        return int(np.argmax(expit(self.decisions(prods, cnts))))

    def act(self, observation, reward, done):
        for session in observation.sessions():
            self.views[int(session['v'])] += 1
        if self.history is not None:
            self.history.observe(observation)
            f = self.history.features(observation.context().time()).tocsr()
            f.sort_indices()
            prods, cnts = f.indices, f.data.astype(np.float64)
        else:
            prods = np.flatnonzero(self.views)
            cnts = self.views[prods]
        a = self.act_on(prods, cnts)
        ps_all = ()
        if getattr(self.config, 'with_ps_all', False):       # logreg_poly.py:155-159: a one-hot vector over the products
            ps_all = np.zeros(self.config.num_products)
            ps_all[a] = 1.0
        return {**super().act(observation, reward, done), 'a': a, 'ps': 1.0, 'ps-a': ps_all}


class LogregPolyAgent(LogregMulticlassIpsAgent):
    """`train` / `train_from_log` / the model built at the first act: LogregMulticlassIpsAgent's; `build()` is this agent's."""

    def __init__(self, config=Configuration(logreg_poly_args)):
        super().__init__(config)

    def ope_policy_checked(self):
        return self._ready().ope_policy_checked()

    @property
    def accepts_device_log(self):
        """test_agent hands Simulator.device_log() to train_from_log exactly when the training features can be built where the log
        lies: `device_weight_history` is set and the weight function stands for a table (feature_feed.weighted_train_data_device)."""
        c = self.config
        if not getattr(c, 'device_weight_history', False) or getattr(c, 'weight_history_function', None) is None:
            return False
        from .views_history import weight_table
        return weight_table(c.weight_history_function) is not None

    def _sample_weights(self, clicks, pss):
        """The fit's sample weights, or None without with_ips.  As in the reference, clipping takes click / ps as the weight to
        clip even where the unclipped weight would be 1 / ps."""
        c = self.config
        if not getattr(c, 'with_ips', False):
            return None
        if getattr(c, 'ips_with_clipping', False):
            return np.minimum(clicks / pss, c.ips_clipping_value)
        return clicks / pss if getattr(c, 'ips_numerator_is_delta', False) else 1.0 / pss

    def build(self):
        """logreg_poly.py:169-194 (n_jobs = -1 does not affect the fit and is left out)."""
        from sklearn.linear_model import LogisticRegression
        feats, actions, deltas, pss = self._training_set()
        c = self.config
        X = poly_design_matrix(feats, actions, c.num_products)
        model = LogisticRegression(solver=getattr(c, 'solver', 'lbfgs'), max_iter=getattr(c, 'max_iter', 5000),
                                   random_state=c.random_seed)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            self.logreg = model.fit(X, deltas, self._sample_weights(deltas, pss))
        self.frozen = LogregPolyFrozenAgent.from_sklearn(c, self.logreg)
        return self.frozen
