"""Time-weighted view features — the `weight_history_function` option of the reference's ViewsFeaturesProvider
(recogym/agents/abstract.py:318-409) and of AbstractFeatureProvider.train_data (abstract.py:190-279).

With `config.weight_history_function = w` a user's feature vector at time T is not the count of views per product but
`sum over the user's earlier views of w(T - t_view)` per product.  The reference builds it from scipy sparse pieces — a
(views x P) int16 one-hot matrix, `.multiply(weights[:, None])`, `.sum(axis=0, dtype=float32)` — with the product ids and the
times cast to np.int16 on the way (wrapping beyond 32 767 like the reference).  The features feed a float division and a
cumulative sum whose last bits decide sampled actions, so this module makes the SAME scipy / numpy calls on the same dtypes
instead of re-deriving the arithmetic: bit-identical by construction (pinned on fixtures of the unmodified reference).

Agents with a weight function report no device policy and `generate_logs` walks them one user at a time — but the likelihood
agent with `device_weight_history`: `weight_table` turns the function into a table over the int16 clock differences, `weighted_list`
states the rule the device holds to on that table, and the agent's acts run in the device loop.
"""
import numpy as np
from scipy import sparse


def weighted_views(products, times, now, weight_fn, num_products):
    """1 x P float32 np.matrix: the reference's `weighted_views.sum(axis=0, dtype=np.float32)` for the views (products, times)
    seen at time `now` (all three in the reference's int16)."""
    n = len(products)
    ixs = [np.int16(i) for i in range(n)]
    views = sparse.coo_matrix((np.ones(n, dtype=np.int16), (ixs, list(products))), shape=(n, num_products), dtype=np.int16)
    weights = weight_fn(np.int16(now) - np.array(list(times)))
    return views.multiply(weights[:, np.newaxis]).sum(axis=0, dtype=np.float32)


class ViewsHistory:
    """The with-history state of a ViewsFeaturesProvider: observe() the organic sessions, features(now) -> what the
    reference's `features(observation)` returns (a coo_matrix when is_sparse, else a dense (1, P) array)."""

    def __init__(self, num_products, weight_fn, is_sparse=False):
        self.num_products = int(num_products)
        self.weight_fn = weight_fn
        self.is_sparse = is_sparse
        self.reset()

    def reset(self):
        self.products = []
        self.times = []

    def observe(self, observation):
        for session in observation.sessions():
            self.products.append(np.int16(session['v']))
            self.times.append(np.int16(session['t']))

    def features(self, now):
        views = sparse.coo_matrix(weighted_views(self.products, self.times, now, self.weight_fn, self.num_products), copy=False)
        return views if self.is_sparse else np.array(views.todense())


WEIGHT_TABLE_LEN = 32768       # differences of two int16 clock values in [0, 32767]

# sub-arrays of arange(WEIGHT_TABLE_LEN) a weight function is evaluated on again to prove it elementwise: contiguous slices, single
# elements (the reference passes one-element arrays for a one-view history), a reversed slice
_PROBES = (slice(0, 1), slice(5, 6), slice(87, 88), slice(32767, 32768), slice(0, 100), slice(100, 2000), slice(30000, 32768),
           slice(200, 50, -1))


def weight_table(fn):
    """The weight function as a table over the int16 differences 0 .. 32767 -> (table, is_f32), or None where no table can stand
    for it.  The reference casts every time to np.int16 before `fn` sees it, so inside the clock range [0, 32767] `fn` is only ever
    evaluated on arrays of such differences: `table = fn(np.arange(32768, dtype=np.int16))`.  Accepted: a float32 or float64
    ndarray of that shape with finite values that `fn` reproduces bit for bit, dtype included, on each of `_PROBES` — a function
    that is not elementwise (`t / t.sum()`), returns a scalar, or raises gives None, and its agent keeps the host path."""
    arg = np.arange(WEIGHT_TABLE_LEN, dtype=np.int16)
    try:
        with np.errstate(all='ignore'):
            table = fn(arg.copy())
            if not isinstance(table, np.ndarray) or table.shape != arg.shape or table.dtype not in (np.float32, np.float64):
                return None
            if not np.isfinite(table).all():
                return None
            bits = table.view(np.uint32 if table.dtype == np.float32 else np.uint64)
            for s in _PROBES:
                part = fn(arg[s].copy())
                if not isinstance(part, np.ndarray) or part.dtype != table.dtype or part.shape != bits[s].shape:
                    return None
                if not np.array_equal(part.view(bits.dtype), bits[s]):
                    return None
    except Exception:
        return None
    return np.ascontiguousarray(table), bool(table.dtype == np.float32)


def weighted_list(products, times, now, table, is_f32):
    """`weighted_views` as a rule on the table of `weight_table` -> (products ascending, float32 values) of the products whose
    feature is not 0: a product's feature is the SEQUENTIAL sum, in view order and in the table's dtype, of table[now - t] over
    its views, rounded once to float32 (what scipy's multiply / sum(axis=0, dtype=float32) computes).  Every clock value must lie
    in [0, 32767] and no view after `now` (ValueError otherwise: outside that range the reference's int16 cast wraps, which this
    rule does not restate)."""
    dt = np.float32 if is_f32 else np.float64
    assert table.dtype == dt and table.shape == (WEIGHT_TABLE_LEN,)
    prods = np.asarray(products, dtype=np.int64).reshape(-1)
    t = np.asarray(times, dtype=np.int64).reshape(-1)
    now = int(now)
    if not 0 <= now < WEIGHT_TABLE_LEN or (len(t) and (t.min() < 0 or t.max() > now)):
        raise ValueError('a clock value outside [0, 32767], or a view after the act')
    w = table[now - t]
    out_p, out_v = [], []
    for p in np.unique(prods):
        with np.errstate(all='ignore'):
            v = np.float32(np.cumsum(w[prods == p], dtype=dt)[-1])       # cumsum adds one element at a time, in order
        if v != 0:
            out_p.append(p)
            out_v.append(v)
    return np.asarray(out_p, dtype=np.int64), np.asarray(out_v, dtype=np.float32)


def train_data_weighted(log_columns, num_products, weight_fn, is_sparse=True):
    """AbstractFeatureProvider.train_data with a weight function: one weighted feature row per bandit row, built from the views
    of the row's user before it (abstract.py:216-263).  `log_columns` = (t, u, is_bandit, v, a, c, ps) plain arrays in the
    reference's row order.  O(bandit rows x views of the user): the exact form, for the sizes a weighted model is trained on."""
    t, u, is_b, v, a, c, ps = log_columns
    feats, actions, deltas, pss = [], [], [], []
    cur = None
    products, times = [], []
    for i in range(len(u)):
        if u[i] != cur:
            cur, products, times = u[i], [], []
        if not is_b[i]:
            products.append(np.int16(v[i]))
            times.append(np.int16(t[i]))
            continue
        feats.append(sparse.coo_matrix(weighted_views(products, times, np.int16(t[i]), weight_fn, num_products), copy=False))
        actions.append(np.int16(a[i]))
        deltas.append(np.int16(c[i]))
        pss.append(ps[i])
    out = sparse.vstack(feats, format='csr')
    return ((out if is_sparse else np.array(out.todense(), dtype=float)), np.array(actions, dtype=np.int16), np.array(deltas),
            np.array(pss))
