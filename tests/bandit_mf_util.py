"""What the BanditMFSquare device-training tests share: the fixtures, the train calls of a log by a plain Python walk, and a float64
NumPy restatement of one optimiser step (written from the formulas of include/recogym_hip.h, not from the kernel)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# |float64 restatement - the reference's float32 embeddings and square averages| from the same triples, measured over the fixtures
# by tests/make_golden_bandit_mf.py (the largest: bandit_mf_dev_p40_e8, 1.539e-6); the tests allow 4 times it
MEASURED_F64_VS_REFERENCE = 1.54e-6
TOL_F64_VS_REFERENCE = 4 * MEASURED_F64_VS_REFERENCE
# |rg_bmf_steps - the NumPy restatement| on the placed cases of tests/test_bandit_mf_device.py, measured on the first GPU run
# (the largest: P=10 E=5 scale=8.0 global, 8.882e-16); the test allows 4 times it
MEASURED_KERNEL_VS_NUMPY = 8.89e-16
TOL_KERNEL_VS_NUMPY = 4 * MEASURED_KERNEL_VS_NUMPY

ALPHA, EPS = 0.99, 1e-8           # torch.optim.RMSprop's defaults
KEYS = ('ep', 'eu', 'sq_ep', 'sq_eu')


def fixtures():
    return sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith('bandit_mf_dev_') and f.endswith('.npz'))


def load(name):
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    meta = json.loads(str(z['meta']))
    return meta, {k: z[k] for k in z.files if k != 'meta'}


def log_columns(cols, prefix='log_'):
    """A fixture's log as the dict Simulator.log_columns() gives."""
    is_b = cols[prefix + 'z'] == 1
    return dict(t=cols[prefix + 't'].astype(np.float32), u=cols[prefix + 'u'].astype(np.int32), is_bandit=is_b,
                v=np.where(is_b, 0, cols[prefix + 'v']).astype(np.int32), a=np.where(is_b, cols[prefix + 'a'], 0).astype(np.int32),
                c=np.where(is_b, cols[prefix + 'c'], np.nan).astype(np.float32),
                ps=np.where(is_b, cols[prefix + 'ps'], np.nan).astype(np.float64))


def walk_calls(u, is_b, v, a, c, num_organic_users):
    """The train calls of a log, by walking it row by row the way the offline protocol produces them: one call per organic-only
    user (no action), one per bandit row of the others -> [(the session's views, action or None, reward or None)]."""
    calls, session, users_seen, prev = [], [], 0, None
    for r in range(len(u)):
        if prev is None or u[r] != prev:
            if prev is not None and users_seen <= num_organic_users:
                calls.append((session, None, None))       # the organic-only user that just ended
            session = []
            users_seen += 1
            prev = u[r]
        if is_b[r]:
            assert users_seen > num_organic_users
            calls.append((session, int(a[r]), int(c[r])))
            session = []
        else:
            session.append(int(v[r]))
    if prev is not None and users_seen <= num_organic_users:
        calls.append((session, None, None))
    return calls


def walk_steps(calls, first_call, mini_batch, pending=(), last_view=None):
    """The reference's train over the calls -> (the triple list of every optimiser step, the triples left pending, the last
    product viewed)."""
    steps, stored, k = [], [tuple(t) for t in pending], first_call
    for session, action, reward in calls:
        if session:
            last_view = session[-1]
        k += 1
        if k % mini_batch == 0:
            steps.append(stored)
            stored = []
        elif action is not None:
            stored = stored + [(last_view, action, reward)]
    return steps, stored, last_view


def walk_triples(calls, first_call, mini_batch, pending=()):
    """walk_steps in log_triples' form -> (triples (n, 3), step_offsets (n_steps + 2), n_calls, last_view or -1)."""
    steps, stored, last_view = walk_steps(calls, first_call, mini_batch, pending)
    rows = steps + [stored]
    flat = np.asarray([t for s in rows for t in s], dtype=np.int32).reshape(-1, 3)
    off = np.cumsum([0] + [len(s) for s in rows]).astype(np.int64)
    return flat, off, len(calls), -1 if last_view is None else last_view


def synthetic_log(seed, n_users, n_org, P, long_users=()):
    """Users of random lengths that open with an organic row; `long_users`: (user, rows) with rows > 64, among them runs of more than
    64 bandit rows (the fill has to carry a view over a whole chunk) and trailing organic rows (views that belong to no call)."""
    r = np.random.RandomState(seed)
    u, is_b = [], []
    long_users = dict(long_users)
    for user in range(n_users):
        n = long_users.get(user, int(r.randint(1, 30)))
        b = r.rand(n) < 0.6
        if user in long_users:
            b[5:5 + (195 if n >= 300 else 70)] = True          # the next chunk opens without a view of its own; at 300 rows two chunks have none
            b[n - 3:] = False
        b[0] = False
        if user < n_org:
            b[:] = False
        u += [user + 3] * n
        is_b += b.tolist()
    u, is_b = np.asarray(u, dtype=np.int64), np.asarray(is_b, dtype=bool)
    idx = r.randint(0, P, size=len(u))
    return dict(u=u, is_bandit=is_b, v=np.where(is_b, 0, idx), a=np.where(is_b, idx, 0), c=np.where(is_b, (r.rand(len(u)) < 0.3).astype(np.float64), np.nan))


class NumpyModel:
    """Ep (P, E), Eu (P, E) and RMSprop's two square averages, float64."""

    def __init__(self, ep, eu, sq=None):
        self.ep, self.eu = (np.array(x, dtype=np.float64) for x in (ep, eu))
        self.sq = [np.zeros_like(x) for x in (self.ep, self.eu)] if sq is None else [np.array(x, dtype=np.float64) for x in sq]

    def step(self, triples, lr, alpha=ALPHA, eps=EPS):
        """One optimiser step over the triples (l, a, r): z_s = <Ep[a_s], Eu[l_s]>, d_s = (sigmoid(z_s) - r_s) / n
        (from exp(-|z|), sigmoid(z) - 1 taken as -sigmoid(-z): nothing overflows, nothing cancels),
        g_Ep[a] = sum_{a_s = a} d_s Eu[l_s], g_Eu[l] = sum_{l_s = l} d_s Ep[a_s]; then RMSprop on every parameter.  No triple:
        nothing."""
        t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
        n = len(t)
        if n == 0:
            return
        l, a, r = t[:, 0], t[:, 1], t[:, 2].astype(np.float64)
        z = np.einsum('se,se->s', self.ep[a], self.eu[l])
        x = np.exp(-np.abs(z))
        mag = np.where((z >= 0) != (r != 0), 1.0, x) / (1.0 + x)          # sigmoid(z) for r = 0, sigmoid(-z) = 1 - sigmoid(z) for r = 1
        d = np.where(r != 0, -mag, mag) / n
        g_ep, g_eu = np.zeros_like(self.ep), np.zeros_like(self.eu)
        np.add.at(g_ep, a, d[:, None] * self.eu[l])
        np.add.at(g_eu, l, d[:, None] * self.ep[a])
        for p, q, g in ((self.ep, self.sq[0], g_ep), (self.eu, self.sq[1], g_eu)):
            q *= alpha
            q += (1.0 - alpha) * g * g
            p -= lr * (g / (np.sqrt(q) + eps))

    def arrays(self):
        return [self.ep, self.eu] + self.sq

    def logits(self):
        """[last view][action]"""
        return self.eu @ self.ep.T

    def table(self):
        return self.logits().argmax(axis=1)
