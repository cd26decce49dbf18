"""What the OrganicMFSquare tests share: the fixtures, the observations of the offline protocol rebuilt from a log, the train calls
of a log by a plain Python walk, and a float64 NumPy restatement of one optimiser step (written from the formulas of
include/recogym_hip.h, not from the kernel)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# |float64 restatement - the reference's float32 weights and square averages| from the same pairs, measured over the fixtures by
# tests/make_golden_organic_mf.py (the largest: organic_mf_p40_e8, 3.92e-6); the tests allow 4 times it
MEASURED_F64_VS_REFERENCE = 3.92e-6
TOL_F64_VS_REFERENCE = 4 * MEASURED_F64_VS_REFERENCE
# |rg_omf_steps - the NumPy restatement| on the placed cases of tests/test_organic_mf_device.py, measured on the first GPU run (the
# largest: P = 65, E = 8 in LDS, 3.41e-13); the test allows 4 times it
MEASURED_KERNEL_VS_NUMPY = 3.41e-13
TOL_KERNEL_VS_NUMPY = 4 * MEASURED_KERNEL_VS_NUMPY

ALPHA, EPS = 0.99, 1e-8           # torch.optim.RMSprop's defaults


def fixtures():
    return sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith('organic_mf_') and f.endswith('.npz'))


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


def walk_calls(u, is_b, v, num_organic_users):
    """The sessions of the train calls of a log, by walking it row by row the way the offline protocol produces them: one call
    per organic-only user, one per bandit row of the others; trailing organic rows of such a user are dropped."""
    calls, session, users_seen, prev = [], [], 0, None
    for r in range(len(u)):
        if prev is None or u[r] != prev:
            if prev is not None and users_seen <= num_organic_users:
                calls.append(session)                 # the organic-only user that just ended
            session = []
            users_seen += 1
            prev = u[r]
        if is_b[r]:
            assert users_seen > num_organic_users
            calls.append(session)
            session = []
        else:
            session.append(int(v[r]))
    if prev is not None and users_seen <= num_organic_users:
        calls.append(session)
    return calls


def walk_steps(calls, first_call, mini_batch, pending=()):
    """The reference's train over the calls' sessions -> (the pair list of every optimiser step, the pairs left pending)."""
    steps, stored, k = [], list(pending), first_call
    for session in calls:
        k += 1
        if k % mini_batch == 0:
            steps.append(stored)
            stored = []
        else:
            stored = stored + list(zip(session[:-1], session[1:]))
    return steps, stored


def observations(u, t, is_b, v, a, c, num_organic_users):
    """(observation, action, reward, done) of every train call, as recogym_amd's offline protocol hands them to agent.train."""
    from recogym_amd.envs.context import DefaultContext
    from recogym_amd.envs.observation import Observation
    from recogym_amd.envs.session import OrganicSessions
    out, sessions, users_seen, prev, last_ctx = [], OrganicSessions(), 0, None, None
    n = len(u)
    for r in range(n):
        if prev is None or u[r] != prev:
            if prev is not None and users_seen <= num_organic_users:
                out.append((Observation(last_ctx, sessions), None, None, True))
            sessions = OrganicSessions()
            users_seen += 1
            prev = u[r]
        last_ctx = DefaultContext(t[r], int(u[r]))
        if is_b[r]:
            done = r + 1 == n or u[r + 1] != u[r]
            out.append((Observation(last_ctx, sessions), {'t': t[r], 'u': int(u[r]), 'a': int(a[r]), 'ps': 1.0, 'ps-a': ()}, int(c[r]), done))
            sessions = OrganicSessions()
        else:
            sessions.next(last_ctx, int(v[r]))
    if prev is not None and users_seen <= num_organic_users:
        out.append((Observation(last_ctx, sessions), None, None, True))
    return out


class NumpyModel:
    """emb (P, E), w (P, E), bias (P) and RMSprop's three square averages, float64."""

    def __init__(self, emb, w, bias, sq=None):
        self.emb, self.w, self.bias = (np.array(x, dtype=np.float64) for x in (emb, w, bias))
        self.sq = [np.zeros_like(x) for x in (self.emb, self.w, self.bias)] if sq is None else [np.array(x, dtype=np.float64) for x in sq]

    def step(self, pairs, lr, alpha=ALPHA, eps=EPS):
        """One optimiser step over the pairs (i, j): per distinct input i, G[i] = n_i softmax(w emb[i] + bias) - N[i][.];
        g_emb[i] = G[i] w, g_w = sum_i G[i]^T emb[i], g_bias = sum_i G[i]; then RMSprop on every parameter.  No pair: nothing."""
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        if len(pairs) == 0:
            return
        P = len(self.bias)
        g_emb, g_w, g_b = np.zeros_like(self.emb), np.zeros_like(self.w), np.zeros_like(self.bias)
        for i in np.unique(pairs[:, 0]):
            N = np.bincount(pairs[pairs[:, 0] == i, 1], minlength=P).astype(np.float64)
            z = self.w @ self.emb[i] + self.bias
            ex = np.exp(z - z.max())
            G = N.sum() * ex / ex.sum() - N
            g_emb[i] = G @ self.w
            g_w += np.outer(G, self.emb[i])
            g_b += G
        for p, q, g in ((self.emb, self.sq[0], g_emb), (self.w, self.sq[1], g_w), (self.bias, self.sq[2], g_b)):
            q *= alpha
            q += (1.0 - alpha) * g * g
            p -= lr * (g / (np.sqrt(q) + eps))

    def arrays(self):
        return [self.emb, self.w, self.bias] + self.sq

    def table(self):
        return (self.emb @ self.w.T + self.bias[None, :]).argmax(axis=1)
