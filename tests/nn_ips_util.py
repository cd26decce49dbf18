"""Shared by the NnIpsAgent fixtures' generator and tests: a fixture's net, and the device rule over every act of a log."""
import numpy as np

import golden_util as gu
from recogym_amd.agents.nn_ips import UNRESOLVED, NnModel, nn_forward, nn_ps_bound, nn_rule

FIXTURES = ['nn_ips_p10', 'nn_ips_p10_sigma0', 'nn_ips_p40', 'nn_ips_p10_loaded', 'nn_ips_p40_loaded']
KEYS = ('w1', 'b1', 'w2', 'b2', 'w3', 'b3')


def fixture_state(meta, cols):
    """The fixture's six float32 arrays: its own, or those of the fixture it names."""
    if 'nn_w1' not in cols:
        cols = gu.load(meta['weights_from'])[1]
    return {k: cols['nn_' + k] for k in KEYS}


def acts_of_log(cols, P):
    """One act per change of a user's view history that a bandit row needed -> list of (rows served, products, counts)."""
    out = []
    u, z, v = cols['u'], cols['z'], cols['v']
    for lo in np.flatnonzero(np.r_[True, u[1:] != u[:-1]]):
        views = np.zeros(P, dtype=np.int64)
        cur = None
        i = lo
        while i < len(u) and u[i] == u[lo]:
            if z[i] == 0:
                views[v[i]] += 1
                cur = None
            else:
                if cur is None:
                    prods = np.flatnonzero(views)
                    cur = ([], prods, views[prods].copy())
                    out.append(cur)
                cur[0].append(i)
            i += 1
    return out


def rule_over_log(cols, P, state):
    """nn_rule on every act of a log -> list of dict(rows, user, t, t_lockstep, action, flags, ps, bound): `bound` is nn_ps_bound of
    the act, (user, t) the entry the device lists for an unresolved act in run-ahead rounds (the event index of the last organic row
    before the act: a round lists the user at that event), (user, t_lockstep) the entry of a run with an event per launch — DESIGN.md
    4f: "an organic user is listed at the event that completes the history, a bandit user at the act's own event": the same index
    where the act serves nothing but the trailing row of a user that stops from the organic state, one more (the act's first bandit
    row) everywhere else."""
    m = NnModel(state)
    first, last = {}, {}
    for i, uu in enumerate(cols['u']):
        first.setdefault(int(uu), i)
        last[int(uu)] = i
    out = []
    for rows, prods, cnts in acts_of_log(cols, P):
        action, flags, z, ps = nn_rule(prods, cnts, m)
        M1 = nn_forward(prods, cnts, m)[3]
        user = int(cols['u'][rows[0]])
        t = rows[0] - first[user] - 1
        out.append(dict(rows=rows, user=user, t=t, t_lockstep=t if rows == [last[user]] else t + 1, action=action, flags=flags, ps=float(ps),
                        bound=nn_ps_bound(len(prods), M1, m.H, m.A2, m.A3, P)))
    return out


def check_log_against_rule(cols, P, state, what=''):
    """Every resolved act of the rule has the log's action, and the restated ps lies within nn_ps_bound of the log's on every row
    whose action the rule shares -> (acts, unresolved, distinct actions of the log)."""
    acts = rule_over_log(cols, P, state)
    for act in acts:
        for i in act['rows']:
            if not act['flags'] & UNRESOLVED:
                assert act['action'] == cols['a'][i], (what, act['user'], i, act['action'], int(cols['a'][i]))
            if act['action'] == cols['a'][i]:
                assert abs(act['ps'] / cols['ps'][i] - 1.0) <= act['bound'], (what, act['user'], i, act['ps'], cols['ps'][i], act['bound'])
    return acts, sum(1 for a in acts if a['flags'] & UNRESOLVED), len(set(cols['a'][cols['z'] == 1].tolist()))
