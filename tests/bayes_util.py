"""Shared by the BayesianAgentVB fixtures' generator and tests: a fixture's model, and the device rule's census over a log."""
import numpy as np

import golden_util as gu
from recogym_amd.agents.bayesian_poly_vb import SATURATED, UNRESOLVED, ZSAT, bayes_abs_sum, bayes_decisions, bayes_rule, bayes_transpose

FIXTURES = ['bayes_p4', 'bayes_p10_s120', 'bayes_p10_s120_sigma0', 'bayes_p4_shifted']


def fixture_lambda(meta, cols):
    """The fixture's posterior draws (S, P^2): its own array, or the one of the fixture it names (plus the constant the generator
    added inside the reference's model object, where it names one)."""
    if 'bayes_lambda' in cols:
        return cols['bayes_lambda']
    lam = gu.load(meta['lambda_from'])[1]['bayes_lambda']
    return lam + meta['lambda_shift'] if meta.get('lambda_shift') is not None else lam


def rule_census(cols, P, Lambda):
    """bayes_rule on bayes_decisions for every act of a log (one act per change of a user's view history that a bandit row needed)
    -> dict(acts, saturated, unresolved, lower_wins, max_z); asserts the logged action on every bandit row a resolved act serves.  lower_wins: saturated
    acts whose action is not the one with the largest decisions (the lowest saturated index won, as in the reference)."""
    lam_t = bayes_transpose(Lambda, P)
    out = dict(acts=0, saturated=0, unresolved=0, lower_wins=0, max_z=-np.inf)
    u, z, v, a = cols['u'], cols['z'], cols['v'], cols['a']
    for lo in np.flatnonzero(np.r_[True, u[1:] != u[:-1]]):
        views = np.zeros(P, dtype=np.int64)
        act = None
        i = lo
        while i < len(u) and u[i] == u[lo]:
            if z[i] == 0:
                views[v[i]] += 1
                act = None
            else:
                if act is None:
                    prods = np.flatnonzero(views)
                    dec = bayes_decisions(prods, views[prods], lam_t)
                    act = bayes_rule(dec, len(prods), bayes_abs_sum(prods, views[prods], lam_t))
                    out['acts'] += 1
                    out['saturated'] += act[1] & SATURATED
                    out['unresolved'] += (act[1] & UNRESOLVED) >> 1
                    out['lower_wins'] += int(bool(act[1] & SATURATED) and act[0] != int(np.argmax(dec.mean(axis=1))))
                    out['max_z'] = max(out['max_z'], float(dec.max()))
                assert act[1] & UNRESOLVED or act[0] == a[i], (int(u[i]), i, act, int(a[i]))       # a resolved act is the reference's
            i += 1
    return out


def placed(P):
    """(name, z vector (S = 1), expected action, expected flags): with a one-view history (count 1) z[a] = lam_t[p][a][0] exactly."""
    lo, hi = (0, 1) if P == 2 else (P // 3, P - 1)

    def vec(z_lo, z_hi, base=-3.0):
        z = np.full(P, base)
        z[lo], z[hi] = z_lo, z_hi
        return z
    last = np.full(P, -1.0)
    last[P - 1] = 7.0
    cases = [
        ('adjacent doubles', vec(1.0, np.nextafter(1.0, 2.0)), None, UNRESOLVED),
        ('2^-20 apart, larger at the higher index', vec(1.0, 1.0 + 2.0 ** -20), hi, 0),
        ('2^-20 apart, larger at the lower index', vec(1.0 + 2.0 ** -20, 1.0), lo, 0),
        ('exact tie', vec(3.25, 3.25), lo, UNRESOLVED),
        ('two saturated actions', vec(45.0, 45.0), lo, SATURATED),
        ('saturated pair, larger z at the higher index', vec(41.0, 90.0), lo, SATURATED),
        ('expit(39) is 1.0 but 39 is below ZSAT', vec(39.0, 45.0), hi, SATURATED | UNRESOLVED),
        ('exactly ZSAT', vec(ZSAT, 20.0), lo, SATURATED),
        ('one double below ZSAT: the ordinary zone', vec(np.nextafter(ZSAT, 0.0), 20.0), lo, 0),
        ('below ZSAT, two means of exactly 1.0', vec(39.0, 38.0), lo, UNRESOLVED),
        ('the maximum in the last action', last, P - 1, 0),
        ('negative decisions', vec(-700.0, -699.0, base=-745.0), None, UNRESOLVED),
    ]
    last_lane = max((a for a in range(P) if a % 64 == 63), default=None)
    if last_lane is not None:
        lane63 = np.full(P, -1.0)
        lane63[last_lane] = 7.0
        cases.append(('the maximum in action 64 k + 63', lane63, last_lane, 0))
    return cases
