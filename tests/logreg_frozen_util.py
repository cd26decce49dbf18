"""The frozen multinomial LogReg act (RG_POLICY_LOGREG_FROZEN) on histories a test places itself: the float64 reference, a second
decision in exact rational arithmetic, NumPy emulations of the two screens (they CLASSIFY a case, they never supply an expected
value), and the builders of tests/test_logreg_frozen_device.py.  Plain NumPy, no GPU.

The device act (recogym_amd/csrc/rg_advance.hip): k_logreg_screen scores every class from an fp16 copy of coef^T in K_SPLIT class
ranges of range_len(C) classes, lanes of 8 consecutive classes, batches of 512; k_logreg_decide takes the classes within
thr = 2 B16 of the maximum, at most K_CAND per range, into float64 in scipy's order; a range with more (or more than CAND_CAP while
it streams) sends the act to the float64 walk over all classes.  k_logreg_acts is the fp32 form with the band 2 (nd + 3) 2^-24 Ahat.

Every builder shares one layout.  A model has `bg` history products (0 and P - 1 among them) and `trig` trigger products.  A GROUP
of classes carries the shared column u (0.5 .. 1) on the bg rows, +1 on its own trigger and -1 on every other trigger; every other
class is <= 0 everywhere.  A user views exactly one trigger (count n_q) and nd - 1 bg products, so its contest is among the
members of ONE group: they lead every other group by 2 n_q and every other class by more, and n_q is sized against the band."""
import functools
from collections import namedtuple
from fractions import Fraction

import numpy as np

K_SPLIT, K_CAND, CAND_CAP, BATCH = 8, 8, 64, 512
NDS = (1, 2, 7, 8, 9, 11, 12, 13, 16, 33)      # the first eight rows leave in one round trip, the rest four at a time
HIST_ENTRIES = 255                              # the default capacity of a view history (kDefaultHistoryCap - 1)
# (both are float32 values: the fp16 copy is the same whether a conversion rounds float64 once or through float32)
W_A = 1.0 + 2.0 ** -11 - 2.0 ** -23             # fp16 copy 1.0 (just below the tie)
W_B = 1.0 + 2.0 ** -11 + 2.0 ** -23             # fp16 copy 1 + 2^-10 (just above it)
W_BONUS = 2.0 ** -25 * (1.0 - 2.0 ** -20)       # fp16 copy 0 (below half the smallest subnormal)

Case = namedtuple('Case', 'label coef_t intercept classes nd prod cnt want_c want_a exact16 exact32 proof')


def range_len(C):
    """Classes per range of k_logreg_screen (a multiple of 8)."""
    return ((C + K_SPLIT - 1) // K_SPLIT + 7) & ~7


# ---------------------------------------------------------------------------------------------------------------------------
# the reference and its cross-checks
# ---------------------------------------------------------------------------------------------------------------------------
def scores64(coef_t, intercept, products, counts):
    """Per class: s = 0.0; viewed products ascending, s = s + float64(count) * coef_t[p, c]; then s = s + intercept[c]."""
    s = np.zeros(coef_t.shape[1], dtype=np.float64)
    for p, n in zip(products, counts):
        s = s + np.float64(n) * coef_t[int(p)]
    return s + intercept


def reference(coef_t, intercept, classes, products, counts):
    """-> (class index, action): the first maximum of scores64."""
    order = np.argsort(np.asarray(products, dtype=np.int64), kind='stable')
    s = scores64(coef_t, intercept, np.asarray(products)[order], np.asarray(counts)[order])
    c = int(np.argmax(s))
    return c, int(classes[c])


def reverse_decision(coef_t, intercept, products, counts):
    """The class float64 picks when the terms are added in DESCENDING product order (intercept last)."""
    order = np.argsort(np.asarray(products, dtype=np.int64), kind='stable')[::-1]
    return int(np.argmax(scores64(coef_t, intercept, np.asarray(products)[order], np.asarray(counts)[order])))


def exact_decision(coef_t, intercept, products, counts):
    """The first maximum in exact rational arithmetic over the doubles.  Only the classes whose float64 score lies within the
    float64 summation's own error bound of the float64 maximum can be the exact argmax: Fractions for those."""
    products, counts = np.asarray(products, dtype=np.int64), np.asarray(counts, dtype=np.int64)
    s = scores64(coef_t, intercept, products, counts)
    mag = np.abs(intercept).copy()
    for p, n in zip(products, counts):
        mag += float(n) * np.abs(coef_t[p])
    err = (len(products) + 2) * 2.0 ** -52 * float(mag.max())
    cand = np.flatnonzero(s >= s.max() - 2.0 * err)
    best, best_c = None, -1
    for c in cand:
        v = Fraction(float(intercept[c]))
        for p, n in zip(products, counts):
            v += int(n) * Fraction(float(coef_t[p, c]))
        if best is None or v > best:
            best, best_c = v, int(c)
    return best_c


def bounds32(coef_t, intercept):
    """(wmax float32 (P,), bmax): the bounds the Simulator uploads (recogym_amd.sim.logreg_fp32), rounded up."""
    wmax = (np.abs(coef_t).max(axis=1) * (1.0 + 1e-6)).astype(np.float32) * np.float32(1.0 + 1e-6)
    return wmax.astype(np.float32), float(np.abs(intercept).max()) * (1.0 + 1e-6)


def _fma32(a, b, acc):
    """float32 fma of float32 operands (the product of a count below 2^24 and a float32 is exact in float64)."""
    return (np.float64(a) * b.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def thr16(wmax, bmax, products, counts):
    """k_logreg_screen's band in float64: thr = 2 B16 1.01, B16 = (A 2^-11 + V 2^-25 + (nd + 3) 2^-24 (bmax + A)) 1.02."""
    A = float(sum(float(n) * float(wmax[int(p)]) for p, n in zip(products, counts)))
    V = float(sum(float(n) for n in counts))
    return 2.0 * 1.01 * 1.02 * (A * 2.0 ** -11 + V * 2.0 ** -25 + (len(products) + 3) * 2.0 ** -24 * (bmax + A)) + 1e-30


def band32(wmax, bmax, products, counts):
    """k_logreg_acts' band in float64: 2 (nd + 3) 2^-24 Ahat 1.01."""
    ahat = bmax + float(sum(float(n) * float(wmax[int(p)]) for p, n in zip(products, counts)))
    return 2.0 * (len(products) + 3) * 2.0 ** -24 * ahat * 1.01


def emulate_screen16(coef_t, intercept, products, counts, cols=None):
    """The fp16 screen's scores of the classes `cols` (default all): fp16 weights, an fp32 fma chain, intercept first, history
    order.  It classifies a case; no expected value comes from it."""
    cols = slice(None) if cols is None else np.asarray(cols)
    acc = intercept[cols].astype(np.float32)
    for p, n in zip(products, counts):
        acc = _fma32(np.float32(n), coef_t[int(p), cols].astype(np.float16).astype(np.float32), acc)
    return acc


def emulate_acts32(coef_t, intercept, products, counts, cols=None):
    """The fp32 form's scores: fp32 weights, an fp32 fma chain, intercept first, history order."""
    cols = slice(None) if cols is None else np.asarray(cols)
    acc = intercept[cols].astype(np.float32)
    for p, n in zip(products, counts):
        acc = _fma32(np.float32(n), coef_t[int(p), cols].astype(np.float32), acc)
    return acc


# ---------------------------------------------------------------------------------------------------------------------------
# the layout the builders share
# ---------------------------------------------------------------------------------------------------------------------------
class Layout:
    def __init__(self, C, P=None, seed=0, n_trig=64, classes=None):
        P = C + 320 if P is None else P
        self.C, self.P, self.RC = C, P, range_len(C)
        self.rng = rng = np.random.RandomState(1000 * seed + C)
        n_bg = min(HIST_ENTRIES + 1, P - n_trig)
        assert n_bg >= 34 and n_trig >= 1
        inner = rng.permutation(np.arange(1, P - 1))
        self.bg = np.sort(np.concatenate([[0, P - 1], inner[:n_bg - 2]]))
        self.trig = np.sort(inner[n_bg - 2:n_bg - 2 + n_trig])
        if classes is None:
            # a sorted strict subset of the products, never arange: product 0 is no class, so classes[c] > c for every c
            hidden = np.concatenate([[0], 1 + rng.choice(P - 1, P - C - 1, replace=False)])
            classes = np.setdiff1d(np.arange(P), hidden)
        self.classes = np.asarray(classes, dtype=np.int32)
        assert len(self.classes) == C
        self.coef_t = np.zeros((P, C), dtype=np.float64)
        rows = np.concatenate([self.bg, self.trig])
        # the other classes: in every row and range the values -(0.01 .. 1) evenly spread in a random order, so that no range of a
        # clear-winner case crowds more than K_CAND classes into a band below its own maximum (local_candidates holds that)
        for lo in range(0, C, self.RC):
            m = min(self.RC, C - lo)
            rank = np.argsort(rng.random_sample((len(rows), m)), axis=1)
            self.coef_t[rows, lo:lo + m] = -(0.01 + 0.99 * (rank + 0.5 * rng.random_sample((len(rows), m))) / m)
        self.intercept = -rng.uniform(0.0, 0.05, C)
        self.u = rng.uniform(0.5, 1.0, P)
        self.nds = tuple(n for n in NDS if n <= n_bg) + (min(HIST_ENTRIES, n_bg + 1),)
        self.groups = []           # (trigger index, members)
        self.users = []            # (group, products, counts)

    def group(self, members, col=None, beta=0.0):
        """A group on the next free trigger: `col[k]` (default u) on the bg rows and the own trigger's sign, per member k."""
        j = len(self.groups)
        assert j < len(self.trig), 'out of triggers'
        for i, k in enumerate(members):
            assert 0 <= k < self.C and not any(k in m for _, m in self.groups) and k not in members[:i], k
            w = self.u if col is None else col[i]
            self.coef_t[self.bg, k] = w[self.bg] if np.ndim(w) else w
            self.coef_t[self.trig, k] = -1.0
            self.coef_t[self.trig[j], k] = 1.0 if np.ndim(w) else w
            self.intercept[k] = beta
        self.groups.append((j, list(members)))
        return j

    def history(self, j, nd, thousands, frac, extra=1):
        """One trigger (count ceil(frac V_bg) + extra) and nd - 1 bg products: 0 and P - 1 among them from nd = 3 on."""
        rng = self.rng
        if nd >= 3:
            rest = np.concatenate([[0, self.P - 1], rng.choice(self.bg[1:-1], nd - 3, replace=False)])
        else:
            rest = rng.choice([0, self.P - 1], nd - 1, replace=False)
        cnt = rng.randint(1000, 4000, len(rest)) if thousands else np.ones(len(rest), dtype=np.int64)
        n_q = int(np.ceil(frac * cnt.sum())) + extra
        prod = np.concatenate([rest, [self.trig[j]]]).astype(np.int64)
        cnt = np.concatenate([cnt, [n_q]]).astype(np.int64)
        order = np.argsort(prod)
        assert cnt.max() < 2 ** 24          # (a count the fp32 forms hold exactly)
        return prod[order], cnt[order]

    def users_for(self, j, frac, extra=1, nds=None, certified=False):
        """certified: a history is drawn again until no range crowds its candidate list (local_candidates)."""
        wmax, bmax = bounds32(self.coef_t, self.intercept) if certified else (None, None)
        for nd in (self.nds if nds is None else nds):
            for thousands in (False, True):
                for attempt in range(50):
                    p, c = self.history(j, nd, thousands, frac, extra)
                    if not certified:
                        break
                    kept, streamed = local_candidates(scores64(self.coef_t, self.intercept, p, c), thr16(wmax, bmax, p, c), self.C)
                    if kept <= K_CAND and streamed <= CAND_CAP:
                        break
                else:
                    raise AssertionError(('no uncrowded history', self.C, j, nd, thousands))
                self.users.append((j, p, c))

    def case(self, label, exact16, exact32_ties, proof_fn):
        """Every user's reference decision, the exact-arithmetic agreement, and the builder's own proof `proof_fn(user index, group,
        products, counts, float64 scores, thr16, band32) -> None` (asserts).  exact16: the fp16 form takes float64 for every act
        (True), for none (False); exact32_ties: the fp32 form's band holds more than one class at nd <= 32."""
        n, stride = len(self.users), max(len(p) for _, p, _ in self.users)
        nd = np.array([len(p) for _, p, _ in self.users], dtype=np.uint32)
        prod, cnt = np.zeros((n, stride), dtype=np.uint32), np.zeros((n, stride), dtype=np.uint32)
        want_c, want_a = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        wmax, bmax = bounds32(self.coef_t, self.intercept)
        gaps = []
        for i, (j, p, c) in enumerate(self.users):
            prod[i, :len(p)], cnt[i, :len(p)] = p, c
            assert (np.diff(p) > 0).all() and (c > 0).all()
            want_c[i], want_a[i] = reference(self.coef_t, self.intercept, self.classes, p, c)
            if not label.startswith('order'):
                assert exact_decision(self.coef_t, self.intercept, p, c) == want_c[i], (label, i)
            s = scores64(self.coef_t, self.intercept, p, c)
            t16, b32 = thr16(wmax, bmax, p, c), band32(wmax, bmax, p, c)
            if j is not None:
                # the contest is the group's own: every class outside it trails by more than three bands
                members = self.groups[j][1]
                out = np.ones(self.C, dtype=bool)
                out[members] = False
                assert want_c[i] in members
                if out.any():
                    gaps.append((s[members].min() - s[out].max()) / max(t16, b32))
                    assert gaps[-1] > 3.0, (label, i, gaps[-1])
            proof_fn(i, j, p, c, s, t16, b32)
        long32 = (nd > 32) | (nd == 0)
        e16 = np.full(n, bool(exact16))
        e32 = long32 | bool(exact32_ties) if self.C > 1 else long32
        used = set(np.unique(prod[np.arange(stride)[None, :] < nd[:, None]]).tolist())
        proof = dict(users=n, groups=len(self.groups), min_group_gap_in_bands=min(gaps) if gaps else None,
                     products_0_and_last=bool({0, self.P - 1} <= used), nds=sorted(set(nd.tolist())))
        assert (self.classes != np.arange(self.C)).all() or label.startswith('bench')
        return Case(label, self.coef_t, self.intercept, self.classes, nd, prod, cnt, want_c, want_a, e16, e32, proof)


def local_candidates(s, thr, C):
    """Per range of the screen, from the float64 scores s: how many classes lie within 2 thr of the range's maximum (the screen's
    scores are within thr / 2 of s, so its list of kept candidates is among them) and how many a range can stream into its list,
    batch by batch against the running maximum -> the largest of each over the ranges."""
    RC, kept, streamed = range_len(C), 0, 0
    for lo in range(0, C, RC):
        r = s[lo:lo + RC]
        kept = max(kept, int((r >= r.max() - 2.0 * thr).sum()))
        run, total = -np.inf, 0
        for b in range(0, len(r), BATCH):
            run = max(run, float(r[b:b + BATCH].max()))
            total += int((r[b:b + BATCH] >= run - 2.0 * thr).sum())
        streamed = max(streamed, total)
    return kept, streamed


def bench_classes(C, P, shift=0):
    """The benchmark-size class map: classes[c] = (c + shift) % P keeps the model small.  shift = 0 leaves classes[c] == c below P;
    shift = 1 makes every class index differ from its action."""
    return ((np.arange(C) + shift) % P).astype(np.int32)


def winner_positions(C):
    """Class indices where a planted winner meets a border of the screen: lanes of 8, ranges, batches of 512, the two halves of
    one 32-bit word, a ragged last range."""
    RC = range_len(C)
    last_lo = ((C - 1) // RC) * RC                # first class of the last range that holds a class
    mid = (C // 2) & ~1
    want = [0, 7, 8, RC - 1, RC, last_lo - 1, last_lo, C - 1, 511, 512, 1023, 1024, mid, mid + 1, 2 * RC + 510, 2 * RC + 513]
    return sorted({k for k in want if 0 <= k < C})


def pair_positions(C):
    """(lower, higher) class pairs: inside one lane's 8 classes (one 32-bit word; two words), across lanes, across batches, across
    ranges, and far apart; the ones that fit C, on disjoint classes."""
    RC = range_len(C)
    want = [(2, 3), (5, 6), (7, 8), (RC - 1, RC), (1, C - 1), (511, 512), (RC + 9, 3 * RC + 4), (0, 4), (RC + 511, RC + 512), (0, 1)]
    out, used = [], set()
    for a, b in want:
        if 0 <= a < b < C and not {a, b} & used:
            out.append((a, b))
            used |= {a, b}
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the builders
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clear_winners(C, P=None, bench=False, nds=None, shift=0):
    """A planted winner per group whose gap to the runner-up is >= 100 bands.  The groups' intercepts climb by 2 per group: a screen
    that loses the trigger's row (a history row skipped) sees a LATER group ahead by more than the band of a count-1 history."""
    L = Layout(C, P, seed=1, n_trig=min(64, 30 if bench else 64), classes=bench_classes(C, P, shift) if bench else None)
    pos = winner_positions(C)
    for g, k in enumerate(pos):
        L.group([k], beta=2.0 * g)
    for j in range(len(pos)):
        L.users_for(j, 0.06, extra=2 * len(pos) + 2, nds=nds, certified=True)

    def proof(i, j, p, c, s, t16, b32):
        top = np.sort(s)[-2:]
        assert len(top) == 1 or top[1] - top[0] >= 100.0 * max(t16, b32), (i, top, t16)
        kept, streamed = local_candidates(s, t16, C)                            # no range sends the act to the walk
        assert kept <= K_CAND and streamed <= CAND_CAP, (i, kept, streamed)
    return L.case('bench_clear' if bench else 'clear', False, False, proof)


def _pairs(C, label, dintercept, exact32_ties=True, P=None, bench=False, nds=None, shift=0):
    L = Layout(C, P, seed=2, n_trig=30 if bench else 64, classes=bench_classes(C, P, shift) if bench else None)
    pairs = pair_positions(C)
    if bench:
        pairs = [(a, b) for a, b in pairs if L.classes[a] != L.classes[b]]
    for a, b in pairs:
        j = L.group([a, b])
        L.intercept[b] += dintercept
    for j in range(len(pairs)):
        L.users_for(j, 0.01, nds=nds)
    later = dintercept > 0

    def proof(i, j, p, c, s, t16, b32):
        a, b = L.groups[j][1]
        assert np.array_equal(L.coef_t[:, a], L.coef_t[:, b])                   # bit-identical columns: identical screen scores
        assert (s[b] > s[a]) if later else (s[b] == s[a])
        assert int(np.argmax(s)) == (b if later else a)
    return L, L.case(label, True, exact32_ties, proof)


@functools.lru_cache(maxsize=None)
def exact_ties(C, P=None, bench=False, nds=None, shift=0):
    """Duplicated column and intercept: the lower class index wins."""
    return _pairs(C, 'bench_ties' if bench else 'ties', 0.0, P=P, bench=bench, nds=nds, shift=shift)[1]


@functools.lru_cache(maxsize=None)
def near_ties(C, P=None):
    """The later class of a duplicated pair is ahead by 1e-9 in the intercept: it must win."""
    return _pairs(C, 'near_ties', 1e-9, P=P)[1]


@functools.lru_cache(maxsize=None)
def band_edge_pairs(C, P=None, bench=False, nds=None, shift=0):
    """Per pair: class a carries W_A on every viewed row of the layout (fp16 copy 1.0), class b carries W_B (fp16 copy 1 + 2^-10): the
    fp16 screen puts b ahead by V1 2^-10, most of the band, where V1 is the views of those rows.  Rounding is monotonic, so b leads
    on those rows in float64 too, by V1 2^-22; a wins the act on one more product, the BONUS row, where only the a's carry a weight,
    W_BONUS, whose fp16 copy is 0: viewed 9 V1 + 9 times it is worth more than 9/8 of b's lead.  (The row's wmax is 2^-25: the
    band does not notice it.)  a is the lower index and the higher index in turn; nd >= 2 (the trigger and the bonus row)."""
    L = Layout(C, P, seed=3, n_trig=30 if bench else 64, classes=bench_classes(C, P, shift) if bench else None)
    pairs = pair_positions(C)
    if bench:
        pairs = [(a, b) for a, b in pairs if L.classes[a] != L.classes[b]]
    bonus = int(L.trig[-1])                      # (the last trigger serves no group)
    L.coef_t[bonus, :] = 0.0
    ab = []
    for g, (lo, hi) in enumerate(pairs):
        a, b = (lo, hi) if g % 2 == 0 else (hi, lo)
        L.group([a, b], col=[W_A, W_B])
        L.coef_t[bonus, [a, b]] = [W_BONUS, 0.0]
        ab.append((a, b))
    assert len(pairs) < len(L.trig)
    for j in range(len(pairs)):
        for nd in (L.nds if nds is None else nds):
            if nd < 2:
                continue
            for thousands in (False, True):
                p, c = L.history(j, nd - 1, thousands, 0.01)
                p, c = np.append(p, bonus), np.append(c, 9 * int(c.sum()) + 9)
                order = np.argsort(p)
                assert c.max() < 2 ** 24
                L.users.append((j, p[order], c[order]))
    ratios = []

    def proof(i, j, p, c, s, t16, b32):
        a, b = ab[j]
        assert s[a] > s[b] and int(np.argmax(s)) == a                           # float64 orders the pair a first
        for w in (W_A, W_B, W_BONUS):                                           # one rounding or two: the same fp16 copy
            assert np.float32(w) == w and np.float16(w) == np.float16(np.float32(w))
        e = emulate_screen16(L.coef_t, L.intercept, p, c, [a, b])
        ratios.append(float(e[1] - e[0]) / t16)
        assert 0.75 < ratios[-1] < 1.0, (i, ratios[-1])                         # ... the screen b first, by most of its band
    case = L.case('bench_band_edge' if bench else 'band_edge', True, True, proof)
    case.proof.update(min_ratio=min(ratios), max_ratio=max(ratios))
    return case


def _leaders(L):
    """A LEADER at offset 0 of every range: the shared column on the bg rows, 0 on every trigger.  It trails the viewed group by n_q
    and leads every other group by n_q (ten bands), so a range that holds only groups the user did not view has ONE candidate, not a
    crowd of tied ones that would send every act to the walk."""
    lead = [lo for lo in range(0, L.C, L.RC)]
    for k in lead:
        L.coef_t[L.bg, k] = L.u[L.bg]
        L.coef_t[L.trig, k] = 0.0
        L.intercept[k] = 0.0
    return lead


def _own_ranges_only(L, lead, members, s, t16):
    """Every range that holds no member has one class within two bands of its maximum: its leader."""
    own = {k // L.RC for k in members}
    for r, lo in enumerate(range(0, L.C, L.RC)):
        if r not in own:
            rs = s[lo:lo + L.RC]
            assert int(np.argmax(rs)) == 0 and int((rs >= rs.max() - 2.0 * t16).sum()) == 1, (r, members[:2])


@functools.lru_cache(maxsize=None)
def overflow_cases(C):
    """Candidates beyond K_CAND per range (needs ranges of >= 72 classes): 8 duplicates in one range (they fit: decide's float64), 9 in
    one range (the walk: by construction, 9 bit-identical columns in one range are 9 candidates), nine groups of 9 whose g-th
    member IN THE SCREEN'S LIST ORDER is ahead by 1e-9 (whichever candidate a screen dropped, one group loses its winner), and 16
    spread two per range (decide)."""
    RC = range_len(C)
    assert RC >= 72
    L = Layout(C, seed=4)
    lead = _leaders(L)
    nine = [1, 2, 3, 11, 20, 29, 38, 47, 56]
    L.group([10, 11, 19, 28, 37, 46, 55, 64])                                   # 8 in range 0
    L.group([RC + o for o in nine])                                             # 9 in range 1
    winners = {}
    for g in range(9):                                                          # ranges 2 .. 5 (never the last), up to three per range
        r, shift = 2 + g % 4, 6 * (g // 4)
        members = [r * RC + o + shift for o in nine]
        j = L.group(members)
        # (the screen lists a batch's candidates class-in-lane major, then by lane: the g-th of THAT order)
        win = sorted(members, key=lambda k: ((k - r * RC) % 8, (k - r * RC) // 8))[g]
        L.intercept[win] += 1e-9
        winners[j] = win
    spread = [r * RC + o for r in range(K_SPLIT) for o in (4, 5)]
    assert spread[-1] < C
    j_spread = L.group(spread)
    for j in range(len(L.groups)):
        L.users_for(j, 0.01)

    def proof(i, j, p, c, s, t16, b32):
        members = L.groups[j][1]
        for k in members[1:]:
            assert np.array_equal(L.coef_t[:, k], L.coef_t[:, members[0]])      # bit-identical columns
        per_range = np.bincount(np.asarray(members) // RC, minlength=K_SPLIT)
        top = int(np.argmax(s))
        _own_ranges_only(L, lead, members, s, t16)
        if j in winners:
            assert top == winners[j] and per_range.max() == 9
        elif j == j_spread:
            assert top == spread[0] and (per_range == 2).all()
        else:
            assert top == members[0] and per_range.max() == len(members) in (8, 9)
    return L.case('overflow', True, True, proof)


@functools.lru_cache(maxsize=None)
def climb_cases(C):
    """A range of 70 classes with one column whose intercepts climb by 1e-5: all within the band of the last one (the narrowest
    band of these histories is 1.0e-3): the walk; the last class wins.  The 70 lie in ONE 512-class batch, and the screen cuts a
    whole batch against the running maximum AFTER the batch's own maximum is folded in: all 70 are listed (past CAND_CAP = 64) and
    all 70 survive the final cut (past K_CAND) — this case does not tell the two rules apart; stream_cases does."""
    RC = range_len(C)
    assert RC >= 72
    L = Layout(C, seed=7)
    lead = _leaders(L)
    climb = [6 * RC + o for o in range(2, 72)]
    j = L.group(climb)
    for i, k in enumerate(climb):
        L.intercept[k] += 1e-5 * i
    L.users_for(j, 0.01)

    def proof(i, j, p, c, s, t16, b32):
        for k in climb[1:]:
            assert np.array_equal(L.coef_t[:, k], L.coef_t[:, climb[0]])
        _own_ranges_only(L, lead, climb, s, t16)
        assert len(climb) == 70 > CAND_CAP and int(np.argmax(s)) == climb[-1]
        assert s[climb].max() - s[climb].min() < 0.75 * t16, (s[climb].max() - s[climb].min(), t16)
    return L.case('overflow_climb', True, True, proof)


@functools.lru_cache(maxsize=None)
def stream_cases(C, P=None, bench=False):
    """The streaming list passes CAND_CAP = 64 although ONE class survives: only CAND_CAP marks the overflow.  64 bit-identical
    columns in the first 512-class batch of range 1 fill the list exactly; one class W in a LATER batch of that range is ahead of
    them by more than two bands (the 64 carry +0.5 on the trigger, W carries +1), so listing it is the 65th entry while the final
    cut would keep W alone.  The walk settles the act (lr_exact) and W wins.  This cannot be built inside one batch: a batch is cut
    against the running maximum after its own maximum is folded in, so whatever a single batch lists survives that batch's cut;
    a list longer than what survives needs a later batch to raise the maximum, i.e. ranges longer than 512 classes (C > 4096)."""
    RC = range_len(C)
    assert RC > BATCH
    L = Layout(C, P, seed=8, n_trig=30 if bench else 64, classes=bench_classes(C, P, 1) if bench else None)
    lead = _leaders(L)
    full = [RC + 8 + o for o in range(CAND_CAP)]                                 # lanes 1 .. 8 of the first batch
    W = RC + (RC - 1) // BATCH * BATCH + 3                                      # the range's last batch
    assert full[-1] < RC + BATCH <= W < min(2 * RC, C)
    j = L.group(full + [W])
    L.coef_t[L.trig[j], full] = 0.5
    L.users_for(j, 0.02)
    wmax, bmax = bounds32(L.coef_t, L.intercept)

    def proof(i, j, p, c, s, t16, b32):
        for k in full[1:]:
            assert np.array_equal(L.coef_t[:, k], L.coef_t[:, full[0]])         # bit-identical columns: 64 equal screen scores
        _own_ranges_only(L, lead, full + [W], s, t16)
        kept, streamed = local_candidates(s, t16, C)
        assert int(np.argmax(s)) == W and kept == 1 and streamed == CAND_CAP + 1, (i, kept, streamed)
        e = emulate_screen16(L.coef_t, L.intercept, p, c, full + [W])
        assert (e[:-1] == e[0]).all() and e[-1] - e[0] > 2.0 * t16               # ... in the emulated screen too
    return L.case('bench_stream' if bench else 'overflow_stream', True, True, proof)


@functools.lru_cache(maxsize=None)
def all_zero(C, P=None):
    """The all-zero model: every class ties and the answer is classes[0] (every class is a candidate: the walk where a range holds
    more than K_CAND classes, decide's float64 otherwise)."""
    L = Layout(C, P, seed=5)
    L.coef_t[:] = 0.0
    L.intercept[:] = 0.0
    for nd in (1, 2, 9, 13):
        p = np.sort(L.rng.choice(L.bg, nd, replace=False))
        L.users.append((None, p, np.full(nd, 3 if nd % 2 else 1500, dtype=np.int64)))

    def proof(i, j, p, c, s, t16, b32):
        assert (s == 0.0).all()
    case = L.case('all_zero', True, True, proof)
    assert (case.want_c == 0).all()
    return case


@functools.lru_cache(maxsize=None)
def order_cases(C, walk=False):
    """Cancellation: class A carries (x, L, -L) over three ascending products, class B (y, 0, 0) with 0 < y < x << ulp(L): float64 in
    scipy's order gives A = 0 < B = y, exact arithmetic and the reverse order give A = x > y.  Expected is scipy's order: B.  The fp16
    copies of x and y are 0, so the screen ties the two exactly and decide's float64 sum settles them; `walk`: B is duplicated
    nine more times in its range (ten candidates there: logreg_act_wave settles them; needs ranges of >= 16 classes)."""
    RC = range_len(C)
    L = Layout(C, seed=6)
    Lw, x, y = 16384.0, 4e-13, 2e-13
    L.coef_t[:] = 0.0
    L.intercept[:] = 0.25
    p1, p2, p3 = (int(v) for v in L.bg[[1, 40, 90]])
    L.coef_t[p1, :] = -1000.0
    kA, kB = (RC - 1, RC) if RC < C else (2, 5)
    dups = [RC + 1 + o for o in range(9)] if walk else []
    assert not walk or (RC >= 16 and dups[-1] < C)
    L.coef_t[[p1, p2, p3], kA] = [x, Lw, -Lw]
    for k in [kB] + dups:
        L.coef_t[[p1, p2, p3], k] = [y, 0.0, 0.0]
    fill = [int(v) for v in L.bg[[0, 20, 60, 120, 200, -1]]]
    for n in (1, 3):
        for extra in (0, 2, 6):
            p = np.sort(np.array([p1, p2, p3] + fill[:extra]))
            L.users.append((None, p, np.full(len(p), n, dtype=np.int64)))

    def proof(i, j, p, c, s, t16, b32):
        assert int(np.argmax(s)) == kB and s[kA] == 0.25 and s[kB] > 0.25
        assert exact_decision(L.coef_t, L.intercept, p, c) == kA == reverse_decision(L.coef_t, L.intercept, p, c)
        e = emulate_screen16(L.coef_t, L.intercept, p, c)
        assert e[kA] == e[kB] == e.max() and int((e >= e.max() - t16).sum()) == 2 + len(dups)       # an exact tie in the screen
    return L.case('order_walk' if walk else 'order', True, True, proof)


FP32_REACHED = {1: 0.2475, 2: 0.396, 32: 0.905}


@functools.lru_cache(maxsize=None)
def fp32_band_pairs(C):
    """The fp32 form's band-edge pairs.  The pair's trigger is the LOWEST product of the history (count 1) and nd - 1 small-term
    products follow.  Class a: trigger weight 1 + 2^-24 - 2^-40 (fp32 copy 1.0), small terms 2^-24 (1 - 2^-10) — each below half an
    ulp of the running sum 1.0, so the fp32 chain stays at 1.0; intercept 2^-28 (lost as well).  Class b: trigger weight
    1 + 2^-24 + 2^-40 (fp32 copy 1 + 2^-23), small terms 2^-24 (1 + 2^-10) — each above half an ulp, a whole ulp gained per row.
    a wins in float64 by >= 2^-33 - 2^-39; the fp32 chain puts b ahead by nd 2^-23.  Against the band 2 (nd + 3) 2^-24 Ahat 1.01
    with Ahat ~ 1 that is nd / (1.01 (nd + 3)): FP32_REACHED — 0.2475, 0.396 and 0.905 at nd = 1, 2, 32 (more cannot be reached
    at nd = 1, 2: weight rounding and nd roundings of a sum <= Ahat bound the inversion by 2 (nd + 1) 2^-24 Ahat ... of which the
    intercept's and the first row's cannot both be spent)."""
    pairs = pair_positions(C)
    G, S = len(pairs), 31
    P = C + G + S + 3
    rng = np.random.RandomState(77 + C)
    classes = np.setdiff1d(np.arange(P), np.concatenate([[0], 1 + rng.choice(P - 1, P - C - 1, replace=False)])).astype(np.int32)
    trig, small = np.arange(1, 1 + G), np.arange(P - S, P)
    coef_t = np.zeros((P, C))
    coef_t[trig] = -rng.uniform(0.01, 0.1, (G, C))
    coef_t[small] = -rng.uniform(0.01, 0.1, (S, C)) * 2.0 ** -24
    intercept = -rng.uniform(0.0, 0.05, C) * 2.0 ** -28
    ab, users = [], []
    for g, (lo, hi) in enumerate(pairs):
        a, b = (lo, hi) if g % 2 == 0 else (hi, lo)
        for k, w, ws in ((a, 1.0 + 2.0 ** -24 - 2.0 ** -40, 2.0 ** -24 * (1 - 2.0 ** -10)), (b, 1.0 + 2.0 ** -24 + 2.0 ** -40, 2.0 ** -24 * (1 + 2.0 ** -10))):
            coef_t[trig, k] = -1.0
            coef_t[trig[g], k] = w
            coef_t[small, k] = ws
        intercept[a], intercept[b] = 2.0 ** -28, 0.0
        ab.append((a, b))
        for nd in (1, 2, 32):
            users.append((g, np.concatenate([[trig[g]], small[:nd - 1]]), np.ones(nd, dtype=np.int64)))
    n = len(users)
    nd = np.array([len(p) for _, p, _ in users], dtype=np.uint32)
    prod, cnt = np.zeros((n, 32), dtype=np.uint32), np.zeros((n, 32), dtype=np.uint32)
    want_c, want_a, ratios = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), {1: [], 2: [], 32: []}
    wmax, bmax = bounds32(coef_t, intercept)
    for i, (g, p, c) in enumerate(users):
        prod[i, :len(p)], cnt[i, :len(p)] = p, c
        a, b = ab[g]
        s = scores64(coef_t, intercept, p, c)
        want_c[i], want_a[i] = reference(coef_t, intercept, classes, p, c)
        assert want_c[i] == a == exact_decision(coef_t, intercept, p, c) and s[a] > s[b]
        e = emulate_acts32(coef_t, intercept, p, c)
        band = band32(wmax, bmax, p, c)
        ratio = float(e[b] - e[a]) / band
        ratios[len(p)].append(ratio)
        assert int(np.argmax(e)) == b and FP32_REACHED[len(p)] / 2 < ratio < 1.0, (i, len(p), ratio)
        rest = np.delete(e, [a, b])
        assert not len(rest) or e[a] - rest.max() > 100 * band
    proof = dict(users=n, reached={k: (min(v), max(v)) for k, v in ratios.items() if v})
    return Case('fp32_band_edge', coef_t, intercept, classes, nd, prod, cnt, want_c, want_a, np.ones(n, bool), np.ones(n, bool), proof)


def fp16_builders(C):
    """Every builder that applies at C classes (fp16 form)."""
    out = [clear_winners(C), exact_ties(C), near_ties(C), band_edge_pairs(C), all_zero(C), order_cases(C)]
    if range_len(C) >= 16:
        out.append(order_cases(C, walk=True))
    if range_len(C) >= 72:
        out += [overflow_cases(C), climb_cases(C)]
    if range_len(C) > BATCH:
        out.append(stream_cases(C))
    return out
