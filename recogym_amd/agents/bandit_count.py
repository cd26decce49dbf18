"""BanditCount — reference: recogym/agents/bandit_count.py.

`pulls_a[l, a]` / `clicks_a[l, a]` count the recommendations of `a` (and their clicks) made while the last viewed product
was `l`; `ctr = (clicks_a + 1) / (pulls_a + 2)`; the action is `ctr[last view].argmax()` and the logged `ps` is that CTR
value (a float64, not a probability).  After training the agent is a frozen function of the last viewed product:
RG_POLICY_LAST_VIEW_TABLE with a float64 `ps` table.

Two things the reference does are reproduced, not fixed:

* `ix` of a train call is `last_product_viewed` BEFORE the call's own session is looked at, and it carries over user
  boundaries: a user's first recommendation is counted under the previous user's last view;
* on the first call of all `last_product_viewed` is None, and NumPy's `pulls_a[None, a] += 1` adds 1 to the whole row `a`.

`ctr` is always derived from the two tables (the reference keeps a copy that `load` leaves stale).
"""
import numpy as np

from .. import _abi
from ..envs.configuration import Configuration
from .abstract import Agent
from . import count_tables as ct
from .last_view_table import LastViewTableAgent

bandit_count_args = {
    'num_products': 10,
    'with_ps_all': False,
}

# rg_count_policy decides by exact integer cross-multiplication; its order is the order of the rounded float64 quotients
# while every denominator stays below 2^26 (distinct fractions are then more than an ulp apart)
_EXACT_ORDER_BELOW = 1 << 26


class BanditCount(Agent):
    needs_training = True
    accepts_device_log = True

    def __init__(self, config=Configuration(bandit_count_args)):
        super().__init__(config)
        self._pulls = ct.CountTable(config.num_products)
        self._clicks = ct.CountTable(config.num_products)
        self.last_product_viewed = None
        self._frozen = None

    @property
    def pulls_a(self):
        return self._pulls.dense()

    @property
    def clicks_a(self):
        return self._clicks.dense()

    @property
    def ctr(self):
        return (self.clicks_a + 1) / (self.pulls_a + 2)

    # -- training ---------------------------------------------------------------------------------------
    def _count(self, ix, a, click):
        if ix is None or ix < 0:                     # pulls_a[None, a] += 1: the whole row (bandit_count.py:57-58)
            self._pulls.add_row(a, 1)
            if click:
                self._clicks.add_row(a, 1)
        else:
            self._pulls.add(ix, a, 1)
            if click:
                self._clicks.add(ix, a, 1)

    def train(self, observation, action, reward, done=False):
        if action is not None and reward is not None:
            ix = self.last_product_viewed
            self.update_lpv(observation)
            self._count(ix, int(action['a']), int(reward) != 0)
            self._frozen = None

    def train_from_log(self, log, num_organic_users=0):
        """The train calls of the offline protocol over a whole log (bench_agents.py:90-190), in one reduction."""
        P = int(self.config.num_products)
        dl = ct.as_device_log(log)
        if dl is not None:
            dev = dl.rows.device
            self.last_product_viewed, _ = ct.count_train(dl, P, pulls=self._pulls.device(dev), clicks=self._clicks.device(dev),
                                                         carry=self.last_product_viewed)
        else:
            u, is_b, v, a, click = ct.log_arrays(log)
            ix, act, clk, self.last_product_viewed = ct.bandit_updates(u, is_b, v, a, click, P, self.last_product_viewed)
            for k in np.flatnonzero(ix < 0):
                self._count(None, int(act[k]), bool(clk[k]))
            ok = ix >= 0
            self._pulls.add(ix[ok], act[ok], 1)
            self._clicks.add(ix[ok & clk], act[ok & clk], 1)
        self._frozen = None

    def train_online_from_log(self, log, mask=None):
        """The train calls evaluate_agent's loop makes over a log (one per bandit row that is not a phantom row), restricted to
        the rows `mask` lets through (one entry per row of the log; None = all).  `last_product_viewed` walks over those rows
        only; every row that meets None adds to a whole table row."""
        P = int(self.config.num_products)
        dl = ct.as_device_log(log)
        if dl is not None:
            dev = dl.rows.device
            self.last_product_viewed, _ = ct.count_train_online(dl, P, pulls=self._pulls.device(dev), clicks=self._clicks.device(dev),
                                                                carry=self.last_product_viewed, mask=mask)
        else:
            u, is_b, v, a, click, phantom = ct.online_arrays(log)
            ix, act, clk, self.last_product_viewed = ct.online_bandit_updates(
                u, is_b, v, a, click, P, ct.counted_rows(is_b, phantom, mask), self.last_product_viewed)
            none = ix < 0
            if none.any():
                n = np.bincount(act[none], minlength=P)
                c = np.bincount(act[none & clk], minlength=P)
                for k in np.flatnonzero(n):
                    self._pulls.add_row(int(k), int(n[k]))
                    if c[k]:
                        self._clicks.add_row(int(k), int(c[k]))
            ok = ~none
            self._pulls.add(ix[ok], act[ok], 1)
            self._clicks.add(ix[ok & clk], act[ok & clk], 1)
        self._frozen = None

    # -- acting -----------------------------------------------------------------------------------------
    def frozen(self):
        """The argmax table and its CTR values as a LastViewTableAgent, rebuilt only after training changed the counts."""
        if self._frozen is None:
            P = int(self.config.num_products)
            dev = self._pulls.dev.device if self._pulls.dev is not None else \
                (self._clicks.dev.device if self._clicks.dev is not None else None)
            if dev is not None:
                pulls, clicks = self._pulls.device(dev), self._clicks.device(dev)
                if int(pulls.max().item()) + 2 < _EXACT_ORDER_BELOW:
                    table, wc, wn = ct.count_policy(P, _abi.RG_COUNT_BANDIT, pulls=pulls, clicks=clicks)
                    ps = (wc.astype(np.float64) + 1) / (wn.astype(np.float64) + 2)      # NumPy's own float64 divide
                else:
                    table, ps = ct.host_argmax_rows(P, lambda lo, hi: (clicks[lo:hi].cpu().numpy().astype(np.float64) + 1)
                                                    / (pulls[lo:hi].cpu().numpy().astype(np.float64) + 2))
            else:
                table, ps = ct.host_argmax_rows(P, lambda lo, hi: (self._clicks.rows_dense(lo, hi) + 1)
                                                / (self._pulls.rows_dense(lo, hi) + 2))
            self._frozen = LastViewTableAgent(self.config, table, ps, ps64=True)
        return self._frozen

    def device_policy(self):
        return self.frozen().device_policy()

    def ope_policy(self):
        return self.frozen().ope_policy()

    def update_lpv(self, observation):
        if observation.sessions():
            self.last_product_viewed = int(observation.sessions()[-1]['v'])

    def act(self, observation, reward, done):
        self.update_lpv(observation)
        fz = self.frozen()
        fz.last_product_viewed = self.last_product_viewed
        return fz.act(observation, reward, done)

    # -- persistence (bandit_count.py:69-79) ----------------------------------------------------------------
    def save(self, location):
        np.save(location + 'pulls_a.npy', self.pulls_a)
        np.save(location + 'clicks_a.npy', self.clicks_a)

    def load(self, location):
        self._pulls.set_dense(np.load(location + 'pulls_a.npy'))
        self._clicks.set_dense(np.load(location + 'clicks_a.npy'))
        self._frozen = None

    def reset(self):
        pass
