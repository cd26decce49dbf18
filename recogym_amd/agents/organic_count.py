"""OrganicCount — reference: recogym/agents/organic_count.py.

`co_counts[i, j]` = sum over the training sessions of views(i) x views(j); the action is the product most often seen together
with the last viewed one: `co_counts[last view].argmax()` (the first index on ties, 0 for a product never seen), `ps = 1`.
After training the agent is a frozen function of the last viewed product, so it runs inside the device step loop as
RG_POLICY_LAST_VIEW_TABLE and has a replay form for off-policy evaluation.

Training: `train` keeps the reference's call-by-call semantics (a sparse update instead of the dense outer product, the same
numbers); `train_from_log` reduces a whole log at once — on the device (`rg_count_train`, the table stays there) for a
Simulator or a DeviceLog, with array operations on the host for a DataFrame / `log_columns()` dict.
"""
import numpy as np

from .. import _abi
from ..envs.configuration import Configuration
from .abstract import Agent
from . import count_tables as ct
from .last_view_table import LastViewTableAgent

organic_count_args = {
    'num_products': 10,
    'with_ps_all': False,
}


class OrganicCount(Agent):
    needs_training = True
    accepts_device_log = True        # test_agent hands Simulator.device_log() to train_from_log instead of log_columns()

    def __init__(self, config=Configuration(organic_count_args)):
        super().__init__(config)
        self._co = ct.CountTable(config.num_products)
        self.corr = None
        self.last_product_viewed = None
        self._frozen = None

    @property
    def co_counts(self):
        """The reference's float64 array, materialised on demand."""
        return self._co.dense()

    # -- training ---------------------------------------------------------------------------------------
    def train(self, observation, action, reward, done=False):
        if observation.sessions():
            p, c = np.unique([int(s['v']) for s in observation.sessions()], return_counts=True)
            m = len(p)
            self._co.add(np.repeat(p, m), np.tile(p, m), np.repeat(c, m) * np.tile(c, m))
            self._frozen = None

    def train_from_log(self, log, num_organic_users=0):
        """The train calls of the offline protocol over a whole log (bench_agents.py:90-190), in one reduction."""
        P = int(self.config.num_products)
        dl = ct.as_device_log(log)
        if dl is not None:
            ct.count_train(dl, P, co=self._co.device(dl.rows.device))
        else:
            u, is_b, v, _, _ = ct.log_arrays(log)
            self._co.add(*ct.organic_updates(u, is_b, v, P))
        self._frozen = None

    def train_online_from_log(self, log, mask=None):
        """The train calls evaluate_agent's loop makes over a log (one per bandit row that is not a phantom row, with the organic
        rows directly in front of it as its session; none for a user's trailing organic rows), restricted to the rows `mask`
        lets through (one entry per row of the log; None = all): rg_count_train_online for a Simulator / DeviceLog, array
        operations for a DataFrame / column dict."""
        P = int(self.config.num_products)
        dl = ct.as_device_log(log)
        if dl is not None:
            ct.count_train_online(dl, P, co=self._co.device(dl.rows.device), mask=mask)
        else:
            u, is_b, v, _, _, phantom = ct.online_arrays(log)
            self._co.add(*ct.online_organic_updates(u, is_b, v, P, ct.counted_rows(is_b, phantom, mask)))
        self._frozen = None

    # -- acting -----------------------------------------------------------------------------------------
    def frozen(self):
        """The argmax table as a LastViewTableAgent, rebuilt only after training changed the counts."""
        if self._frozen is None:
            P = int(self.config.num_products)
            if self._co.dev is not None:
                table, _, _ = ct.count_policy(P, _abi.RG_COUNT_ORGANIC, co=self._co.device(self._co.dev.device))
            else:
                table, _ = ct.host_argmax_rows(P, self._co.rows_dense)
            self._frozen = LastViewTableAgent(self.config, table)
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
