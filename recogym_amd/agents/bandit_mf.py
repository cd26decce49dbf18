"""BanditMFSquareAgent — reference: recogym/agents/bandit_mf.py.

Matrix-factorisation bandit: logit(a | last product viewed l) = <E_p[a], E_u[l]>, trained online
with mini-batches through `train`, acting by argmax.  Here:

* inference is the frozen per-product table of LastViewTableAgent inside the device step loop;
* training keeps the reference's arithmetic (torch nn.Embedding x 2, BCEWithLogitsLoss, RMSprop,
  one optimiser step every `mini_batch_size` train calls on the samples gathered since the last one
  — the call that triggers the step contributes no sample, bandit_mf.py:110-126) but is fed from a
  whole log at once: `train_from_log` rebuilds the (last product viewed, action, reward) triple of
  every train call with array operations (forward fill of the organic views) and replays the
  optimiser steps.  `train` (observation by observation) is kept and produces the same weights.  This is the HOST route: the
  reference's bits, no GPU needed;
* with the configuration key `device_training = True`, `train_from_log` reduces the log to its triple list on the device
  (`rg_bmf_samples`) and runs the whole chain of RMSprop steps in one launch (`rg_bmf_steps`, float64): the DEVICE route, whose
  weights are close to the reference's, not its bits.  `log_triples` is the host statement of the reduction.
"""
import ctypes as C
import warnings

import numpy as np

from .. import _abi
from ..envs.configuration import Configuration
from .abstract import Agent
from . import count_tables as ct
from .last_view_table import LastViewTableAgent

bandit_mf_square_args = {
    'num_products': 10,
    'embed_dim': 5,
    'mini_batch_size': 32,
    'learning_rate': 0.01,
    'with_ps_all': False,
}


def log_triples(u, is_b, v, a, c, num_organic_users, first_call, mini_batch, pending=None, num_products=None):
    """The host statement of rg_bmf_samples.  The train CALLS of a log are log_pairs' (organic_mf.py): one per organic-only user
    (the first `num_organic_users` users; no action, so no sample), then one per bandit row of every other user.  Every call sets
    the last product viewed to the last view of its session when that is not empty; a user opens with an organic row, so at a
    bandit row it is the nearest organic row in front of it in the same user.  Call number k = first_call + 1 + (calls in front);
    k % mini_batch == 0 triggers an optimiser step over the samples stored since the last trigger and stores nothing itself; any
    other call with an action stores (last product viewed, action, reward).
    -> (triples int32 (n, 3) in log order, `pending` in front; step_offsets int64 (n_steps + 2): rows 0 .. n_steps-1 are the steps,
    row n_steps what lies behind the last trigger; n_calls; last_view = the last view at the last call, -1 without a call)."""
    u, is_b = np.asarray(u), np.asarray(is_b, dtype=bool)
    v, a = np.asarray(v, dtype=np.int64), np.asarray(a, dtype=np.int64)
    click = np.nan_to_num(np.asarray(c, dtype=np.float64)) != 0
    n, mb, first_call = len(u), int(mini_batch), int(first_call)
    pend = np.zeros((0, 3), dtype=np.int32) if pending is None else np.asarray(pending, dtype=np.int32).reshape(-1, 3)
    new_user = np.r_[True, u[1:] != u[:-1]] if n else np.zeros(0, dtype=bool)
    uidx = np.cumsum(new_user) - 1
    n_users = int(uidx[-1]) + 1 if n else 0
    n_org = int(num_organic_users)
    if n_org > n_users:
        raise ValueError(f'{n_org} organic-only users in a log of {n_users} users')
    if n and is_b[new_user].any():
        raise ValueError('a user opens with a bandit row')
    if (is_b & (uidx < n_org)).any():
        raise ValueError('an organic-only user has a bandit row')
    if num_products is not None and n:
        if v[~is_b].min(initial=0) < 0 or v[~is_b].max(initial=0) >= num_products:
            raise ValueError(f'the log views products outside [0, {num_products})')
        if a[is_b].min(initial=0) < 0 or a[is_b].max(initial=0) >= num_products:
            raise ValueError(f'the log has actions outside [0, {num_products})')
    # the forward fill of the organic views: every user opens with one, so it never crosses into another user at a bandit row
    src = np.maximum.accumulate(np.where(~is_b, np.arange(n), -1)) if n else np.zeros(0, dtype=np.int64)
    lpv = v[np.maximum(src, 0)]
    last_row = np.flatnonzero(np.r_[new_user[1:], True]) if n else np.zeros(0, dtype=np.int64)
    b_rows = np.flatnonzero(is_b)
    pos = np.concatenate([last_row[:n_org], b_rows]).astype(np.int64)      # the calls in order: the organic-only users come first
    n_calls = len(pos)
    k = first_call + 1 + np.arange(n_calls)
    keep = (np.arange(n_calls) >= n_org) & (k % mb != 0)
    rows = pos[keep]
    new = np.stack([lpv[rows], a[rows], click[rows].astype(np.int64)], axis=1).astype(np.int32).reshape(-1, 3)
    triples = np.concatenate([pend, new])
    step = np.concatenate([np.zeros(len(pend), dtype=np.int64), (k // mb - first_call // mb)[keep]])
    n_steps = (first_call + n_calls) // mb - first_call // mb
    offsets = np.searchsorted(step, np.arange(n_steps + 2), side='left').astype(np.int64)
    offsets[n_steps + 1] = len(triples)
    return triples, offsets, n_calls, (int(lpv[pos[-1]]) if n_calls else -1)


class BanditMFSquareAgent(Agent):
    needs_training = True

    def __init__(self, config=Configuration(bandit_mf_square_args), product_embedding=None, user_embedding=None):
        """Initial embeddings: given arrays (P, embed_dim), else torch's nn.Embedding default init under
        the current torch seed (product table first, then user table, like the reference's __init__)."""
        import torch
        from torch import nn, optim
        super().__init__(config)
        P, E = config.num_products, config.embed_dim
        self.product_embedding = nn.Embedding(P, E)
        self.user_embedding = nn.Embedding(P, E)
        with torch.no_grad():
            if product_embedding is not None:
                self.product_embedding.weight.copy_(torch.as_tensor(np.asarray(product_embedding, dtype=np.float32)))
            if user_embedding is not None:
                self.user_embedding.weight.copy_(torch.as_tensor(np.asarray(user_embedding, dtype=np.float32)))
        params = list(self.product_embedding.parameters()) + list(self.user_embedding.parameters())
        self.optimizer = optim.RMSprop(params, lr=getattr(config, 'learning_rate', 0.01))
        self.loss = nn.BCEWithLogitsLoss()
        self.batch = getattr(config, 'mini_batch_size', 32)
        self.last_product_viewed = None
        self.curr_step = 0
        self.train_data = ([], [], [])
        self._table = None
        self._dev = None                   # the device route's float64 state and the float32 values it last wrote
        self._warned = False
        self.last_device_stats = None

    def _params(self):
        return [self.product_embedding.weight, self.user_embedding.weight]

    # -- the reference's train, call by call ------------------------------------------------------
    def _update(self, lpvs, actions, rewards):
        import torch
        if len(lpvs) == 0:
            return
        self.optimizer.zero_grad()
        a = self.product_embedding(torch.as_tensor(np.asarray(actions, dtype=np.int64)))
        b = self.user_embedding(torch.as_tensor(np.asarray(lpvs, dtype=np.int64)))
        logit = torch.sum(a * b, dim=1)
        loss = self.loss(logit, torch.as_tensor(np.asarray(rewards, dtype=np.float32)))
        loss.backward()
        self.optimizer.step()
        self._table = None

    def train(self, observation, action, reward, done=False):
        if observation.sessions():
            self.last_product_viewed = observation.sessions()[-1]['v']
        self.curr_step += 1
        if self.curr_step % self.batch == 0:
            self._update(*self.train_data)
            self.train_data = ([], [], [])
        elif action is not None and reward is not None:
            self.train_data[0].append(self.last_product_viewed)
            self.train_data[1].append(action['a'])
            self.train_data[2].append(reward)

    # -- the same, from a whole log -----------------------------------------------------------------
    def train_from_log(self, log, num_organic_users=0):
        """`log`: DataFrame of generate_logs or Simulator.log_columns() in the reference's row order (the
        first `num_organic_users` users are organic-only: the offline protocol calls train once for
        each of them with action None, bench_agents.py:168-175).  Equivalent to the train calls the
        reference's offline protocol makes, in the same order."""
        from .feature_feed import _columns_of, device_log_columns
        dl = ct.as_device_log(log)
        if self.device_route():
            if dl is None:
                import torch
                u, is_b, v, a, click = ct.log_arrays(log)
                dl = ct.columns_to_device_log(u, is_b, v, a, click, int(self.config.num_products),
                                              torch.device('cuda', torch.cuda.current_device()))
            return self._train_device(dl, int(num_organic_users))
        if dl is not None:
            log = device_log_columns(dl)
        u, is_b, v, a, c, _ = _columns_of(log)
        n = len(u)
        # last product viewed at every row = forward fill of the organic views (never empty: a user
        # starts with an organic row); it deliberately carries over user boundaries like the reference
        idx = np.where(~is_b, np.arange(n), -1)
        np.maximum.accumulate(idx, out=idx)
        lpv_all = np.where(idx >= 0, v[np.maximum(idx, 0)], -1)
        # the train calls: one per organic-only user (after its rows), one per bandit row
        first_main = 0
        call_pos, call_has = [], []
        if num_organic_users:
            users = u[np.r_[True, u[1:] != u[:-1]]]
            org_users = users[:num_organic_users]
            last_row = np.flatnonzero(np.r_[u[1:] != u[:-1], True])
            call_pos.append(last_row[:num_organic_users])
            call_has.append(np.zeros(num_organic_users, dtype=bool))
            first_main = int(last_row[num_organic_users - 1]) + 1
            del org_users
        b_rows = np.flatnonzero(is_b)
        b_rows = b_rows[b_rows >= first_main]
        call_pos.append(b_rows)
        call_has.append(np.ones(len(b_rows), dtype=bool))
        pos = np.concatenate(call_pos)
        has = np.concatenate(call_has)
        k = self.curr_step + 1 + np.arange(len(pos))               # 1-based call numbers
        lpv, act, rew = lpv_all[pos], a[pos], np.nan_to_num(c[pos])
        if self.last_product_viewed is not None:                     # (a call before any view of this log)
            lpv = np.where(lpv < 0, self.last_product_viewed, lpv)
        step_calls = np.flatnonzero(k % self.batch == 0)
        start = 0
        pend = tuple(list(x) for x in self.train_data)
        for sc in step_calls:
            sel = np.flatnonzero(has[start:sc]) + start                # samples since the last step; call sc itself adds none
            self._update(pend[0] + lpv[sel].tolist(), pend[1] + act[sel].tolist(), pend[2] + rew[sel].tolist())
            pend = ([], [], [])
            start = sc + 1
        sel = np.flatnonzero(has[start:]) + start
        self.train_data = (pend[0] + lpv[sel].tolist(), pend[1] + act[sel].tolist(), pend[2] + rew[sel].tolist())
        self.curr_step += len(pos)
        if len(pos) and lpv_all[pos[-1]] >= 0:
            self.last_product_viewed = int(lpv_all[n - 1]) if lpv_all[n - 1] >= 0 else self.last_product_viewed

    # -- the device route ---------------------------------------------------------------------------
    def device_route(self):
        """True where train_from_log takes the device route: `device_training` set, a GPU, BCEWithLogitsLoss with default
        arguments, torch's RMSprop without momentum, and P, E and the mini-batch within rg_bmf_steps' caps (beyond them: the host
        route after one RuntimeWarning)."""
        import torch
        from torch import nn
        if not getattr(self.config, 'device_training', False):
            return False
        lf = self.loss
        if type(lf) is not nn.BCEWithLogitsLoss or lf.weight is not None or lf.pos_weight is not None or lf.reduction != 'mean':
            return False
        g = self.optimizer.param_groups[0]
        if type(self.optimizer) is not torch.optim.RMSprop or g.get('momentum', 0) != 0 or g.get('centered', False) \
                or g.get('weight_decay', 0) != 0 or g.get('maximize', False):
            return False
        if not ct.device_present():
            return False
        P, E, mb = int(self.config.num_products), int(self.config.embed_dim), int(self.batch)
        lds_max, p_max, step_max = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        if _abi.load().rg_bmf_limits(E, C.byref(lds_max), C.byref(p_max), C.byref(step_max)) != 0 or P > p_max.value \
                or mb - 1 > step_max.value:                    # (a step holds at most mini_batch_size - 1 samples)
            if not self._warned:
                warnings.warn(f'BanditMFSquareAgent: P = {P}, E = {E}, mini_batch_size = {mb} lie beyond the device training\'s caps; '
                              'training on the host', RuntimeWarning, stacklevel=3)
                self._warned = True
            return False
        return True

    @property
    def accepts_device_log(self):
        """test_agent hands Simulator.device_log() to train_from_log instead of log_columns() where the device route is on."""
        return self.device_route()

    def _ensure_optimizer_state(self):
        """RMSprop creates a parameter's state at its first step: one step on zero gradients creates it and moves nothing."""
        import torch
        params = self._params()
        if all('square_avg' in self.optimizer.state[p] for p in params):
            return
        for p in params:
            p.grad = torch.zeros_like(p)
        self.optimizer.step()
        for p in params:
            p.grad = None
            st = self.optimizer.state[p]
            st['step'] = st['step'] - 1

    def _arrays32(self):
        """(Ep, Eu, their two square averages) as the torch modules and the optimiser hold them, float32."""
        params = self._params()
        out = [p.detach().cpu().numpy().astype(np.float32) for p in params]
        for p in params:
            st = self.optimizer.state.get(p, {})
            out.append(st['square_avg'].detach().cpu().numpy().astype(np.float32) if 'square_avg' in st
                       else np.zeros(tuple(p.shape), dtype=np.float32))
        return out

    def _device_state(self, device):
        """The four float64 device arrays; re-read from the torch side when anything there differs from what was last written."""
        import torch
        cur = self._arrays32()
        d = self._dev
        if d is None or d['state'][0].device != device or any(not np.array_equal(x, y) for x, y in zip(cur, d['wrote'])):
            d = dict(state=[torch.from_numpy(x.astype(np.float64)).to(device).contiguous() for x in cur], wrote=cur)
            self._dev = d
        return d['state']

    def _write_back(self, steps_taken):
        import torch
        state = self._dev['state']
        new = [x.cpu().numpy().astype(np.float32) for x in state]
        self._ensure_optimizer_state()
        with torch.no_grad():
            for k, p in enumerate(self._params()):
                p.copy_(torch.from_numpy(new[k]))
                st = self.optimizer.state[p]
                st['square_avg'].copy_(torch.from_numpy(new[2 + k]))
                st['step'] = st['step'] + steps_taken
        self._dev['wrote'] = self._arrays32()
        self._table = None

    def _train_device(self, dl, num_organic_users):
        import torch
        lib = _abi.load()
        P, E = int(self.config.num_products), int(self.config.embed_dim)
        if int(dl.num_products) != P:
            raise ValueError(f'the log has {dl.num_products} products, the agent {P}')
        device = dl.rows.device
        n_rows, n_users = int(dl.rows.shape[0]), int(dl.offsets.numel()) - 1
        pend = np.stack([np.asarray(x, dtype=np.float64) for x in self.train_data], axis=1).astype(np.int32).reshape(-1, 3)
        n_pend = len(pend)
        g = self.optimizer.param_groups[0]
        with torch.cuda.device(device):
            stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            d_pend = torch.from_numpy(pend).to(device) if n_pend else None
            triples = torch.empty((max(n_pend + n_rows, 1), 3), dtype=torch.int32, device=device)
            step_cap = (self.curr_step % self.batch + n_rows) // self.batch + 2
            offs = torch.empty(step_cap, dtype=torch.int64, device=device)
            out = torch.zeros(8, dtype=torch.int64, device=device)
            need = lib.rg_bmf_samples_workspace_bytes(n_rows, n_pend)
            ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=device)
            _abi.check(lib.rg_bmf_samples(dl.rows.data_ptr(), dl.offsets.data_ptr(), n_users, num_organic_users, n_rows, P, self.curr_step,
                                          self.batch, None if d_pend is None else d_pend.data_ptr(), n_pend, triples.data_ptr(),
                                          n_pend + n_rows, offs.data_ptr(), step_cap, out.data_ptr(), ws.data_ptr(), need, stream),
                       'rg_bmf_samples')
            res = out.cpu().numpy()
            if res[0]:
                raise _abi.RecoGymHipError(f'rg_bmf_samples: error bits {int(res[0])}')
            n_calls, n_steps, n_triples, last_view = int(res[1]), int(res[2]), int(res[3]), int(res[5])
            del ws
            taken = 0
            if n_steps:
                keep = self._dev
                state = self._device_state(device)
                model = _abi.RgBmfModel(P, E, *[x.data_ptr() for x in state])
                need2 = lib.rg_bmf_steps_workspace_bytes(P, E)
                ws2 = torch.empty((need2 + 7) // 8, dtype=torch.int64, device=device)
                out2 = torch.zeros(4, dtype=torch.int64, device=device)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                _abi.check(lib.rg_bmf_steps(C.byref(model), float(g['lr']), float(g['alpha']), float(g['eps']), triples.data_ptr(), n_triples,
                                            offs.data_ptr(), n_steps, 0, out2.data_ptr(), ws2.data_ptr(), need2, stream), 'rg_bmf_steps')
                t1.record()
                res2 = out2.cpu().numpy()
                if res2[0]:                                    # (the kernel left the model as it was)
                    self._dev = keep
                    raise _abi.RecoGymHipError(f'rg_bmf_steps: RG_EINVAL, error bits {int(res2[0])}')
                taken = int(res2[1])
                self.last_device_stats = dict(calls=n_calls, steps=taken, empty_steps=int(res2[2]), samples=int(res2[3]),
                                              steps_ms=float(t0.elapsed_time(t1)))
            tail = offs[n_steps:n_steps + 2].cpu().numpy()
            left = triples[int(tail[0]):int(tail[1])].cpu().numpy()
            self.train_data = (left[:, 0].tolist(), left[:, 1].tolist(), left[:, 2].tolist())
        if taken:
            self._write_back(taken)
        self.curr_step += n_calls
        if last_view >= 0:
            self.last_product_viewed = last_view

    def load_state_dict(self, state):
        """{'product_embedding': ..., 'user_embedding': ..., 'optimizer': ...} as state_dict() gives it."""
        self.product_embedding.load_state_dict(state['product_embedding'])
        self.user_embedding.load_state_dict(state['user_embedding'])
        if 'optimizer' in state:
            self.optimizer.load_state_dict(state['optimizer'])
        self._table = None

    def state_dict(self):
        return dict(product_embedding=self.product_embedding.state_dict(), user_embedding=self.user_embedding.state_dict(),
                    optimizer=self.optimizer.state_dict())

    # -- acting ---------------------------------------------------------------------------------------
    def frozen(self):
        if self._table is None:
            self._table = LastViewTableAgent.from_bandit_mf(
                self.config, self.product_embedding.weight.detach().numpy(),
                self.user_embedding.weight.detach().numpy())
        return self._table

    def device_policy(self):
        return self.frozen().device_policy()

    def act(self, observation, reward, done):
        return self.frozen().act(observation, reward, done)

    def reset(self):
        pass
