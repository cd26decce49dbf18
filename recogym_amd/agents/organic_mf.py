"""OrganicMFSquare — reference: recogym/agents/organic_mf.py.

Predicts the next viewed product from the last one: logits(l) = W emb[l] + b (nn.Embedding(P, E), nn.Linear(E, P)), trained on
cross-entropy over the consecutive views of every stored session with RMSprop, one optimiser step every `mini_batch_size` train
calls (the call that triggers the step contributes no session, organic_mf.py:103-116); it acts by argmax.  Here:

* inference is the frozen per-product table of LastViewTableAgent inside the device step loop (`ps` = 1);
* `train` keeps the reference's arithmetic call by call (one torch forward and backward per pair of consecutive views);
* `train_from_log` rebuilds the sessions of every train call of a whole log with array operations (`log_pairs`) and replays the
  optimiser steps through torch — the reference's bits, no GPU needed (the HOST route) — or, with the configuration key
  `device_training = True`, reduces the log to its pair list on the device (`rg_omf_pairs`) and runs the whole chain of RMSprop
  steps in one launch (`rg_omf_steps`, float64): the DEVICE route, whose weights are close to the reference's, not its bits
  (DESIGN.md 4l).

A mini-batch enters the gradient only through its pairs (i, j) — view i directly followed by view j inside a session — so the
pending sessions are kept as pairs, in the order the reference would loop over them.
"""
import ctypes as C
import warnings

import numpy as np

from .. import _abi
from ..envs.configuration import Configuration
from .abstract import Agent
from . import count_tables as ct
from .last_view_table import LastViewTableAgent


def _defaults():
    import torch
    return {
        'num_products': 10,
        'embed_dim': 5,
        'mini_batch_size': 32,
        'loss_function': torch.nn.CrossEntropyLoss(),
        'optim_function': torch.optim.RMSprop,
        'learning_rate': 0.01,
        'with_ps_all': False,
    }


organic_mf_square_args = _defaults()


# ----------------------------------------------------------------------------------------------------------
# the train calls of a log, as pairs grouped by optimiser step
# ----------------------------------------------------------------------------------------------------------
def log_pairs(u, is_b, v, num_organic_users, first_call, mini_batch, pending=None, num_products=None):
    """The host statement of rg_omf_pairs.  The train CALLS of a log in the reference's row order: one per organic-only user (the
    first `num_organic_users` users; the session = the user's rows), then one per bandit row of every other user (the session = the
    organic rows of that user since its previous bandit row); a user's trailing organic rows belong to no call.  Call number
    k = first_call + 1 + (calls in front); k % mini_batch == 0 triggers an optimiser step over the sessions stored since the last
    trigger and drops its own session.
    -> (pairs int32 (n, 2) in log order, `pending` in front; step_offsets int64 (n_steps + 2): rows 0 .. n_steps-1 are the steps,
    row n_steps what lies behind the last trigger; n_calls)."""
    u, is_b, v = np.asarray(u), np.asarray(is_b, dtype=bool), np.asarray(v, dtype=np.int64)
    n, mb, first_call = len(u), int(mini_batch), int(first_call)
    pend = np.zeros((0, 2), dtype=np.int32) if pending is None else np.asarray(pending, dtype=np.int32).reshape(-1, 2)
    new_user = np.r_[True, u[1:] != u[:-1]] if n else np.zeros(0, dtype=bool)
    uidx = np.cumsum(new_user) - 1
    n_users = int(uidx[-1]) + 1 if n else 0
    n_org = int(num_organic_users)
    if n_org > n_users:
        raise ValueError(f'{n_org} organic-only users in a log of {n_users} users')
    if n and is_b[new_user].any():
        raise ValueError('a user opens with a bandit row')
    organic_only = uidx < n_org
    if (is_b & organic_only).any():
        raise ValueError('an organic-only user has a bandit row')
    if num_products is not None and n and (v[~is_b].min(initial=0) < 0 or v[~is_b].max(initial=0) >= num_products):
        raise ValueError(f'the log views products outside [0, {num_products})')
    b_rows = np.flatnonzero(is_b)                                   # the calls of the other users, in order
    n_calls = n_org + len(b_rows)
    # a pair: row r and row r + 1 are organic rows of one user
    r = np.flatnonzero(~is_b[:-1] & ~is_b[1:] & ~new_user[1:]) if n > 1 else np.zeros(0, dtype=np.int64)
    nxt = np.searchsorted(b_rows, r)                                # the next bandit row behind r closes r's session ...
    nxt_row = np.r_[b_rows, -1][np.minimum(nxt, len(b_rows))]
    closed = organic_only[r] | ((nxt_row >= 0) & (uidx[np.maximum(nxt_row, 0)] == uidx[r]))      # ... when it is the same user's
    call = np.where(organic_only[r], uidx[r], n_org + nxt)
    k = first_call + 1 + call
    keep = closed & (k % mb != 0)
    step = (k // mb - first_call // mb)[keep]
    pairs = np.concatenate([pend, np.stack([v[r[keep]], v[r[keep] + 1]], axis=1).astype(np.int32)])
    step = np.concatenate([np.zeros(len(pend), dtype=np.int64), step])
    n_steps = (first_call + n_calls) // mb - first_call // mb
    offsets = np.searchsorted(step, np.arange(n_steps + 2), side='left').astype(np.int64)
    offsets[n_steps + 1] = len(pairs)
    return pairs, offsets, n_calls


def session_pairs(views):
    v = [int(x) for x in views]
    return list(zip(v[:-1], v[1:]))


class OrganicMFSquare(Agent):
    needs_training = True

    def __init__(self, config=Configuration(organic_mf_square_args), product_embedding=None, output_weight=None, output_bias=None):
        """Initial weights: given arrays (embedding (P, E), Linear weight (P, E), Linear bias (P)), else torch's default
        initialisation under the current torch seed, the embedding first and the Linear layer second like the reference's __init__."""
        import torch
        from torch import nn
        super().__init__(config)
        P, E = int(config.num_products), int(config.embed_dim)
        self.product_embedding = nn.Embedding(P, E)
        self.output_layer = nn.Linear(E, P)
        with torch.no_grad():
            for given, param in ((product_embedding, self.product_embedding.weight), (output_weight, self.output_layer.weight),
                                 (output_bias, self.output_layer.bias)):
                if given is not None:
                    param.copy_(torch.as_tensor(np.asarray(given, dtype=np.float32)))
        optim = getattr(config, 'optim_function', torch.optim.RMSprop)
        self.optimizer = optim(self._params(), lr=getattr(config, 'learning_rate', 0.01))
        self.loss_function = getattr(config, 'loss_function', None) or nn.CrossEntropyLoss()
        self.batch = int(getattr(config, 'mini_batch_size', 32))
        self.last_product_viewed = None
        self.curr_step = 0
        self.train_data = []               # the pairs (i, j) of the sessions stored since the last optimiser step
        self._table = None
        self._dev = None                   # the device route's float64 state and the float32 values it last wrote
        self._warned = False

    def _params(self):
        return [self.product_embedding.weight, self.output_layer.weight, self.output_layer.bias]

    # -- the reference's update_weights, pair by pair --------------------------------------------------------------
    def _update(self, pairs):
        import torch
        if len(pairs) == 0:
            return                         # every .grad would stay None: the reference's step changes nothing then
        self.optimizer.zero_grad()
        for i, j in pairs:
            product = torch.Tensor([int(i)])
            logit = self.output_layer(self.product_embedding(product.long()))
            loss = self.loss_function(logit, torch.LongTensor([int(j)]))
            loss.backward()
        self.optimizer.step()
        self._table = None

    def train(self, observation, action, reward, done=False):
        self.curr_step += 1
        if self.curr_step % self.batch == 0:
            self._update(self.train_data)
            self.train_data = []
        elif observation is not None:
            self.train_data.extend(session_pairs(s['v'] for s in observation.sessions()))

    # -- the same, from a whole log ---------------------------------------------------------------------------------
    def device_route(self):
        """True where train_from_log takes the device route: `device_training` set, a GPU, CrossEntropyLoss with default
        arguments, torch's RMSprop without momentum, and P and E within rg_omf_steps' caps (beyond them: the host route after one
        RuntimeWarning)."""
        import torch
        from torch import nn
        if not getattr(self.config, 'device_training', False):
            return False
        lf = self.loss_function
        if type(lf) is not nn.CrossEntropyLoss or lf.weight is not None or lf.ignore_index != -100 or lf.reduction != 'mean' \
                or getattr(lf, 'label_smoothing', 0.0) != 0.0:
            return False
        g = self.optimizer.param_groups[0]
        if type(self.optimizer) is not torch.optim.RMSprop or g.get('momentum', 0) != 0 or g.get('centered', False) \
                or g.get('weight_decay', 0) != 0 or g.get('maximize', False):
            return False
        if not ct.device_present():
            return False
        P, E = int(self.config.num_products), int(self.config.embed_dim)
        lds_max, p_max = C.c_uint32(0), C.c_uint32(0)
        if _abi.load().rg_omf_limits(E, C.byref(lds_max), C.byref(p_max)) != 0 or P > p_max.value:
            if not self._warned:
                warnings.warn(f'OrganicMFSquare: P = {P}, E = {E} lie beyond the device training\'s caps; training on the host',
                              RuntimeWarning, stacklevel=3)
                self._warned = True
            return False
        return True

    @property
    def accepts_device_log(self):
        """test_agent hands Simulator.device_log() to train_from_log instead of log_columns() where the device route is on."""
        return self.device_route()

    def train_from_log(self, log, num_organic_users=0):
        """The train calls of the offline protocol over a whole log (bench_agents.py:168-190): a DataFrame of generate_logs,
        Simulator.log_columns(), a Simulator or a DeviceLog, in the reference's row order."""
        dl = ct.as_device_log(log)
        P = int(self.config.num_products)
        if self.device_route():
            if dl is None:
                u, is_b, v, a, click = ct.log_arrays(log)
                import torch
                dl = ct.columns_to_device_log(u, is_b, v, a, click, P, torch.device('cuda', torch.cuda.current_device()))
            return self._train_device(dl, int(num_organic_users))
        if dl is not None:
            from .feature_feed import device_log_columns
            log = device_log_columns(dl)
        u, is_b, v, _, _ = ct.log_arrays(log)
        pairs, off, n_calls = log_pairs(u, is_b, v, num_organic_users, self.curr_step, self.batch, self.train_data, P)
        n_steps = len(off) - 2
        for s in range(n_steps):
            self._update(pairs[off[s]:off[s + 1]].tolist())
        self.train_data = [tuple(p) for p in pairs[off[n_steps]:off[n_steps + 1]].tolist()]
        self.curr_step += n_calls

    # -- the device route -------------------------------------------------------------------------------------------
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
        """(emb, w, bias, their three square averages) as the torch modules and the optimiser hold them, float32."""
        params = self._params()
        out = [p.detach().cpu().numpy().astype(np.float32) for p in params]
        for p in params:
            st = self.optimizer.state.get(p, {})
            out.append(st['square_avg'].detach().cpu().numpy().astype(np.float32) if 'square_avg' in st
                       else np.zeros(tuple(p.shape), dtype=np.float32))
        return out

    def _device_state(self, device):
        """The six float64 device arrays; re-read from the torch side when anything there differs from what was last written."""
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
                st['square_avg'].copy_(torch.from_numpy(new[3 + k]))
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
        pend = np.asarray(self.train_data, dtype=np.int32).reshape(-1, 2)
        n_pend = len(pend)
        g = self.optimizer.param_groups[0]
        with torch.cuda.device(device):
            stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            d_pend = torch.from_numpy(pend).to(device) if n_pend else None
            pairs = torch.empty((max(n_pend + n_rows, 1), 2), dtype=torch.int32, device=device)
            step_cap = (self.curr_step % self.batch + n_rows) // self.batch + 2
            offs = torch.empty(step_cap, dtype=torch.int64, device=device)
            out = torch.zeros(8, dtype=torch.int64, device=device)
            need = lib.rg_omf_pairs_workspace_bytes(n_rows, n_pend)
            ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=device)
            _abi.check(lib.rg_omf_pairs(dl.rows.data_ptr(), dl.offsets.data_ptr(), n_users, num_organic_users, n_rows, P, self.curr_step,
                                        self.batch, None if d_pend is None else d_pend.data_ptr(), n_pend, pairs.data_ptr(),
                                        n_pend + n_rows, offs.data_ptr(), step_cap, out.data_ptr(), ws.data_ptr(), need, stream),
                       'rg_omf_pairs')
            res = out.cpu().numpy()
            if res[0]:
                raise _abi.RecoGymHipError(f'rg_omf_pairs: error bits {int(res[0])}')
            n_calls, n_steps, n_pairs = int(res[1]), int(res[2]), int(res[3])
            del ws
            taken = 0
            if n_steps:
                state = self._device_state(device)
                model = _abi.RgOmfModel(P, E, *[x.data_ptr() for x in state])
                need2 = lib.rg_omf_steps_workspace_bytes(P, E)
                ws2 = torch.empty((need2 + 7) // 8, dtype=torch.int64, device=device)
                out2 = torch.zeros(4, dtype=torch.int64, device=device)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                _abi.check(lib.rg_omf_steps(C.byref(model), float(g['lr']), float(g['alpha']), float(g['eps']), pairs.data_ptr(), n_pairs,
                                            offs.data_ptr(), n_steps, 0, out2.data_ptr(), ws2.data_ptr(), need2, stream), 'rg_omf_steps')
                t1.record()
                res2 = out2.cpu().numpy()
                if res2[0]:
                    raise _abi.RecoGymHipError(f'rg_omf_steps: error bits {int(res2[0])}')
                taken = int(res2[1])
                self.last_device_stats = dict(calls=n_calls, steps=taken, empty_steps=int(res2[2]), pairs=int(res2[3]),
                                              steps_ms=float(t0.elapsed_time(t1)))
            tail = offs[n_steps:n_steps + 2].cpu().numpy()
            self.train_data = [tuple(p) for p in pairs[int(tail[0]):int(tail[1])].cpu().numpy().tolist()]
        if taken:
            self._write_back(taken)
        self.curr_step += n_calls

    # -- acting -----------------------------------------------------------------------------------------------------
    def frozen(self):
        if self._table is None:
            self._table = LastViewTableAgent.from_organic_mf(
                self.config, self.product_embedding.weight.detach().cpu().numpy(), self.output_layer.weight.detach().cpu().numpy(),
                self.output_layer.bias.detach().cpu().numpy())
        return self._table

    def load_state_dict(self, state):
        """{'product_embedding': ..., 'output_layer': ..., 'optimizer': ...} as state_dict() gives it."""
        self.product_embedding.load_state_dict(state['product_embedding'])
        self.output_layer.load_state_dict(state['output_layer'])
        if 'optimizer' in state:
            self.optimizer.load_state_dict(state['optimizer'])
        self._table = None

    def state_dict(self):
        return dict(product_embedding=self.product_embedding.state_dict(), output_layer=self.output_layer.state_dict(),
                    optimizer=self.optimizer.state_dict())

    def device_policy(self):
        return self.frozen().device_policy()

    def ope_policy(self):
        return self.frozen().ope_policy()

    def act(self, observation, reward, done):
        if observation is not None and observation.sessions():
            self.last_product_viewed = int(observation.sessions()[-1]['v'])
        fz = self.frozen()
        fz.last_product_viewed = self.last_product_viewed
        return fz.act(observation, reward, done)

    def reset(self):
        pass
