"""Simulator — thin Python owner of one `rg_sim` handle (include/recogym_hip.h).

PyTorch-ROCm is plumbing here: it owns the device buffers (tables, workspace, log) and the
stream; every bit of simulation work happens in librecogym_hip.so's HIP kernels.  There is no
CPU fallback — constructing a Simulator without a HIP device raises.
"""
import ctypes as C
import math
import os
from collections import namedtuple

import numpy as np
import torch

from . import _abi
from .envs.static_params import draw_tables, make_rg_config

# decoded log rows (host side), same field names as the oracle's rows
ROW_DTYPE = np.dtype([('u', np.uint32), ('t', np.uint32), ('z', np.int32), ('v', np.int32),
                      ('a', np.int32), ('c', np.int32), ('phantom', np.int32),
                      ('ps', np.float64)])
ROW_DTYPE_PCLICK = np.dtype(ROW_DTYPE.descr + [('p_click', np.float64)])

# A sorted log on the device (Simulator.device_log): rows (n, 4) int32 rg_event records in the reference's order, offsets
# (users + 1) int64, ps = float64 tensor | the exact float 1/P of the uniform loggers | None (the row's float32 value),
# first_user = the id of user 0, num_products, time = the float64 clock of a NormalTimeGenerator (else None)
DeviceLog = namedtuple('DeviceLog', 'rows offsets ps first_user num_products time')


def require_device(device=None):
    lib = _abi.load()
    if not torch.cuda.is_available() or lib.rg_device_count() <= 0:
        raise _abi.RecoGymHipError(
            'recogym_amd needs a HIP device (MI355X / gfx950); there is no CPU fallback')
    return torch.device(device if device is not None else f'cuda:{torch.cuda.current_device()}')


def default_log_capacity(config, n_users):
    """Rows a run emits: each user lives ~Geometric(prob_leave) events plus its phantom row."""
    p_stop = max(float(config.prob_leave_organic), 1e-6)
    mean = 1.0 / p_stop + 1.0
    rows = n_users * (mean + 1.0) + 8.0 * mean * math.sqrt(n_users) + 4096
    # the user-major walk (sigma_omega = 0) reserves raw-log rows per wave in chunks and leaves a few percent of
    # them unused: up to 63 per chunk of >= 256 rows and the rest of every wave's last chunk
    return int(rows * 1.04 + min(rows * 0.3, 4.0e6) + 65536)


def decode_rows(raw, uniform_ps=None, ps64=None, p_click=None):
    """(n,4) int32 array of rg_event records -> structured host rows.  `ps64` / `p_click`: the float64
    side arrays in the same order (Simulator.sorted_aux_host), else ps is the row's float32 value."""
    raw = np.ascontiguousarray(raw).view(np.uint32).reshape(-1, 4)
    n = raw.shape[0]
    out = np.zeros(n, dtype=ROW_DTYPE if p_click is None else ROW_DTYPE_PCLICK)
    code = raw[:, 2]
    is_b = (code & _abi.RG_EV_BANDIT) != 0
    idx = (code & _abi.RG_EV_INDEX_MASK).astype(np.int32)
    out['u'] = raw[:, 0]
    out['t'] = raw[:, 1]
    out['z'] = is_b
    out['v'] = np.where(is_b, -1, idx)
    out['a'] = np.where(is_b, idx, -1)
    out['c'] = np.where(is_b, (code & _abi.RG_EV_CLICK) != 0, -1)
    out['phantom'] = (code & _abi.RG_EV_PHANTOM) != 0
    ps = raw[:, 3].copy().view(np.float32).astype(np.float64) if ps64 is None else ps64
    if p_click is not None:
        out['p_click'] = np.where(is_b & (out['phantom'] == 0), p_click, np.nan)
    if uniform_ps is not None:
        ps = np.where(is_b, uniform_ps, np.nan)     # exact 1/P of the uniform policies
    out['ps'] = np.where(is_b, ps, np.nan)
    return out


def logreg_fp32(coef_t, intercept):
    """float64 device tensors coef_t (P, C) / intercept (C,) -> (coef32_t, intercept32, wmax, bmax): the fp32 copies of the
    certified fast scores and the bounds of their margin certificate, wmax[p] >= max_c |coef_t[p][c]| and bmax >= max_c
    |intercept[c]|, rounded up (the step loop's k_logreg_acts and the replay's k_ope_logreg share them)."""
    w32 = coef_t.to(torch.float32)
    b32 = intercept.to(torch.float32)
    wmax = (coef_t.abs().amax(dim=1) * (1.0 + 1e-6)).to(torch.float32) * (1.0 + 1e-6)
    bmax = float(intercept.abs().max().item()) * (1.0 + 1e-6)
    return w32.contiguous(), b32.contiguous(), wmax.contiguous(), bmax


def logreg_device_model(logreg, num_products, device):
    """A policy dict's `logreg` entry (coef_t (P, C) = sklearn's coef_.T, intercept (C,), classes (C,): host arrays, or tensors, which are
    taken as they are) -> ((coef_t, intercept float64, classes int32) on `device`, logreg_fp32's (coef32_t, intercept32, wmax, bmax) for
    the argmax form — None with select_randomly or fp32 = False): what rg_sim_set_logreg / rg_sim_set_logreg_fp32 and
    rg_ope_replay_logreg take."""
    def put(x, np_type, t_type):
        if torch.is_tensor(x):
            return x.to(device=device, dtype=t_type).contiguous()
        return torch.as_tensor(np.ascontiguousarray(x, dtype=np_type)).to(device)
    coef_t = put(logreg['coef_t'], np.float64, torch.float64)
    intercept = put(logreg['intercept'], np.float64, torch.float64)
    classes = put(logreg['classes'], np.int32, torch.int32)
    assert coef_t.shape == (int(num_products), classes.numel()) and intercept.shape == (classes.numel(),)
    fp32 = logreg.get('fp32', True) and not logreg.get('select_randomly')
    return (coef_t, intercept, classes), (logreg_fp32(coef_t, intercept) if fp32 else None)


def poly_device_model(logreg_poly, num_products, device):
    """A policy dict's `logreg_poly` entry (wf (P,), wa (P,), wk (P, P) [action][product], intercept, optionally expit_steps) ->
    ((wf, wa, wk, b) host arrays, (wf, wa, wk_t, th) float64 tensors on `device`): wk transposed to [viewed product][action] (lanes
    over actions read a row contiguously) and the table of expit's top steps — what rg_sim_set_logreg_poly and
    rg_ope_replay_poly take.  evaluate_agent.ope_replay accepts the result as the entry's `device_model` key."""
    from .agents.logreg_poly import expit_steps
    P = int(num_products)
    wf, wa, wk = (np.ascontiguousarray(logreg_poly[k], dtype=np.float64) for k in ('wf', 'wa', 'wk'))
    assert wf.shape == (P,) and wa.shape == (P,) and wk.shape == (P, P)
    th = logreg_poly.get('expit_steps')
    th = expit_steps() if th is None else np.ascontiguousarray(th, dtype=np.float64)
    dev = tuple(torch.from_numpy(x).to(device) for x in (wf, wa, np.ascontiguousarray(wk.T), th))
    return (wf, wa, wk, float(logreg_poly['intercept'])), dev


def bayes_device_model(bayes_vb, num_products, device):
    """A policy dict's `bayes_vb` entry (lam (S, P^2): BayesianAgentVB's posterior draws) -> (Lambda on the host, lam_t (P, P, S)
    float64 tensor on `device`): the model transposed to [viewed product][action][sample], the sample axis contiguous (the 64 lanes
    of a wave read 512 contiguous bytes per (p, a)) — what rg_sim_set_bayes_vb takes."""
    from .agents.bayesian_poly_vb import bayes_transpose
    lam = np.ascontiguousarray(bayes_vb['lam'], dtype=np.float64)
    return lam, torch.from_numpy(bayes_transpose(lam, num_products)).to(device)


def bayes_host_act(views, num_products, Lambda):
    """The host act of BayesianAgentVB on the organic views `views` (product ids, any order): the reference's expression on the
    dense int16 counts — what the device's unresolved acts are judged by."""
    from .agents.bayesian_poly_vb import reference_act
    X = np.bincount(np.asarray(views, dtype=np.int64), minlength=int(num_products)).astype(np.int16).reshape(1, -1)
    return reference_act(X, Lambda)[0]


def nn_device_model(nn_ips, device):
    """A policy dict's `nn_ips` entry (state: the six float32 arrays of NnIpsAgent's net) -> (the frozen host agent's net, NnModel on
    the host, the six float64 tensors on `device` in rg_sim_set_nn_ips's order: the matrices transposed)."""
    from .agents.nn_ips import NnIpsFrozenAgent, NnModel
    from .envs.configuration import Configuration
    m = NnModel(nn_ips['state'])
    host = NnIpsFrozenAgent(Configuration({'num_products': m.P}), nn_ips['state'])
    return host, m, [torch.from_numpy(x).to(device) for x in m.arrays()]


def nn_host_act(views, num_products, agent):
    """The host act of NnIpsAgent on the organic views `views` (product ids, any order): torch's fp32 forward on the dense float32
    counts, first maximum — what the device's unresolved acts are judged by."""
    x = np.bincount(np.asarray(views, dtype=np.int64), minlength=int(num_products))
    return agent.act_on(np.flatnonzero(x), x[np.flatnonzero(x)])[0]


def mlr_device_model(mlr, device):
    """A policy dict's `mlr` entry (state: dict(W (P, P) float32, [action][viewed product])) -> (the frozen host agent, the float64
    table [viewed product][action] on `device`, rg_sim_set_mlr's layout)."""
    from .agents.pytorch_mlr import PyTorchMLRFrozenAgent, mlr_table
    from .envs.configuration import Configuration
    W = np.asarray(mlr['state']['W'], dtype=np.float32)
    host = PyTorchMLRFrozenAgent(Configuration({'num_products': W.shape[0]}), W)
    return host, torch.from_numpy(mlr_table(W)).to(device)


def mlr_host_act(views, num_products, agent):
    """The host act of PyTorchMLRAgent on the organic views `views` (product ids, any order): the reference's fp32 dot on the dense
    float32 counts, first maximum — what the device's unresolved acts are judged by."""
    x = np.bincount(np.asarray(views, dtype=np.int64), minlength=int(num_products))
    return agent.act_on(np.flatnonzero(x), x[np.flatnonzero(x)])[0]


def poly_host_act(views, model):
    """The host act of the likelihood agent on the organic views `views` (product ids, any order) under model = (wf, wa, wk, b):
    the decisions in the contract's order, scipy's expit, first maximum — what the device's unresolved acts are judged by."""
    from scipy.special import expit
    from .agents.logreg_poly import poly_decisions
    prods, cnts = np.unique(np.asarray(views, dtype=np.int64), return_counts=True)
    return int(np.argmax(expit(poly_decisions(prods, cnts, *model))))


def weighted_host_act(prods, times, now, weight_history, model):
    """The likelihood agent's act on a time-weighted history, on the host: views_history.weighted_list on the int16 casts of the
    clock values, the decisions in the contract's order, scipy's expit, first maximum.  -> the action, or -1 where a clock value
    lies outside [0, 32767] (no act of the device form stands there)."""
    from scipy.special import expit
    from .agents.logreg_poly import poly_decisions
    from .agents.views_history import weighted_list
    times, now = np.asarray(times, dtype=np.float64), np.asarray(now, dtype=np.float64).reshape(-1)
    if len(now) != 1 or not (0 <= now[0] < 32768) or (len(times) and not ((times >= 0) & (times < 32768)).all()):
        return -1
    try:
        p, val = weighted_list(prods, np.trunc(times).astype(np.int64), int(np.trunc(now[0])), weight_history['table'],
                               weight_history['f32'])
    except ValueError:
        return -1
    return int(np.argmax(expit(poly_decisions(p, val.astype(np.float64), *model))))


def poly_replay_verify(dl, acts, overflow, model):
    """replay_verify for the likelihood agent: `model`: (wf, wa, wk, b) on the host, the host act poly_host_act."""
    return replay_verify(dl, acts, overflow, lambda views: poly_host_act(views, model))


def replay_verify(dl, acts, overflow, host_act):
    """The host's confirmation of the acts a replay unit could not resolve (rg_ope_replay_poly, rg_ope_replay_nn,
    rg_ope_replay_bayes: Simulator.poly_verify's counterpart for a replay).  `dl`: the replayed DeviceLog; `acts`: (n, 3) array of
    (user index, position of the bandit row the act was computed at within the user's rows, action taken); `overflow`: the list did
    not hold them all; `host_act(views)`: the agent's action on the organic views `views` (product ids in log order) on the host.
    The history of a listed act is the user's organic rows BEFORE that position; only the listed users' rows leave the device.
    -> True when the replay stands: every listed act confirmed, no overflow."""
    if overflow:
        return False
    acts = np.asarray(acts, dtype=np.int64).reshape(-1, 3)
    if not len(acts):
        return True
    users = np.unique(acts[:, 0])
    at = torch.as_tensor(users, device=dl.offsets.device)
    begin, end = dl.offsets[at].cpu().numpy(), dl.offsets[at + 1].cpu().numpy()
    code = {int(u): dl.rows[int(b):int(e), 2].contiguous().cpu().numpy().view(np.uint32) for u, b, e in zip(users, begin, end)}
    for user, pos, a in acts:
        c = code[int(user)][:int(pos)]
        if int(host_act(c[(c & _abi.RG_EV_BANDIT) == 0] & _abi.RG_EV_INDEX_MASK)) != int(a):
            return False
    return True


def weighted_replay_verify(dl, t, acts, overflow, weight_history, model):
    """replay_verify for the likelihood agent on a time-weighted history (rg_ope_replay_poly_w).  `t`: the clock value of every row
    of `dl` (a tensor beside dl.rows: dl.time, or the rows' event index); `acts`: (n, 3) array of (user index, position of the bandit
    row within the user's rows, action taken); `weight_history`: dict(table, f32); `model`: (wf, wa, wk, b) on the host.  The act of
    a listed row is judged by weighted_host_act on the user's organic rows BEFORE that position, with their clock values, at the
    clock value of the row itself; -1 from it (a clock value outside [0, 32767]) refutes like any other action than the listed one.
    Only the listed users' rows leave the device.  -> True when the replay stands: every listed act confirmed, no overflow."""
    if overflow:
        return False
    acts = np.asarray(acts, dtype=np.int64).reshape(-1, 3)
    if not len(acts):
        return True
    users = np.unique(acts[:, 0])
    at = torch.as_tensor(users, device=dl.offsets.device)
    begin, end = dl.offsets[at].cpu().numpy(), dl.offsets[at + 1].cpu().numpy()
    code = {int(u): dl.rows[int(b):int(e), 2].contiguous().cpu().numpy().view(np.uint32) for u, b, e in zip(users, begin, end)}
    clock = {int(u): t[int(b):int(e)].cpu().numpy().astype(np.float64) for u, b, e in zip(users, begin, end)}
    for user, pos, a in acts:
        c, tt = code[int(user)], clock[int(user)]
        if int(pos) >= len(c):
            return False
        organic = (c[:int(pos)] & _abi.RG_EV_BANDIT) == 0
        got = weighted_host_act(c[:int(pos)][organic] & _abi.RG_EV_INDEX_MASK, tt[:int(pos)][organic], tt[int(pos)], weight_history, model)
        if got < 0 or got != int(a):
            return False
    return True


class Simulator:
    """N concurrent users of one reco-gym-v1 environment on one GPU.

    config       env Configuration (env_1_args keys)
    n_users      capacity (users per reset range)
    policy       _abi.RG_POLICY_*; policy_seed / ouc = the agent's parameters
    epoch        added to config.random_seed (reset_random_seed(epoch), abstract.py:59-62)
    log_capacity rows of device log to allocate; 0 = counters only; None = estimate
    ps_float64   keep the propensity of every bandit row in float64 beside the 16-byte row (the dtype of
                 the reference's `ps` column); default: on for the policies whose ps is not a constant
    p_click      also keep the click probability of every bandit row (parity checks)
    epsilon_greedy  dict(epsilon, seed, pure_new): the EpsilonGreedy overlay over `policy` (agents/epsilon_greedy.py;
                 rg_sim_set_epsilon_greedy, or rg_sim_set_epsilon_greedy_model where the policy is the frozen LogReg argmax or
                 the likelihood agent, or rg_sim_set_epsilon_greedy_model_ps where it is NnIpsAgent or BayesianAgentVB) — the
                 explore table and both propensity factors are NumPy's, built here
    logreg_poly  dict(wf (P,), wa (P,), wk (P, P) [action][product], intercept): the likelihood agent's fitted model
                 (RG_POLICY_LOGREG_POLY; agents/logreg_poly.py) — the table of expit's top steps is built and uploaded here.
                 After a run, `poly_verify(columns)` recomputes the acts the device could not resolve on the host.
                 An optional entry `weight_history = dict(table=, f32=)` (agents/views_history.weight_table) makes the act's
                 features the time-weighted ones: a fresh act per bandit event at the event's clock value; such a
                 run is lock-step and needs a log.  debug_set_timed_history / debug_weighted_acts reach the device function.
    nn_ips       dict(state = dict(w1, b1, w2, b2, w3, b3)): NnIpsAgent's net (RG_POLICY_NN_IPS; agents/nn_ips.py), widened to float64,
                 transposed and uploaded here; ps is the model's output, kept in float64.  Its unresolved acts share the likelihood
                 agent's list, counter (`poly_unresolved`) and `poly_verify`, which judges them by torch's fp32 forward.
    mlr          dict(state = dict(W (P, P) float32)): PyTorchMLRAgent's weight (RG_POLICY_MLR; agents/pytorch_mlr.py), widened to
                 float64, transposed and uploaded here; ps = 1.  Its unresolved acts share the likelihood agent's list, counter
                 (`poly_unresolved`) and `poly_verify`, which judges them by the reference's fp32 dot.
    bayes_vb     dict(lam (S, P^2)): BayesianAgentVB's posterior draws (RG_POLICY_BAYES_VB; agents/bayesian_poly_vb.py), transposed
                 and uploaded here.  Its unresolved acts share the likelihood agent's list, counter (`poly_unresolved`) and
                 `poly_verify`, which judges them by the reference's own expression.
    """

    def __init__(self, config, n_users, policy=_abi.RG_POLICY_UNIFORM_ENV, policy_seed=None,
                 ouc=None, epoch=0, log_capacity=None, device=None, tables=None, policy_table=None,
                 policy_ps=None, logreg=None, ps_float64=None, p_click=False, env0=None, policy_ps64=False,
                 epsilon_greedy=None, logreg_poly=None, bayes_vb=None, nn_ips=None, mlr=None):
        if policy == _abi.RG_POLICY_LOGREG_FROZEN and ((logreg or {}).get('int8') or os.environ.get('RECOGYM_LOGREG') == 'int8'):
            # (refused, not ignored: a caller that labels the act's bytes from this switch would report 1 B per weight for an fp16 run)
            raise ValueError("the 8-bit LogReg screen is retired (measured slower than the fp16 screen): drop logreg['int8'] / RECOGYM_LOGREG=int8")
        self.lib = _abi.load()
        self.device = require_device(device)
        self.config = config
        self.n_users = int(n_users)
        # env0: the dict draw_env0_tables(config) returns — reco-gym-v0 (env_kind = 1), every draw a table look-up
        self.env0 = env0
        self.rg_config = make_rg_config(config, config.random_seed + epoch, policy, policy_seed,
                                        ouc, env_kind=1 if env0 is not None else 0,
                                        lr_select_randomly=bool(logreg and logreg.get('select_randomly')))
        self.policy = policy
        self.time_mode = int(self.rg_config.time_mode)
        self.epsilon_greedy = epsilon_greedy
        # the loggers whose propensity is the constant 1 / P (its exact float64 value is filled in at decode time)
        self.uniform_ps = policy in (_abi.RG_POLICY_UNIFORM_ENV, _abi.RG_POLICY_RANDOM_AGENT) and epsilon_greedy is None
        self.ps_float64 = ((policy in (_abi.RG_POLICY_ORGANIC_USER_COUNT, _abi.RG_POLICY_LAST_VIEW_TABLE)
                            or bool(logreg and logreg.get('select_randomly')) or epsilon_greedy is not None
                            or policy == _abi.RG_POLICY_NN_IPS)
                           if ps_float64 is None else bool(ps_float64))
        self.keep_p_click = bool(p_click)
        host_tables = () if env0 is not None else (tables if tables is not None else draw_tables(config))
        self.host_tables = host_tables
        with torch.cuda.device(self.device):
            self.tables = [torch.from_numpy(np.ascontiguousarray(t)).to(self.device)
                           for t in host_tables]
            need = self.lib.rg_sim_workspace_bytes(C.byref(self.rg_config), self.n_users)
            if need == 0:
                raise _abi.RecoGymHipError('rg_sim_workspace_bytes: ' +
                                           self.lib.rg_last_error().decode())
            self.workspace = self._poison(torch.empty(need, dtype=torch.uint8, device=self.device))
            self._h = C.c_void_p()
            _abi.check(self.lib.rg_sim_create(C.byref(self._h), C.byref(self.rg_config),
                                              self.n_users, self.workspace.data_ptr(), need),
                       'rg_sim_create')
            if epsilon_greedy is not None:
                # before the tables: the overlay keeps the run in the lock-step kernels
                from .agents.epsilon_greedy import explore_table
                eps, pure_new = float(epsilon_greedy['epsilon']), bool(epsilon_greedy.get('pure_new', True))
                if pure_new and config.num_products < 2:
                    raise _abi.RecoGymHipError('rg_sim_set_epsilon_greedy: RG_EINVAL: epsilon_pure_new needs at least 2 products')
                cdf, prob = explore_table(config.num_products, pure_new)
                self.eg_cdf = torch.from_numpy(cdf).to(self.device)
                # (a model inside — its cached act is the greedy action — has an entry point of its own)
                model = policy in (_abi.RG_POLICY_LOGREG_FROZEN, _abi.RG_POLICY_LOGREG_POLY)
                what = 'rg_sim_set_epsilon_greedy_model' if model else 'rg_sim_set_epsilon_greedy'
                if policy in (_abi.RG_POLICY_NN_IPS, _abi.RG_POLICY_BAYES_VB):
                    what = 'rg_sim_set_epsilon_greedy_model_ps'       # (NnIpsAgent's greedy row logs (1 - eps) * the model's own ps)
                _abi.check(getattr(self.lib, what)(self._h, eps, int(epsilon_greedy['seed']) & 0xFFFFFFFFFFFFFFFF,
                                                   int(pure_new), self.eg_cdf.data_ptr(), eps * prob, 1.0 - eps), what)
            if env0 is not None:
                p = np.ascontiguousarray(env0['click_probs'], dtype=np.float64)
                qn, px1 = np.empty_like(p), np.empty_like(p)
                _abi.check(self.lib.rg_env0_click_thresholds(p.ctypes.data, p.size, qn.ctypes.data, px1.ctypes.data),
                           'rg_env0_click_thresholds')
                self.tables = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(self.device)
                               for x in (env0['cdf_init'], env0['cdf_cluster'], p, qn, px1)]
                _abi.check(self.lib.rg_sim_set_env0_tables(self._h, self.tables[0].data_ptr(), self.tables[1].data_ptr(),
                                                           int(env0['cluster_size']), self.tables[2].data_ptr(),
                                                           self.tables[3].data_ptr(), self.tables[4].data_ptr(), self._stream()),
                           'rg_sim_set_env0_tables')
            else:
                _abi.check(self.lib.rg_sim_set_tables(self._h, *[t.data_ptr() for t in self.tables],
                                                      self._stream()), 'rg_sim_set_tables')
            if policy == _abi.RG_POLICY_LAST_VIEW_TABLE:
                self.policy_table = torch.as_tensor(np.ascontiguousarray(policy_table, dtype=np.int32)).to(self.device)
                # policy_ps64: the `ps` table stays float64 on the device (BanditCount's CTR values are not float32 numbers)
                self.policy_ps = None if policy_ps is None else \
                    torch.as_tensor(np.ascontiguousarray(policy_ps, dtype=np.float64 if policy_ps64 else np.float32)).to(self.device)
                set_table = self.lib.rg_sim_set_policy_table_f64 if policy_ps64 else self.lib.rg_sim_set_policy_table
                _abi.check(set_table(self._h, self.policy_table.data_ptr(),
                                     None if self.policy_ps is None else self.policy_ps.data_ptr()), 'rg_sim_set_policy_table')
            if policy == _abi.RG_POLICY_LOGREG_FROZEN:
                # dict(coef_t (P, C) float64 = sklearn coef_.T, intercept (C,), classes (C,))
                n_fit = int(np.asarray(logreg['classes']).size)
                if n_fit % 8 and logreg.get('fp16', True) and logreg.get('fp32', True) and not logreg.get('select_randomly'):
                    # the fp16 screening pass reads 8 classes per 16-byte load: pad with copies of the LAST class (same
                    # column, intercept and action: an exact tie with it, whichever of them wins the action is the same)
                    pad = 8 - n_fit % 8
                    logreg = dict(logreg,
                                  coef_t=np.concatenate([logreg['coef_t'], np.repeat(np.asarray(logreg['coef_t'])[:, -1:], pad, axis=1)], axis=1),
                                  intercept=np.concatenate([logreg['intercept'], np.repeat(np.asarray(logreg['intercept'])[-1:], pad)]),
                                  classes=np.concatenate([logreg['classes'], np.repeat(np.asarray(logreg['classes'])[-1:], pad)]))
                self.logreg, fp32 = logreg_device_model(logreg, config.num_products, self.device)
                _abi.check(self.lib.rg_sim_set_logreg(self._h, self.logreg[0].data_ptr(), self.logreg[1].data_ptr(),
                                                      self.logreg[2].data_ptr(), self.logreg[2].numel()),
                           'rg_sim_set_logreg')
                if fp32 is not None:
                    # fp32 copies for the certified fast scores (the float64 arrays stay the arbiter); bounds rounded up
                    *self.logreg32, bmax = fp32
                    self.logreg32 = tuple(self.logreg32)
                    _abi.check(self.lib.rg_sim_set_logreg_fp32(self._h, self.logreg32[0].data_ptr(), self.logreg32[1].data_ptr(),
                                                               self.logreg32[2].data_ptr(), C.c_float(bmax)), 'rg_sim_set_logreg_fp32')
                    # screening pass from a half copy of coef^T (half the row bytes; float64 decides among the candidates):
                    # RECOGYM_LOGREG=fp32 keeps the fp32 scores only (A/B)
                    n_cls = int(self.logreg[2].numel())
                    if (logreg.get('fp16', True) and n_cls % 8 == 0 and os.environ.get('RECOGYM_LOGREG', 'fp16') != 'fp32'
                            and float(self.logreg[0].abs().max().item()) < 6.0e4):
                        self.logreg16 = self.logreg[0].to(torch.float16).contiguous()
                        _abi.check(self.lib.rg_sim_set_logreg_fp16(self._h, self.logreg16.data_ptr()), 'rg_sim_set_logreg_fp16')
            self.weight_history = None
            # _host_act(views) -> the attached model's act on a user's views, by the host's arithmetic (poly_verify; the
            # time-weighted likelihood agent's takes clock values too and is called there).  The model is bound as a default
            # argument, not through self: a Simulator that is dropped unclosed is still released by its reference count.
            self._host_act = None
            if policy == _abi.RG_POLICY_LOGREG_POLY:
                self.logreg_poly_host, self.logreg_poly = poly_device_model(logreg_poly, int(config.num_products), self.device)
                self._host_act = lambda views, model=self.logreg_poly_host: poly_host_act(views, model)
                _abi.check(self.lib.rg_sim_set_logreg_poly(self._h, *[t.data_ptr() for t in self.logreg_poly[:3]],
                                                           C.c_double(self.logreg_poly_host[3]), self.logreg_poly[3].data_ptr(),
                                                           int(self.logreg_poly[3].numel())), 'rg_sim_set_logreg_poly')
                # logreg_poly['weight_history'] = dict(table=, f32=) (agents/views_history.weight_table): the act's features are
                # time-weighted sums, not counts — the table goes up widened to float64
                self.weight_history = logreg_poly.get('weight_history')
                if self.weight_history is not None:
                    table = np.ascontiguousarray(self.weight_history['table'])
                    assert table.dtype == (np.float32 if self.weight_history['f32'] else np.float64), table.dtype
                    self.wh_table = torch.from_numpy(table.astype(np.float64)).to(self.device)
                    _abi.check(self.lib.rg_sim_set_weight_history(self._h, self.wh_table.data_ptr(), int(self.wh_table.numel()),
                                                                  int(bool(self.weight_history['f32']))), 'rg_sim_set_weight_history')
            self.bayes_vb_host = None
            if policy == _abi.RG_POLICY_BAYES_VB:
                self.bayes_vb_host, self.bayes_vb = bayes_device_model(bayes_vb, int(config.num_products), self.device)
                _abi.check(self.lib.rg_sim_set_bayes_vb(self._h, self.bayes_vb.data_ptr(), int(self.bayes_vb.shape[2])),
                           'rg_sim_set_bayes_vb')
                self._host_act = lambda views, P=config.num_products, model=self.bayes_vb_host: bayes_host_act(views, P, model)
            self.nn_ips_host = None
            if policy == _abi.RG_POLICY_NN_IPS:
                self.nn_ips_host, self.nn_ips_model, self.nn_ips = nn_device_model(nn_ips, self.device)
                _abi.check(self.lib.rg_sim_set_nn_ips(self._h, *[x.data_ptr() for x in self.nn_ips], int(self.nn_ips_model.H)),
                           'rg_sim_set_nn_ips')
                self._host_act = lambda views, P=config.num_products, model=self.nn_ips_host: nn_host_act(views, P, model)
            self.mlr_host = None
            if policy == _abi.RG_POLICY_MLR:
                self.mlr_host, self.mlr = mlr_device_model(mlr, self.device)
                _abi.check(self.lib.rg_sim_set_mlr(self._h, self.mlr.data_ptr()), 'rg_sim_set_mlr')
                self._host_act = lambda views, P=config.num_products, model=self.mlr_host: mlr_host_act(views, P, model)
            self.poly_unresolved = self.poly_refuted = None
            self.poly_overflow = False
            if log_capacity is None:
                log_capacity = default_log_capacity(config, self.n_users)
            self.log = None
            self.set_log_capacity(log_capacity)

    # -- plumbing ---------------------------------------------------------------------------
    @staticmethod
    def _poison(t):
        """RECOGYM_POISON=1 (a debugging aid): fill every buffer handed to the library with 0xA5 bytes, so that a
        kernel reading memory nothing initialised fails every time instead of when the allocator recycles a block."""
        if os.environ.get('RECOGYM_POISON'):
            t.view(torch.uint8).fill_(0xA5)
        return t

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def set_log_capacity(self, rows):
        self.log_capacity = int(rows)
        with torch.cuda.device(self.device):
            self.log = (self._poison(torch.empty((self.log_capacity, 4), dtype=torch.int32, device=self.device))
                        if rows else None)
        _abi.check(self.lib.rg_sim_set_log(self._h, self.log.data_ptr() if rows else None,
                                           self.log_capacity), 'rg_sim_set_log')
        self.aux_time = None
        if rows and self.time_mode:
            with torch.cuda.device(self.device):
                self.aux_time = self._poison(torch.empty(self.log_capacity, dtype=torch.float64, device=self.device))
            _abi.check(self.lib.rg_sim_set_log_time(self._h, self.aux_time.data_ptr()), 'rg_sim_set_log_time')
        self.aux_ps = self.aux_p_click = None
        if rows and (self.ps_float64 or self.keep_p_click):
            with torch.cuda.device(self.device):
                if self.ps_float64:
                    self.aux_ps = self._poison(torch.empty(self.log_capacity, dtype=torch.float64, device=self.device))
                if self.keep_p_click:
                    self.aux_p_click = self._poison(torch.empty(self.log_capacity, dtype=torch.float64, device=self.device))
            _abi.check(self.lib.rg_sim_set_log_aux(
                self._h, None if self.aux_ps is None else self.aux_ps.data_ptr(),
                None if self.aux_p_click is None else self.aux_p_click.data_ptr()), 'rg_sim_set_log_aux')

    def close(self):
        if getattr(self, '_h', None) is not None and self._h:
            self.lib.rg_sim_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- the step loop ----------------------------------------------------------------------
    def reseed(self, seed, policy_seed=None):
        ps = self.rg_config.policy_seed if policy_seed is None else policy_seed
        self.rg_config.seed = seed
        self.rg_config.policy_seed = ps
        _abi.check(self.lib.rg_sim_reseed(self._h, seed, ps), 'rg_sim_reseed')

    def set_option(self, name, value):
        """A run-path tuning knob by name (rg_sim_set_option; include/recogym_hip.h lists them)."""
        _abi.check(self.lib.rg_sim_set_option(self._h, name.encode(), int(value)), f'rg_sim_set_option({name})')

    def get_option(self, name):
        v = C.c_int64(0)
        _abi.check(self.lib.rg_sim_get_option(self._h, name.encode(), C.byref(v)), f'rg_sim_get_option({name})')
        return int(v.value)

    def reset_users(self, first_user_id=0, n=None, organic_only_below=0):
        n = self.n_users if n is None else int(n)
        self.first_user_id = int(first_user_id)
        self.n_active = n
        with torch.cuda.device(self.device):
            _abi.check(self.lib.rg_sim_reset_users(self._h, self.first_user_id, n,
                                                   int(organic_only_below), self._stream()),
                       'rg_sim_reset_users')

    def step(self, actions=None):
        """One Markov transition for every live user; `actions` (int32 tensor, one per user of
        the reset range) only with the external policy."""
        ptr = None
        if actions is not None:
            assert actions.dtype == torch.int32 and actions.is_cuda
            ptr = actions.data_ptr()
        with torch.cuda.device(self.device):
            _abi.check(self.lib.rg_sim_step(self._h, ptr, self._stream()), 'rg_sim_step')

    def step_user(self, action=None):
        """One Markov transition of a ONE-user external-policy simulator with a single read-back (rg_sim_step_user) ->
        (decoded row or None, state, clock)."""
        res = _abi.RgStepResult()
        with torch.cuda.device(self.device):
            _abi.check(self.lib.rg_sim_step_user(self._h, -1 if action is None else int(action), C.byref(res), self._stream()),
                       'rg_sim_step_user')
        row = None
        if res.has_row:
            raw = np.array([[res.row.u, res.row.t, res.row.code, 0]], dtype=np.uint32)
            raw[0, 3] = np.float32(res.row.ps).view(np.uint32)
            row = decode_rows(raw.view(np.int32), ps64=np.array([res.ps]) if self.aux_ps is not None else None,
                              p_click=np.array([res.p_click]) if self.aux_p_click is not None else None)[0]
        return row, int(res.state), float(res.time)

    def run(self, max_steps=1 << 16):
        """rg_sim_run; raises when the run is incomplete (uncertified draws beyond the float64 resolve scratch)."""
        with torch.cuda.device(self.device):
            _abi.check(self.lib.rg_sim_run(self._h, max_steps, self._stream()), 'rg_sim_run')

    def counters(self):
        out = (C.c_int64 * _abi.RG_CNT_N)()
        with torch.cuda.device(self.device):
            _abi.check(self.lib.rg_sim_read_counters(self._h, out, self._stream()),
                       'rg_sim_read_counters')
        names = ['organic', 'bandit', 'clicks', 'phantom', 'live', 'step', 'log_rows',
                 'log_dropped', 'exact_draws', 'hist_overflow', 'exact_sweeps', 'exact_overflow', 'lr_acts', 'lr_rows',
                 'lr_exact', 'memo_hits']
        res = {k: int(out[i]) for i, k in enumerate(names)}
        res['anchored'] = int(out[_abi.RG_CNT_ANCHORED])
        res['bad_actions'] = int(out[_abi.RG_CNT_BAD_ACTION])        # external actions outside [0, P) that reached the device
        res['poly_table'] = int(out[_abi.RG_CNT_POLY_TABLE])         # likelihood agent: acts decided on the expit step table
        res['poly_unresolved'] = int(out[_abi.RG_CNT_POLY_UNRESOLVED])   # ... acts listed for the host (poly_verify)
        res['wh_clock_range'] = int(out[_abi.RG_CNT_WH_CLOCK_RANGE])     # ... weighted acts that met a clock value outside [0, 32767]
        res['bayes_saturated'] = int(out[_abi.RG_CNT_BAYES_SATURATED])   # BayesianAgentVB: acts decided in the saturated zone
        return res

    def debug_set_history(self, nd, products, counts):
        """rg_sim_debug_set_history: per user index of the reset range, nd[i] distinct products products[i, j] (ascending) with
        view counts counts[i, j]."""
        products, counts = np.ascontiguousarray(products, dtype=np.uint32), np.ascontiguousarray(counts, dtype=np.uint32)
        assert products.shape == counts.shape and products.shape[0] == self.n_active == len(nd)
        with torch.cuda.device(self.device):
            d = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)).to(self.device) for x in (nd, products, counts)]
            _abi.check(self.lib.rg_sim_debug_set_history(self._h, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                                         int(products.shape[1]), self._stream()), 'rg_sim_debug_set_history')
            torch.cuda.synchronize(self.device)

    def _debug_model_acts(self, what, extras):
        """The debug entry point `what` of a model agent -> (actions, flags, *extras): the act of every user index on its current
        history, into poisoned tensors.  extras: the trailing shape of each float64 output beyond actions and flags."""
        n = self.n_active
        with torch.cuda.device(self.device):
            act = torch.full((n,), -1, dtype=torch.int32, device=self.device)
            fl = torch.full((n,), 255, dtype=torch.uint8, device=self.device)
            out = [torch.full((n, *shape), float('nan'), dtype=torch.float64, device=self.device) for shape in extras]
            _abi.check(getattr(self.lib, what)(self._h, act.data_ptr(), fl.data_ptr(), *[x.data_ptr() for x in out], self._stream()), what)
            torch.cuda.synchronize(self.device)
        return (act.cpu().numpy().astype(np.int64), fl.cpu().numpy().astype(np.int64), *[x.cpu().numpy() for x in out])

    def debug_bayes_acts(self):
        """rg_sim_debug_bayes_acts -> (actions, flags, q (n, P)): BayesianAgentVB's act of every user index on its current history
        and the device's means."""
        return self._debug_model_acts('rg_sim_debug_bayes_acts', [(int(self.config.num_products),)])

    def debug_nn_acts(self):
        """rg_sim_debug_nn_acts -> (actions, flags, z (n, P), ps (n,)): NnIpsAgent's act of every user index on its current history,
        the device's logits and propensity."""
        return self._debug_model_acts('rg_sim_debug_nn_acts', [(int(self.config.num_products),), ()])

    def debug_mlr_acts(self):
        """rg_sim_debug_mlr_acts -> (actions, flags, z (n, P)): PyTorchMLRAgent's act of every user index on its current history, the
        device's scores."""
        return self._debug_model_acts('rg_sim_debug_mlr_acts', [(int(self.config.num_products),)])

    def debug_logreg_acts(self):
        """rg_sim_debug_logreg_acts -> actions: the frozen LogReg's act of every user index on its current history, by the step loop's
        kernels (the counters and the launch ledger count as in a step).  Reset the users again before a run."""
        n = self.n_active
        with torch.cuda.device(self.device):
            act = torch.full((n,), -1, dtype=torch.int32, device=self.device)
            _abi.check(self.lib.rg_sim_debug_logreg_acts(self._h, act.data_ptr(), self._stream()), 'rg_sim_debug_logreg_acts')
            torch.cuda.synchronize(self.device)
        return act.cpu().numpy().astype(np.int64)

    def debug_set_timed_history(self, n_views, products, times16):
        """rg_sim_debug_set_timed_history: per user index of the reset range, n_views[i] views (products[i, j] at clock value
        times16[i, j], in view order) as its time-weighted history."""
        products = np.ascontiguousarray(products, dtype=np.uint32)
        times16 = np.ascontiguousarray(times16, dtype=np.uint16)
        assert products.shape == times16.shape and products.shape[0] == self.n_active == len(n_views)
        with torch.cuda.device(self.device):
            d = [torch.from_numpy(np.ascontiguousarray(n_views, dtype=np.uint32).view(np.int32)).to(self.device),
                 torch.from_numpy(products.view(np.int32)).to(self.device), torch.from_numpy(times16.view(np.int16)).to(self.device)]
            _abi.check(self.lib.rg_sim_debug_set_timed_history(self._h, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                                               int(products.shape[1]), self._stream()), 'rg_sim_debug_set_timed_history')
            torch.cuda.synchronize(self.device)

    def debug_weighted_acts(self, now16, stride=None):
        """rg_sim_debug_weighted_acts at the clock values now16 -> (actions, flags, list lengths, list products (n, stride), list
        values (n, stride) float32): the weighted act of every user index and the feature list it was taken on."""
        n = self.n_active
        now16 = np.ascontiguousarray(now16, dtype=np.uint16)
        assert now16.shape == (n,)
        stride = int(stride or max(1, min(int(self.config.num_products), self.get_option('hist_cap') - 1)))
        with torch.cuda.device(self.device):
            now = torch.from_numpy(now16.view(np.int16)).to(self.device)
            act = torch.full((n,), -1, dtype=torch.int32, device=self.device)
            fl = torch.full((n,), 255, dtype=torch.uint8, device=self.device)
            ln = torch.zeros(n, dtype=torch.int32, device=self.device)
            lp = torch.full((n, stride), -1, dtype=torch.int32, device=self.device)
            lv = torch.zeros((n, stride), dtype=torch.float32, device=self.device)
            _abi.check(self.lib.rg_sim_debug_weighted_acts(self._h, now.data_ptr(), act.data_ptr(), fl.data_ptr(), ln.data_ptr(),
                                                           lp.data_ptr(), lv.data_ptr(), stride, self._stream()),
                       'rg_sim_debug_weighted_acts')
            torch.cuda.synchronize(self.device)
        # (the values leave the device as bytes: a float32 subnormal must not pass through an arithmetic conversion)
        return (act.cpu().numpy().astype(np.int64), fl.cpu().numpy().astype(np.int64), ln.cpu().numpy().astype(np.int64),
                lp.cpu().numpy().astype(np.int64), lv.view(torch.int32).cpu().numpy().view(np.float32))

    def poly_unresolved_acts(self):
        """The acts of the run the likelihood agent's device rule could not resolve -> ((n, 3) uint32 array of (user id, t, action
        taken), overflow): t is the event index the act was computed at, its history the user's organic rows with index <= t."""
        out = np.zeros((4096, 3), dtype=np.uint32)
        n, over = C.c_uint32(0), C.c_uint32(0)
        with torch.cuda.device(self.device):
            _abi.check(self.lib.rg_sim_read_poly_unresolved(self._h, out.ctypes.data, out.shape[0], C.byref(n), C.byref(over),
                                                            self._stream()), 'rg_sim_read_poly_unresolved')
        return out[:n.value].copy(), bool(over.value)

    def poly_verify(self, columns=None):
        """Recompute every unresolved act on the host — the views are the log's organic rows of that user up to the act's event,
        the arithmetic is the host act's (scipy's expit) — and keep the outcome in `poly_unresolved` (the listed acts),
        `poly_refuted` (those whose action the host does not confirm) and `poly_overflow`.  -> True when the device log stands:
        nothing refuted, no overflow of the list.  `columns`: log_columns() of this run, where the caller has them already."""
        acts, self.poly_overflow = self.poly_unresolved_acts()
        self.poly_unresolved = acts
        self.poly_refuted = acts[:0]
        if len(acts):
            cols = self.log_columns() if columns is None else columns
            u = np.asarray(cols['u']).view(np.uint32)
            organic = ~np.asarray(cols['is_bandit'], dtype=bool)
            v = np.asarray(cols['v'])
            # the row's EVENT INDEX = its position among its user's rows (the `t` column is the clock of a NormalTimeGenerator)
            first = np.flatnonzero(np.r_[True, u[1:] != u[:-1]])
            t = np.arange(len(u)) - np.repeat(first, np.diff(np.r_[first, len(u)]))
            bad = []
            clock = self._clock64(cols) if self.weight_history is not None else None
            for user, t_act, a in acts:
                if clock is not None:
                    # a time-weighted act: the user's views before the listed row, their clock values and the row's own
                    mine = u == user
                    host = weighted_host_act(v[mine & organic & (t < t_act)], clock[mine & organic & (t < t_act)],
                                             clock[mine & (t == t_act)], self.weight_history, self.logreg_poly_host)
                else:
                    host = self._host_act(v[organic & (u == user) & (t <= t_act)])
                if host != int(a):
                    bad.append((user, t_act, a))
            self.poly_refuted = np.asarray(bad, dtype=np.uint32).reshape(-1, 3)
        return not self.poly_overflow and len(self.poly_refuted) == 0

    def _clock64(self, cols):
        """The clock value of every row of log_columns() as the device holds it: float64 under a NormalTimeGenerator (the `t`
        column is its float32 rounding, which can cross an integer), the event index otherwise."""
        if not self.time_mode:
            return np.asarray(cols['t'], dtype=np.float64)
        out, offsets = self.sorted_log()
        return self.sorted_time(offsets, int(out.shape[0])).cpu().numpy().astype(np.float64)

    def set_profiling(self, on=True):
        _abi.check(self.lib.rg_sim_set_profiling(self._h, int(on)), 'rg_sim_set_profiling')

    def profile(self):
        """-> dict(draw_mfma_ms, draw_search_ms, draw_exact_ms, advance_ms, steps, tail_ms), HIP events."""
        out = (C.c_double * 10)()
        _abi.check(self.lib.rg_sim_get_profile(self._h, out), 'rg_sim_get_profile')
        return dict(draw_mfma_ms=out[0], draw_search_ms=out[1], draw_exact_ms=out[2],
                    advance_ms=out[3], steps=int(out[4]), tail_ms=out[5], walk1_ms=out[6], walk2_ms=out[7],
                    logreg_ms=out[8])

    def states(self):
        with torch.cuda.device(self.device):
            st = torch.empty(self.n_users, dtype=torch.int8, device=self.device)
            _abi.check(self.lib.rg_sim_export_state(self._h, st.data_ptr(), self._stream()),
                       'rg_sim_export_state')
        return st[:self.n_active]

    def walk_fate(self):
        """uint8 per user of the reset range after a walked run: bit 0 = went through the float64 batch and round 2, bit 1 =
        finished by the last round (rg_sim_debug_walk_fate; the sampled-oracle check picks its users with it)."""
        with torch.cuda.device(self.device):
            fl = torch.zeros(self.n_users, dtype=torch.uint8, device=self.device)
            _abi.check(self.lib.rg_sim_debug_walk_fate(self._h, fl.data_ptr(), self._stream()), 'rg_sim_debug_walk_fate')
        return fl[:self.n_active]

    def omega(self):
        with torch.cuda.device(self.device):
            om = torch.empty((self.n_active, self.config.K), dtype=torch.float64,
                             device=self.device)
            _abi.check(self.lib.rg_sim_export_omega(self._h, om.data_ptr(), self._stream()),
                       'rg_sim_export_omega')
        return om

    # -- logs -------------------------------------------------------------------------------
    def sorted_log(self):
        """Device log in the reference's row order -> (rows,4) int32 tensor + int64 offsets."""
        if self.log is None:
            raise _abi.RecoGymHipError('this Simulator keeps counters only (log_capacity=0)')
        n = self.n_active
        with torch.cuda.device(self.device):
            offsets = torch.empty(n + 1, dtype=torch.int64, device=self.device)
            scratch = torch.empty(n + (n + 255) // 256 + 1, dtype=torch.int64, device=self.device)
            cnt = self.counters()
            total = cnt['organic'] + cnt['bandit'] + cnt['phantom']
            if cnt['log_dropped']:
                raise _abi.RecoGymHipError(
                    f'log overflow: capacity {self.log_capacity}, '
                    f'{cnt["log_rows"] + cnt["log_dropped"]} rows emitted')
            out = torch.empty((total, 4), dtype=torch.int32, device=self.device)
            _abi.check(self.lib.rg_sim_sort_log(self._h, offsets.data_ptr(), scratch.data_ptr(),
                                                out.data_ptr(), total, self._stream()),
                       'rg_sim_sort_log')
        return out, offsets

    def sorted_time(self, offsets, total):
        """The time column in the order of sorted_log() (float64): the clock of a NormalTimeGenerator, else the event index."""
        with torch.cuda.device(self.device):
            out = torch.empty(total, dtype=torch.float64, device=self.device)
            _abi.check(self.lib.rg_sim_sort_log_time(self._h, offsets.data_ptr(), out.data_ptr(), total, self._stream()),
                       'rg_sim_sort_log_time')
        return out

    def user_times(self):
        """Current clock of every user of the reset range (float64 device tensor)."""
        with torch.cuda.device(self.device):
            out = torch.empty(self.n_active, dtype=torch.float64, device=self.device)
            _abi.check(self.lib.rg_sim_export_time(self._h, out.data_ptr(), self._stream()), 'rg_sim_export_time')
        return out

    def sorted_aux(self, offsets, total):
        """The float64 side arrays (ps, p_click) in the order of sorted_log(); None where not kept."""
        with torch.cuda.device(self.device):
            ps = None if self.aux_ps is None else torch.empty(total, dtype=torch.float64, device=self.device)
            pc = None if self.aux_p_click is None else torch.empty(total, dtype=torch.float64, device=self.device)
            if ps is not None or pc is not None:
                _abi.check(self.lib.rg_sim_sort_log_aux(
                    self._h, offsets.data_ptr(), None if ps is None else ps.data_ptr(),
                    None if pc is None else pc.data_ptr(), total, self._stream()), 'rg_sim_sort_log_aux')
        return ps, pc

    def device_log(self):
        """The log for an off-policy evaluation on the device (evaluate_agent.evaluate_IPS & co.): a DeviceLog whose `ps` follows
        log_columns()' rule — the exact 1/P of the uniform loggers, else the float64 side array, else the row's float32 value."""
        rows, offsets = self.sorted_log()
        ps64, _ = self.sorted_aux(offsets, rows.shape[0])
        if self.uniform_ps:
            ps = 1.0 / float(self.config.num_products)
        else:
            ps = ps64
        time = self.sorted_time(offsets, rows.shape[0]) if self.time_mode else None
        return DeviceLog(rows, offsets, ps, self.first_user_id, int(self.config.num_products), time)

    def sorted_log_host(self):
        """-> ((n, 4) int32 host array of the log in the reference's row order, exact `ps` of the
        uniform policies or None)."""
        out, _ = self.sorted_log()
        uniform = None
        if self.uniform_ps:
            uniform = 1.0 / float(self.config.num_products)
        return out.cpu().numpy(), uniform

    def log_columns(self, on_device=False, chunk_rows=1 << 25, copy=True):
        """The log in the reference's row order, decoded ON THE DEVICE into the columns of the reference's DataFrame
        (SURVEY.md §8f-2): dict(t f32, u i32, is_bandit bool, v i32, a i32, c f32 (NaN on organic rows), ps f64 (NaN)).

        To the host (the default) the columns travel in chunks of `chunk_rows` rows: chunk i is decoded into one of two staging
        sets on the simulator's stream while chunk i - 1 crosses PCIe on a copy stream, straight into PINNED host buffers the
        simulator keeps between calls (allocated on the first call, grown when a log is longer).  `copy=True` (the default)
        returns arrays that OWN their memory; `copy=False` returns zero-copy NumPy views of those pinned buffers — valid only
        until the next log_columns() of this simulator, which reuses them, and page-locked for as long as anything references them
        (for callers that control that lifetime: bench.py's materialise figure, a DataFrame built and dropped at once)."""
        out, offsets = self.sorted_log()
        ps64, _ = self.sorted_aux(offsets, out.shape[0])
        n = int(out.shape[0])
        uniform = self.uniform_ps
        t_sorted = self.sorted_time(offsets, n) if self.time_mode else None

        def decode(lo, hi, dst=None):
            """columns of rows [lo, hi) as device tensors (into the staging set `dst` when given)"""
            rows = out[lo:hi]
            code = rows[:, 2]
            is_b = (code & _abi.RG_EV_BANDIT) != 0
            idx = code & _abi.RG_EV_INDEX_MASK
            zero = torch.zeros((), dtype=torch.int32, device=out.device)
            nan32 = torch.full((), float('nan'), dtype=torch.float32, device=out.device)
            nan64 = torch.full((), float('nan'), dtype=torch.float64, device=out.device)
            if uniform:
                ps_b = torch.full((), 1.0 / float(self.config.num_products), dtype=torch.float64, device=out.device)   # exact 1/P
            elif ps64 is not None:
                ps_b = ps64[lo:hi]                                  # float64 as the policy computed it
            else:
                ps_b = rows[:, 3].contiguous().view(torch.float32).to(torch.float64)
            cols = dict(
                t=(t_sorted[lo:hi] if t_sorted is not None else rows[:, 1]).to(torch.float32),
                u=rows[:, 0].contiguous(),
                is_bandit=is_b,
                v=torch.where(is_b, zero, idx),
                a=torch.where(is_b, idx, zero),
                c=torch.where(is_b, ((code & _abi.RG_EV_CLICK) != 0).to(torch.float32), nan32),
                ps=torch.where(is_b, ps_b, nan64),
            )
            if dst is not None:
                for k, v in cols.items():
                    dst[k][:hi - lo].copy_(v)
                return dst
            return cols

        with torch.cuda.device(self.device):
            if on_device:
                return decode(0, n)
            host = self._host_columns(n)
            if n == 0:
                return {k: v[:0].numpy() for k, v in host.items()}
            chunk = int(max(1, min(chunk_rows, n)))
            if getattr(self, '_copy_stream', None) is None:
                self._copy_stream = torch.cuda.Stream(device=self.device)
            cs = self._copy_stream
            stage = getattr(self, '_stage_cols', None)
            if stage is None or stage[0]['u'].shape[0] < chunk:
                stage = self._stage_cols = [{k: torch.empty(chunk, dtype=v.dtype, device=self.device) for k, v in host.items()}
                                            for _ in range(2)]
            done = [None, None]
            main = torch.cuda.current_stream(self.device)
            for i, lo in enumerate(range(0, n, chunk)):
                hi = min(lo + chunk, n)
                if done[i & 1] is not None:
                    main.wait_event(done[i & 1])        # the copy that last read this staging set has finished
                decode(lo, hi, stage[i & 1])
                ready = torch.cuda.Event()
                ready.record(main)
                cs.wait_event(ready)
                with torch.cuda.stream(cs):
                    for k, v in host.items():
                        v[lo:hi].copy_(stage[i & 1][k][:hi - lo], non_blocking=True)
                    done[i & 1] = torch.cuda.Event()
                    done[i & 1].record(cs)
            cs.synchronize()
            return {k: (v[:n].numpy().copy() if copy else v[:n].numpy()) for k, v in host.items()}

    _HOST_COLS = (('t', torch.float32), ('u', torch.int32), ('is_bandit', torch.bool), ('v', torch.int32), ('a', torch.int32),
                  ('c', torch.float32), ('ps', torch.float64))

    def _host_columns(self, n):
        """Host buffers of log_columns(): pinned (page-locked: PCIe DMA at full rate, asynchronous copies), kept between calls.
        Where the host cannot spare the memory page-locked (less than twice the need is available) they are ordinary arrays."""
        have = getattr(self, '_host_cols', None)
        if have is not None and have['u'].shape[0] >= n:
            return have
        cap = int(n * 1.02) + 4096
        need = cap * sum(torch.empty((), dtype=d).element_size() for _, d in self._HOST_COLS)
        pin = True
        try:
            avail = next(int(l.split()[1]) * 1024 for l in open('/proc/meminfo') if l.startswith('MemAvailable'))
            pin = need * 2 < avail
        except Exception:       # noqa: BLE001 — no /proc/meminfo: pin
            pass
        self._host_cols = None
        self._host_cols = {k: torch.empty(cap, dtype=d, pin_memory=pin) for k, d in self._HOST_COLS}
        self._host_cols_pinned = pin
        return self._host_cols

    def log_columns_device(self):
        """log_columns() left on the device (torch tensors), e.g. for
        agents.feature_feed.train_data_from_log_torch."""
        return self.log_columns(on_device=True)

    def raw_log(self):
        """The raw (unsorted) device log without its unused entries: (rows, 4) int32 tensor.  The user-major
        walk reserves rows per wave in chunks and marks what it leaves unused (code 0xFFFFFFFF)."""
        n = min(self.counters()['log_rows'], self.log_capacity)
        raw = self.log[:n]
        if not bool((raw[:, 2] == -1).any()):
            return raw                                  # lock-step runs leave no unused entries: a view, no copy
        # piecewise: torch's masked select mis-indexes results beyond 2^31 bytes on this stack
        step = 1 << 24
        return torch.cat([raw[i:i + step][raw[i:i + step, 2] != -1] for i in range(0, n, step)])

    @staticmethod
    def _mix64(x):
        """splitmix64 finaliser on int64 tensors (arithmetic wraps modulo 2^64; shifts made logical by masking)."""
        def shr(v, k):
            return (v >> k) & ((1 << (64 - k)) - 1)
        x = x + (-7046029254386353131)                     # 0x9E3779B97F4A7C15
        x = (x ^ shr(x, 30)) * (-4658895280553007687)      # 0xBF58476D1CE4E5B9
        x = (x ^ shr(x, 27)) * (-7723592293110705685)      # 0x94D049BB133111EB
        return x ^ shr(x, 31)

    def log_digest(self, phantom=True):
        """Order-independent checksum of the run's log: one sum (modulo 2^64) per column of the 16-byte row (u, t, code,
        ps bits) and one over the float64 `ps` side array's bit patterns, every row weighted by a 64-bit hash of its key
        (u, t) — a key occurs once per run, so values swapped between rows do not cancel.  Unused entries of a walked run
        are skipped.  `phantom`: the trailing phantom row of every user (kept beside the raw log) is folded in too, which
        costs one rg_sim_sort_log (the digest is then taken over the sorted log).  Equal digests of two runs = a checksum
        match of the same multiset of rows, whatever order the execution form emitted them in; digests of disjoint user
        shards add up (mod 2^64) to the digest of the whole run."""
        if phantom:
            rows_all, offsets = self.sorted_log()
            ps64, _ = self.sorted_aux(offsets, rows_all.shape[0])
            n = int(rows_all.shape[0])
        else:
            n = min(self.counters()['log_rows'], self.log_capacity)
            rows_all, ps64 = self.log, self.aux_ps
        chk = [0, 0, 0, 0, 0]
        step = 1 << 25
        for lo in range(0, n, step):
            rows = rows_all[lo:min(lo + step, n)].to(torch.int64)
            live = (rows[:, 2] != -1)
            w = self._mix64((rows[:, 0] << 32) | (rows[:, 1] & 0xFFFFFFFF)) * live.to(torch.int64)
            for i in range(4):
                chk[i] = (chk[i] + int((rows[:, i] * w).sum().item())) % (1 << 64)
            if ps64 is not None:
                is_b = live & ((rows[:, 2] & _abi.RG_EV_BANDIT) != 0)
                bits = ps64[lo:min(lo + step, n)].view(torch.int64)
                chk[4] = (chk[4] + int((torch.where(is_b, bits, torch.zeros_like(bits)) * w).sum().item())) % (1 << 64)
        return chk

    def rows(self):
        """Decoded host rows in the reference's order."""
        out, offsets = self.sorted_log()
        ps64, pc = self.sorted_aux(offsets, out.shape[0])
        uniform = None
        if self.uniform_ps:
            uniform = 1.0 / float(self.config.num_products)
        rows = decode_rows(out.cpu().numpy(), uniform, None if ps64 is None else ps64.cpu().numpy(),
                           None if pc is None else pc.cpu().numpy())
        if self.time_mode:         # 't' stays the event index; 'time' = the generator's clock
            import numpy.lib.recfunctions as rfn
            rows = rfn.append_fields(rows, 'time', self.sorted_time(offsets, out.shape[0]).cpu().numpy(), usemask=False)
        return rows
