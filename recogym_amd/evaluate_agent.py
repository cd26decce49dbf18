"""verify_agents — reference: recogym/evaluate_agent.py:732-750.

A/B-test a dict of agents on the same environment: every agent sees identical env draws (common
random numbers — here by construction: env draws are keyed by (seed, user id, t)), and the result
is the DataFrame [Agent, 0.025, 0.500, 0.975] of Beta CTR-posterior quantiles.

Off-policy evaluation — reference: recogym/evaluate_agent.py:753-908 (evaluate_IPS, evaluate_SNIPS,
verify_agents_IPS, verify_agents_SNIPS, evaluate_recall_at_k, verify_agents_recall_at_k).

`reco_log` is a DataFrame with the reference's columns (t, u, z, v, a, c, ps), a Simulator or a
Simulator.device_log().  Users 0 .. max(u) - 1 are evaluated (the reference's range(max(reco_log.u)):
the user with the largest id is not), each user's rows in frame order.  Where a HIP device is present,
the agent has a replay form (ope_policy_of) and the log qualifies, the rows are replayed on the device
by rg_ope_replay (the frozen LogReg policy: by rg_ope_replay_logreg, an EpsilonGreedy target: by rg_ope_replay_eg); otherwise the
host loop below runs:
the reference's loop made linear (one stable group-by instead of six frame filters per user), the same
act() calls in the same order."""
import ctypes as C
from copy import deepcopy

import numpy as np
import pandas as pd
from scipy.stats.distributions import beta

from . import _abi
from .bench_agents import evaluate_counts
from .envs.context import DefaultContext
from .envs.observation import Observation
from .envs.session import OrganicSessions


def verify_agents(env, number_of_users, agents):
    stat = {'Agent': [], '0.025': [], '0.500': [], '0.975': []}
    for agent_id in agents:
        successes, failures = evaluate_counts(deepcopy(env), agents[agent_id], number_of_users)
        stat['Agent'].append(agent_id)
        stat['0.025'].append(beta.ppf(0.025, successes + 1, failures + 1))
        stat['0.500'].append(beta.ppf(0.500, successes + 1, failures + 1))
        stat['0.975'].append(beta.ppf(0.975, successes + 1, failures + 1))
    return pd.DataFrame().from_dict(stat)


# ------------------------------------------------------------------------------------------------
# the host loop
# ------------------------------------------------------------------------------------------------
def _no_ps_all(prob_policy):
    # the reference's `prob_policy != ()`: present iff not the empty tuple (numpy >= 1.25 raises on an array != ())
    return isinstance(prob_policy, tuple) and len(prob_policy) == 0


def _frame_columns(reco_log):
    """DataFrame -> (t as the frame holds it, u int64, is_bandit, v int64 (-1 = NA), a int64, c, ps float64)."""
    u = reco_log['u'].to_numpy(dtype=np.int64)
    is_b = (reco_log['z'] == 'bandit').to_numpy()
    v = reco_log['v'].astype('Float64').to_numpy(dtype=np.float64, na_value=-1).astype(np.int64)
    a = reco_log['a'].astype('Float64').to_numpy(dtype=np.float64, na_value=-1).astype(np.int64)
    c = np.array(reco_log['c'])
    ps = np.array(reco_log['ps'], dtype=np.float64)
    return np.array(reco_log['t']), u, is_b, v, a, c, ps


def _user_ranges(u):
    """Stable group-by on u: (order, n_users = max(u), start[n_users + 1]) with the rows of user i at order[start[i]:start[i+1]]."""
    n_users = int(u.max())                     # (an empty frame raises here, as the reference's max() does)
    order = np.argsort(u, kind='stable')
    start = np.searchsorted(u[order], np.arange(n_users + 1), side='left')
    return order, n_users, start


def _host_loop(agent, reco_log, visit):
    """The reference's per-user walk; visit(u, rows, jj, prob_policy) is called at every bandit row."""
    t, u, is_b, v, a, c, ps = _frame_columns(reco_log)
    order, n_users, start = _user_ranges(u)
    cols = dict(t=t, is_b=is_b, v=v, a=a, c=c, ps=ps)
    for uid in range(n_users):
        idx = order[start[uid]:start[uid + 1]]
        session = OrganicSessions()
        agent.reset()
        for jj, i in enumerate(idx):
            if not is_b[i]:
                session.next(DefaultContext(t[i], uid), int(v[i]))
            else:
                prob_policy = agent.act(Observation(DefaultContext(t[i], uid), session), 0, False)['ps-a']
                visit(uid, idx, jj, prob_policy, cols)
                session = OrganicSessions()


def _host_ips(agent, reco_log):
    ee = []

    def visit(uid, idx, jj, prob_policy, cols):
        i = idx[jj]
        if not _no_ps_all(prob_policy):
            ee.append(cols['c'][i] * prob_policy[int(cols['a'][i])] / cols['ps'][i])
    _host_loop(agent, reco_log, visit)
    return ee


def _host_snips(agent, reco_log):
    rewards, p_ratio = [], []

    def visit(uid, idx, jj, prob_policy, cols):
        i = idx[jj]
        rewards.append(cols['c'][i])
        p_ratio.append(prob_policy[int(cols['a'][i])] / cols['ps'][i])
    _host_loop(agent, reco_log, visit)
    return rewards, p_ratio


# ------------------------------------------------------------------------------------------------
# the device replay
# ------------------------------------------------------------------------------------------------
def ope_policy_of(agent):
    """-> dict(kind, num_products, policy_seed, ouc | table | logreg) when the agent's `ps-a` has a replay form on the device, else None.
    This package's agents say so themselves (ope_policy()); the reference's own classes are duck-typed where pi does not
    depend on their MT stream: RandomAgent, and OrganicUserEventCounterAgent unless exploit_explore with epsilon > 0.  A reference
    EpsilonGreedy object never qualifies: both its explore coin and (pure_new) the greedy action its pi excludes come from MT
    streams — it stays on the host loop, whatever it wraps."""
    if hasattr(agent, 'ope_policy'):
        return agent.ope_policy()
    cfg = getattr(agent, 'config', None)
    if cfg is None or not getattr(cfg, 'with_ps_all', False):
        return None
    name = type(agent).__name__
    if name == 'EpsilonGreedy':
        return None
    if name == 'RandomAgent':
        return dict(kind=_abi.RG_POLICY_RANDOM_AGENT, num_products=int(cfg.num_products), policy_seed=0)
    if name == 'OrganicUserEventCounterAgent' and getattr(cfg, 'weight_history_function', None) is None \
            and not (cfg.exploit_explore and cfg.epsilon > 0):
        return dict(kind=_abi.RG_POLICY_ORGANIC_USER_COUNT, num_products=int(cfg.num_products), policy_seed=0,
                    ouc=dict(select_randomly=bool(cfg.select_randomly), epsilon=float(cfg.epsilon),
                             exploit_explore=bool(cfg.exploit_explore), reverse_pop=bool(getattr(cfg, 'reverse_pop', False))))
    return None


def _draws(pol):
    if pol.get('epsilon_greedy') is not None:
        return True                            # an EpsilonGreedy target always flips its coin, keyed by the event index
    o = pol.get('ouc')
    return bool(o and o['exploit_explore'] and o['epsilon'] != 0.0)


def _device_present():
    try:
        import torch
    except ImportError:
        return False
    # (a device without the library is a build error, not a reason for the host loop: load() raises)
    return torch.cuda.is_available() and _abi.load().rg_device_count() > 0


def _frame_to_device(reco_log, pol, device):
    """DataFrame -> (DeviceLog of users 0 .. max(u)-1, or None when the log must stay on the host loop)."""
    import torch
    from .sim import DeviceLog
    t, u, is_b, v, a, c, ps = _frame_columns(reco_log)
    order, n_users, start = _user_ranges(u)
    order = order[:start[-1]]                  # rows of users < max(u)
    tt = np.asarray(t, dtype=np.float64)[order]
    if _draws(pol) and not np.array_equal(tt, np.floor(tt)):
        return None                            # a NormalTimeGenerator clock: the draw key is the float t
    b = is_b[order]
    nonempty = start[1:] > start[:-1]
    if b[start[:-1][nonempty]].any():
        return None                            # a user opens with a bandit row (state left over from the previous user)
    idx = np.where(b, a[order], v[order])
    if idx.size and (idx.min() < 0 or idx.max() >= pol['num_products']):
        return None
    raw = np.zeros((order.size, 4), dtype=np.uint32)
    raw[:, 0] = u[order]
    raw[:, 1] = tt.astype(np.uint32)
    cc = np.nan_to_num(np.asarray(c, dtype=np.float64)[order]) != 0
    raw[:, 2] = idx.astype(np.uint32) | np.where(b, _abi.RG_EV_BANDIT, 0).astype(np.uint32) \
        | np.where(b & cc, _abi.RG_EV_CLICK, 0).astype(np.uint32)
    raw[:, 3] = ps[order].astype(np.float32).view(np.uint32)
    rows = torch.from_numpy(raw.view(np.int32)).to(device)
    offsets = torch.from_numpy(start.astype(np.int64)).to(device)
    return DeviceLog(rows, offsets, torch.from_numpy(np.ascontiguousarray(ps[order])).to(device), 0,
                     pol['num_products'], None)


def _as_device_log(reco_log):
    from .sim import DeviceLog, Simulator
    if isinstance(reco_log, Simulator):
        return reco_log.device_log()
    if isinstance(reco_log, DeviceLog):
        return reco_log
    return None


def _device_log_to_frame(dl):
    """A device log the replay cannot take -> the reference's DataFrame (for the host loop)."""
    from .envs.reco_env_v1 import rows_to_dataframe
    from .sim import decode_rows
    ps = dl.ps
    rows = decode_rows(dl.rows.cpu().numpy(), uniform_ps=ps if isinstance(ps, float) else None,
                       ps64=ps.cpu().numpy() if ps is not None and not isinstance(ps, float) else None)
    df = rows_to_dataframe(rows, dl.num_products)
    if dl.time is not None:
        df['t'] = dl.time.cpu().numpy().astype(np.float32)
    return df


def _masked(x, mask, step=1 << 24):
    # piecewise: torch's masked select mis-indexes results beyond 2^31 bytes on this stack (Simulator.raw_log)
    import torch
    return torch.cat([x[i:i + step][mask[i:i + step]] for i in range(0, x.shape[0], step)]) if x.shape[0] else x[:0]


def _logreg_model(lr, num_products, device):
    """A policy dict's `logreg` entry -> (RgOpeLogreg, the device tensors it points into): the model moved to the log's device,
    with the fp32 copy and the certificate's bounds the step loop uses (sim.logreg_fp32) for the argmax form."""
    import torch
    from .sim import logreg_fp32
    def put(x, np_type, t_type):            # (arrays that already are tensors, e.g. on the device, are taken as they are)
        if torch.is_tensor(x):
            return x.to(device=device, dtype=t_type).contiguous()
        return torch.as_tensor(np.ascontiguousarray(x, dtype=np_type)).to(device)
    coef_t = put(lr['coef_t'], np.float64, torch.float64)
    intercept = put(lr['intercept'], np.float64, torch.float64)
    classes = put(lr['classes'], np.int32, torch.int32)
    assert coef_t.shape == (num_products, classes.numel()) and intercept.shape == (classes.numel(),)
    keep = [coef_t, intercept, classes]
    sr = bool(lr.get('select_randomly'))
    m = _abi.RgOpeLogreg(num_products=int(num_products), n_classes=int(classes.numel()), select_randomly=int(sr), reserved=0,
                         coef_t=coef_t.data_ptr(), intercept=intercept.data_ptr(), classes=classes.data_ptr(),
                         coef32_t=None, intercept32=None, wmax=None, bmax=0.0, reserved2=0)
    if not sr and lr.get('fp32', True):
        w32, b32, wmax, bmax = logreg_fp32(coef_t, intercept)
        keep += [w32, b32, wmax]
        m.coef32_t, m.intercept32, m.wmax, m.bmax = w32.data_ptr(), b32.data_ptr(), wmax.data_ptr(), bmax
    return m, keep


def ope_replay(agent, dl, pol=None, n_users=None, stats=None, eg_out=None):
    """Replay a DeviceLog under `agent` on the device -> (ratio r = pi[a] / ps, click c as float64, sums) for the bandit rows of
    the log's first `n_users` users (default: all but the last, whose id is max(u)), in log order (device tensors);
    sums = float64 tensor (n, sum c r, sum r).  None where the agent has no replay form or the log does not qualify (a user
    that opens with a bandit row; a float clock under a policy that draws).  `stats` (a dict, frozen LogReg policies only)
    receives rg_ope_replay_logreg's workspace words: error, acts, exact (acts decided by float64 scores), rows_read.  `eg_out` (a
    dict, EpsilonGreedy targets only) receives `greedy` (uint8) and `h0` (int32) of the same bandit rows (device tensors)."""
    import torch
    pol = ope_policy_of(agent) if pol is None else pol
    if pol is None or int(pol['num_products']) != int(dl.num_products):
        return None
    n_eval = max(int(dl.offsets.numel()) - 2, 0) if n_users is None else int(n_users)
    device = dl.rows.device
    offsets = dl.offsets[:n_eval + 1].contiguous()
    lens = offsets[1:] - offsets[:-1]
    if n_eval:
        firsts = dl.rows[offsets[:-1][lens > 0], 2]
        if bool(((firsts & _abi.RG_EV_BANDIT) != 0).any()):
            return None
        if _draws(pol) and dl.time is not None:
            return None
    max_rows = int(lens.max().item()) if n_eval else 0
    lib = _abi.load()
    eg = pol.get('epsilon_greedy')
    if eg is not None and pol.get('kind') not in (_abi.RG_POLICY_RANDOM_AGENT, _abi.RG_POLICY_LAST_VIEW_TABLE):
        return None
    if pol.get('logreg') is not None:
        # the frozen LogReg policy has an entry point of its own; the model moves to the log's device once per call
        cp, keep = _logreg_model(pol['logreg'], int(pol['num_products']), device)
        size_fn, replay_fn, what = lib.rg_ope_logreg_workspace_bytes, lib.rg_ope_replay_logreg, 'rg_ope_replay_logreg'
    else:
        o = pol.get('ouc') or {}
        table = pol.get('table')
        keep = None if table is None else torch.as_tensor(np.ascontiguousarray(table, dtype=np.int32)).to(device)
        cp = _abi.RgOpePolicy(kind=int(pol['kind']), num_products=int(pol['num_products']),
                              policy_seed=int(pol.get('policy_seed') or 0) & 0xFFFFFFFFFFFFFFFF,
                              ouc_select_randomly=int(bool(o.get('select_randomly', True))),
                              ouc_exploit_explore=int(bool(o.get('exploit_explore', True))),
                              ouc_reverse_pop=int(bool(o.get('reverse_pop', False))), reserved=0,
                              ouc_epsilon=float(o.get('epsilon', 0.0)),
                              table=None if keep is None else keep.data_ptr())
        size_fn, replay_fn, what = lib.rg_ope_workspace_bytes, lib.rg_ope_replay, 'rg_ope_replay'
        if eg is not None:
            from .agents.epsilon_greedy import explore_table
            pure_new = bool(eg.get('pure_new', True))
            ce = _abi.RgOpeEg(epsilon=float(eg['epsilon']), seed=int(eg['seed']) & 0xFFFFFFFFFFFFFFFF, pure_new=int(pure_new),
                              reserved=0, prob_explore=explore_table(int(pol['num_products']), pure_new)[1])
            size_fn, what = lib.rg_ope_eg_workspace_bytes, 'rg_ope_replay_eg'
    with torch.cuda.device(device):
        need = size_fn(C.byref(cp), n_eval, max_rows)
        if need == 0:
            raise _abi.RecoGymHipError(what + ' workspace: ' + lib.rg_last_error().decode())
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        total = int(offsets[-1].item()) if n_eval else 0
        ratio = torch.empty(max(total, 1), dtype=torch.float64, device=device)
        sums = torch.empty(3, dtype=torch.float64, device=device)
        ps = dl.ps
        if ps is None:
            mode, ps_ptr, ps_const = _abi.RG_OPE_PS_ROW, None, 0.0
        elif isinstance(ps, float):
            mode, ps_ptr, ps_const = _abi.RG_OPE_PS_CONST, None, float(ps)
        else:
            mode, ps_ptr, ps_const = _abi.RG_OPE_PS_ARRAY, ps.data_ptr(), 0.0
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        if eg is not None:
            want = eg_out is not None
            greedy = torch.zeros(max(total, 1), dtype=torch.uint8, device=device) if want else None
            h0 = torch.zeros(max(total, 1), dtype=torch.int32, device=device) if want else None
            _abi.check(lib.rg_ope_replay_eg(C.byref(cp), C.byref(ce), dl.rows.data_ptr(), offsets.data_ptr(), n_eval, max_rows,
                                            mode, ps_ptr, ps_const, ratio.data_ptr(), None, sums.data_ptr(),
                                            greedy.data_ptr() if want else None, h0.data_ptr() if want else None,
                                            ws.data_ptr(), need, stream), what)
        else:
            _abi.check(replay_fn(C.byref(cp), dl.rows.data_ptr(), offsets.data_ptr(), n_eval, max_rows, mode, ps_ptr,
                                 ps_const, ratio.data_ptr(), None, sums.data_ptr(), ws.data_ptr(), need, stream), what)
        if stats is not None and pol.get('logreg') is not None:
            words = ws[:32].view(torch.int64).cpu().numpy()
            stats.update(error=int(words[0]), acts=int(words[1]), exact=int(words[2]), rows_read=int(words[3]))
        code = dl.rows[:total, 2]
        is_b = (code & _abi.RG_EV_BANDIT) != 0
        r = _masked(ratio[:total], is_b)
        c = _masked(((code & _abi.RG_EV_CLICK) != 0).to(torch.float64), is_b)
        if eg is not None and eg_out is not None:
            eg_out.update(greedy=_masked(greedy[:total], is_b), h0=_masked(h0[:total], is_b))
    return r, c, sums


def epsilon_greedy_branches(agent, reco_log):
    """-> (greedy uint8, h0 int32) device tensors over the bandit rows of a device log (a Simulator or its device_log()), in log
    order: which acts of the EpsilonGreedy `agent` were greedy, and the inner agent's action at every one of them (the `h0`
    the reference's act reports on explored acts) — rg_event has no bit for either, the replay recomputes them from the
    addressed draws.  All users of the log are covered.  None where the agent has no replay form or the log does not qualify."""
    dl = _as_device_log(reco_log)
    pol = ope_policy_of(agent)
    if dl is None or pol is None or pol.get('epsilon_greedy') is None:
        return None
    out = {}
    if ope_replay(agent, dl, pol, n_users=int(dl.offsets.numel()) - 1, eg_out=out) is None:
        return None
    return out['greedy'], out['h0']


def _device_or_none(agent, reco_log):
    """-> (r, c, sums, from_frame) from the device replay, or None (the host loop)."""
    dl = _as_device_log(reco_log)
    if dl is None and not _device_present():
        return None
    pol = ope_policy_of(agent)
    if pol is None:
        return None
    if dl is None:
        import torch
        dl = _frame_to_device(reco_log, pol, torch.device(f'cuda:{torch.cuda.current_device()}'))
        if dl is None:
            return None
        out = ope_replay(agent, dl, pol, n_users=int(dl.offsets.numel()) - 1)    # (users 0 .. max(u) - 1 only)
        return None if out is None else (*out, True)
    out = ope_replay(agent, dl, pol)
    return None if out is None else (*out, False)


def _host_of(reco_log):
    dl = _as_device_log(reco_log)
    return reco_log if dl is None else _device_log_to_frame(dl)


# ------------------------------------------------------------------------------------------------
# the reference's surface
# ------------------------------------------------------------------------------------------------
def evaluate_IPS(agent, reco_log):
    """c * pi[a] / ps for every bandit row of users 0 .. max(u)-1 whose agent returned a `ps-a` (reference
    evaluate_agent.py:753-780): a list for a DataFrame, a float64 device tensor for a device log."""
    dev = _device_or_none(agent, reco_log)
    if dev is not None:
        r, c, _, from_frame = dev
        ee = c * r
        return list(ee.cpu().numpy()) if from_frame else ee
    return _host_ips(agent, _host_of(reco_log))


def evaluate_SNIPS(agent, reco_log):
    """(rewards c, p_ratio pi[a] / ps) over the same rows (reference evaluate_agent.py:783-810); an agent without `ps-a`
    fails, as in the reference."""
    dev = _device_or_none(agent, reco_log)
    if dev is not None:
        r, c, _, from_frame = dev
        if from_frame:
            return list(c.cpu().numpy().astype(np.array(reco_log['c']).dtype)), list(r.cpu().numpy())
        return c, r
    return _host_snips(agent, _host_of(reco_log))


def _two_pass_std(x):
    """np.std(x): sqrt(sum((x - mean)^2) / n), two passes (numpy for host lists, torch for device tensors)."""
    if isinstance(x, list) or isinstance(x, np.ndarray):
        return np.mean(x), np.std(x), len(x)
    n = x.numel()
    mean = x.sum() / n
    return float(mean.item()), float((((x - mean) ** 2).sum() / n).sqrt().item()), n


def verify_agents_IPS(reco_log, agents):
    stat = {'Agent': [], '0.025': [], '0.500': [], '0.975': []}
    for agent_id in agents:
        ee = evaluate_IPS(agents[agent_id], reco_log)
        mean_ee, std_ee, n = _two_pass_std(ee)
        se_ee = std_ee / np.sqrt(n)
        stat['Agent'].append(agent_id)
        stat['0.025'].append(mean_ee - 2 * se_ee)
        stat['0.500'].append(mean_ee)
        stat['0.975'].append(mean_ee + 2 * se_ee)
    return pd.DataFrame().from_dict(stat)


def verify_agents_SNIPS(reco_log, agents):
    stat = {'Agent': [], '0.025': [], '0.500': [], '0.975': []}
    for agent_id in agents:
        rewards, p_ratio = evaluate_SNIPS(agents[agent_id], reco_log)
        if isinstance(rewards, list):
            ee = np.asarray(rewards) * np.asarray(p_ratio)
            mean_ee = np.sum(ee) / np.sum(p_ratio)
            _, std_ee, n = _two_pass_std(ee)
        else:
            ee = rewards * p_ratio
            mean_ee = float((ee.sum() / p_ratio.sum()).item())
            _, std_ee, n = _two_pass_std(ee)
        se_ee = std_ee / np.sqrt(n)
        stat['Agent'].append(agent_id)
        stat['0.025'].append(mean_ee - 2 * se_ee)
        stat['0.500'].append(mean_ee)
        stat['0.975'].append(mean_ee + 2 * se_ee)
    return pd.DataFrame().from_dict(stat)


def evaluate_recall_at_k(agent, reco_log, k=5):
    """Hits of the next organic view in the top-k of `ps-a` after an unclicked bandit row (reference
    evaluate_agent.py:832-870).  Host only: np.argpartition breaks ties in an order of its own."""
    hits = []

    def visit(uid, idx, jj, prob_policy, cols):
        i = idx[jj]
        if jj + 1 < len(idx) and not cols['is_b'][idx[jj + 1]] and not cols['c'][i]:
            top_k = set(np.argpartition(prob_policy, -k)[-k:])
            hits.append(1 if cols['v'][idx[jj + 1]] in top_k else 0)
    _host_loop(agent, _host_of(reco_log), visit)
    return hits


def verify_agents_recall_at_k(reco_log, agents, k=5):
    stat = {'Agent': [], '0.025': [], '0.500': [], '0.975': []}
    for agent_id in agents:
        hits = evaluate_recall_at_k(agents[agent_id], reco_log, k=k)
        mean_hits = np.mean(hits)
        se_hits = np.std(hits) / np.sqrt(len(hits))
        stat['Agent'].append(agent_id)
        stat['0.025'].append(mean_hits - 2 * se_hits)
        stat['0.500'].append(mean_hits)
        stat['0.975'].append(mean_hits + 2 * se_hits)
    return pd.DataFrame().from_dict(stat)
