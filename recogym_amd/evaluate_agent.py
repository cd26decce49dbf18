"""verify_agents — reference: recogym/evaluate_agent.py:732-750.

A/B-test a dict of agents on the same environment: every agent sees identical env draws (common
random numbers — here by construction: env draws are keyed by (seed, user id, t)), and the result
is the DataFrame [Agent, 0.025, 0.500, 0.975] of Beta CTR-posterior quantiles.

Off-policy evaluation — reference: recogym/evaluate_agent.py:753-908 (evaluate_IPS, evaluate_SNIPS,
verify_agents_IPS, verify_agents_SNIPS, evaluate_recall_at_k, verify_agents_recall_at_k).

`reco_log` is a DataFrame with the reference's columns (t, u, z, v, a, c, ps), a Simulator or a
Simulator.device_log().  Users 0 .. max(u) - 1 are evaluated (the reference's range(max(reco_log.u)):
the user with the largest id is not), each user's rows in frame order.  Where a HIP device is present,
the agent has a replay form (ope_policy_of; the likelihood agent's and, with `device_replay`, NnIpsAgent's and BayesianAgentVB's, which
the host confirms: ope_checked_policy_of) and the log qualifies, the rows are replayed on the device by one of the ten entry points of
the table _REPLAY_ENTRY — a plain policy, the frozen LogReg policy, the likelihood agent, the NN or the Bayes agent, each bare or under
an EpsilonGreedy wrapper (`device_models` for a model inside).
ope_replay is four steps: the log qualifies (_replay_users), the policy dict finds its entry point (_replay_target), one call,
and the workspace's head decoded once from the layouts _abi names (_replay_head).  recall@k has two device forms of its own
(recall_replay): where `ps-a` is a function of the act, the top-k set of every act that occurs is built on the host by
np.argpartition itself and the device tests membership (rg_ope_recall_hits); the sampling LogReg's softmax is ranked on the device
(rg_ope_recall_logreg) and the rows inside its margin are decided on the host.  Otherwise the host loop below runs:
the reference's loop made linear (one stable group-by instead of six frame filters per user), the same
act() calls in the same order.

The exploration study — reference: recogym/evaluate_agent.py:51-447 (evaluate_agent, build_agent_init, build_agents,
gather_agent_stats, generate_epsilons, format_epsilon, gather_exploration_stats; the plot functions are not part of this package).
`evaluate_agent` lets an agent act on a block of users, trains a copy on what the TrainingApproach lets through, swaps the copy in
and repeats.  Over agents with a device form whose training copy can reduce a device log (`train_online_from_log`: OrganicCount,
BanditCount, also inside EpsilonGreedy) every step is one device run, one pass over its log for the statistics
(rg_evolution_stats) and one filtered reduction into the tables (rg_count_train_online); only the step's counters leave the
device.  Every other agent takes the host route: the reference's loop over env.reset / step / step_offline.  Both routes are
single-process; sharding the study over ranks is out of scope.  The module itself is callable —
`recogym_amd.evaluate_agent(env, agent, ...)` is the function, as `recogym.evaluate_agent` is in the reference."""
import ctypes as C
import warnings
from collections import namedtuple
from copy import deepcopy

import numpy as np
import pandas as pd
from scipy.stats.distributions import beta

from . import _abi
from .bench_agents import evaluate_counts
from .constants import AgentInit, AgentStats, EvolutionCase, RoiMetrics, TrainingApproach  # noqa: F401
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


def ope_checked_policy_of(agent):
    """-> the policy dict of an agent whose replay form needs a host step before its result stands (`ope_policy_checked()`: the
    likelihood agent and, behind the configuration key `device_replay`, NnIpsAgent and BayesianAgentVB, whose device rules list the
    acts they cannot resolve — ope_replay confirms them with sim.replay_verify and the unit's host act), else None.  Kept apart from ope_policy_of, whose forms are exact as the device leaves them.  The dict's `logreg_poly` entry
    holds wf, wa, wk, intercept (host arrays), `weight_history` (dict(table, f32)) where the agent acts on a time-weighted view history
    (rg_ope_replay_poly_w instead of rg_ope_replay_poly), and may carry two optional keys: `expit_steps` (a step table other than
    expit_steps()) and `device_model` (sim.poly_device_model's result for the log's device: a caller that replays several logs
    under one model keeps it there instead of moving it per call; ope_replay asserts the device)."""
    hook = getattr(agent, 'ope_policy_checked', None)
    return hook() if hook is not None else None


def _draws(pol):
    if pol.get('epsilon_greedy') is not None:
        return True                            # an EpsilonGreedy target always flips its coin, keyed by the event index
    o = pol.get('ouc')
    return bool(o and o['exploit_explore'] and o['epsilon'] != 0.0)


def _weighted(pol):
    """The policy dict is the likelihood agent's on a time-weighted view history (rg_ope_replay_poly_w, never rg_ope_replay_poly)."""
    return (pol.get('logreg_poly') or {}).get('weight_history') is not None


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
    # a time-weighted target reads the clock: the truncation of the frame's own `t` values (what the reference's int16 cast makes of
    # them inside the clock range), in float64 — whole numbers up to 32767 pass ope_replay's float32 cast unchanged
    time = torch.from_numpy(np.trunc(tt)).to(device) if _weighted(pol) else None
    return DeviceLog(rows, offsets, torch.from_numpy(np.ascontiguousarray(ps[order])).to(device), 0,
                     pol['num_products'], time)


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
    """A policy dict's `logreg` entry -> (RgOpeLogreg, the device tensors it points into): the model moved to the log's device as
    the step loop's is (sim.logreg_device_model), with the fp32 copy and the certificate's bounds for the argmax form."""
    from .sim import logreg_device_model
    (coef_t, intercept, classes), fp32 = logreg_device_model(lr, num_products, device)
    m = _abi.RgOpeLogreg(num_products=int(num_products), n_classes=int(classes.numel()), select_randomly=int(bool(lr.get('select_randomly'))),
                         reserved=0, coef_t=coef_t.data_ptr(), intercept=intercept.data_ptr(), classes=classes.data_ptr(),
                         coef32_t=None, intercept32=None, wmax=None, bmax=0.0, reserved2=0)
    keep = [coef_t, intercept, classes]
    if fp32 is not None:
        w32, b32, wmax, bmax = fp32
        keep += [w32, b32, wmax]
        m.coef32_t, m.intercept32, m.wmax, m.bmax = w32.data_ptr(), b32.data_ptr(), wmax.data_ptr(), bmax
    return m, keep


def _replay_policy_of(agent):
    """-> the agent's policy dict, exact (ope_policy_of) or to be confirmed on the host (ope_checked_policy_of), else None."""
    pol = ope_policy_of(agent)
    return ope_checked_policy_of(agent) if pol is None else pol


# The one place that knows which entry point serves which policy dict: (the unit, under an EpsilonGreedy wrapper) -> (workspace-size
# function, replay function).  The unit also names the head its workspace carries (_abi.OPE_HEADS; 'plain': none).
_REPLAY_ENTRY = {
    ('plain', False): ('rg_ope_workspace_bytes', 'rg_ope_replay'),
    ('plain', True): ('rg_ope_eg_workspace_bytes', 'rg_ope_replay_eg'),
    ('logreg', False): ('rg_ope_logreg_workspace_bytes', 'rg_ope_replay_logreg'),
    ('logreg', True): ('rg_ope_logreg_workspace_bytes', 'rg_ope_replay_logreg_eg'),       # (the wrapper round a model: the plain
    ('poly', False): ('rg_ope_poly_workspace_bytes', 'rg_ope_replay_poly'),               # unit's workspace, list and head words)
    ('poly', True): ('rg_ope_poly_workspace_bytes', 'rg_ope_replay_poly_eg'),
    ('poly_w', False): ('rg_ope_poly_w_workspace_bytes', 'rg_ope_replay_poly_w'),        # (time-weighted: no wrapper form)
    ('nn', False): ('rg_ope_nn_workspace_bytes', 'rg_ope_replay_nn'),
    ('nn', True): ('rg_ope_nn_workspace_bytes', 'rg_ope_replay_nn_eg'),
    ('mlr', False): ('rg_ope_mlr_workspace_bytes', 'rg_ope_replay_mlr'),
    ('mlr', True): ('rg_ope_mlr_workspace_bytes', 'rg_ope_replay_mlr_eg'),                # (recall@k's way to the act of every row)
    ('bayes', False): ('rg_ope_bayes_workspace_bytes', 'rg_ope_replay_bayes'),
    ('bayes', True): ('rg_ope_bayes_workspace_bytes', 'rg_ope_replay_bayes_eg'),
}
# the one warning of a replay that is given up: the host refuted an unresolved act, or the device's list of them overflowed
_REFUTED = {
    'poly': 'the likelihood agent\'s replay has acts the host does not confirm (or more unresolved acts than the '
            'device lists): the off-policy evaluation takes the host loop',
    'poly_w': 'the time-weighted likelihood agent\'s replay has acts the host does not confirm (or more unresolved acts than the '
              'device lists): the off-policy evaluation takes the host loop',
    'nn': 'the replay of NnIpsAgent has acts that torch\'s forward on the host does not confirm (or more unresolved acts than the '
          'device lists): the off-policy evaluation takes the host loop',
    'mlr': 'the replay of PyTorchMLRAgent has acts that the reference\'s fp32 dot on the host does not confirm (or more unresolved acts '
           'than the device lists): the off-policy evaluation takes the host loop',
    'bayes': 'the replay of BayesianAgentVB has acts that the reference\'s expression on the host does not confirm (or more unresolved '
             'acts than the device lists): the off-policy evaluation takes the host loop',
}
# the one warning of a time-weighted replay whose log leaves the clock differences the device's table covers (head word `range`)
_CLOCK_RANGE = ('the time-weighted likelihood agent\'s replay met clock values outside [0, 32767], where the reference\'s int16 cast '
                'wraps, or a view after its act (a clock that runs backwards inside a user): the off-policy evaluation takes the host loop')
# structs: what leads the argument list (the policy or model, then the wrapper); keep: the tensors they point into; size_fn / replay_fn /
# what: the entry point and its name; unit / head: the unit and the word names of its workspace's head or None; host_act: where the unit
# lists unresolved acts, the agent's act on the host, host_act(views) -> action (sim.replay_verify), else None; weighted: (weight_history,
# host model) of the time-weighted unit, whose entry point takes d_t16 and d_act and whose acts sim.weighted_replay_verify judges
_ReplayTarget = namedtuple('_ReplayTarget', 'structs keep size_fn replay_fn what unit head host_act weighted', defaults=(None,))


def _replay_target(pol, device):
    """A policy dict -> the _ReplayTarget that replays it on `device`, or None where an EpsilonGreedy wrapper has no replay form round
    what it wraps (an inner policy that samples its act)."""
    import torch
    P = int(pol['num_products'])
    eg, host_act, weighted = pol.get('epsilon_greedy'), None, None
    if eg is not None and (pol.get('kind') not in (_abi.RG_POLICY_RANDOM_AGENT, _abi.RG_POLICY_LAST_VIEW_TABLE, _abi.RG_POLICY_LOGREG_FROZEN,
                                                    _abi.RG_POLICY_LOGREG_POLY, _abi.RG_POLICY_NN_IPS, _abi.RG_POLICY_BAYES_VB, _abi.RG_POLICY_MLR) or (pol.get('logreg') or {}).get('select_randomly')
                           or _weighted(pol)):          # (the time-weighted likelihood agent has no wrapper form either)
        return None
    if pol.get('logreg_poly') is not None:
        # the likelihood agent: the model and the step table move to the log's device as the step loop's do (sim.poly_device_model)
        # (`device_model`, optional: that function's result for this device, where the caller keeps the model there between calls)
        from . import sim
        unit, poly = 'poly', pol['logreg_poly']
        poly_host, keep = poly.get('device_model') or sim.poly_device_model(poly, P, device)
        assert all(t.device == device and t.dtype == torch.float64 for t in keep), 'device_model lies on another device than the log'
        cp = _abi.RgOpePoly(num_products=P, n_steps=int(keep[3].numel()), wf=keep[0].data_ptr(), wa=keep[1].data_ptr(),
                            wk_t=keep[2].data_ptr(), th=keep[3].data_ptr(), intercept=poly_host[3])
        host_act = lambda views: sim.poly_host_act(views, poly_host)                    # noqa: E731
        wh = poly.get('weight_history')
        if wh is not None:
            # the time-weighted form: its own unit, with the table beside the model (a float32 table widens exactly)
            unit, host_act, weighted = 'poly_w', None, (wh, poly_host)
            wtab = torch.from_numpy(np.ascontiguousarray(wh['table']).astype(np.float64)).to(device)
            cp = _abi.RgOpePolyW(model=cp, table=wtab.data_ptr(), n=int(wtab.numel()), accumulate_f32=int(bool(wh['f32'])))
            keep = [*keep, wtab]
    elif pol.get('nn_ips') is not None:
        # NnIpsAgent's argmax form: the six arrays move to the log's device as the step loop's do (sim.nn_device_model)
        from . import sim
        unit = 'nn'
        nn_host, nn, keep = sim.nn_device_model(pol['nn_ips'], device)
        assert nn.P == P, (nn.P, P)
        cp = _abi.RgOpeNn(P, nn.H, *[t.data_ptr() for t in keep])
        host_act = lambda views: sim.nn_host_act(views, P, nn_host)                     # noqa: E731
    elif pol.get('mlr') is not None and eg is not None and float(eg['epsilon']) != 0.0:
        return None      # (rg_ope_replay_mlr_eg serves the wrapper that never explores only: recall@k's way to the acts)
    elif pol.get('mlr') is not None:
        # PyTorchMLRAgent: the table moves widened and transposed, as the step loop's does (sim.mlr_device_model)
        from . import sim
        unit = 'mlr'
        mlr_host, wt = sim.mlr_device_model(pol['mlr'], device)
        assert int(wt.shape[0]) == P, (wt.shape, P)
        cp, keep = _abi.RgOpeMlr(P, wt.data_ptr()), [wt]
        host_act = lambda views: sim.mlr_host_act(views, P, mlr_host)                   # noqa: E731
    elif pol.get('bayes_vb') is not None:
        # BayesianAgentVB: the posterior samples move transposed, as the step loop's do (sim.bayes_device_model)
        from . import sim
        unit = 'bayes'
        lam, lam_t = sim.bayes_device_model(pol['bayes_vb'], P, device)
        cp, keep = _abi.RgOpeBayes(P, int(lam.shape[0]), lam_t.data_ptr()), [lam_t]
        host_act = lambda views: sim.bayes_host_act(views, P, lam)                      # noqa: E731
    elif pol.get('logreg') is not None:
        # the frozen LogReg policy: the model moves to the log's device once per call
        unit = 'logreg'
        cp, keep = _logreg_model(pol['logreg'], P, device)
    else:
        unit, o, table = 'plain', pol.get('ouc') or {}, pol.get('table')
        keep = None if table is None else torch.as_tensor(np.ascontiguousarray(table, dtype=np.int32)).to(device)
        cp = _abi.RgOpePolicy(kind=int(pol['kind']), num_products=P, policy_seed=int(pol.get('policy_seed') or 0) & 0xFFFFFFFFFFFFFFFF,
                              ouc_select_randomly=int(bool(o.get('select_randomly', True))),
                              ouc_exploit_explore=int(bool(o.get('exploit_explore', True))),
                              ouc_reverse_pop=int(bool(o.get('reverse_pop', False))), reserved=0,
                              ouc_epsilon=float(o.get('epsilon', 0.0)), table=None if keep is None else keep.data_ptr())
    structs = [cp]
    if eg is not None:
        from .agents.epsilon_greedy import explore_table
        pure_new = bool(eg.get('pure_new', True))
        structs.append(_abi.RgOpeEg(epsilon=float(eg['epsilon']), seed=int(eg['seed']) & 0xFFFFFFFFFFFFFFFF, pure_new=int(pure_new),
                                    reserved=0, prob_explore=explore_table(P, pure_new)[1]))
    lib = _abi.load()
    size_name, what = _REPLAY_ENTRY[unit, eg is not None]
    return _ReplayTarget(structs, keep, getattr(lib, size_name), getattr(lib, what), what, unit, _abi.OPE_HEADS.get(unit), host_act, weighted)


def _replay_users(dl, pol, n_users):
    """-> (n_eval, the offsets of the log's first n_eval users, the rows of the longest of them), or None where the log does not
    qualify: a user that opens with a bandit row; a float clock under a policy that draws."""
    n_eval = max(int(dl.offsets.numel()) - 2, 0) if n_users is None else int(n_users)
    offsets = dl.offsets[:n_eval + 1].contiguous()
    if not n_eval:
        return 0, offsets, 0
    lens = offsets[1:] - offsets[:-1]
    firsts = dl.rows[offsets[:-1][lens > 0], 2]
    if bool(((firsts & _abi.RG_EV_BANDIT) != 0).any()) or (_draws(pol) and dl.time is not None):
        return None
    return n_eval, offsets, int(lens.max().item())


def _replay_head(ws, names):
    """The head of a history-keeping unit's workspace after the call, read once -> dict(word name: int; `overflow`: bool)."""
    import torch
    words = ws[:_abi.OPE_HEAD_BYTES].view(torch.int64).cpu().numpy()
    return {name: bool(words[i]) if name == 'overflow' else int(words[i]) for i, name in enumerate(names)}


def ope_replay(agent, dl, pol=None, n_users=None, stats=None, eg_out=None, act_out=None):
    """Replay a DeviceLog under `agent` on the device -> (ratio r = pi[a] / ps, click c as float64, sums) for the bandit rows of
    the log's first `n_users` users (default: all but the last, whose id is max(u)), in log order (device tensors);
    sums = float64 tensor (n, sum c r, sum r).  None where the agent has no replay form or the log does not qualify (a user
    that opens with a bandit row; a float clock under a policy that draws).  `stats` (a dict, frozen LogReg policies only)
    receives the head words of the LogReg unit's workspace: error, acts, exact (acts decided by float64 scores), rows_read; under the
    likelihood agent, NnIpsAgent, BayesianAgentVB and PyTorchMLRAgent those of their units (_abi.OPE_HEADS: 'poly', 'nn', 'bayes',
    'mlr').  Their replay
    is None, after one RuntimeWarning, also where the host refutes an unresolved act or the device's list of them overflowed (under an
    EpsilonGreedy wrapper the listed acts are the GREEDY ones; with pure_new a wrong one changes pi on explored rows too).  `eg_out` (a
    dict, EpsilonGreedy targets only) receives `greedy` (uint8) and `h0` (int32) of the same bandit rows (device tensors); where it
    comes in with `per_row=True` also `greedy_rows` / `h0_rows`, one entry per row of the evaluated users (0 on organic rows).
    The time-weighted likelihood agent (rg_ope_replay_poly_w) reads the rows' clock — dl.time where the log has one, else the event
    index — and is None, after one RuntimeWarning, also where a clock value leaves [0, 32767] or a view lies after its act (`stats['range']`); `act_out` (a dict,
    that target only) receives `act_rows` (int32), the act at every bandit row, one entry per row of the evaluated users."""
    import torch
    pol = _replay_policy_of(agent) if pol is None else pol
    if pol is None or int(pol['num_products']) != int(dl.num_products):
        return None
    users = _replay_users(dl, pol, n_users)
    if users is None:
        return None
    n_eval, offsets, max_rows = users
    device = dl.rows.device
    target = _replay_target(pol, device)
    if target is None:
        return None
    wrapped = pol.get('epsilon_greedy') is not None
    with torch.cuda.device(device):
        need = target.size_fn(C.byref(target.structs[0]), n_eval, max_rows)
        if need == 0:
            raise _abi.RecoGymHipError(target.what + ' workspace: ' + _abi.load().rg_last_error().decode())
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
        # the wrapper's two optional outputs go between the sums and the workspace
        want = wrapped and eg_out is not None
        greedy = torch.zeros(max(total, 1), dtype=torch.uint8, device=device) if want else None
        h0 = torch.zeros(max(total, 1), dtype=torch.int32, device=device) if want else None
        eg_ptrs = [greedy.data_ptr() if want else None, h0.data_ptr() if want else None] if wrapped else []
        # the time-weighted unit's two: the int16 clock ahead of the ps source, the optional acts ahead of the workspace
        t16_ptrs, act_ptrs = [], []
        if target.weighted is not None:
            from .agents.feature_feed import device_clock16
            # (the `t` column of the log's frame, float32: log_columns' and _device_log_to_frame's — the host loop casts that)
            clock = (dl.time if dl.time is not None else dl.rows[:, 1]).to(torch.float32)
            t16 = device_clock16(clock)
            acts = torch.zeros(max(total, 1), dtype=torch.int32, device=device) if act_out is not None else None
            t16_ptrs, act_ptrs = [t16.data_ptr()], [None if acts is None else acts.data_ptr()]
        _abi.check(target.replay_fn(*[C.byref(x) for x in target.structs], dl.rows.data_ptr(), offsets.data_ptr(), n_eval, max_rows, *t16_ptrs,
                                    mode, ps_ptr, ps_const, ratio.data_ptr(), None, sums.data_ptr(), *eg_ptrs, *act_ptrs, ws.data_ptr(), need,
                                    C.c_void_p(torch.cuda.current_stream(device).cuda_stream)), target.what)
        if target.head is not None:
            head = _replay_head(ws, target.head)
            if stats is not None:
                stats.update(head)
            if head.get('range'):
                warnings.warn(_CLOCK_RANGE, RuntimeWarning, stacklevel=2)
                return None
            if head['error']:
                # error bits after the validation passed: a history list overflowed — the ratios are not to be trusted
                raise _abi.RecoGymHipError(f'{target.what}: the replay reported error bits {head["error"]:#x} (a view history outgrew its list)')
            if head.get('unresolved'):
                # the acts the device's rule could not resolve: confirmed on the host, or the whole replay is given up (no patching)
                from .sim import replay_verify, weighted_replay_verify
                n_listed = min(head['unresolved'], _abi.OPE_POLY_LIST_CAP)
                listed = ws[_abi.OPE_HEAD_BYTES:_abi.OPE_HEAD_BYTES + _abi.OPE_POLY_LIST_ENTRY_BYTES * n_listed]
                listed = listed.view(torch.int32).cpu().numpy().view(np.uint32).reshape(-1, 3)
                if target.weighted is not None:
                    stands = weighted_replay_verify(dl, clock, listed, head['overflow'], *target.weighted)
                else:
                    stands = replay_verify(dl, listed, head['overflow'], target.host_act)
                if not stands:
                    warnings.warn(_REFUTED[target.unit], RuntimeWarning, stacklevel=2)
                    return None
        code = dl.rows[:total, 2]
        is_b = (code & _abi.RG_EV_BANDIT) != 0
        r = _masked(ratio[:total], is_b)
        c = _masked(((code & _abi.RG_EV_CLICK) != 0).to(torch.float64), is_b)
        if target.weighted is not None and act_out is not None:
            act_out.update(act_rows=acts[:total])
        if want:
            eg_out.update(greedy=_masked(greedy[:total], is_b), h0=_masked(h0[:total], is_b))
            if eg_out.pop('per_row', False):   # (recall_replay: the two arrays as the device wrote them, one entry per row of the log)
                eg_out.update(greedy_rows=greedy[:total], h0_rows=h0[:total])
    return r, c, sums


def epsilon_greedy_branches(agent, reco_log):
    """-> (greedy uint8, h0 int32) device tensors over the bandit rows of a device log (a Simulator or its device_log()), in log
    order: which acts of the EpsilonGreedy `agent` were greedy, and the inner agent's action at every one of them (the `h0`
    the reference's act reports on explored acts) — rg_event has no bit for either, the replay recomputes them from the
    addressed draws.  All users of the log are covered.  None where the agent has no replay form or the log does not qualify."""
    dl = _as_device_log(reco_log)
    pol = _replay_policy_of(agent)
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
    pol = _replay_policy_of(agent)
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


# ------------------------------------------------------------------------------------------------
# recall@k on the device
# ------------------------------------------------------------------------------------------------
# entries (distinct keys that occur x k) of the largest sets table recall_sets builds on the host: one np.argpartition over P
# entries per key; beyond it the host loop is the better route
RECALL_TABLE_MAX = 1 << 22
_NO_FLIP = dict(epsilon=0.0, seed=0, pure_new=False)    # the wrapper that never explores: eg_threshold(0) = 0, every act greedy


def _recall_form(pol):
    """-> 'table' (the top-k set is a function of a key: rg_ope_recall_hits), 'rank' (the sampling LogReg's softmax:
    rg_ope_recall_logreg) or None (OrganicUserEventCounter: `ps-a` depends on the whole count vector; a wrapper round it)."""
    kind, eg = pol.get('kind'), pol.get('epsilon_greedy')
    if (pol.get('logreg') or {}).get('select_randomly'):
        return 'rank' if eg is None else None
    if kind in (_abi.RG_POLICY_RANDOM_AGENT, _abi.RG_POLICY_LAST_VIEW_TABLE, _abi.RG_POLICY_LOGREG_FROZEN, _abi.RG_POLICY_LOGREG_POLY,
                _abi.RG_POLICY_NN_IPS, _abi.RG_POLICY_BAYES_VB, _abi.RG_POLICY_MLR):
        return 'table'
    return None


def _recall_k_ok(pol, k):
    return isinstance(k, (int, np.integer)) and not isinstance(k, bool) and 1 <= k <= int(pol['num_products'])


def recall_sets(agent_or_pol, keys, k):
    """The top-k sets of a target whose `ps-a` is a function of a key -> int32 [len(keys), k], ascending within a key, or None
    where len(keys) * k exceeds RECALL_TABLE_MAX.  key = 2 g + explored: g the (inner) agent's act, explored the EpsilonGreedy
    flip (0 without a wrapper); a bare RandomAgent has the one key 0.  Per key the vector is built with the arithmetic and dtype
    of the agent's host act — one-hot, (1 - eps) * one-hot or * (ones / P), eps * the normalised explore vector (epsilon_pure_new:
    a zero at g), ones / P — and np.argpartition(vec, -k)[-k:] itself picks the set: NumPy's order among ties by construction."""
    pol = agent_or_pol if isinstance(agent_or_pol, dict) else _replay_policy_of(agent_or_pol)
    if pol is None or _recall_form(pol) != 'table' or not _recall_k_ok(pol, k):
        raise ValueError('recall_sets: the target has no key form of `ps-a`, or k is outside 1 .. P')
    keys = np.asarray(keys, dtype=np.int64).ravel()
    if keys.size * int(k) > RECALL_TABLE_MAX:
        return None
    P, eg = int(pol['num_products']), pol.get('epsilon_greedy')
    uniform = pol['kind'] == _abi.RG_POLICY_RANDOM_AGENT
    sets = np.empty((keys.size, int(k)), dtype=np.int32)
    for i, key in enumerate(keys):
        g, explored = int(key) >> 1, bool(int(key) & 1)
        if explored:
            vec = np.ones(P)
            if eg['pure_new']:
                vec[g] = 0.0
            vec = eg['epsilon'] * (vec / np.sum(vec))
        else:
            if uniform:
                vec = np.ones(P) / P
            else:
                vec = np.zeros(P)
                vec[g] = 1.0
            if eg is not None:
                vec = (1.0 - eg['epsilon']) * vec
        sets[i] = np.sort(np.argpartition(vec, -k)[-k:])
    return sets


def _recall_resolve(dl, offsets, lr, listed, k):
    """The rows the ranking form left inside its margin, one by one on the host: the act's view counts from the user's rows up to
    the row, the agent's own proba (logreg_frozen.view_proba), np.argpartition -> (row index in the log, hit) per listed row."""
    from .agents.logreg_frozen import view_proba
    P = int(dl.num_products)
    start = offsets.cpu().numpy()
    out = []
    for user, pos, v in listed:
        b = int(start[user])
        code = dl.rows[b:b + int(pos), 2].cpu().numpy().view(np.uint32)
        organic = (code & _abi.RG_EV_BANDIT) == 0
        views = np.bincount((code[organic] & _abi.RG_EV_INDEX_MASK).astype(np.int64), minlength=P)
        proba = view_proba(lr['coef_t'], lr['intercept'], views)
        out.append((b + int(pos), 1 if int(v) in set(np.argpartition(proba, -k)[-k:]) else 0))
    return out


def recall_replay(agent, dl, k=5, n_users=None, list_cap=None, stats=None):
    """recall@k of `agent` over a DeviceLog on the device -> (hit uint8 over the counted rows of the log's first `n_users` users
    (default: all but the last), in log order; counts int64 (counted, hits)), device tensors — or None: the host loop.  A bandit
    row is counted when it has no click and the user's next row is organic.
      table form  RandomAgent, the last-view tables, the frozen LogReg argmax, the likelihood agent, NnIpsAgent and BayesianAgentVB
                  (ope_policy_checked), and
                  EpsilonGreedy round any of them where ope_replay accepts it: the rg_ope_replay_*_eg entry points write the
                  act at every bandit row (`h0`) and the flip (`greedy`) — a bare target goes through them with epsilon = 0 —
                  recall_sets builds the set of every key that occurs and rg_ope_recall_hits tests membership.  The time-weighted
                  likelihood agent has no wrapper form: its act of every row is the plain entry point's d_act (key 2 act).
      rank form   the sampling LogReg: rg_ope_recall_logreg; the rows inside its margin are decided on the host, and a list
                  that overflowed gives the call up after one RuntimeWarning.  `list_cap`: the list's entries (default
                  _abi.OPE_RECALL_LIST_CAP); `stats` (a dict) receives the head words (_abi.OPE_RECALL_HEAD).
    None where the target has neither form (OrganicUserEventCounter, a wrapper round it), k is outside 1 .. P (before a device
    is touched: the host loop keeps NumPy's behaviour there), the log does not qualify, or the sets table would exceed
    RECALL_TABLE_MAX entries."""
    pol = _replay_policy_of(agent)
    if pol is None or not _recall_k_ok(pol, k):
        return None
    form = _recall_form(pol)
    if form is None or int(pol['num_products']) != int(dl.num_products):
        return None
    import torch
    k = int(k)
    users = _replay_users(dl, pol, n_users)
    if users is None:
        return None
    n_eval, offsets, max_rows = users
    device = dl.rows.device
    lib = _abi.load()
    with torch.cuda.device(device):
        total = int(offsets[-1].item()) if n_eval else 0
        hit = torch.empty(max(total, 1), dtype=torch.uint8, device=device)
        counts = torch.empty(2, dtype=torch.int64, device=device)
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        if form == 'rank':
            m, keep = _logreg_model(pol['logreg'], int(pol['num_products']), device)
            cap = int(list_cap) if list_cap else _abi.OPE_RECALL_LIST_CAP
            need = lib.rg_ope_recall_logreg_workspace_bytes(C.byref(m), n_eval, max_rows, cap)
            if need == 0:
                raise _abi.RecoGymHipError('rg_ope_recall_logreg workspace: ' + lib.rg_last_error().decode())
            ws = torch.empty(need, dtype=torch.uint8, device=device)
            _abi.check(lib.rg_ope_recall_logreg(C.byref(m), dl.rows.data_ptr(), offsets.data_ptr(), n_eval, max_rows, k, cap, hit.data_ptr(),
                                                counts.data_ptr(), ws.data_ptr(), need, stream), 'rg_ope_recall_logreg')
            head = _replay_head(ws, _abi.OPE_RECALL_HEAD)
            if stats is not None:
                stats.update(head)
            if head['error']:
                raise _abi.RecoGymHipError(f'rg_ope_recall_logreg: the replay reported error bits {head["error"]:#x} (a view history outgrew its list)')
            if head['overflow']:
                warnings.warn('recall@k: more rows inside the ranking margin than the device lists: the evaluation takes the host loop',
                              RuntimeWarning, stacklevel=2)
                return None
            if head['unresolved']:
                listed = ws[_abi.OPE_HEAD_BYTES:_abi.OPE_HEAD_BYTES + _abi.OPE_RECALL_LIST_ENTRY_BYTES * head['unresolved']]
                listed = listed.view(torch.int32).cpu().numpy().view(np.uint32).reshape(-1, 3)
                decided = _recall_resolve(dl, offsets, pol['logreg'], listed, k)
                at = torch.tensor([r for r, _ in decided], dtype=torch.int64, device=device)
                hit[at] = torch.tensor([h for _, h in decided], dtype=torch.uint8, device=device)
                counts[1] += sum(h for _, h in decided)
        else:
            if pol['kind'] == _abi.RG_POLICY_RANDOM_AGENT and pol.get('epsilon_greedy') is None:
                key = torch.zeros(max(total, 1), dtype=torch.int32, device=device)          # one constant vector: one key
                present, sets_pol = np.zeros(1, dtype=np.int64), pol
            else:
                if _weighted(pol):
                    # the time-weighted likelihood agent has no wrapper form: the act of every row from the plain entry point's d_act
                    sets_pol, out = pol, {}
                    if ope_replay(agent, dl, pol, n_users=n_eval, act_out=out) is None:
                        return None
                    raw = out['act_rows'] * 2
                else:
                    sets_pol = pol if pol.get('epsilon_greedy') is not None else dict(pol, epsilon_greedy=_NO_FLIP)
                    out = dict(per_row=True)
                    if ope_replay(agent, dl, sets_pol, n_users=n_eval, eg_out=out) is None:
                        return None
                    raw = out['h0_rows'] * 2 + (1 - out['greedy_rows'].to(torch.int32))
                is_b = (dl.rows[:total, 2] & _abi.RG_EV_BANDIT) != 0
                uniq = torch.unique(_masked(raw, is_b))                                       # ascending; only this leaves the device
                present = uniq.cpu().numpy().astype(np.int64)
                if not present.size:
                    present, uniq = np.zeros(1, dtype=np.int64), torch.zeros(1, dtype=torch.int32, device=device)
                key = torch.searchsorted(uniq, raw).clamp_(max=present.size - 1).to(torch.int32)   # (organic rows: never read)
                if key.numel() == 0:
                    key = torch.zeros(1, dtype=torch.int32, device=device)
            sets = recall_sets(sets_pol, present, k)
            if sets is None:
                return None
            d_sets = torch.from_numpy(sets).to(device)
            _abi.check(lib.rg_ope_recall_hits(dl.rows.data_ptr(), offsets.data_ptr(), n_eval, key.data_ptr(), int(present.size),
                                              d_sets.data_ptr(), k, hit.data_ptr(), counts.data_ptr(), stream), 'rg_ope_recall_hits')
            if stats is not None:
                stats.update(keys=int(present.size))
        hit = hit[:total]
        return _masked(hit, hit != _abi.RG_RECALL_NOT_COUNTED), counts


def _recall_device_or_none(agent, reco_log, k):
    """-> (hit, counts, from_frame) from the device, or None (the host loop): _device_or_none's rules."""
    dl = _as_device_log(reco_log)
    if dl is None and not _device_present():
        return None
    pol = _replay_policy_of(agent)
    if pol is None or not _recall_k_ok(pol, k) or _recall_form(pol) is None:
        return None
    if dl is None:
        import torch
        dl = _frame_to_device(reco_log, pol, torch.device(f'cuda:{torch.cuda.current_device()}'))
        if dl is None:
            return None
        out = recall_replay(agent, dl, k, n_users=int(dl.offsets.numel()) - 1)    # (users 0 .. max(u) - 1 only)
        return None if out is None else (*out, True)
    out = recall_replay(agent, dl, k)
    return None if out is None else (*out, False)


def _host_recall(agent, reco_log, k):
    hits = []

    def visit(uid, idx, jj, prob_policy, cols):
        i = idx[jj]
        if jj + 1 < len(idx) and not cols['is_b'][idx[jj + 1]] and not cols['c'][i]:
            top_k = set(np.argpartition(prob_policy, -k)[-k:])
            hits.append(1 if cols['v'][idx[jj + 1]] in top_k else 0)
    _host_loop(agent, _host_of(reco_log), visit)
    return hits


def evaluate_recall_at_k(agent, reco_log, k=5):
    """Hits (1 / 0) of the next organic view in the top-k of `ps-a`, for every unclicked bandit row of users 0 .. max(u)-1 that an
    organic row of the same user follows (reference evaluate_agent.py:832-870): a list of ints for a DataFrame, an int64 device
    tensor for a device log.  On the device (recall_replay) where the target's top-k set is a function of its act — built per
    act by np.argpartition itself, whose order among ties no rank rule reproduces — or a softmax the device can rank;
    OrganicUserEventCounter, whose `ps-a` is neither, and every k outside 1 .. P take the host loop."""
    dev = _recall_device_or_none(agent, reco_log, k)
    if dev is not None:
        import torch
        hit, _, from_frame = dev
        return [int(h) for h in hit.cpu().numpy()] if from_frame else hit.to(torch.int64)
    return _host_recall(agent, reco_log, k)


def verify_agents_recall_at_k(reco_log, agents, k=5):
    stat = {'Agent': [], '0.025': [], '0.500': [], '0.975': []}
    for agent_id in agents:
        hits = evaluate_recall_at_k(agents[agent_id], reco_log, k=k)
        if isinstance(hits, list):
            mean_hits = np.mean(hits)
            se_hits = np.std(hits) / np.sqrt(len(hits))
        else:
            import torch
            mean_hits, std_hits, n = _two_pass_std(hits.to(torch.float64))
            se_hits = std_hits / np.sqrt(n)
        stat['Agent'].append(agent_id)
        stat['0.025'].append(mean_hits - 2 * se_hits)
        stat['0.500'].append(mean_hits)
        stat['0.975'].append(mean_hits + 2 * se_hits)
    return pd.DataFrame().from_dict(stat)


# ------------------------------------------------------------------------------------------------
# the exploration study
# ------------------------------------------------------------------------------------------------
EpsilonDelta = .02
EpsilonSteps = 6  # Including epsilon = 0.0.
EpsilonPrecision = 2
EvolutionEpsilons = (0.00, 0.01, 0.02, 0.03, 0.05, 0.08)

_SLIDING = (TrainingApproach.SLIDING_WINDOW_ALL_DATA, TrainingApproach.SLIDING_WINDOW_EXPLORATION_DATA)
_EXPLORATION = (TrainingApproach.ALL_EXPLORATION_DATA, TrainingApproach.SLIDING_WINDOW_EXPLORATION_DATA)


def evolution_stats(u, t, is_b, a, click, num_products, phantom=None, epsilon_greedy=None, greedy=None):
    """The statistics of one evolution step from log columns (NumPy; the host form of rg_evolution_stats) -> (counts int64 [4]:
    successes, failures, successes_greedy, failures_greedy; clicks per action int64 [P]; explored bool per row).  An act is a bandit
    row that is not a phantom row.  `epsilon_greedy` = dict(epsilon, seed): the wrapper's explore flip is recomputed from the
    addressed draw of (seed, u, t); `greedy` (per row, non-zero = greedy) replaces it where the log recorded it; neither: the
    acting agent has no wrapper, no act is greedy and none explored."""
    from . import rng
    is_b = np.asarray(is_b, dtype=bool)
    act = is_b if phantom is None else is_b & ~np.asarray(phantom, dtype=bool)
    click = np.asarray(click).astype(bool) & act
    a = np.asarray(a, dtype=np.int64)
    if act.any() and (a[act].min() < 0 or a[act].max() >= num_products):
        raise ValueError(f'the log has actions outside [0, {num_products})')
    explored = np.zeros(len(is_b), dtype=bool)
    is_greedy = np.zeros(len(is_b), dtype=bool)
    if greedy is not None:
        is_greedy = act & (np.asarray(greedy) > 0)
        explored = act & ~is_greedy
    elif epsilon_greedy is not None:
        eps = float(epsilon_greedy['epsilon'])
        thr = eps / (eps + (1.0 - eps))
        for i in np.flatnonzero(act):
            _, u0, _ = rng.policy_uniforms(int(epsilon_greedy['seed']), int(u[i]), int(t[i]))
            explored[i] = not (thr <= u0)
        is_greedy = act & ~explored
    counts = np.array([click.sum(), (act & ~click).sum(), (click & is_greedy).sum(), (act & ~click & is_greedy).sum()], dtype=np.int64)
    return counts, np.bincount(a[click], minlength=int(num_products)).astype(np.int64), explored


def evolution_stats_device(dl, epsilon_greedy=None, counts=None, action_clicks=None):
    """rg_evolution_stats over a DeviceLog -> (counts int64 [4], clicks per action int64 [P], explored uint8 per row), device
    tensors; `counts` / `action_clicks` are added to where given."""
    import torch
    lib = _abi.load()
    device = dl.rows.device
    P = int(dl.num_products)
    n_users = int(dl.offsets.numel()) - 1
    eg = None
    if epsilon_greedy is not None:
        eg = _abi.RgOpeEg(epsilon=float(epsilon_greedy['epsilon']), seed=int(epsilon_greedy['seed']) & 0xFFFFFFFFFFFFFFFF,
                          pure_new=int(bool(epsilon_greedy.get('pure_new', True))), reserved=0, prob_explore=0.0)
    with torch.cuda.device(device):
        counts = torch.zeros(4, dtype=torch.int64, device=device) if counts is None else counts
        action_clicks = torch.zeros(P, dtype=torch.int64, device=device) if action_clicks is None else action_clicks
        explored = torch.zeros(max(int(dl.rows.shape[0]), 1), dtype=torch.uint8, device=device)
        need = lib.rg_evolution_workspace_bytes(P)
        ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=device)
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        _abi.check(lib.rg_evolution_stats(None if eg is None else C.byref(eg), dl.rows.data_ptr(), dl.offsets.data_ptr(), n_users, P,
                                          explored.data_ptr(), counts.data_ptr(), action_clicks.data_ptr(), ws.data_ptr(), need,
                                          stream), 'rg_evolution_stats')
    return counts, action_clicks, explored[:int(dl.rows.shape[0])]


def training_mask(training_approach, is_act, explored, samples, sliding_window_samples):
    """Which rows of a step's log train the next agent -> (mask with one entry per row, or None = every act; the running
    `samples` after the step).  is_act / explored: NumPy arrays or torch tensors, one entry per row (explored = None: the acting
    agent reports no `greedy`).  `samples` counts the acts of all steps so far; the sliding-window approaches keep the acts at
    which it is a multiple of `sliding_window_samples`, tested after the increment (evaluate_agent.py:103-114)."""
    n_acts = int(is_act.sum())
    if training_approach in (TrainingApproach.ALL_DATA, TrainingApproach.LAST_STEP):
        return None, samples + n_acts
    if training_approach not in _SLIDING and training_approach not in _EXPLORATION:
        raise AssertionError(f'Unknown Training Approach: {training_approach}')
    if n_acts == 0:
        return is_act, samples
    mask = is_act
    if training_approach in _SLIDING:
        if isinstance(is_act, np.ndarray):
            cum = np.cumsum(is_act, dtype=np.int64)
        else:
            import torch
            cum = torch.cumsum(is_act.to(torch.int64), 0)
        mask = mask & ((cum + int(samples)) % int(sliding_window_samples) == 0)
    if training_approach in _EXPLORATION:
        if explored is None:
            raise KeyError('greedy')
        mask = mask & (explored != 0)
    return mask, samples + n_acts


def _is_epsilon_greedy(agent):
    from .agents.epsilon_greedy import EpsilonGreedy
    return isinstance(agent, EpsilonGreedy)


def _trainable(agent):
    from .bench_agents import _learns
    return _learns(agent.agent if _is_epsilon_greedy(agent) else agent)


def _device_route(env, agent):
    from .envs.reco_env_v1 import device_policy_of
    if not hasattr(env, 'simulate') or getattr(env, 'agent', None) is not None or not _device_present():
        return False
    if _trainable(agent) and not hasattr(agent, 'train_online_from_log'):
        return False
    pol = device_policy_of(agent)
    # the likelihood agent's device acts need the host's confirmation of the unresolved ones, which generate_logs
    # gives and this study's device loop does not: host route
    return pol is not None and pol.get('policy') not in (_abi.RG_POLICY_LOGREG_POLY, _abi.RG_POLICY_BAYES_VB, _abi.RG_POLICY_NN_IPS, _abi.RG_POLICY_MLR)


def _new_rewards(num_products):
    rewards = {EvolutionCase.SUCCESS: [], EvolutionCase.SUCCESS_GREEDY: [], EvolutionCase.FAILURE: [],
               EvolutionCase.FAILURE_GREEDY: [], EvolutionCase.ACTIONS: dict()}
    for action_id in range(num_products):
        rewards[EvolutionCase.ACTIONS][action_id] = [0]
    return rewards


def _evolve_device(env, agent, initial_agent, n_init, num_step_users, num_steps, training_approach, window):
    import torch
    from .envs.reco_env_v1 import device_policy_of
    P = int(env.config.num_products)
    learns = _trainable(agent)
    if n_init and learns:
        _, sim = env.simulate(n_init, None, first_user_id=0, log=True)
        agent.train_online_from_log(sim.device_log(), None)
        sim.close()
    uid = n_init
    rewards = _new_rewards(P)
    training_agent = deepcopy(agent)
    samples = 0
    for _ in range(num_steps):
        if device_policy_of(agent) is None:
            raise RuntimeError(f'{type(agent).__name__} lost its device form during the study')
        eg = agent._overlay() if _is_epsilon_greedy(agent) else None
        if num_step_users:
            _, sim = env.simulate(num_step_users, agent, first_user_id=uid, log=True)
            dl = sim.device_log()
            counts, clicks, explored = evolution_stats_device(dl, eg)
            code = dl.rows[:, 2]
            is_act = ((code & _abi.RG_EV_BANDIT) != 0) & ((code & _abi.RG_EV_PHANTOM) == 0)
            mask, samples = training_mask(training_approach, is_act, explored if eg is not None else None, samples, window)
            if learns:
                training_agent.train_online_from_log(dl, mask)
            host = torch.cat([counts, clicks]).cpu().numpy()         # all that leaves the device
            sim.close()
        else:
            host = np.zeros(4 + P, dtype=np.int64)
        uid += num_step_users
        for action_id in range(P):
            rewards[EvolutionCase.ACTIONS][action_id][-1] += int(host[4 + action_id])
            rewards[EvolutionCase.ACTIONS][action_id].append(0)
        agent = training_agent
        training_agent = deepcopy(initial_agent if training_approach == TrainingApproach.LAST_STEP else agent)
        rewards[EvolutionCase.SUCCESS].append(int(host[0]))
        rewards[EvolutionCase.SUCCESS_GREEDY].append(int(host[2]))
        rewards[EvolutionCase.FAILURE].append(int(host[1]))
        rewards[EvolutionCase.FAILURE_GREEDY].append(int(host[3]))
    return rewards, agent


def _evolve_host(env, agent, initial_agent, n_init, num_step_users, num_steps, training_approach, window):
    """The reference's loop (evaluate_agent.py:59-146) over the per-user path of the environment."""
    unique_user_id = 0
    for u in range(n_init):
        env.reset(unique_user_id + u)
        agent.reset()
        new_observation, reward, done, _ = env.step(None)
        if done:
            continue            # the first organic session ended the episode: nothing to act on
        while True:
            old_observation = new_observation
            action, new_observation, reward, done, _ = env.step_offline(new_observation, reward, False)
            agent.train(old_observation, action, reward, done)
            if done:
                break
    unique_user_id += n_init
    rewards = _new_rewards(int(env.config.num_products))
    training_agent = deepcopy(agent)
    samples = 0
    for _ in range(num_steps):
        successes = successes_greedy = failures = failures_greedy = 0
        for u in range(num_step_users):
            env.reset(unique_user_id + u)
            agent.reset()
            new_observation, reward, done, _ = env.step(None)
            while not done:
                old_observation = new_observation
                action = agent.act(old_observation, reward, done)
                new_observation, reward, done, info = env.step(action['a'])
                samples += 1
                if training_approach == TrainingApproach.ALL_DATA or training_approach == TrainingApproach.LAST_STEP:
                    should_update_training_data = True
                elif training_approach == TrainingApproach.SLIDING_WINDOW_ALL_DATA:
                    should_update_training_data = samples % window == 0
                elif training_approach == TrainingApproach.ALL_EXPLORATION_DATA:
                    should_update_training_data = not action['greedy']
                elif training_approach == TrainingApproach.SLIDING_WINDOW_EXPLORATION_DATA:
                    should_update_training_data = (not action['greedy']) and samples % window == 0
                else:
                    assert False, f'Unknown Training Approach: {training_approach}'
                if should_update_training_data:
                    training_agent.train(old_observation, action, reward, done)
                if reward:
                    successes += 1
                    if 'greedy' in action and action['greedy']:
                        successes_greedy += 1
                    rewards[EvolutionCase.ACTIONS][int(action['a'])][-1] += 1
                else:
                    if 'greedy' in action and action['greedy']:
                        failures_greedy += 1
                    failures += 1
        unique_user_id += num_step_users
        agent = training_agent
        for action_id in range(env.config.num_products):
            rewards[EvolutionCase.ACTIONS][action_id].append(0)
        training_agent = deepcopy(initial_agent if training_approach == TrainingApproach.LAST_STEP else agent)
        rewards[EvolutionCase.SUCCESS].append(successes)
        rewards[EvolutionCase.SUCCESS_GREEDY].append(successes_greedy)
        rewards[EvolutionCase.FAILURE].append(failures)
        rewards[EvolutionCase.FAILURE_GREEDY].append(failures_greedy)
    return rewards, agent


def evolve(env, agent, num_initial_train_users=100, num_step_users=1000, num_steps=10,
           training_approach=TrainingApproach.ALL_DATA, sliding_window_samples=10000, route=None):
    """evaluate_agent that also hands back the agent trained last -> (rewards, agent).  `route`: 'device' / 'host' forces one
    (None: the device route where the agents have the forms it needs)."""
    initial_agent = deepcopy(agent)
    device = _device_route(env, agent) if route is None else route == 'device'
    fn = _evolve_device if device else _evolve_host
    return fn(env, agent, initial_agent, int(num_initial_train_users), int(num_step_users), int(num_steps), training_approach,
              sliding_window_samples)


def evaluate_agent(env, agent, num_initial_train_users=100, num_step_users=1000, num_steps=10,
                   training_approach=TrainingApproach.ALL_DATA, sliding_window_samples=10000):
    """Reference evaluate_agent.py:51-146 -> {EvolutionCase.SUCCESS / SUCCESS_GREEDY / FAILURE / FAILURE_GREEDY: one count per
    step, EvolutionCase.ACTIONS: {action: clicks per step, and a trailing 0}}.  `agent` is trained in place on the initial
    users, as in the reference.  One deviation: an initial user whose first organic session already ended the
    episode contributes nothing (the reference lets it act once more and can revive it)."""
    return evolve(env, agent, num_initial_train_users, num_step_users, num_steps, training_approach, sliding_window_samples)[0]


def build_agent_init(agent_key, ctor, def_args):
    return {agent_key: {AgentInit.CTOR: ctor, AgentInit.DEF_ARGS: def_args}}


def build_agents(agents_init_data, new_env_args):
    from .envs.configuration import Configuration
    agents = dict()
    for agent_key in agents_init_data:
        agent_init_data = agents_init_data[agent_key]
        ctor = agent_init_data[AgentInit.CTOR]
        def_args = agent_init_data[AgentInit.DEF_ARGS]
        agents[agent_key] = ctor(Configuration({**def_args, **new_env_args}))
    return agents


def gather_agent_stats(env, env_args, extra_env_args, agents_init_data,
                       user_samples=(100, 1000, 2000, 3000, 5000, 8000, 10000, 13000, 14000, 15000),
                       num_online_users: int = 15000, num_epochs: int = 1, epoch_with_random_reset: bool = False,
                       num_organic_offline_users: int = 100, with_cache: bool = False):
    """Reference evaluate_agent.py:185-281 over this package's test_agent -> {AgentStats.SAMPLES: user_samples,
    AgentStats.AGENTS: {name: {AgentStats.Q0_025 / Q0_500 / Q0_975: one value per sample size}}}.  The reference's
    multiprocessing.Pool is an in-process loop over the sample sizes here: every worker process would open the GPU, and the
    results do not depend on it (draws are addressed by (seed, user, t), not taken from a shared stream)."""
    from .bench_agents import test_agent
    new_env_args = {**env_args, **extra_env_args}
    new_env = deepcopy(env)
    new_env.init_gym(new_env_args)
    agents = build_agents(agents_init_data, new_env_args)
    agent_stats = {AgentStats.SAMPLES: user_samples, AgentStats.AGENTS: dict()}
    for agent_key in agents:
        stats = {AgentStats.Q0_025: [], AgentStats.Q0_500: [], AgentStats.Q0_975: []}
        for num_offline_users in user_samples:
            result = test_agent(deepcopy(new_env), deepcopy(agents[agent_key]), num_offline_users, num_online_users,
                                num_organic_offline_users, num_epochs, epoch_with_random_reset, with_cache)
            stats[AgentStats.Q0_025].append(result[1])
            stats[AgentStats.Q0_500].append(result[0])
            stats[AgentStats.Q0_975].append(result[2])
        agent_stats[AgentStats.AGENTS][agent_key] = stats
    return agent_stats


def generate_epsilons(epsilon_step=EpsilonDelta, iterations=EpsilonSteps):
    return [0.00, 0.01, 0.02, 0.03, 0.05, 0.08]


def format_epsilon(epsilon):
    return ("{0:." + f"{EpsilonPrecision}" + "f}").format(round(epsilon, EpsilonPrecision))


def gather_exploration_stats(env, env_args, extra_env_args, agents_init_data, training_approach, num_initial_train_users=1000,
                             num_step_users=1000, epsilons=EvolutionEpsilons, num_evolution_steps=6):
    """Reference evaluate_agent.py:344-447 -> {agent name: {format_epsilon(eps): the rewards dict of evaluate_agent for
    EpsilonGreedy(eps) over a copy of the agent}}.  The reference's multiprocessing.Pool is an in-process loop over the epsilon
    values here (see gather_agent_stats)."""
    from .agents.epsilon_greedy import EpsilonGreedy, epsilon_greedy_args
    from .envs.configuration import Configuration
    agent_evolution_stats = dict()
    new_env_args = {**env_args, **extra_env_args}
    new_env = deepcopy(env)
    new_env.init_gym(new_env_args)
    agents = build_agents(agents_init_data, new_env_args)
    for agent_key in agents:
        agent_stats = dict()
        for epsilon in epsilons:
            agent = EpsilonGreedy(Configuration({**epsilon_greedy_args, **new_env_args, 'epsilon': epsilon}), deepcopy(agents[agent_key]))
            rewards = evaluate_agent(deepcopy(new_env), agent, num_initial_train_users, num_step_users, num_evolution_steps,
                                     training_approach)
            assert len(rewards[EvolutionCase.SUCCESS]) == len(rewards[EvolutionCase.FAILURE]) == num_evolution_steps
            agent_stats[format_epsilon(epsilon)] = {k: rewards[k] for k in (EvolutionCase.SUCCESS, EvolutionCase.SUCCESS_GREEDY,
                                                                             EvolutionCase.FAILURE, EvolutionCase.FAILURE_GREEDY,
                                                                             EvolutionCase.ACTIONS)}
        agent_evolution_stats[agent_key] = agent_stats
    return agent_evolution_stats


class _CallableModule(type(np)):
    """`recogym_amd.evaluate_agent` is this module (verify_agents, evaluate_IPS, ... live in it) and, called, the function of
    the same name — the reference's package exports the function under the module's name."""

    def __call__(self, *args, **kwargs):
        return evaluate_agent(*args, **kwargs)


import sys as _sys  # noqa: E402

_sys.modules[__name__].__class__ = _CallableModule
