"""ctypes mirror of include/recogym_hip.h and the loader of librecogym_hip.so.

There is no CPU fallback: if the HIP library is missing or no HIP device is visible the
compute entry points raise.  (The float64 CPU restatement under oracle/ is test
infrastructure and is never imported from this package.)
"""
import ctypes as C
import os

RG_ABI_VERSION = 15

RG_STATE_ORGANIC, RG_STATE_BANDIT, RG_STATE_STOP = 0, 1, 2

RG_POLICY_UNIFORM_ENV = 0
RG_POLICY_RANDOM_AGENT = 1
RG_POLICY_ORGANIC_USER_COUNT = 2
RG_POLICY_EXTERNAL = 3
RG_POLICY_LAST_VIEW_TABLE = 4
RG_POLICY_LOGREG_FROZEN = 5
RG_POLICY_LOGREG_POLY = 6
RG_POLICY_BAYES_VB = 8      # (7 is not assigned: include/recogym_hip.h)
RG_POLICY_NN_IPS = 10       # (9 is not assigned: include/recogym_hip.h)
RG_POLICY_MLR = 12           # (11 is not assigned: include/recogym_hip.h)

RG_EV_BANDIT = 0x80000000
RG_EV_CLICK = 0x40000000
RG_EV_PHANTOM = 0x20000000
RG_EV_INDEX_MASK = 0x1FFFFFFF

(RG_CNT_ORGANIC, RG_CNT_BANDIT, RG_CNT_CLICKS, RG_CNT_PHANTOM, RG_CNT_LIVE, RG_CNT_STEP,
 RG_CNT_LOG_ROWS, RG_CNT_LOG_DROPPED, RG_CNT_EXACT_DRAWS, RG_CNT_HIST_OVERFLOW,
 RG_CNT_EXACT_SWEEPS, RG_CNT_EXACT_OVERFLOW, RG_CNT_LR_ACTS, RG_CNT_LR_ROWS, RG_CNT_LR_EXACT, RG_CNT_MEMO_HITS) = range(16)
RG_CNT_ANCHORED = 24
RG_CNT_BAD_ACTION = 25
RG_CNT_POLY_TABLE = 26
RG_CNT_POLY_UNRESOLVED = 27
RG_CNT_WH_CLOCK_RANGE = 28
RG_CNT_BAYES_SATURATED = 29
RG_CNT_N = 32

RG_ERRORS = {-1: 'RG_EINVAL', -2: 'RG_ENODEV', -3: 'RG_ENOMEM', -4: 'RG_ESTATE', -5: 'RG_ELIMIT'}


class RgConfig(C.Structure):
    """struct rg_config (include/recogym_hip.h)."""
    _fields_ = [
        ('num_products', C.c_uint32),
        ('K', C.c_uint32),
        ('seed', C.c_uint64),
        ('policy_seed', C.c_uint64),
        ('trans_cdf', (C.c_double * 3) * 2),
        ('sigma_omega_initial', C.c_double),
        ('sigma_omega', C.c_double),
        ('change_omega_for_bandits', C.c_uint32),
        ('policy', C.c_uint32),
        ('ouc_select_randomly', C.c_uint32),
        ('ouc_exploit_explore', C.c_uint32),
        ('ouc_reverse_pop', C.c_uint32),
        ('ouc_history_cap', C.c_uint32),
        ('ouc_epsilon', C.c_double),
        ('time_mode', C.c_uint32),
        ('env_kind', C.c_uint32),
        ('time_mu', C.c_double),
        ('time_sigma', C.c_double),
        ('lr_select_randomly', C.c_uint32),
        ('reserved1', C.c_uint32),
    ]


class RgEvent(C.Structure):
    """struct rg_event: one 16-byte device log row."""
    _fields_ = [('u', C.c_uint32), ('t', C.c_uint32), ('code', C.c_uint32), ('ps', C.c_float)]


class RgStepResult(C.Structure):
    """struct rg_step_result: what rg_sim_step_user reads back."""
    _fields_ = [('row', RgEvent), ('state', C.c_int32), ('has_row', C.c_int32), ('time', C.c_double), ('ps', C.c_double),
                ('p_click', C.c_double)]


RG_OPE_PS_ARRAY, RG_OPE_PS_CONST, RG_OPE_PS_ROW = 0, 1, 2


class RgOpePolicy(C.Structure):
    """struct rg_ope_policy: the target policy of rg_ope_replay."""
    _fields_ = [('kind', C.c_uint32), ('num_products', C.c_uint32), ('policy_seed', C.c_uint64),
                ('ouc_select_randomly', C.c_uint32), ('ouc_exploit_explore', C.c_uint32), ('ouc_reverse_pop', C.c_uint32),
                ('reserved', C.c_uint32), ('ouc_epsilon', C.c_double), ('table', C.c_void_p)]


class RgOpeLogreg(C.Structure):
    """struct rg_ope_logreg: the frozen LogReg model of rg_ope_replay_logreg (device arrays)."""
    _fields_ = [('num_products', C.c_uint32), ('n_classes', C.c_uint32), ('select_randomly', C.c_uint32), ('reserved', C.c_uint32),
                ('coef_t', C.c_void_p), ('intercept', C.c_void_p), ('classes', C.c_void_p),
                ('coef32_t', C.c_void_p), ('intercept32', C.c_void_p), ('wmax', C.c_void_p),
                ('bmax', C.c_float), ('reserved2', C.c_uint32)]


class RgOpePoly(C.Structure):
    """struct rg_ope_poly: the likelihood agent's model of rg_ope_replay_poly (device arrays)."""
    _fields_ = [('num_products', C.c_uint32), ('n_steps', C.c_uint32), ('wf', C.c_void_p), ('wa', C.c_void_p), ('wk_t', C.c_void_p),
                ('th', C.c_void_p), ('intercept', C.c_double)]


class RgOpePolyW(C.Structure):
    """struct rg_ope_poly_w: the likelihood agent's model plus the weight table of rg_ope_replay_poly_w (device arrays)."""
    _fields_ = [('model', RgOpePoly), ('table', C.c_void_p), ('n', C.c_uint32), ('accumulate_f32', C.c_uint32)]


class RgOpeNn(C.Structure):
    """struct rg_ope_nn: NnIpsAgent's net of rg_ope_replay_nn (device arrays, rg_sim_set_nn_ips's layout)."""
    _fields_ = [('num_products', C.c_uint32), ('num_hidden', C.c_uint32), ('w1t', C.c_void_p), ('b1', C.c_void_p), ('w2t', C.c_void_p),
                ('b2', C.c_void_p), ('w3t', C.c_void_p), ('b3', C.c_void_p)]


class RgOpeBayes(C.Structure):
    """struct rg_ope_bayes: BayesianAgentVB's posterior samples of rg_ope_replay_bayes (a device array, rg_sim_set_bayes_vb's layout)."""
    _fields_ = [('num_products', C.c_uint32), ('num_samples', C.c_uint32), ('lam_t', C.c_void_p)]


class RgOpeMlr(C.Structure):
    """struct rg_ope_mlr: PyTorchMLRAgent's table of rg_ope_replay_mlr (a device array, rg_sim_set_mlr's layout)."""
    _fields_ = [('num_products', C.c_uint32), ('wt', C.c_void_p)]


class RgOpeEg(C.Structure):
    """struct rg_ope_eg: the EpsilonGreedy wrapper of rg_ope_replay_eg."""
    _fields_ = [('epsilon', C.c_double), ('seed', C.c_uint64), ('pure_new', C.c_uint32), ('reserved', C.c_uint32),
                ('prob_explore', C.c_double)]


# What a history-keeping replay unit leaves in its workspace (include/recogym_hip.h, the prose of rg_ope_replay_logreg and of
# rg_ope_replay_poly, near lines 530-533 and 560-566): a head of OPE_HEAD_BYTES whose first int64 words are named here, in word order, per
# unit; after the likelihood agent's head its unresolved acts, up to OPE_POLY_LIST_CAP entries of three uint32 (user index, position of
# the bandit row within the user's rows, action taken).
OPE_HEAD_BYTES = 256
OPE_HEADS = {'logreg': ('error', 'acts', 'exact', 'rows_read'),
             'poly': ('error', 'acts', 'table', 'lower', 'unresolved', 'overflow', 'rows_read'),
             'poly_w': ('error', 'acts', 'table', 'lower', 'unresolved', 'overflow', 'rows_read', 'range'),
             'nn': ('error', 'acts', 'unresolved', 'overflow', 'rows_read'),
             'mlr': ('error', 'acts', 'unresolved', 'overflow', 'rows_read'),
             'bayes': ('error', 'acts', 'saturated', 'unresolved', 'overflow', 'rows_read')}
OPE_POLY_LIST_CAP = 4096
OPE_POLY_LIST_ENTRY_BYTES = 12
# recall@k (rg_ope_recall_hits, rg_ope_recall_logreg): the values of d_hit; the ranking form's head words and, from byte
# OPE_HEAD_BYTES of its workspace, its list of unresolved rows: three uint32 (user index, position of the row within the user's
# rows, next view), OPE_RECALL_LIST_CAP entries unless the call names another capacity
RG_RECALL_MISS, RG_RECALL_HIT, RG_RECALL_NOT_COUNTED, RG_RECALL_UNRESOLVED = 0, 1, 2, 3
OPE_RECALL_HEAD = ('error', 'acts', 'exact', 'rows_read', 'unresolved', 'overflow')
OPE_RECALL_LIST_CAP = 4096
OPE_RECALL_LIST_ENTRY_BYTES = 12

RG_COUNT_ORGANIC, RG_COUNT_BANDIT = 0, 1


class RgCountTables(C.Structure):
    """struct rg_count_tables: the caller-owned int64 device tables of rg_count_train / rg_count_policy."""
    _fields_ = [('num_products', C.c_uint32), ('reserved', C.c_uint32), ('co_counts', C.c_void_p), ('pulls', C.c_void_p),
                ('clicks', C.c_void_p)]


class RgOmfModel(C.Structure):
    """struct rg_omf_model: OrganicMFSquare's float64 device arrays (the model and RMSprop's square averages) of rg_omf_steps."""
    _fields_ = [('num_products', C.c_uint32), ('embed_dim', C.c_uint32), ('emb', C.c_void_p), ('w', C.c_void_p), ('bias', C.c_void_p),
                ('sq_emb', C.c_void_p), ('sq_w', C.c_void_p), ('sq_bias', C.c_void_p)]

class RgBmfModel(C.Structure):
    """struct rg_bmf_model: BanditMFSquare's float64 device arrays (the two embeddings and RMSprop's square averages) of rg_bmf_steps."""
    _fields_ = [('num_products', C.c_uint32), ('embed_dim', C.c_uint32), ('ep', C.c_void_p), ('eu', C.c_void_p), ('sq_ep', C.c_void_p),
                ('sq_eu', C.c_void_p)]


# every symbol include/recogym_hip.h declares, with its ctypes signature
_SIM = C.c_void_p
SYMBOLS = {
    'rg_last_error': (C.c_char_p, []),
    'rg_abi_version': (C.c_int, []),
    'rg_device_count': (C.c_int, []),
    'rg_sim_workspace_bytes': (C.c_size_t, [C.POINTER(RgConfig), C.c_uint64]),
    'rg_sim_create': (C.c_int, [C.POINTER(_SIM), C.POINTER(RgConfig), C.c_uint64, C.c_void_p,
                                C.c_size_t]),
    'rg_sim_destroy': (C.c_int, [_SIM]),
    'rg_sim_set_option': (C.c_int, [_SIM, C.c_char_p, C.c_int64]),
    'rg_sim_get_option': (C.c_int, [_SIM, C.c_char_p, C.POINTER(C.c_int64)]),
    'rg_sim_set_tables': (C.c_int, [_SIM, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    'rg_env0_click_thresholds': (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    'rg_sim_set_env0_tables': (C.c_int, [_SIM, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'rg_sim_set_policy_table': (C.c_int, [_SIM, C.c_void_p, C.c_void_p]),
    'rg_sim_set_policy_table_f64': (C.c_int, [_SIM, C.c_void_p, C.c_void_p]),
    'rg_sim_set_epsilon_greedy': (C.c_int, [_SIM, C.c_double, C.c_uint64, C.c_uint32, C.c_void_p, C.c_double, C.c_double]),
    'rg_sim_set_epsilon_greedy_model': (C.c_int, [_SIM, C.c_double, C.c_uint64, C.c_uint32, C.c_void_p, C.c_double, C.c_double]),
    'rg_sim_set_epsilon_greedy_model_ps': (C.c_int, [_SIM, C.c_double, C.c_uint64, C.c_uint32, C.c_void_p, C.c_double, C.c_double]),
    'rg_eg_explore_actions': (C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    'rg_sim_set_logreg': (C.c_int, [_SIM, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    'rg_sim_set_logreg_fp32': (C.c_int, [_SIM, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float]),
    'rg_sim_set_logreg_fp16': (C.c_int, [_SIM, C.c_void_p]),
    'rg_sim_set_logreg_poly': (C.c_int, [_SIM, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_uint32]),
    'rg_sim_set_bayes_vb': (C.c_int, [_SIM, C.c_void_p, C.c_uint32]),
    'rg_sim_set_nn_ips': (C.c_int, [_SIM, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    'rg_sim_set_mlr': (C.c_int, [_SIM, C.c_void_p]),
    'rg_sim_set_weight_history': (C.c_int, [_SIM, C.c_void_p, C.c_uint32, C.c_uint32]),
    'rg_sim_read_poly_unresolved': (C.c_int, [_SIM, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_void_p]),
    'rg_sim_set_log': (C.c_int, [_SIM, C.c_void_p, C.c_uint64]),
    'rg_sim_reset_users': (C.c_int, [_SIM, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]),
    'rg_sim_reseed': (C.c_int, [_SIM, C.c_uint64, C.c_uint64]),
    'rg_sim_step': (C.c_int, [_SIM, C.c_void_p, C.c_void_p]),
    'rg_sim_step_user': (C.c_int, [_SIM, C.c_int32, C.POINTER(RgStepResult), C.c_void_p]),
    'rg_sim_run': (C.c_int, [_SIM, C.c_uint32, C.c_void_p]),
    'rg_sim_read_counters': (C.c_int, [_SIM, C.POINTER(C.c_int64), C.c_void_p]),
    'rg_sim_set_profiling': (C.c_int, [_SIM, C.c_int]),
    'rg_sim_get_profile': (C.c_int, [_SIM, C.POINTER(C.c_double)]),
    'rg_sim_export_state': (C.c_int, [_SIM, C.c_void_p, C.c_void_p]),
    'rg_sim_export_omega': (C.c_int, [_SIM, C.c_void_p, C.c_void_p]),
    'rg_sim_sort_log': (C.c_int, [_SIM, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                  C.c_void_p]),
    'rg_sim_set_log_aux': (C.c_int, [_SIM, C.c_void_p, C.c_void_p]),
    'rg_sim_sort_log_aux': (C.c_int, [_SIM, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                      C.c_void_p]),
    'rg_sim_set_log_time': (C.c_int, [_SIM, C.c_void_p]),
    'rg_sim_sort_log_time': (C.c_int, [_SIM, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    'rg_sim_export_time': (C.c_int, [_SIM, C.c_void_p, C.c_void_p]),
    'rg_sim_debug_set_omega': (C.c_int, [_SIM, C.c_void_p, C.c_void_p]),
    'rg_sim_debug_set_uniforms': (C.c_int, [_SIM, C.c_void_p]),
    'rg_sim_debug_set_row_base': (C.c_int, [_SIM, C.c_uint64]),
    'rg_sim_debug_uncertified': (C.c_int, [_SIM, C.c_void_p, C.c_void_p]),
    'rg_sim_debug_walk_fate': (C.c_int, [_SIM, C.c_void_p, C.c_void_p]),
    'rg_sim_debug_click_decisions': (C.c_int, [_SIM, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'rg_sim_debug_set_history': (C.c_int, [_SIM, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    'rg_sim_debug_ouc_acts': (C.c_int, [_SIM, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'rg_sim_debug_poly_acts': (C.c_int, [_SIM, C.c_void_p, C.c_void_p, C.c_void_p]),
    'rg_sim_debug_bayes_acts': (C.c_int, [_SIM, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'rg_sim_debug_nn_acts': (C.c_int, [_SIM, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'rg_sim_debug_mlr_acts': (C.c_int, [_SIM, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'rg_sim_debug_logreg_acts': (C.c_int, [_SIM, C.c_void_p, C.c_void_p]),
    'rg_sim_debug_set_timed_history': (C.c_int, [_SIM, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    'rg_sim_debug_weighted_acts': (C.c_int, [_SIM, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                             C.c_void_p]),
    'rg_weighted_feed_workspace_bytes': (C.c_size_t, [C.c_uint64, C.c_uint32]),
    'rg_weighted_feed': (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                   C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'rg_ope_workspace_bytes': (C.c_size_t, [C.POINTER(RgOpePolicy), C.c_uint64, C.c_uint32]),
    'rg_ope_replay': (C.c_int, [C.POINTER(RgOpePolicy), C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p,
                                C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'rg_ope_logreg_workspace_bytes': (C.c_size_t, [C.POINTER(RgOpeLogreg), C.c_uint64, C.c_uint32]),
    'rg_ope_replay_logreg': (C.c_int, [C.POINTER(RgOpeLogreg), C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                       C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                       C.c_void_p]),
    'rg_ope_poly_workspace_bytes': (C.c_size_t, [C.POINTER(RgOpePoly), C.c_uint64, C.c_uint32]),
    'rg_ope_replay_poly': (C.c_int, [C.POINTER(RgOpePoly), C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                     C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.c_void_p]),
    'rg_ope_poly_w_workspace_bytes': (C.c_size_t, [C.POINTER(RgOpePolyW), C.c_uint64, C.c_uint32]),
    # (rg_ope_replay_poly's arguments with d_t16 ahead of ps_mode and d_act ahead of the workspace)
    'rg_ope_replay_poly_w': (C.c_int, [C.POINTER(RgOpePolyW), C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32,
                                       C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                       C.c_void_p]),
    'rg_ope_eg_workspace_bytes': (C.c_size_t, [C.POINTER(RgOpePolicy), C.c_uint64, C.c_uint32]),
    'rg_ope_replay_eg': (C.c_int, [C.POINTER(RgOpePolicy), C.POINTER(RgOpeEg), C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                   C.c_uint32, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_size_t, C.c_void_p]),
    'rg_ope_replay_logreg_eg': (C.c_int, [C.POINTER(RgOpeLogreg), C.POINTER(RgOpeEg), C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                          C.c_uint32, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'rg_ope_replay_poly_eg': (C.c_int, [C.POINTER(RgOpePoly), C.POINTER(RgOpeEg), C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                        C.c_uint32, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    **{name.format(unit): (res, [C.POINTER(model), *args])
       for unit, model in (('nn', RgOpeNn), ('bayes', RgOpeBayes))
       for name, res, args in (
           ('rg_ope_{}_workspace_bytes', C.c_size_t, [C.c_uint64, C.c_uint32]),
           # (after the model: rg_ope_replay_poly's / rg_ope_replay_poly_eg's arguments)
           ('rg_ope_replay_{}', C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_double, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
           ('rg_ope_replay_{}_eg', C.c_int, [C.POINTER(RgOpeEg), C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p,
                                             C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_size_t, C.c_void_p]))},
    'rg_ope_mlr_workspace_bytes': (C.c_size_t, [C.POINTER(RgOpeMlr), C.c_uint64, C.c_uint32]),
    'rg_ope_replay_mlr': (C.c_int, [C.POINTER(RgOpeMlr), C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_double,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'rg_ope_replay_mlr_eg': (C.c_int, [C.POINTER(RgOpeMlr), C.POINTER(RgOpeEg), C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                       C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_size_t, C.c_void_p]),
    'rg_ope_recall_hits': (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    'rg_ope_recall_logreg_workspace_bytes': (C.c_size_t, [C.POINTER(RgOpeLogreg), C.c_uint64, C.c_uint32, C.c_uint32]),
    'rg_ope_recall_logreg': (C.c_int, [C.POINTER(RgOpeLogreg), C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'rg_count_workspace_bytes': (C.c_size_t, []),
    'rg_count_train': (C.c_int, [C.POINTER(RgCountTables), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_size_t,
                                 C.c_void_p]),
    'rg_count_policy': (C.c_int, [C.POINTER(RgCountTables), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'rg_evolution_workspace_bytes': (C.c_size_t, [C.c_uint32]),
    'rg_evolution_stats': (C.c_int, [C.POINTER(RgOpeEg), C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'rg_count_online_workspace_bytes': (C.c_size_t, [C.c_uint32, C.c_uint64]),
    'rg_count_train_online': (C.c_int, [C.POINTER(RgCountTables), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_size_t, C.c_void_p]),
    'rg_omf_pairs_workspace_bytes': (C.c_size_t, [C.c_uint64, C.c_uint64]),
    'rg_omf_pairs': (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p,
                               C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'rg_omf_limits': (C.c_int, [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    'rg_omf_steps_workspace_bytes': (C.c_size_t, [C.c_uint32, C.c_uint32]),
    'rg_omf_steps': (C.c_int, [C.POINTER(RgOmfModel), C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                               C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'rg_bmf_samples_workspace_bytes': (C.c_size_t, [C.c_uint64, C.c_uint64]),
    'rg_bmf_samples': (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p,
                                 C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'rg_bmf_limits': (C.c_int, [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    'rg_bmf_steps_workspace_bytes': (C.c_size_t, [C.c_uint32, C.c_uint32]),
    'rg_bmf_steps': (C.c_int, [C.POINTER(RgBmfModel), C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                               C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
}

LIB_NAME = 'librecogym_hip.so'
_lib = None


def lib_path():
    # RECOGYM_HIP_LIB: another build of the same source (A/B measurements of compile-time switches)
    return os.environ.get('RECOGYM_HIP_LIB') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc', LIB_NAME)


class RecoGymHipError(RuntimeError):
    pass


def load():
    """Load librecogym_hip.so (built by __graft_entry__.build()); raise loudly if absent."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise RecoGymHipError(
            f'{path} is missing: build it with `python -c "import __graft_entry__ as g; '
            f'g.build()"` (hipcc --offload-arch=gfx950). There is no CPU fallback.')
    lib = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)       # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    if lib.rg_abi_version() != RG_ABI_VERSION:
        raise RecoGymHipError(f'ABI mismatch: library {lib.rg_abi_version()} != {RG_ABI_VERSION}')
    _lib = lib
    return lib


def check(rc, what=''):
    if rc < 0:
        lib = load()
        msg = lib.rg_last_error()
        raise RecoGymHipError(
            f'{what}: {RG_ERRORS.get(rc, rc)}: {msg.decode() if msg else ""}')
    return rc
