/*
 * recogym_hip.h — C ABI of librecogym_hip.so, the MI355X-native reco-gym-v1 step loop.
 *
 * The reference has no FFI: its boundary is the duck-typed Python class surface of
 * recogym/envs/abstract.py + reco_env_v1.py.  This header is the boundary a
 * native replacement of that path exports; every entry point cites the reference method(s)
 * whose work it takes over.  The Python mirror of the reference classes that binds these
 * symbols with ctypes lives in recogym_amd/ (see INTEGRATION.md for the stub a reference
 * maintainer would add).
 *
 * Conventions
 *   - plain C types only; device buffers are passed as raw pointers owned by the caller
 *     (PyTorch-ROCm tensors in the Python host), streams as `void*` (a hipStream_t);
 *   - every function returns 0 on success or a negative RG_E* code; rg_last_error() holds the
 *     message of the last failure on the calling thread;
 *   - nothing here allocates caller-visible memory: the caller sizes one workspace with
 *     rg_sim_workspace_bytes() and hands it to rg_sim_create();
 *   - no entry point synchronises the device except rg_sim_read_counters(), rg_sim_run() (a
 *     host loop that polls the live-user count) and rg_sim_destroy();
 *   - a handle is thread-compatible (one handle per thread / per GPU), not thread-safe;
 *   - there is NO CPU fallback: without a HIP device every compute entry point fails with
 *     RG_ENODEV.  The float64 CPU restatement used by the tests is a different library
 *     (oracle/, test infrastructure only).
 */
#ifndef RECOGYM_HIP_H
#define RECOGYM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* v8: the entry point of the 8-bit LogReg screen (v6; opt-in, measured slower than the fp16 screen) is gone;
 * options pipe_mode and resident_grid are gone, pipe_groups takes 0 or 1. */
/* v9 (additive): rg_count_train / rg_count_policy (the OrganicCount and BanditCount agents' tables from a sorted device log) and
 * rg_sim_set_policy_table_f64 (RG_POLICY_LAST_VIEW_TABLE with a float64 `ps` table). */
/* v10 (additive): rg_ope_logreg_workspace_bytes / rg_ope_replay_logreg (the off-policy replay of the frozen LogReg policy). */
/* v11 (additive): rg_sim_set_epsilon_greedy (the EpsilonGreedy overlay of the lock-step kernels), rg_eg_explore_actions (its table
 * search on caller-supplied uniforms) and rg_ope_eg_workspace_bytes / rg_ope_replay_eg (the off-policy replay of an EpsilonGreedy
 * target). */
/* v12 (additive): rg_evolution_workspace_bytes / rg_evolution_stats (the counters of one step of the epsilon-greedy evolution study)
 * and rg_count_online_workspace_bytes / rg_count_train_online (the count agents' train calls under a row filter). */
/* v13 (additive): RG_POLICY_LOGREG_POLY with rg_sim_set_logreg_poly, rg_sim_read_poly_unresolved and rg_sim_debug_poly_acts (the
 * likelihood agent LogregPolyAgent in the step loop), and the counters RG_CNT_POLY_TABLE / RG_CNT_POLY_UNRESOLVED. */
/* v14 (additive): rg_ope_poly_workspace_bytes / rg_ope_replay_poly (the off-policy replay of the likelihood agent). */
/* v14, additive since: rg_sim_set_epsilon_greedy_model (the EpsilonGreedy overlay round the frozen LogReg argmax and the likelihood
 * agent in the step loop) and rg_ope_replay_logreg_eg / rg_ope_replay_poly_eg (the off-policy replay of such a wrapper).  New
 * symbols only: nothing an existing caller sees has changed, and the version stays 14. */
/* v14, additive since: rg_sim_set_weight_history, rg_sim_debug_set_timed_history, rg_sim_debug_weighted_acts and the counter
 * RG_CNT_WH_CLOCK_RANGE (the likelihood agent's act on a time-weighted view history), and rg_weighted_feed_workspace_bytes /
 * rg_weighted_feed (its training features from a sorted device log). */
/* v14, additive since: RG_POLICY_BAYES_VB with rg_sim_set_bayes_vb and rg_sim_debug_bayes_acts (the posterior-sample act of
 * BayesianAgentVB in the step loop) and the counter RG_CNT_BAYES_SATURATED; its unresolved acts share the likelihood agent's list,
 * counter and reader (RG_CNT_POLY_UNRESOLVED, rg_sim_read_poly_unresolved). */
/* v14, additive since: RG_POLICY_NN_IPS with rg_sim_set_nn_ips and rg_sim_debug_nn_acts (the three-layer perceptron act of NnIpsAgent
 * in the step loop, the first argmax policy whose logged propensity is a model output) and the flag RG_NN_UNRESOLVED; its unresolved
 * acts share the same list, counter and reader. */
/* v14, additive since: rg_ope_nn_workspace_bytes / rg_ope_replay_nn / rg_ope_replay_nn_eg and rg_ope_bayes_workspace_bytes /
 * rg_ope_replay_bayes / rg_ope_replay_bayes_eg (the off-policy replay of those two agents, plain and under EpsilonGreedy). */
/* v14, additive since: rg_sim_set_epsilon_greedy_model_ps (the EpsilonGreedy overlay round NnIpsAgent and BayesianAgentVB in the
 * step loop; the greedy row of the former logs (1 - epsilon) times the model's own propensity). */
/* v14, additive since: RG_POLICY_MLR with rg_sim_set_mlr and rg_sim_debug_mlr_acts (the argmax act of PyTorchMLRAgent in the step
 * loop) and the flag RG_MLR_UNRESOLVED; its unresolved acts share the same list, counter and reader; and rg_ope_mlr_workspace_bytes /
 * rg_ope_replay_mlr / rg_ope_replay_mlr_eg (its off-policy replay). */
/* v15: rg_sim_debug_logreg_acts (the frozen LogReg's act kernels on placed histories). */
/* v15, additive since: rg_ope_poly_w_workspace_bytes / rg_ope_replay_poly_w (the off-policy replay of the likelihood agent on a
 * time-weighted view history).  New symbols only: the version stays 15. */
/* v15, additive since: rg_omf_pairs_workspace_bytes / rg_omf_pairs / rg_omf_limits / rg_omf_steps_workspace_bytes / rg_omf_steps
 * (OrganicMFSquare's training from a sorted device log: the pair list of every optimiser step, and the chain of RMSprop steps in
 * one launch).  New symbols only: the version stays 15. */
/* v15, additive since: rg_bmf_samples_workspace_bytes / rg_bmf_samples / rg_bmf_limits / rg_bmf_steps_workspace_bytes / rg_bmf_steps
 * and struct rg_bmf_model (BanditMFSquare's training from a sorted device log). */
#define RG_ABI_VERSION 15

/* error codes */
#define RG_OK 0
#define RG_EINVAL (-1)   /* bad argument / configuration */
#define RG_ENODEV (-2)   /* no HIP device, or a HIP runtime error */
#define RG_ENOMEM (-3)   /* workspace / log buffer too small */
#define RG_ESTATE (-4)   /* call sequence error (e.g. step before reset_users) */
#define RG_ELIMIT (-5)   /* a hard limit was hit (max steps, log overflow) */

/* Markov states — recogym/envs/abstract.py:41-43 */
#define RG_STATE_ORGANIC 0
#define RG_STATE_BANDIT 1
#define RG_STATE_STOP 2

/* policies that run on the device — the `agent` argument of generate_logs
 * (abstract.py:241-254) */
#define RG_POLICY_UNIFORM_ENV 0   /* agent=None: uniform action from the ENV stream, abstract.py:209-221 */
#define RG_POLICY_RANDOM_AGENT 1  /* RandomAgent, agents/random_agent.py:22-33 */
#define RG_POLICY_ORGANIC_USER_COUNT 2 /* OrganicUserEventCounterAgent, agents/organic_user_count.py:45-96 */
#define RG_POLICY_EXTERNAL 3      /* actions supplied by the caller per step (gym.Env.step, abstract.py:123) */
#define RG_POLICY_LAST_VIEW_TABLE 4 /* frozen policy a = table[last product viewed]: BanditMFSquare inference,
                                     agents/bandit_mf.py:52-87 (argmax_a <E_p[a], E_u[lpv]> is a P-entry table) */
#define RG_POLICY_LOGREG_FROZEN 5 /* frozen LogregMulticlassIpsAgent (select_randomly = False), agents/logreg_ips.py:60-87:
                                     a = classes[argmax_c (sum_p views[p] W[c][p] + b[c])] over the user's view counts
                                     (ViewsFeaturesProvider, agents/abstract.py:316-409), ps = 1 */
#define RG_POLICY_LOGREG_POLY 6   /* frozen LogregPolyAgent (the likelihood agent), agents/logreg_poly.py:143-167: a = the first index of
                                     the maximum of predict_proba[:, 1] = expit(decision) over one decision per action, on the
                                     polynomial features of the user's view counts — rg_sim_set_logreg_poly has the contract; ps = 1.
                                     Routed like RG_POLICY_LOGREG_FROZEN (lock-step / rounds, no tail kernel). */
/* (7 is not assigned and stays refused as an unknown policy: the recorded create plan, tests/golden/create_plan.json, holds
 * policy 7 as its refused policy number) */
#define RG_POLICY_BAYES_VB 8      /* frozen BayesianAgentVB, agents/bayesian_poly_vb.py:71-91: a = the first index of the maximum over the
                                     actions of mean_s expit(sum_p views[p] Lambda[s][p P + a]) over the posterior samples s —
                                     rg_sim_set_bayes_vb has the contract; ps = 1.  Routed like RG_POLICY_LOGREG_POLY. */
/* (9 is not assigned either and stays refused: tests/test_bayes_vb_host.py holds policy 9 as a refused number) */
#define RG_POLICY_NN_IPS 10       /* frozen NnIpsAgent, agents/nn_ips.py:43-63,111-137: prob = softmax(W3 sigmoid(W2 sigmoid(W1 x + b1) + b2) + b3)
                                     over the user's view counts x, a = the first index of the maximum, ps = prob[a] (not 1) —
                                     rg_sim_set_nn_ips has the contract.  Routed like RG_POLICY_LOGREG_POLY. */
/* (11 is not assigned either and stays refused: tests/test_nn_ips_host.py holds policy 11 as a refused number) */
#define RG_POLICY_MLR 12          /* frozen PyTorchMLRAgent, agents/pytorch_mlr.py:30-32,59-84: a = the first index of the maximum of x W^T
                                     over the user's view counts x (fp32), ps = 1 — rg_sim_set_mlr has the contract.  Routed like
                                     RG_POLICY_LOGREG_POLY. */

/*
 * Everything the step loop needs from `env.config` (a Configuration built from env_1_args,
 * reco_env_v1.py:18-29 + abstract.py:20-31) and from the agent's config.  POD, no pointers.
 */
typedef struct rg_config {
    uint32_t num_products;          /* P   — config.num_products */
    uint32_t K;                     /* K   — config.K */
    uint64_t seed;                  /* config.random_seed + epoch — abstract.py:59-62 */
    uint64_t policy_seed;           /* the agent's config.random_seed (env seed for UNIFORM_ENV) */
    /* Normalised cumulative transition rows, i.e. what RandomState.choice(3, p=T[s]) compares
     * its uniform against: cdf = cumsum(T[s]); cdf /= cdf[-1]   (reco_env_v1.py:54-61,87).
     * Row 0 = organic, row 1 = bandit.  Computed on the host in float64 exactly as numpy does. */
    double trans_cdf[2][3];
    double sigma_omega_initial;     /* reco_env_v1.py:80 */
    double sigma_omega;             /* reco_env_v1.py:96 */
    uint32_t change_omega_for_bandits; /* reco_env_v1.py:95 */
    uint32_t policy;                /* RG_POLICY_* */
    /* OrganicUserEventCounter parameters (organic_user_count_args, organic_user_count.py:7-27) */
    uint32_t ouc_select_randomly;
    uint32_t ouc_exploit_explore;
    uint32_t ouc_reverse_pop;
    uint32_t ouc_history_cap;       /* max organic views kept per user on the device (0 = default) */
    double ouc_epsilon;
    /* time generator (envs/features/time/): 0 = DefaultTimeGenerator (t = event index, default_time_generator.py:10-13);
     * 1 = NormalTimeGenerator (normal_time_generator.py:23-26): event n of a user happens at T_n = sum_{i<n} |mu + sigma z_i|,
     * and the drift that follows it is scaled by T_{n+1} - T_n (reco_env_v1.py:89-98).  Lock-step execution only. */
    uint32_t time_mode;
    uint32_t env_kind;              /* 0 = reco-gym-v1 (the latent-factor model); 1 = reco-gym-v0 (reco_env_v0.py: the cluster toy model,
                                     * every draw a table look-up — rg_sim_set_env0_tables instead of rg_sim_set_tables; K is ignored,
                                     * pass 1).  Lock-step execution only. */
    double time_mu;                 /* config.normal_time_mu (default 0) */
    double time_sigma;              /* config.normal_time_sigma (default 1) */
    /* RG_POLICY_LOGREG_FROZEN with select_randomly = True (logreg_ips.py:61-72): the action is SAMPLED from predict_proba —
     * softmax of the decision function, rng.choice(num_products, p = proba), ps = proba[action] — with the second policy
     * uniform of the event (words 2,3).  Needs every product as a class (classes = 0 .. P-1) and P <= 1024; lock-step only. */
    uint32_t lr_select_randomly;
    uint32_t reserved1;
} rg_config;

/*
 * One emitted log row, 16 bytes — the device-side form of one row of the DataFrame that
 * generate_logs builds (abstract.py:256-290,318-327).
 *   code bit 31 : z  (0 = organic, 1 = bandit)
 *   code bit 30 : c  (click; bandit rows only)
 *   code bit 29 : phantom (the trailing never-drawn bandit row, abstract.py:311-316)
 *   code bits 0..28 : v (organic) or a (bandit)
 */
typedef struct rg_event {
    uint32_t u;      /* user id */
    uint32_t t;      /* per-user event index == DefaultTimeGenerator time */
    uint32_t code;
    float ps;        /* propensity of the logged action (NaN on organic rows) */
} rg_event;

#define RG_EV_BANDIT 0x80000000u
#define RG_EV_CLICK 0x40000000u
#define RG_EV_PHANTOM 0x20000000u
#define RG_EV_INDEX_MASK 0x1FFFFFFFu

/* counters returned by rg_sim_read_counters */
#define RG_CNT_ORGANIC 0        /* organic rows */
#define RG_CNT_BANDIT 1         /* real bandit rows (phantom excluded) */
#define RG_CNT_CLICKS 2         /* sum of c over bandit rows — bench_agents.py:203-206 */
#define RG_CNT_PHANTOM 3        /* phantom rows (one per finished non-organic-only user) */
#define RG_CNT_LIVE 4           /* users not yet in state stop */
#define RG_CNT_STEP 5           /* Markov transitions performed per user so far (== current t) */
#define RG_CNT_LOG_ROWS 6       /* rows written to the log buffer */
#define RG_CNT_LOG_DROPPED 7    /* rows that did not fit (capacity exceeded) */
#define RG_CNT_EXACT_DRAWS 8    /* organic draws resolved by the float64 path */
#define RG_CNT_HIST_OVERFLOW 9  /* views DROPPED from a full view-history row (OrganicUserEventCounter, the frozen LogReg, the likelihood
                                   agent).  A row has hist_cap = ((ouc_history_cap or 255) + 1 + 15) & ~15 entries (the read-only option
                                   "hist_cap": 15 -> 16, 16 -> 32, 31 -> 32, 47 -> 48, 0 -> 256) and keeps keep = hist_cap - 1 distinct
                                   products.  A view of a kept product raises its count and the row's view total; a view of a new
                                   product with fewer than `keep` kept is inserted in ascending product order, total + 1; a view of a
                                   new product at `keep` kept leaves the row and the total as they are and adds ONE to this counter —
                                   per dropped view, not per user — and the policy acts on the kept counts from then on.  The organic
                                   row is logged either way.  Zero means every act of the run saw its user's whole history; a caller
                                   that needs that runs again with a larger ouc_history_cap when it is not (RecoEnv1.simulate does).
                                   Held on every run form by tests/test_history_capacity.py */
#define RG_CNT_EXACT_SWEEPS 10  /* float64 product sweeps those draws needed (== EXACT_DRAWS unless sigma_omega = 0,
                                   where a user's float64 sums are taken once and reused) */
#define RG_CNT_EXACT_OVERFLOW 11 /* uncertified draws beyond what the float64 resolve scratch covers in a step (25 % of the
                                   live users): the run is incomplete and must be reported — never reached by the
                                   reference's parameter ranges */
#define RG_CNT_LR_ACTS 12       /* RG_POLICY_LOGREG_FROZEN: acts computed (one per change of a user's view history that an event needed) */
#define RG_CNT_LR_ROWS 13       /* ... and the coef^T rows (viewed products) those acts read */
#define RG_CNT_LR_EXACT 14      /* ... acts the fp32 scores could not certify (decided by float64 scores) */
#define RG_CNT_MEMO_HITS 15     /* sigma_omega = 0, user-major walk: organic draws answered by the user's memo of certified draws */
#define RG_CNT_ANCHORED 24      /* sigma_omega = 0 walk: the part of RG_CNT_EXACT_DRAWS that the float64-ANCHORED certificate resolved
                                   (the user's float64 prefix at the start of the draw's 64-product chunk + fp32 inside it) instead
                                   of a float64 walk of the chunk's products */
#define RG_CNT_BAD_ACTION 25   /* RG_POLICY_EXTERNAL: events whose action was outside [0, num_products): rg_sim_step evaluates them with
                                 * product 0 (it must not index beta / mu_b with them) and LOGS a = 0 — a caller bug made visible here
                                 * (rg_sim_step_user rejects the same input with RG_EINVAL before it reaches the device) */
#define RG_CNT_POLY_TABLE 26     /* RG_POLICY_LOGREG_POLY: acts whose best decision lies on the expit step table (decided exactly there) */
#define RG_CNT_POLY_UNRESOLVED 27 /* ... acts below the table with a lower-index decision inside the margin W of the best one: the action
                                   * taken is the first maximal decision; the act is listed for the host (rg_sim_read_poly_unresolved) */
#define RG_CNT_WH_CLOCK_RANGE 28 /* RG_POLICY_LOGREG_POLY with a weight table: acts on a time-weighted history that met a clock value outside
                                   * [0, 32767] — the act's own, a view's, a view after the act, or a difference beyond the table.  The
                                   * weight was the table's at the clamped index; the caller discards the result */
#define RG_CNT_BAYES_SATURATED 29 /* RG_POLICY_BAYES_VB: acts decided in the saturated zone (some action's decisions all >= RG_BAYES_ZSAT) */
#define RG_CNT_N 32             /* out[] of rg_sim_read_counters; slots 16..23 are internal */

typedef struct rg_sim rg_sim;

const char* rg_last_error(void);
int rg_abi_version(void);

/* number of visible HIP devices (0 on a CPU-only box; never an error) */
int rg_device_count(void);

/* Bytes of device workspace a simulator over `n_users` concurrent users needs
 * (omega, state lists, per-step counters, fp32 table copies, policy history). 0 on bad config. */
size_t rg_sim_workspace_bytes(const rg_config* cfg, uint64_t n_users);

/* AbstractEnv.init_gym (abstract.py:64-88) minus the table draws: binds a configuration and a
 * caller-owned device workspace to a handle.  Host-only; performs no device work. */
int rg_sim_create(rg_sim** out, const rg_config* cfg, uint64_t n_users, void* d_workspace,
                  size_t workspace_bytes);
int rg_sim_destroy(rg_sim* sim);

/* Run-path tuning knobs by name (none changes a result or the workspace layout; the defaults are the measured optima, DESIGN.md
 * §4 / §9).  rg_sim_create takes their initial values from the RECOGYM_* environment variables of the same meaning (the A/B
 * tests' way in; rg_sim_workspace_bytes and rg_sim_create each read the environment once, as one record, so set the variables before
 * the pair of calls); after that the library never reads the environment.  Names: walk_bias, walk_refill,
 * walk_handover, walk_click_batch, walk_search_batch, walk_helpers (0 .. 7), walk_click_join, walk_line64, pipe_groups (1: the walked
 * run keeps its list lengths on the device; 0: the host reads them back), pipe_occ1, pipe_occ2, pipe_xblocks,
 * pipe_min_users, exact_mix, exact_tile, slices (-1 = by population), sweep_prefix_off, tail_below (a value above 0 is
 * refused where rg_sim_create keeps it 0: the LogReg family of policies and per-user clocks),
 * repack_every, run_ahead (events a round of a run to the end may take a user through, 0 = an event per launch), lr_part_cap (acts
 * of a step the frozen-LogReg fp16 screen takes; can only be lowered), sweep_lds (1: the unsliced sweep of a run whose draws are
 * not cached keeps its tile prefixes in LDS and searches them there, k_draw_tp; 0: k_draw_bf16p's scratch + search), debug.
 * Read-only: sweep_lds_kernel (1 where k_draw_tp serves the configuration).
 * Read-only, a test hook — the LAUNCH LEDGER: launched_<family> = launches of that kernel family since rg_sim_create, counted on
 * the host next to each launch.  Families: draw_f64 (the float64 kernels as the sweep of every organic user), draw_fp32
 * (k_draw_mfma), draw16_fused / draw16_sliced (k_draw_bf16 / k_draw_bf16p / k_draw_f16w as one sweep with the search fused in /
 * over product slices), search (k_draw_search behind the slices), draw_tp (k_draw_tp / k_draw_tpw), pick (k_pick), draw_cached
 * (k_draw_cached), sweep_xh (k_sweep_xh), exact_m / exact_tile / exact_h (the float64 sums: a user per lane / a product per lane /
 * the walk's mixed batch), walk (k_walk), walk2 (k_walk2), walk_solo (k_walk_solo), park_compact (k_park_compact: round 1's list
 * made dense, between round 1 and the float64 batch of a walked run with device-side list lengths), advance (k_advance), advance_run
 * (k_advance_run), tail (k_tail), repack, env0 (k_draw_env0), logreg_screen, logreg_acts, logreg_sample, logreg_poly (k_poly_acts), sort_tiled / sort_plain
 * (the ordered log's scatter).  What rg_sim_create chose for the fast draw: draw_kh, draw_n1 (the class: KH, k-steps N1),
 * draw_split (0 none, 1 three-way bf16, 2 two-way fp16, 3 two-way fp16 wide), draw_kernel (0 float64 only, 1 fp32 MFMA, 2 a 16-bit
 * sweep), draw_pipelined (1: that sweep is k_draw_bf16p), xh_class (100 KH + 10 NH + NL of k_sweep_xh where it serves the walked
 * run, else 0) and xh_waves (its waves per block, else 0).  What else rg_sim_create decided (tests/test_create_plan.py pins all of
 * it): walk_form (0 lock-step, 1 k_walk, 2 k_walk2), walk_occ (blocks per CU the walk kernel is compiled for), walk_solo (the last
 * round is k_walk_solo's), use_cache (the per-user sum cache is in use), fin_in_sweep (the sweep leaves the finalize output itself),
 * handover_auto (walk_handover follows the reset range), draw_smem / mfma_smem / xh_smem / tp_smem (dynamic LDS bytes of the 16-bit
 * sweep, k_draw_mfma, k_sweep_xh, k_draw_tp / k_draw_tpw), tp_nts (LDS row stride of a user's tile prefixes), tp_cpt (chunks per tile
 * of the wide sweep), draw_threads (block size of the draw kernel), exact_rows (rows of the float64 chunk-sum scratch), hist_cap
 * (history entries per user row), repack_min (users below which slot == user index), ablate (timing-experiment bits).
 * The last walked run's round-1 list, from the run's one read-back (0 before any): park_slots (the entries its waves reserved,
 * 64 at a time: users and padding), park_users (the users parked at an uncertified draw), handed_over (the users its draining
 * waves handed on), batch_users (the list entries the float64 batch swept for: park_users + handed_over, the dense list
 * k_park_compact made of them).  A run with host-side list lengths (pipe_groups = 0, or fewer than pipe_min_users) counts no kinds
 * and makes no dense list: park_users = handed_over = -1, batch_users = park_slots = the list it read back.
 * Setting any of them fails like an unknown name.
 * RG_EINVAL for an unknown name or a value out of range. */
int rg_sim_set_option(rg_sim* sim, const char* name, int64_t value);
int rg_sim_get_option(rg_sim* sim, const char* name, int64_t* value);

/* env_kind = 1 — RecoEnv0.set_static_params (reco_env_v0.py:22-47), as the tables its draws compare against, float64 device
 * arrays computed on the host exactly as numpy / the C library do (the device only compares):
 *   cdf_init    [P]               cumsum(ones(P) / P) / last          — reset: choice(P, p = initial_product_probs), :52-54
 *   cdf_cluster [cluster_size]    cumsum of a row of the block-diagonal product_transition inside its cluster, / last
 *                                 (every cluster's row has the same values) — update_product_view: choice(P, p = T[view]), :65-67
 *   click_p     [P][P]            click_probs[action][view] = f(P / 5 (T + T') + phi), :39-44 (exported as p_click)
 *   click_qn    [P][P]            exp(log(1 - p)): the threshold legacy binomial(1, p) compares its uniform with (numpy
 *                                 random_binomial_inversion; 1 - p where p > 0.5: the draw is then 1 - inversion(1 - p))
 *   click_px1   [P][P]            (p qn) / q of that algorithm's second step (a restart of the inversion, ~1e-16 of the draws)
 * cluster_size = P / num_clusters.  The library keeps the pointers. */
/* Host helper (no device, no handle): from click_probs p[n] the two thresholds of numpy's legacy binomial(1, p) —
 * qn[i] = exp(log(1 - p')) and px1[i] = (p' qn) / (1 - p'), p' = p or 1 - p where p > 0.5 — with the C library's exp / log, the ones
 * numpy's legacy-distributions.c calls: the device compares against exactly these doubles. */
int rg_env0_click_thresholds(const double* p, uint64_t n, double* qn, double* px1);
int rg_sim_set_env0_tables(rg_sim* sim, const double* d_cdf_init, const double* d_cdf_cluster, uint32_t cluster_size,
                           const double* d_click_p, const double* d_click_qn, const double* d_click_px1, void* stream);

/* RecoEnv1.set_static_params / generate_beta results (reco_env_v1.py:51-75,133-174): row-major
 * float64 device arrays Gamma (P,K), mu_organic (P), beta (P,K), mu_bandit (P), drawn on the
 * host from RandomState(seed) so they are bit-identical to the reference's.  The library keeps
 * the pointers (caller keeps them alive) and builds its fp32 tile copies in the workspace. */
int rg_sim_set_tables(rg_sim* sim, const double* d_gamma, const double* d_mu_organic,
                      const double* d_beta, const double* d_mu_bandit, void* stream);

/* RG_POLICY_LAST_VIEW_TABLE: per-product device tables, kept by pointer (caller keeps them alive):
 * d_action[p] = action taken when the user's last organic view was p, d_ps[p] = the `ps` value
 * logged with it (NULL = 1.0; BanditMFSquare logs its logit there, bandit_mf.py:84). */
int rg_sim_set_policy_table(rg_sim* sim, const int32_t* d_action, const float* d_ps);

/* The same with the `ps` table in float64 (BanditCount logs its CTR estimate (clicks + 1) / (pulls + 2) there, bandit_count.py:44,
 * which float32 cannot hold): the float64 side array of the log (rg_sim_set_log_aux) then carries exactly d_ps[p]; the 16-byte
 * row keeps its rounding to float32.  The two calls replace each other. */
int rg_sim_set_policy_table_f64(rg_sim* sim, const int32_t* d_action, const double* d_ps);

/* EpsilonGreedy(config, agent) over the handle's policy (agents/epsilon_greedy.py:30-71; epsilon_select_worse = False): every act
 * flips the explore coin of the addressed draw (eg_seed, user, t) — the draw contract is in recogym_rng.h — and either keeps the
 * inner act with ps = one_minus_eps * ps_inner or takes the explore action with ps = ps_explore.  The device computes none of the
 * constants: d_cdf is the host's NumPy table cumsum(full(n, 1.0 / n)) / last with n = P - 1 (pure_new: the greedy action is
 * excluded) or n = P, float64, caller-owned and kept by pointer; ps_explore = epsilon * (1.0 / n); one_minus_eps = 1.0 - epsilon.
 * Inner policies: RG_POLICY_RANDOM_AGENT, RG_POLICY_ORGANIC_USER_COUNT, RG_POLICY_LAST_VIEW_TABLE (anything else: RG_EINVAL, as
 * are epsilon outside [0, 1], pure_new with fewer than 2 products and a NULL table).  After rg_sim_create and before
 * rg_sim_reset_users (afterwards: RG_ESTATE).  With the overlay on a run stays in the lock-step kernels (k_advance, k_advance_run,
 * k_tail), as with time_mode: the user-major walk has no overlay. */
int rg_sim_set_epsilon_greedy(rg_sim* sim, double epsilon, uint64_t eg_seed, uint32_t pure_new, const double* d_cdf,
                              double ps_explore, double one_minus_eps);

/* The same overlay round a MODEL: legal only for RG_POLICY_LOGREG_FROZEN without lr_select_randomly and for RG_POLICY_LOGREG_POLY
 * (anything else: RG_EINVAL — a sampling LogReg's act is a sampled action whose propensity is not 1, and the policies above have
 * rg_sim_set_epsilon_greedy).  The greedy action g of an act is the model's cached act of the user's view history — classes[argmax],
 * or the likelihood agent's action — with inner propensity 1.0: an explored act takes the table's action and ps_explore, a greedy
 * one g and one_minus_eps * 1.0.  Every event of a run-ahead round flips its own coin, keyed by its own event index.  The act
 * kernels, the view history and the likelihood agent's unresolved list (which lists the GREEDY act) are what they are without the
 * overlay.  Arguments, the other checks and the call window are rg_sim_set_epsilon_greedy's. */
int rg_sim_set_epsilon_greedy_model(rg_sim* sim, double epsilon, uint64_t eg_seed, uint32_t pure_new, const double* d_cdf,
                                    double ps_explore, double one_minus_eps);

/* The same overlay round the two models whose handle is RG_POLICY_NN_IPS or RG_POLICY_BAYES_VB, and round nothing else (any other
 * policy: RG_EINVAL; rg_sim_set_epsilon_greedy_model keeps refusing these two).  The greedy action g of an act is the cached act of
 * k_nn_acts / k_bayes_acts.  Its inner propensity is the act's own: 1.0 for BayesianAgentVB, and for NnIpsAgent the model output
 * prob[g] the act kernel cached beside the action — a greedy row logs one_minus_eps * prob[g], one float64 product (the reference's
 * (1.0 - epsilon) * greedy_action['ps']), an explored one ps_explore.  The act kernels, the view history and the unresolved list are
 * what they are without the overlay: the list holds the GREEDY act of every listed act, and with pure_new a wrong greedy act moves
 * explored actions too, so a caller confirms the listed acts on the host as it does without the overlay (rg_sim_read_poly_unresolved).
 * Arguments, the other checks and the call window are rg_sim_set_epsilon_greedy's. */
int rg_sim_set_epsilon_greedy_model_ps(rg_sim* sim, double epsilon, uint64_t eg_seed, uint32_t pure_new, const double* d_cdf,
                                       double ps_explore, double one_minus_eps);

/* The overlay's explore action on caller-supplied uniforms (stateless; the part rg_sim_debug_ouc_acts plays for
 * OrganicUserEventCounter): d_out[i] = what rng.choice(P, p = product_probas) returns for the uniform d_u1[i] in [0, 1) when the
 * greedy action is d_greedy[i] — NumPy's searchsorted(cumsum(p) / last, u, 'right') — by the device function the step loop uses.
 * d_cdf as above.  Enqueued on `stream`; no synchronisation. */
int rg_eg_explore_actions(uint32_t num_products, uint32_t pure_new, const double* d_cdf, const double* d_u1, const int32_t* d_greedy,
                          uint64_t n, int32_t* d_out, void* stream);

/* RG_POLICY_LOGREG_FROZEN: the fitted model's arrays on the device, kept by pointer: d_coef_t =
 * sklearn's coef_ TRANSPOSED, row-major [num_products][n_classes] float64; d_intercept [n_classes];
 * d_classes [n_classes] = classes_ (the action of every class).  A two-class sklearn model (coef_ of
 * one row) is passed as two classes with a zero first row/intercept.  Scores are accumulated exactly
 * as scipy's CSR x dense product does (viewed products ascending, multiply then add, intercept
 * last), so the argmax is sklearn's predict() bit for bit. */
int rg_sim_set_logreg(rg_sim* sim, const double* d_coef_t, const double* d_intercept,
                      const int32_t* d_classes, uint32_t n_classes);

/* Optional fast path of RG_POLICY_LOGREG_FROZEN (after rg_sim_set_logreg): fp32 copies of coef^T [num_products][n_classes]
 * and intercept [n_classes] (each value rounded to nearest), d_wmax[p] >= max_c |coef_t[p][c]| and bmax >= max_c |intercept[c]|.
 * The policy's act is computed when a user's view history has changed (not once per event); with these arrays the class
 * scores are first taken in fp32 and accepted when the best one leads by more than twice the rounding bound
 * (views + 3) 2^-24 (bmax + sum_p views_p wmax[p]); everything else goes through the float64 walk of rg_sim_set_logreg's
 * arrays, so the logged action is sklearn's predict() bit for bit either way.  All NULL / 0 = float64 only. */
int rg_sim_set_logreg_fp32(rg_sim* sim, const float* d_coef32_t, const float* d_intercept32, const float* d_wmax, float bmax);

/* Optional screening pass on top of rg_sim_set_logreg_fp32 (its intercept32 / wmax / bmax are used): d_coef16_t = coef^T
 * [num_products][n_classes] rounded to nearest IEEE half (every |value| <= 65504; n_classes % 8 == 0).  An act then takes
 * all class scores from the half table (half the bytes of the fp32 one: at 10^4 classes the act is bound by streaming the
 * rows of the viewed products), keeps the classes whose score is within twice the rounding bound
 * sum_p views_p (2^-11 wmax[p] + 2^-25) + (views + 3) 2^-24 (bmax + sum_p views_p wmax[p]) of the best one, and decides among
 * them by float64 scores in scipy's order (rg_sim_set_logreg's arrays): sklearn's predict() bit for bit.  NULL = off. */
int rg_sim_set_logreg_fp16(rg_sim* sim, const uint16_t* d_coef16_t);

/* RG_POLICY_LOGREG_POLY: the fitted binary model of the likelihood agent, float64 device arrays kept by pointer.  With w = coef_[0]:
 * d_wf = w[:P] (the view counts' weights), d_wa = w[P:2P] (the action block, whose stored VALUE is the action's index), d_wk_t =
 * w[2P:].reshape(P, P) TRANSPOSED, [viewed product][action] (lanes over actions read a row contiguously), intercept = intercept_[0].
 * The decision of action a over the n distinct viewed products p_0 < ... < p_(n-1) with counts c_0 .. c_(n-1), float64, multiply
 * then add, in exactly this order (sklearn's decision_function on the reference's features, bit for bit):
 *     s = 0;  for j: s += c_j wf[p_j];   s += a wa[a];   for j: s += c_((a n + j) / P) wk[a][p_j];   z[a] = s + intercept
 * (the cross term's count index is the reference's, reproduced: its transform lays out kron(counts, ones(P)) in slices of n).
 * The action is the FIRST index of the maximum of expit(z).  d_expit_steps[k], k < n_steps, never increasing, is the smallest
 * double whose scipy.special.expit is >= 1 - k 2^-53 (the host finds them by bisection with expit itself).  With z* = max z and
 * a* = its first index: z* >= steps[n_steps - 1]: the action is the lowest index whose decision lies on z*'s step (an exact
 * comparison of doubles; RG_CNT_POLY_TABLE); below: the action is a*, and the act is UNRESOLVED (RG_CNT_POLY_UNRESOLVED, listed)
 * when some a < a* has 0 < z* - z[a] <= W, W = 2^-49 (1 + 2^m), m = ceil(z* 1.4426950408889634) + 1 — an upper bound of
 * 8 2^-52 (1 + exp(z*)), inside which expit may round two decisions to one value; with z* < -700 (expit leaves the normal doubles) every act with a* > 0 is
 * unresolved.  n_steps in [1, 1024]. */
int rg_sim_set_logreg_poly(rg_sim* sim, const double* d_wf, const double* d_wa, const double* d_wk_t, double intercept,
                           const double* d_expit_steps, uint32_t n_steps);

/* RG_POLICY_LOGREG_POLY with the reference's weight_history_function: the act's features are not view counts but, per product,
 * the sum of w(now - t_view) over the user's views.  The reference casts every clock value to int16 first, so inside the clock
 * range [0, 32767] w is the table d_table[0 .. n) over the differences (float64 device array kept by pointer, n <= 32768; a float32
 * table is passed widened, with accumulate_f32 = 1).  A product's feature is the sequential sum of its views' table entries in view
 * order — in double, or with accumulate_f32 every add rounded to float32 with subnormals kept — rounded once to float32; a product
 * whose feature is exactly 0 leaves the list; the decisions are rg_sim_set_logreg_poly's with these values as the counts c_j (an
 * empty list is legal: z[a] = a wa[a] + intercept).  Legal after rg_sim_create and before rg_sim_reset_users, not together with
 * the EpsilonGreedy overlay; allocates the users' timed history rows (n_cap x hist_cap x 8 bytes of device memory, freed by
 * rg_sim_destroy).  The state is readable as option "weight_history".  With it on, a run is lock-step (no walk, no run-ahead, no
 * tail kernel) and needs a log (rg_sim_set_log: the step's views are read back from their rows): every bandit event gets a fresh
 * act at the clock value logged on its own row — the event index, or the NormalTimeGenerator's clock under time_mode = 1 — and so
 * does the trailing row of a stopping user.  The history row holds VIEWS (rg_sim_debug_set_timed_history describes it), so
 * RG_CNT_HIST_OVERFLOW counts views beyond hist_cap - 1 per user; RG_CNT_WH_CLOCK_RANGE counts clock values outside [0, 32767];
 * unresolved acts are listed as ever (rg_sim_read_poly_unresolved), t being the event index of the act's own row: its history is
 * the user's organic rows with a smaller index.  Launches count in the ledger family logreg_poly_w. */
int rg_sim_set_weight_history(rg_sim* sim, const double* d_table, uint32_t n, uint32_t accumulate_f32);

/* RG_POLICY_BAYES_VB: the posterior samples of BayesianAgentVB, one float64 device array kept by pointer: d_lam_t[(p P + a) S + s] =
 * Lambda[s][p P + a], S = num_samples >= 1 (the sample axis contiguous: the 64 lanes of a wave read 512 contiguous bytes per (p, a)).
 * The decisions of action a over the n distinct viewed products p_0 < ... < p_(n-1) with counts c_j, float64, multiply then add, in
 * exactly this order:   z[a][s] = 0;  for j: z[a][s] += c_j lam_t[p_j][a][s];   beside them m[a][s] = sum_j |c_j lam_t[p_j][a][s]| in
 * the same order and M = max m.  q[a] = (sum_s 1 / (1 + exp(-z[a][s]))) / S, the sum taken per lane over s = lane, lane + 64, ... and
 * then over the lanes by a fixed xor butterfly (two runs give the same bits).  ez = (2 n + 4) 2^-53 M and W = ez / 4 +
 * (2 S + 44) 2^-53 bound the distance of q[a] from the reference's value in ANY summation order.  The rule:
 *   n = 0                      action 0;
 *   ez >= 1                    the first maximum of q, UNRESOLVED;
 *   A1 = {a: min_s z[a][s] >= RG_BAYES_ZSAT} not empty:  a_c = min A1, RG_BAYES_SATURATED (RG_CNT_BAYES_SATURATED), and UNRESOLVED
 *                              when some a < a_c has 1 - q[a] <= W (the reference's mean is exactly 1.0 at a_c, and may be at a);
 *   else                       a* = the first maximum of q, UNRESOLVED when another action has q[a*] - q[a] <= 2 W.
 * Unresolved acts are counted and listed as the likelihood agent's (RG_CNT_POLY_UNRESOLVED, rg_sim_read_poly_unresolved).
 * The EpsilonGreedy model overlay on this policy is RG_EINVAL. */
#define RG_BAYES_ZSAT 40.0
#define RG_BAYES_SATURATED 1u
#define RG_BAYES_UNRESOLVED 2u
int rg_sim_set_bayes_vb(rg_sim* sim, const double* d_lam_t, uint32_t num_samples);

/* RG_POLICY_NN_IPS: the net of NnIpsAgent, six float64 device arrays kept by pointer that hold the model's fp32 values widened, the
 * matrices transposed so that the row of a viewed product or hidden unit is contiguous: d_w1t[p H + h] = W1[h][p], d_b1[h],
 * d_w2t[h H + k] = W2[k][h], d_b2[k], d_w3t[k P + a] = W3[a][k], d_b3[a]; H = num_hidden in [1, 1024], num_products <= 4000, every
 * value finite (else RG_EINVAL).  The call reads the arrays once (the absolute row sums A2, A3 below) and synchronises.
 * The act over the n distinct viewed products p_0 < ... < p_(n-1) with counts c_j, float64, multiply then add, in exactly this order:
 *   s1[h] = 0; for j: s1[h] += c_j w1t[p_j][h];  s1[h] += b1[h];  h1 = sg(s1)     m1[h] = sum_j |c_j w1t[p_j][h]| + |b1[h]|, M1 = max m1
 *   s2[k] = 0; for h: s2[k] += w2t[h][k] h1[h];  s2[k] += b2[k];  h2 = sg(s2)
 *   z[a]  = 0; for k: z[a]  += w3t[k][a] h2[k];  z[a]  += b3[a]
 *   a* = the first index of max z;  e[a] = ex(z[a] - z[a*]);  ps = e[a*] / sum, the sum taken per lane over a = lane, lane + 64, ...
 *   and then over the 64 lanes by a fixed xor butterfly.  sg(x) = 1 / (1 + ex(-x)); ex is an exponential made of IEEE operations
 *   only (rg_nn_common.hpp: nn_exp), so that a host restatement gives the same bits (agents/nn_ips.py).
 * W(n, M1, H, A2, A3) (A2 = max_k sum_h |w2t[h][k]| + |b2[k]|, A3 likewise) bounds the distance of every z[a] from the
 * logit of torch's fp32 forward in ANY summation order, plus half the gap below which an fp32 softmax can tie or reorder two logits.
 * The act is RG_NN_UNRESOLVED when some other action has z[a*] - z[a] <= 2 W, or a count exceeds 2^24 (not an fp32 value): counted
 * and listed as the likelihood agent's (RG_CNT_POLY_UNRESOLVED, rg_sim_read_poly_unresolved).  ps goes to the policy's rows.
 * The EpsilonGreedy model overlay on this policy is RG_EINVAL. */
#define RG_NN_UNRESOLVED 2u
int rg_sim_set_nn_ips(rg_sim* sim, const double* d_w1t, const double* d_b1, const double* d_w2t, const double* d_b2,
                      const double* d_w3t, const double* d_b3, uint32_t num_hidden);

/* RG_POLICY_MLR: the weight of PyTorchMLRAgent's one linear layer, one float64 device array kept by pointer that holds the model's
 * fp32 values widened and transposed so that the row of a viewed product is contiguous: d_wt[p P + a] = W[a][p]; num_products in
 * [1, 4000] (a 128 MB table at the most), every value finite (else RG_EINVAL).  The call reads the array once and synchronises.
 * The act over the n distinct viewed products p_0 < ... < p_(n-1) with counts c_j, float64, multiply then add, in exactly this order:
 *   z[a] = 0; for j: z[a] += c_j wt[p_j][a]        m1[a] = sum_j |c_j wt[p_j][a]| (the same order), M1 = max_a m1[a]
 *   a* = the first index of max z
 * E = (n + 5) 2^-24 M1 bounds the distance of every z[a] from the reference's fp32 dot in ANY summation order, fused
 * or not.  The act is RG_MLR_UNRESOLVED unless z[a*] leads every other score by more than 2 E, no count exceeds 2^24 (not an fp32
 * value), the history is not empty and M1 < 2^126 (no fp32 partial sum can overflow): counted and listed as the likelihood agent's
 * (RG_CNT_POLY_UNRESOLVED, rg_sim_read_poly_unresolved).  ps = 1.  The EpsilonGreedy overlays on this policy are RG_EINVAL. */
#define RG_MLR_UNRESOLVED 2u
int rg_sim_set_mlr(rg_sim* sim, const double* d_wt);

/* The unresolved acts of the run so far (since rg_sim_reset_users): out[3 i .. 3 i + 2] = (user id, t, action taken) for the first
 * min(listed, capacity) of them, in no particular order; t is the event index the act was computed at: its history is the user's
 * organic rows with index <= t.  *n_out = entries written, *overflow = 1 when the run had more unresolved acts than the device list
 * holds (4096) or than `capacity`.  `out` is host memory.  Synchronises `stream`. */
int rg_sim_read_poly_unresolved(rg_sim* sim, uint32_t* out, uint32_t capacity, uint32_t* n_out, uint32_t* overflow, void* stream);

/* Where rows go.  d_log == NULL (or capacity 0) disables logging: only counters are kept. */
int rg_sim_set_log(rg_sim* sim, rg_event* d_log, uint64_t capacity);

/* Optional float64 side arrays of the log, `capacity` (of rg_sim_set_log) doubles each, caller-owned device
 * memory; either may be NULL.  d_ps[row] receives the propensity of bandit row `row` in float64 — the dtype of
 * the reference's `ps` column (abstract.py:283-290,318-327; IPS estimators divide by it) — and d_p_click[row]
 * the click probability ff(beta[a].omega + mu_bandit[a]) the click of that row was drawn with
 * (reco_env_v1.py:104-116).  Entries of organic rows are not written.  rg_sim_set_log detaches them. */
int rg_sim_set_log_aux(rg_sim* sim, double* d_ps, double* d_p_click);

/* NormalTimeGenerator only: d_time[row] receives the (float64) time of raw-log row `row`, every row (the 16-byte row's
 * `t` stays the per-user event index, which orders the log).  `capacity` doubles, like the log.  rg_sim_set_log detaches it. */
int rg_sim_set_log_time(rg_sim* sim, double* d_time);

/* RecoEnv1.reset + AbstractEnv.reset (reco_env_v1.py:78-82, abstract.py:90-103) for `n` users
 * with ids first_user_id .. first_user_id+n-1 at once: state <- organic, t <- 0,
 * omega <- sigma_omega_initial * Z(K).  Users with id < organic_only_below are the
 * `num_organic_offline_users` warm-up users of generate_logs (abstract.py:293-297): they emit
 * only their first organic session.  Re-seeds nothing; `seed`/`policy_seed` may be changed
 * between runs with rg_sim_reseed (reset_random_seed(epoch), abstract.py:59-62). */
int rg_sim_reset_users(rg_sim* sim, uint64_t first_user_id, uint64_t n,
                       uint64_t organic_only_below, void* stream);
int rg_sim_reseed(rg_sim* sim, uint64_t seed, uint64_t policy_seed);

/* One Markov transition for every live user (one emitted row per live user, plus the phantom
 * row of users that stop) — the batched form of AbstractEnv.step / step_offline /
 * generate_organic_sessions (abstract.py:105-239) and RecoEnv1.update_product_view /
 * draw_click / update_state (reco_env_v1.py:85-128).  With RG_POLICY_EXTERNAL,
 * d_actions[i] is the action for the i-th user of the reset range (read only for users in the
 * bandit state; a user that stops then gets no phantom row — the caller's agent owns it). */
int rg_sim_step(rg_sim* sim, const int32_t* d_actions, void* stream);

/* AbstractEnv.step for ONE user (the gym.Env episode API: reset / step, abstract.py:123-197) with a single read-back: needs
 * RG_POLICY_EXTERNAL and a one-user reset range.  `action` is the agent's action for a user in the bandit state (ignored in
 * the organic state).  One Markov transition; then *out (host memory) receives, through one pinned-memory copy and ONE stream
 * synchronisation, the row the step emitted, the user's state and clock after it, and the float64 side values of the row. */
typedef struct rg_step_result {
    rg_event row;        /* the emitted row (has_row = 0: none, e.g. no log attached) */
    int32_t state;       /* RG_STATE_* after the transition */
    int32_t has_row;
    double time;         /* the user's clock after the step (event index + 1 with the default time generator) */
    double ps;           /* float64 propensity of the row where the side array is attached, else the row's float32 value */
    double p_click;      /* click probability of a bandit row where that side array is attached, else 0 */
} rg_step_result;
int rg_sim_step_user(rg_sim* sim, int32_t action, rg_step_result* out, void* stream);

/* generate_logs' user loop (abstract.py:299-316) for all users at once: steps until every user
 * reached `stop` or max_steps transitions were made.  Synchronises `stream`.  With max_steps >=
 * 65536 ("to the end") the last users of the run (<= 4096 alive at a 16-step poll, fewer for tables larger than 10^4 x 20; RECOGYM_TAIL overrides) are walked
 * to their end one user per workgroup instead of step by step; rows, counters and the sorted
 * log are the same, RG_CNT_STEP then reports the longest trajectory.  Fails with RG_ELIMIT when the run is incomplete
 * (RG_CNT_EXACT_OVERFLOW != 0, or a user reached the step limit).  The sigma_omega = 0 user-major walk cannot overflow the
 * float64 scratch (it holds a row per user there), so only the step limit applies to it. */
int rg_sim_run(rg_sim* sim, uint32_t max_steps, void* stream);

/* Synchronises `stream` and copies RG_CNT_N counters to the host. */
int rg_sim_read_counters(rg_sim* sim, int64_t* out, void* stream);

/* Measurement aid for bench.py's roofline line: with profiling on, every step records HIP
 * events on the stream the kernels are launched on.  rg_sim_get_profile returns
 * out[0..3] = total milliseconds spent in the MFMA organic-draw kernel, in its search kernel
 * (sliced mode only), in the float64 resolve kernels and in the advance kernel; out[4] =
 * profiled steps; out[5] = milliseconds in the tail kernel (rg_sim_run finishes the last users
 * of a run user by user instead of step by step, or — sigma_omega = 0 — the whole run user-major: k_walk);
 * out[6], out[7] = milliseconds in round 1 / the later rounds of k_walk; out[8] = milliseconds in the frozen-LogReg act
 * kernels (k_logreg_select + k_logreg_acts; not part of out[3]); out[9] reserved.  `out` must hold 10 doubles.  Off by default. */
int rg_sim_set_profiling(rg_sim* sim, int on);
int rg_sim_get_profile(rg_sim* sim, double* out);

/* Current Markov state per user of the reset range (int8, RG_STATE_*), for the gym.Env
 * compatibility path.  d_state has n entries. */
int rg_sim_export_state(rg_sim* sim, int8_t* d_state, void* stream);
/* Copy omega (float64, user-major (n,K)) out, for debugging views (`env.omega`). */
int rg_sim_export_omega(rg_sim* sim, double* d_omega, void* stream);

/* The row order of generate_logs' DataFrame (abstract.py:299-316): the
 * step-major device log is scattered so that each user's rows are contiguous, ordered by t,
 * the phantom row last, users in id order.  Caller-owned device buffers:
 *   d_row_offsets  n+1 int64 — filled with the exclusive prefix of rows per user (last = total)
 *   d_scratch      n + ceil(n/256) int64
 *   d_sorted       sorted_capacity rows
 * Synchronises `stream` once (to read the emitted-row count); fails with RG_ELIMIT when the
 * log buffer overflowed. */
int rg_sim_sort_log(rg_sim* sim, int64_t* d_row_offsets, int64_t* d_scratch, rg_event* d_sorted,
                    uint64_t sorted_capacity, void* stream);

/* The side arrays of rg_sim_set_log_aux in the row order rg_sim_sort_log produced (`d_row_offsets` as filled
 * by it): NaN on organic rows, and for p_click on the phantom row (never drawn).  Either output may be NULL. */
int rg_sim_sort_log_aux(rg_sim* sim, const int64_t* d_row_offsets, double* d_sorted_ps,
                        double* d_sorted_p_click, uint64_t sorted_capacity, void* stream);

/* The time column in the row order of rg_sim_sort_log (phantom rows: the time their act would have had). */
int rg_sim_sort_log_time(rg_sim* sim, const int64_t* d_row_offsets, double* d_sorted_time, uint64_t sorted_capacity,
                         void* stream);
/* Current time of every user of the reset range (n float64; = its event index with the default generator). */
int rg_sim_export_time(rg_sim* sim, double* d_time, void* stream);

/* ---- test hooks (the parity suite's adversarial certificate test; not part of the reference surface) ----
 * rg_sim_debug_set_omega: overwrite omega of the reset range, (n, K) float64 user-major, right after
 * rg_sim_reset_users.  rg_sim_debug_set_uniforms: d_u[i] replaces the uniform of user index i's next organic
 * product draws (NULL restores the addressed draws).  rg_sim_debug_uncertified: d_flags[i] = 1 iff user
 * index i's organic draw of the LAST step was not certified by the matrix-core kernel and went to the
 * float64 resolve (n bytes). */
int rg_sim_debug_set_omega(rg_sim* sim, const double* d_omega, void* stream);
int rg_sim_debug_set_uniforms(rg_sim* sim, const double* d_u);
/* rg_sim_debug_set_row_base: the raw log of every later reset range starts at row `rows` instead of 0 (rg_sim_reset_users marks
 * the entries below it unused, so the attached log must hold them): the regression test of raw-row arithmetic beyond 2^31 rows
 * (a full-size log reaches that line at ~20 M users of BASELINE config 3) without simulating 20 M users.  0 restores the default. */
int rg_sim_debug_set_row_base(rg_sim* sim, uint64_t rows);
int rg_sim_debug_uncertified(rg_sim* sim, uint8_t* d_flags, void* stream);

/* ---- test hooks of the two "decide cheaply, float64 inside a band" paths of the user-major walk ----
 * rg_sim_debug_click_decisions: for user index i of the reset range, the click decision of a bandit event with action
 * d_actions[i] and uniform d_u[i] on the user's current omega (reco_env_v1.py:104-116), by the walk's fp32 form and in
 * float64: d_out[i] bit 0 = the fp32 form decided (outside its error margin), bit 1 = its decision, bit 2 = the
 * float64 decision.  Needs sigma_omega == 0 (where the walk runs).
 * rg_sim_debug_set_history: overwrite the view histories (ViewsFeaturesProvider, agents/abstract.py:347-358) of the reset
 * range right after rg_sim_reset_users: user index i has d_nd[i] distinct products d_products[i * stride + j]
 * (ascending) with d_counts[i * stride + j] views each.
 * rg_sim_debug_ouc_acts: OrganicUserEventCounterModel.act (organic_user_count.py:45-96) of every user index on its
 * current history with d_u1[i] as the uniform of the action draw: d_action / d_ps (float64) as logged, d_flags[i] = 1
 * iff the action was decided by the integer prefix walk (outside its 2^-36 band), 0 = float64 cdf walk. */
/* rg_sim_debug_walk_fate: after a sigma_omega == 0 run "to the end" (the user-major walk), d_flags[i] (n bytes) = bit 0: user
 * index i met a draw the fast certificate rejected (or was handed over by a draining wave) and went through the float64
 * batch and round 2; bit 1: its last events were walked by the last round (a wave per user).  The sampled-oracle parity
 * check picks users of every kind with it. */
int rg_sim_debug_walk_fate(rg_sim* sim, uint8_t* d_flags, void* stream);
int rg_sim_debug_click_decisions(rg_sim* sim, const int32_t* d_actions, const double* d_u, uint8_t* d_out, void* stream);
int rg_sim_debug_set_history(rg_sim* sim, const uint32_t* d_nd, const uint32_t* d_products, const uint32_t* d_counts,
                             uint32_t stride, void* stream);
int rg_sim_debug_ouc_acts(rg_sim* sim, const double* d_u1, int32_t* d_action, double* d_ps, uint8_t* d_flags, void* stream);
/* rg_sim_debug_poly_acts: the RG_POLICY_LOGREG_POLY act of every user index on its current history (rg_sim_debug_set_history), by
 * the device function the step loop uses: d_action[i], d_flags[i] = bit 0: decided on the step table, bit 1: unresolved, bit 2: a
 * lower index than the first maximal decision won (a merge on a step).  Touches neither the counters nor the unresolved list. */
int rg_sim_debug_poly_acts(rg_sim* sim, int32_t* d_action, uint8_t* d_flags, void* stream);
/* rg_sim_debug_bayes_acts: the RG_POLICY_BAYES_VB act of every user index on its current history (rg_sim_debug_set_history), by the
 * device function the step loop uses: d_action[i], d_flags[i] (RG_BAYES_SATURATED | RG_BAYES_UNRESOLVED) and the device's means
 * d_q[i * num_products + a] (with an empty history no mean is computed: 0.5 is written).  Touches neither the counters nor the list. */
int rg_sim_debug_bayes_acts(rg_sim* sim, int32_t* d_action, uint8_t* d_flags, double* d_q, void* stream);
/* rg_sim_debug_nn_acts: the RG_POLICY_NN_IPS act of every user index on its current history (rg_sim_debug_set_history), by the device
 * function the step loop uses: d_action[i], d_flags[i] (RG_NN_UNRESOLVED), the logits d_z[i * num_products + a] and d_ps[i].
 * Touches neither the counters nor the list. */
int rg_sim_debug_nn_acts(rg_sim* sim, int32_t* d_action, uint8_t* d_flags, double* d_z, double* d_ps, void* stream);
/* rg_sim_debug_mlr_acts: the RG_POLICY_MLR act of every user index on its current history (rg_sim_debug_set_history), by the device
 * function the step loop uses: d_action[i], d_flags[i] (RG_MLR_UNRESOLVED) and the scores d_z[i * num_products + a].
 * Touches neither the counters nor the list. */
int rg_sim_debug_mlr_acts(rg_sim* sim, int32_t* d_action, uint8_t* d_flags, double* d_z, void* stream);
/* rg_sim_debug_logreg_acts: the plain RG_POLICY_LOGREG_FROZEN act (argmax; not lr_select_randomly) of every user index on its current
 * history (rg_sim_debug_set_history), right after rg_sim_reset_users, by the kernels the step loop launches, chosen as the step
 * chooses them: k_logreg_screen + k_logreg_decide where the fp16 copy is attached (k_logreg_acts for what lies beyond lr_part_cap),
 * k_logreg_acts otherwise.  Every slot is listed for an act at step 0 in place of k_logreg_select; d_action[i] = the act kept for
 * user index i.  The counters (RG_CNT_LR_ACTS, RG_CNT_LR_ROWS, RG_CNT_LR_EXACT) and the launch ledger count as in a step.  The call
 * leaves step 0's act list filled: rg_sim_step, rg_sim_run and every hook refuse (RG_ESTATE) until rg_sim_reset_users is called again. */
int rg_sim_debug_logreg_acts(rg_sim* sim, int32_t* d_action, void* stream);
/* rg_sim_debug_set_timed_history (after rg_sim_set_weight_history, right after rg_sim_reset_users): the TIMED view history of every
 * user index — d_n[i] views (at most stride), view j of product d_products[i * stride + j] at clock value d_times16[i * stride + j],
 * in view order (times never decreasing).  They go into the user's history row one at a time through the sorted insert that never
 * merges: the row (hist_cap words, as RG_CNT_HIST_OVERFLOW describes it) holds a header (views kept << 32 | entries) and one word
 * (product << 32 | time) per VIEW, ascending; a view that finds keep = hist_cap - 1 entries is dropped and adds one to
 * RG_CNT_HIST_OVERFLOW.  Views of products outside [0, num_products) are skipped.
 * rg_sim_debug_weighted_acts: the weighted act of every user index on its timed row at the clock value d_now16[i]: d_action / d_flags
 * as rg_sim_debug_poly_acts, and beside them the feature list the act was taken on — d_list_n[i] products d_list_prod[i * stride + j]
 * ascending with the float32 features d_list_val32[i * stride + j]; stride >= min(num_products, hist_cap - 1).  An act that met a
 * clock value outside the range adds one to RG_CNT_WH_CLOCK_RANGE.  Counts as a launch of the ledger family logreg_poly_w. */
int rg_sim_debug_set_timed_history(rg_sim* sim, const uint32_t* d_n, const uint32_t* d_products, const uint16_t* d_times16, uint32_t stride,
                                   void* stream);
int rg_sim_debug_weighted_acts(rg_sim* sim, const uint16_t* d_now16, int32_t* d_action, uint8_t* d_flags, uint32_t* d_list_n,
                               uint32_t* d_list_prod, float* d_list_val32, uint32_t stride, void* stream);

/*
 * The training features of an agent with a weight_history_function from a sorted device log (AbstractFeatureProvider.train_data,
 * reference agents/abstract.py:190-279): one row per bandit row, the trailing row included, holding per product the weighted sum
 * of the user's views BEFORE that row at the row's clock value — rg_sim_set_weight_history's rule on the same table (d_table, n,
 * accumulate_f32).  Stateless.  d_rows / d_offsets / n_users / max_user_rows as rg_ope_replay_logreg takes them, validated by the
 * same rules before anything is written (a user that opens with a bandit row, more than max_user_rows rows, a product or an action
 * >= num_products: RG_EINVAL).  d_t16[row] is the row's clock value after the int16 cast, 0xFFFF where it lies outside [0, 32767];
 * d_brow[row] the ordinal of a bandit row among the log's bandit rows.  Two passes over the same arguments:
 *   mode 0  d_len[ordinal] = the number of products whose feature is not 0 (the caller's prefix sum over it is d_crow);
 *   mode 1  the products, ascending, into d_col[d_crow[ordinal] ..] and their float32 features into d_val at the same places.
 * One wave per user carries the user's timed view list in the workspace (nothing is dropped).  The workspace's first int64 words
 * after the call: 0 error bits of the validation, 1 rows whose d_t16 is outside [0, 32767] — not 0: the features are not the
 * reference's, and the caller takes its host loop — 2 bandit rows walked. */
size_t rg_weighted_feed_workspace_bytes(uint64_t n_users, uint32_t max_user_rows);
int rg_weighted_feed(const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users, uint32_t max_user_rows, uint32_t num_products,
                     const uint16_t* d_t16, const double* d_table, uint32_t n, uint32_t accumulate_f32, uint32_t mode,
                     const int64_t* d_brow, int32_t* d_len, const int64_t* d_crow, int32_t* d_col, float* d_val, void* d_workspace,
                     size_t workspace_bytes, void* stream);

/*
 * Off-policy evaluation (evaluate_IPS / evaluate_SNIPS, reference evaluate_agent.py:753-810): replay a sorted log under a
 * target policy.  Stateless (no rg_sim handle).  `kind`: RG_POLICY_RANDOM_AGENT (pi = 1 / P), RG_POLICY_ORGANIC_USER_COUNT
 * (the `ps-a` vector of organic_user_count.py:45-96 over ALL the user's organic rows so far; the explore coin of
 * exploit_explore with epsilon > 0 is the addressed policy draw of (policy_seed, u, t), words 0 and 1) or
 * RG_POLICY_LAST_VIEW_TABLE (one-hot at table[last organic product]).
 */
typedef struct rg_ope_policy {
    uint32_t kind;
    uint32_t num_products;
    uint64_t policy_seed;
    uint32_t ouc_select_randomly;
    uint32_t ouc_exploit_explore;
    uint32_t ouc_reverse_pop;
    uint32_t reserved;
    double ouc_epsilon;
    const int32_t* table;           /* RG_POLICY_LAST_VIEW_TABLE: action per last viewed product (device, P entries) */
} rg_ope_policy;

/* where the logging propensity of a bandit row comes from */
#define RG_OPE_PS_ARRAY 0   /* d_ps[row], float64 (Simulator.sorted_aux / a DataFrame's ps column) */
#define RG_OPE_PS_CONST 1   /* ps_const for every row (the uniform loggers' exact 1 / P) */
#define RG_OPE_PS_ROW 2     /* the row's own float32 ps */

/* rg_ope_workspace_bytes: device workspace rg_ope_replay needs for n_users users the longest of which has max_user_rows rows
 * (0 = error, see rg_last_error).
 * rg_ope_replay: users 0 .. n_users-1 of a sorted log (user i = rows d_offsets[i] .. d_offsets[i+1]-1, each user's first row
 * organic); for every bandit row of them d_ratio[row] = pi(a | the user's rows before it) / ps and, when d_click is not NULL,
 * d_click[row] = c.  Other entries of d_ratio / d_click are not written.  d_sums[0..2] = (bandit rows, sum c r, sum r),
 * reduced in a fixed order (the same bits on every run).  Enqueued on `stream`; no synchronisation. */
size_t rg_ope_workspace_bytes(const rg_ope_policy* pol, uint64_t n_users, uint32_t max_user_rows);
int rg_ope_replay(const rg_ope_policy* pol, const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users,
                  uint32_t max_user_rows, uint32_t ps_mode, const double* d_ps, double ps_const, double* d_ratio,
                  uint8_t* d_click, double* d_sums, void* d_workspace, size_t workspace_bytes, void* stream);

/*
 * Off-policy evaluation of the frozen LogReg policy (LogregFrozenAgent, reference agents/logreg_ips.py:60-87 with
 * with_ps_all = True): replay a sorted log under a fitted multinomial model.  Stateless (no rg_sim handle).  The model arrays are
 * device arrays laid out as rg_sim_set_logreg / rg_sim_set_logreg_fp32 take them.  The policy sees the user's cumulative view
 * counts (all organic rows so far, across sessions).
 *   select_randomly == 0: pi = [classes[argmax_c (intercept[c] + sum_p views_p coef_t[p][c])] == a] — sklearn's predict() bit for
 *     bit: fp32 scores from the optional fp32 group decide where their margin certifies the float64 argmax (the step loop's
 *     certificate), the float64 walk in scipy's summation order everywhere else (first maximum).  An action that is no class of
 *     the model gets 0.
 *   select_randomly != 0: pi = softmax(scores)[a] in float64, the step loop's arithmetic (a log it wrote under the same model
 *     replays to ratios of exactly 1); needs classes[c] == c for c = 0 .. P-1 and P <= 1024.  No policy draw is involved.
 */
typedef struct rg_ope_logreg {
    uint32_t num_products;          /* P <= RG_EV_INDEX_MASK */
    uint32_t n_classes;             /* C >= 1 */
    uint32_t select_randomly;
    uint32_t reserved;
    const double* coef_t;           /* [P][C] float64, as rg_sim_set_logreg */
    const double* intercept;        /* [C] */
    const int32_t* classes;         /* [C] */
    const float* coef32_t;          /* optional [P][C]; NULL = float64 only */
    const float* intercept32;       /* [C], with coef32_t */
    const float* wmax;              /* [P], with coef32_t: >= max_c |coef_t[p][c]| */
    float bmax;                     /* >= max_c |intercept[c]| */
    uint32_t reserved2;
} rg_ope_logreg;

/* rg_ope_logreg_workspace_bytes: device workspace rg_ope_replay_logreg needs for n_users users the longest of which has
 * max_user_rows rows (0 = error, see rg_last_error).
 * rg_ope_replay_logreg: rows, offsets, the ps source and the outputs d_ratio / d_click / d_sums as rg_ope_replay.  The log is
 * validated before any output is written: RG_EINVAL for a user whose first row is a bandit row or that has more than
 * max_user_rows rows, and for a product or an action >= P (such a row never indexes the model).  RG_EINVAL also for null arrays,
 * n_classes == 0, a half-given fp32 group, and select_randomly with n_classes != num_products, P > 1024 or classes that are not
 * 0 .. P-1; RG_ENOMEM for a workspace too small.  Afterwards the workspace's first int64 words hold [0] error bits (0), [1] acts
 * computed (bandit rows whose user's history changed since its previous act; the rows between reuse it), [2] acts decided by
 * float64 scores, [3] coef_t rows read.  Synchronises `stream` once (it reads the validation's verdict), twice with
 * select_randomly (the classes). */
size_t rg_ope_logreg_workspace_bytes(const rg_ope_logreg* model, uint64_t n_users, uint32_t max_user_rows);
int rg_ope_replay_logreg(const rg_ope_logreg* model, const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users,
                         uint32_t max_user_rows, uint32_t ps_mode, const double* d_ps, double ps_const, double* d_ratio,
                         uint8_t* d_click, double* d_sums, void* d_workspace, size_t workspace_bytes, void* stream);

/*
 * Off-policy evaluation of the likelihood agent (LogregPolyFrozenAgent, reference agents/logreg_poly.py:143-167 with
 * with_ps_all = True): replay a sorted log under a fitted binary model of polynomial features.  Stateless (no rg_sim handle).  The
 * model arrays are device arrays as rg_sim_set_logreg_poly takes them, th the table of expit's top steps (n_steps <= 1024, never
 * increasing).  The policy sees the user's cumulative view counts (all organic rows so far, across sessions); the act is the step
 * loop's (k_poly_acts: the same decisions, step table, margin and flags), pi = [action == a], r = pi / ps.
 */
typedef struct rg_ope_poly {
    uint32_t num_products;          /* P <= RG_EV_INDEX_MASK */
    uint32_t n_steps;               /* entries of th, 1 .. 1024 */
    const double* wf;               /* [P] */
    const double* wa;               /* [P] */
    const double* wk_t;             /* [P][P], [viewed product][action] */
    const double* th;               /* [n_steps] */
    double intercept;
} rg_ope_poly;

/* rg_ope_poly_workspace_bytes: device workspace rg_ope_replay_poly needs for n_users users the longest of which has
 * max_user_rows rows (0 = error, see rg_last_error).
 * rg_ope_replay_poly: rows, offsets, the ps source and the outputs d_ratio / d_click / d_sums as rg_ope_replay.  The log is
 * validated before any output is written, by rg_ope_replay_logreg's rules: RG_EINVAL for a user whose first row is a bandit row
 * or that has more than max_user_rows rows, and for a product or an action >= P.  RG_EINVAL also for a null model or model
 * array, n_steps == 0 or > 1024, and rows that are not 16-byte aligned; RG_ENOMEM for a workspace too small.  Afterwards the
 * workspace's first int64 words hold [0] error bits (0), [1] acts computed (bandit rows whose user's history changed since its
 * previous act; the rows between reuse it), [2] acts decided on the step table, [3] acts where a lower index than the first
 * maximal decision won, [4] unresolved acts, [5] non-zero when more than 4096 acts were unresolved, [6] wk_t rows read.  The
 * unresolved acts follow from byte 256: up to 4096 entries of three uint32 (user index, position of the bandit row the act was
 * computed at within the user's rows, action taken), in no fixed order.  The ratios are written with the device's action; a
 * caller that needs the reference's action on such acts recomputes them on the host (recogym_amd.sim.poly_replay_verify).
 * d_sums holds the same bits on every run.  Synchronises `stream` once (it reads the validation's verdict). */
size_t rg_ope_poly_workspace_bytes(const rg_ope_poly* model, uint64_t n_users, uint32_t max_user_rows);
int rg_ope_replay_poly(const rg_ope_poly* model, const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users,
                       uint32_t max_user_rows, uint32_t ps_mode, const double* d_ps, double ps_const, double* d_ratio,
                       uint8_t* d_click, double* d_sums, void* d_workspace, size_t workspace_bytes, void* stream);

/*
 * Off-policy evaluation of the likelihood agent on a TIME-WEIGHTED view history (a weight_history_function, with_ps_all = True):
 * rg_ope_replay_poly's replay with the act of rg_sim_set_weight_history — at every bandit row the user's organic rows before it,
 * each weighted by table[now - t] at the row's own clock value `now`, summed per product by that function's rule (table, n,
 * accumulate_f32 as it and rg_weighted_feed take them), then the likelihood agent's act on that feature list.  d_t16[row] is the
 * row's clock value after the int16 cast, 0xFFFF where it lies outside [0, 32767] (rg_weighted_feed's convention).  Nothing is
 * dropped from a user's views, and no act is shared between bandit rows.
 */
typedef struct rg_ope_poly_w {
    rg_ope_poly model;              /* the likelihood agent's model, as rg_ope_replay_poly takes it */
    const double* table;            /* device: the weight table over clock differences */
    uint32_t n;                     /* 1 .. 32768 entries */
    uint32_t accumulate_f32;        /* the table's dtype rule: every add rounds to float32 */
} rg_ope_poly_w;

/* rg_ope_poly_w_workspace_bytes: device workspace rg_ope_replay_poly_w needs (0 = error, see rg_last_error).
 * rg_ope_replay_poly_w: rows, offsets, the ps source, d_ratio / d_click / d_sums and the validation of the log as
 * rg_ope_replay_poly; d_act (optional, int32 per row) receives the act at every bandit row, organic rows are not written.
 * RG_EINVAL for a null model, model array or table, n outside 1 .. 32768, null d_t16 with n_users > 0 and rows that are not 16-byte
 * aligned; RG_ENOMEM for a workspace too small — all before a device is looked for.  Afterwards the workspace's first int64 words
 * hold rg_ope_replay_poly's in their places — [0] error bits, [1] acts computed (here: every bandit row), [2] decided on the step
 * table, [3] a lower index won, [4] unresolved acts, [5] non-zero when more than 4096 of them, [6] feature-list entries read — and
 * [7] the rows whose d_t16 lies outside [0, 32767] plus the acts at a row inside the range whose feature list met a clamped table
 * index (a view outside the range or AFTER the act — a clock that runs backwards inside a user — or a difference >= n): where it
 * is not 0 the ratios are not the reference's and the caller takes its host loop.  The unresolved acts follow from byte 256 as rg_ope_replay_poly's do, one entry per unresolved bandit row; the host
 * confirms them with recogym_amd.sim.weighted_replay_verify.  d_sums holds the same bits on every run.  Synchronises `stream` once. */
size_t rg_ope_poly_w_workspace_bytes(const rg_ope_poly_w* model, uint64_t n_users, uint32_t max_user_rows);
int rg_ope_replay_poly_w(const rg_ope_poly_w* model, const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users,
                         uint32_t max_user_rows, const uint16_t* d_t16, uint32_t ps_mode, const double* d_ps, double ps_const,
                         double* d_ratio, uint8_t* d_click, double* d_sums, int32_t* d_act, void* d_workspace, size_t workspace_bytes,
                         void* stream);

/*
 * Off-policy evaluation of an EpsilonGreedy target (agents/epsilon_greedy.py:30-71 with with_ps_all = True on the wrapper and the
 * inner agent).  `inner` is an rg_ope_policy of kind RG_POLICY_RANDOM_AGENT (the greedy action is its bounded draw of
 * (policy_seed, u, t)) or RG_POLICY_LAST_VIEW_TABLE (table[last organic product]).  Per bandit row: g = the inner action, the
 * explore coin from (eg.seed, u, t), and pi = what act()['ps-a'][a] holds on that branch —
 *   explored: epsilon * (pure_new && a == g ? 0.0 : prob_explore);   greedy: (1.0 - epsilon) * pi_inner[a]
 * — then r = pi / ps.  prob_explore is the host's 1.0 / (P - 1) (pure_new) or 1.0 / P.
 */
typedef struct rg_ope_eg {
    double epsilon;
    uint64_t seed;                  /* the wrapper's config.random_seed */
    uint32_t pure_new;
    uint32_t reserved;
    double prob_explore;
} rg_ope_eg;

/* rg_ope_replay_eg: rows, offsets, the ps source, d_ratio / d_click / d_sums and the workspace as rg_ope_replay (the same
 * skeleton: the sums are the same bits on every run).  Optional outputs, written on bandit rows only: d_greedy[row] (uint8) = 1
 * where the act was greedy, d_h0[row] (int32) = the inner action g (the `h0` the reference reports on explored acts).  The rows'
 * `t` must be the event index (a log with a float clock does not qualify: the target always draws).  RG_EINVAL for another inner
 * kind, a null table, epsilon outside [0, 1], pure_new with fewer than 2 products. */
size_t rg_ope_eg_workspace_bytes(const rg_ope_policy* inner, uint64_t n_users, uint32_t max_user_rows);
int rg_ope_replay_eg(const rg_ope_policy* inner, const rg_ope_eg* eg, const rg_event* d_rows, const int64_t* d_offsets,
                     uint64_t n_users, uint32_t max_user_rows, uint32_t ps_mode, const double* d_ps, double ps_const,
                     double* d_ratio, uint8_t* d_click, double* d_sums, uint8_t* d_greedy, int32_t* d_h0, void* d_workspace,
                     size_t workspace_bytes, void* stream);

/* The EpsilonGreedy target round a model (with_ps_all on the wrapper and the inner agent): the plain unit's replay — history, act,
 * workspace size and head words, the likelihood agent's unresolved list, the log validation — with the wrapper's pi per bandit
 * row: g = the model's action (shared by the bandit rows up to the next organic row), the explore coin of the row's own
 * (eg.seed, u, t), and
 *   explored: epsilon * (pure_new && a == g ? 0.0 : prob_explore);   greedy: (1.0 - epsilon) * (a == g ? 1.0 : 0.0).
 * d_greedy / d_h0: the optional outputs of rg_ope_replay_eg (h0 = g).  The workspace is rg_ope_logreg_workspace_bytes' /
 * rg_ope_poly_workspace_bytes'.  RG_EINVAL besides the plain unit's: a null eg, epsilon outside [0, 1], pure_new with fewer than 2
 * products, and (LogReg) select_randomly != 0.  With pure_new an unresolved act of the likelihood agent that the host refutes
 * changes pi on explored rows too: the caller gives the whole replay up, as for the plain unit. */
int rg_ope_replay_logreg_eg(const rg_ope_logreg* model, const rg_ope_eg* eg, const rg_event* d_rows, const int64_t* d_offsets,
                            uint64_t n_users, uint32_t max_user_rows, uint32_t ps_mode, const double* d_ps, double ps_const,
                            double* d_ratio, uint8_t* d_click, double* d_sums, uint8_t* d_greedy, int32_t* d_h0,
                            void* d_workspace, size_t workspace_bytes, void* stream);
int rg_ope_replay_poly_eg(const rg_ope_poly* model, const rg_ope_eg* eg, const rg_event* d_rows, const int64_t* d_offsets,
                          uint64_t n_users, uint32_t max_user_rows, uint32_t ps_mode, const double* d_ps, double ps_const,
                          double* d_ratio, uint8_t* d_click, double* d_sums, uint8_t* d_greedy, int32_t* d_h0,
                          void* d_workspace, size_t workspace_bytes, void* stream);

/*
 * Off-policy evaluation of NnIpsAgent's argmax form (NnIpsFrozenAgent, reference agents/nn_ips.py:111-137 with with_ps_all = True,
 * select_randomly off) and of BayesianAgentVB (BayesianVBFrozenAgent, reference agents/bayesian_poly_vb.py:71-91 with with_ps_all =
 * True): replay a sorted log under the model.  Stateless (no rg_sim handle).  The arrays are device arrays laid out as
 * rg_sim_set_nn_ips / rg_sim_set_bayes_vb take them.  The policy sees the user's cumulative view counts (all organic rows so far,
 * across sessions); the act is the step loop's (k_nn_acts / k_bayes_acts: the same order of operations, margin and flags),
 * pi = [action == a], r = pi / ps.  The sampling NN has no replay form (its `ps-a` is torch's fp32 softmax).
 */
typedef struct rg_ope_nn {
    uint32_t num_products;          /* P, 1 .. 4000 */
    uint32_t num_hidden;            /* H, 1 .. 1024 */
    const double* w1t;              /* [P][H] */
    const double* b1;               /* [H] */
    const double* w2t;              /* [H][H] */
    const double* b2;               /* [H] */
    const double* w3t;              /* [H][P] */
    const double* b3;               /* [P] */
} rg_ope_nn;

typedef struct rg_ope_bayes {
    uint32_t num_products;          /* P <= RG_EV_INDEX_MASK */
    uint32_t num_samples;           /* S >= 1; P P S doubles within 2 GiB */
    const double* lam_t;            /* [P][P][S], [viewed product][action][sample] */
} rg_ope_bayes;

/* rg_ope_nn_workspace_bytes / rg_ope_bayes_workspace_bytes: device workspace the unit's replay needs for n_users users the longest
 * of which has max_user_rows rows (0 = error, see rg_last_error).
 * rg_ope_replay_nn / rg_ope_replay_bayes: argument for argument rg_ope_replay_poly after the model, with its validation of the log
 * (RG_EINVAL before anything is written), its unresolved list from byte 256 — up to 4096 entries of three uint32 (user index,
 * position of the bandit row the act was computed at within the user's rows, action taken), in no fixed order: the acts flagged
 * RG_NN_UNRESOLVED (a count above 2^24 among them) / RG_BAYES_UNRESOLVED — and its rule that the ratios are written with the
 * device's action; a caller that needs the reference's action on such acts recomputes them on the host
 * (recogym_amd.sim.replay_verify).  RG_EINVAL also for a null model or array, num_hidden outside 1 .. 1024, num_products above 4000
 * (NN) or RG_EV_INDEX_MASK, num_samples == 0 or a model beyond 2 GiB, and an NN value that is not finite; RG_ENOMEM for a workspace
 * too small.  The first int64 words of the workspace afterwards:
 *   NN     [0] error bits (0), [1] acts computed, [2] unresolved acts, [3] non-zero when more than 4096 were, [4] w1t rows read;
 *   Bayes  [0] error bits (0), [1] acts computed, [2] acts decided in the saturated zone, [3] unresolved acts, [4] non-zero when
 *          more than 4096 were, [5] lam_t rows read.
 * d_sums holds the same bits on every run.  The Bayes unit synchronises `stream` once (the validation's verdict); the NN unit once
 * more before it: the library downloads the net for the margin's absolute row sums and the finiteness check, as rg_sim_set_nn_ips does.
 * rg_ope_replay_nn_eg / rg_ope_replay_bayes_eg: the EpsilonGreedy target round the model, argument for argument
 * rg_ope_replay_poly_eg after the model (the act is the wrapper's greedy action g; d_greedy / d_h0 as there). */
size_t rg_ope_nn_workspace_bytes(const rg_ope_nn* model, uint64_t n_users, uint32_t max_user_rows);
int rg_ope_replay_nn(const rg_ope_nn* model, const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users,
                     uint32_t max_user_rows, uint32_t ps_mode, const double* d_ps, double ps_const, double* d_ratio,
                     uint8_t* d_click, double* d_sums, void* d_workspace, size_t workspace_bytes, void* stream);
int rg_ope_replay_nn_eg(const rg_ope_nn* model, const rg_ope_eg* eg, const rg_event* d_rows, const int64_t* d_offsets,
                        uint64_t n_users, uint32_t max_user_rows, uint32_t ps_mode, const double* d_ps, double ps_const,
                        double* d_ratio, uint8_t* d_click, double* d_sums, uint8_t* d_greedy, int32_t* d_h0,
                        void* d_workspace, size_t workspace_bytes, void* stream);
size_t rg_ope_bayes_workspace_bytes(const rg_ope_bayes* model, uint64_t n_users, uint32_t max_user_rows);
int rg_ope_replay_bayes(const rg_ope_bayes* model, const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users,
                        uint32_t max_user_rows, uint32_t ps_mode, const double* d_ps, double ps_const, double* d_ratio,
                        uint8_t* d_click, double* d_sums, void* d_workspace, size_t workspace_bytes, void* stream);
int rg_ope_replay_bayes_eg(const rg_ope_bayes* model, const rg_ope_eg* eg, const rg_event* d_rows, const int64_t* d_offsets,
                           uint64_t n_users, uint32_t max_user_rows, uint32_t ps_mode, const double* d_ps, double ps_const,
                           double* d_ratio, uint8_t* d_click, double* d_sums, uint8_t* d_greedy, int32_t* d_h0,
                           void* d_workspace, size_t workspace_bytes, void* stream);

/*
 * Off-policy evaluation of PyTorchMLRAgent (PyTorchMLRFrozenAgent, reference agents/pytorch_mlr.py:59-84): replay a sorted log under
 * the model.  Stateless.  wt is a device array laid out as rg_sim_set_mlr takes it; the act is the step loop's (k_mlr_acts: the same
 * order of operations, margin and flags), pi = [action == a], r = pi / ps.
 * rg_ope_mlr_workspace_bytes / rg_ope_replay_mlr: argument for argument rg_ope_replay_nn after the model, with the same validation
 * of the log, the same unresolved list from byte 256 (the acts flagged RG_MLR_UNRESOLVED) and the same rule that the ratios are
 * written with the device's action.  RG_EINVAL also for a null model or array, num_products outside 1 .. 4000 and a value that is
 * not finite.  Head words: [0] error bits (0), [1] acts computed, [2] unresolved acts, [3] non-zero when more than 4096 were,
 * [4] wt rows read.  d_sums holds the same bits on every run.  Synchronises `stream` twice (the verdict of the finiteness
 * check, which runs on the device, and the validation's verdict).
 */
typedef struct rg_ope_mlr {
    uint32_t num_products;          /* P, 1 .. 4000 */
    const double* wt;               /* [P][P], [viewed product][action] */
} rg_ope_mlr;
size_t rg_ope_mlr_workspace_bytes(const rg_ope_mlr* model, uint64_t n_users, uint32_t max_user_rows);
int rg_ope_replay_mlr(const rg_ope_mlr* model, const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users,
                      uint32_t max_user_rows, uint32_t ps_mode, const double* d_ps, double ps_const, double* d_ratio,
                      uint8_t* d_click, double* d_sums, void* d_workspace, size_t workspace_bytes, void* stream);
/* rg_ope_replay_mlr_eg: argument for argument rg_ope_replay_nn_eg after the model (the act is the wrapper's greedy action g;
 * d_greedy / d_h0 as there), but served for epsilon = 0 only — the wrapper that never explores, through which recall@k obtains the
 * act of every bandit row (d_h0); any other epsilon is RG_EINVAL. */
int rg_ope_replay_mlr_eg(const rg_ope_mlr* model, const rg_ope_eg* eg, const rg_event* d_rows, const int64_t* d_offsets,
                         uint64_t n_users, uint32_t max_user_rows, uint32_t ps_mode, const double* d_ps, double ps_const,
                         double* d_ratio, uint8_t* d_click, double* d_sums, uint8_t* d_greedy, int32_t* d_h0,
                         void* d_workspace, size_t workspace_bytes, void* stream);

/*
 * recall@k (evaluate_recall_at_k, reference evaluate_agent.py:832-870) over a sorted log.  A bandit row i of user u is COUNTED
 * when it has no click, row i + 1 lies inside user u's range and row i + 1 is organic; it is a HIT when that row's product is
 * among the k largest entries of the target's `ps-a` at row i.  No row at or beyond d_offsets[n_users] is read.
 * d_hit[row] (uint8, written for EVERY row of the evaluated users): RG_RECALL_MISS, RG_RECALL_HIT, RG_RECALL_NOT_COUNTED
 * (organic rows too) or, from the ranking form only, RG_RECALL_UNRESOLVED.  d_sums (2 int64) = (counted rows, hits): integer
 * sums, the same on every run.
 */
#define RG_RECALL_MISS 0
#define RG_RECALL_HIT 1
#define RG_RECALL_NOT_COUNTED 2
#define RG_RECALL_UNRESOLVED 3
#define RG_OPE_RECALL_LIST_CAP 4096     /* default entries of the ranking form's list of unresolved rows */

/* The table form, for targets whose top-k SET is a function of a small key (a one-hot `ps-a`: the model's act; under EpsilonGreedy
 * the act and the explore flip; one constant vector): d_key[row] (int32, read on counted rows only) selects one of n_keys sets,
 * d_sets[key][0 .. k-1] (int32, ASCENDING within a key) holds the set the caller built — with NumPy's own np.argpartition on
 * the host, so that its order among ties is reproduced by construction — and the device only tests membership.  A counted row
 * whose key is outside [0, n_keys) is marked RG_RECALL_NOT_COUNTED and not counted (the caller builds the keys).  Stateless, no
 * workspace, enqueued on `stream`, no synchronisation.  RG_EINVAL: null arrays, k == 0, n_keys == 0, rows not 16-byte aligned. */
int rg_ope_recall_hits(const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users, const int32_t* d_key, uint32_t n_keys,
                       const int32_t* d_sets, uint32_t k, uint8_t* d_hit, int64_t* d_sums, void* stream);

/* The ranking form, for the sampling LogReg (rg_ope_logreg with select_randomly != 0: the preconditions and the validation of
 * the log are rg_ope_replay_logreg's), whose `ps-a` is a softmax: the replay's own float64 scores and e[j] = exp(s[j] - max),
 * then the rank rule on the e's of the row's act with v = the next organic view.  Two e's are ordered only where they differ by
 * more than 2^-48 relative and do not both lie under 2^-1000 (inside that margin the host's quotients may compare either way):
 *   HIT where at most k classes are not certainly below v;  MISS where at least k classes are certainly above v;
 *   RG_RECALL_UNRESOLVED otherwise: the row is counted in d_sums[0], not in d_sums[1], and appended to the list.
 * Workspace: the first int64 words hold [0] error bits (0), [1] acts computed, [2] the same, [3] coef_t rows read, [4] unresolved
 * rows, [5] non-zero when they outgrew the list; from byte 256 the list: up to list_cap (0 = RG_OPE_RECALL_LIST_CAP; at most
 * 2^20) entries of three uint32 (user index, position of the row within the user's rows, v), in no fixed order.  RG_EINVAL
 * besides rg_ope_replay_logreg's: select_randomly == 0, k outside 1 .. P.  Synchronises `stream` twice. */
size_t rg_ope_recall_logreg_workspace_bytes(const rg_ope_logreg* model, uint64_t n_users, uint32_t max_user_rows, uint32_t list_cap);
int rg_ope_recall_logreg(const rg_ope_logreg* model, const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users,
                         uint32_t max_user_rows, uint32_t k, uint32_t list_cap, uint8_t* d_hit, int64_t* d_sums,
                         void* d_workspace, size_t workspace_bytes, void* stream);

/*
 * The count agents' training (reference agents/organic_count.py:74-82, agents/bandit_count.py:49-62 under the offline protocol
 * of bench_agents.py:90-190): a sorted log reduced to P x P tables of 64-bit integer counters.  Stateless (no rg_sim handle).
 * The tables are caller-owned row-major int64 device arrays; either group (co_counts | pulls + clicks) may be NULL.
 *   co_counts[i][j] += views(i) * views(j) for every session: a maximal run of organic rows inside a user;
 *   pulls[ix][a] += 1, clicks[ix][a] += c for every bandit row (the phantom row included), ix = the last organic view in front
 *   of the PREVIOUS bandit row of the log, whichever user that row belongs to (the agent's last_product_viewed before the call
 *   looks at its own session).
 * Everything is an integer sum: the result does not depend on the order of the updates (the same bits on every run).
 */
typedef struct rg_count_tables {
    uint32_t num_products;          /* P <= RG_EV_INDEX_MASK */
    uint32_t reserved;
    int64_t* co_counts;             /* [P][P] or NULL */
    int64_t* pulls;                 /* [P][P] or NULL (with clicks) */
    int64_t* clicks;                /* [P][P] or NULL (with pulls) */
} rg_count_tables;

#define RG_COUNT_ORGANIC 0
#define RG_COUNT_BANDIT 1

/* rg_count_train: ADDS users 0 .. n_users-1 of a sorted log (user i = rows d_offsets[i] .. d_offsets[i+1]-1, each user's first
 * row organic) to the tables.  d_carry (4 int64, device): [0] in = BanditCount's last_product_viewed before the log (-1 = None),
 * out = after it, so that a second log continues where the first ended; [1] out = the action of the one bandit row that met
 * None (-1: there was none), [2] out = its click: NumPy's `pulls_a[None, a] += 1` adds to the WHOLE row a, and so does this
 * call (pulls[a][:] += 1, clicks[a][:] += c) before it returns; [3] reserved.  d_workspace: rg_count_workspace_bytes() bytes;
 * afterwards its int64 words hold [0] error bits (0), [1] cell updates the log stands for, [2] global atomics issued for them
 * (the rest was summed in LDS first).  Synchronises `stream` twice (it reads the validation's verdict before any table is
 * touched, and the error bits at the end).  RG_EINVAL: P out of range, a half-given pulls / clicks pair, a user whose first
 * row is a bandit row, a row whose product is >= P (such a row is never counted), a workspace too small (RG_ENOMEM). */
size_t rg_count_workspace_bytes(void);
int rg_count_train(const rg_count_tables* tables, const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users,
                   int64_t* d_carry, void* d_workspace, size_t workspace_bytes, void* stream);

/* rg_count_policy: the frozen policy of a trained count agent, per last viewed product l the FIRST index of the maximum of
 * co_counts[l][:] (kind RG_COUNT_ORGANIC; d_win_* are not written) or of (clicks[l][:] + 1) / (pulls[l][:] + 2) (RG_COUNT_BANDIT),
 * decided by exact integer cross-multiplication — the order of NumPy's rounded float64 quotients while pulls + 2 < 2^26, where
 * distinct fractions round to distinct doubles; d_win_clicks[l] / d_win_pulls[l] receive the winning cell's counters, from which
 * the caller takes the logged `ps` with its own float64 divide.  d_action: P int32; d_win_*: P int64.  No synchronisation. */
int rg_count_policy(const rg_count_tables* tables, uint32_t kind, int32_t* d_action, int64_t* d_win_clicks,
                    int64_t* d_win_pulls, void* stream);

/*
 * The epsilon-greedy evolution study (reference evaluate_agent.py:51-146): one step = one run, its log's statistics, and the
 * filtered train calls of the count agents.  Stateless (no rg_sim handle); rows / offsets as rg_count_train.
 *
 * rg_evolution_stats: over every bandit row that is not a phantom row (an ACT): the explore flip of (eg->seed, u, t) — the draw
 * rg_ope_replay_eg uses; eg = NULL: the acting agent has no wrapper, no act is greedy and none explored — then
 *   d_counts[0] += clicks, [1] += acts without a click, [2] += greedy acts with a click, [3] += greedy acts without;
 *   d_action_clicks[a] += 1 for every clicked act of action a (P int64);
 *   d_explored[row] (uint8, one per row of the log, optional) = 1 where the act explored, 0 on every other row.
 * Integer adds only: the same bytes on every run.  d_workspace: rg_evolution_workspace_bytes(P) bytes; the sums are staged there
 * and added to d_counts / d_action_clicks only when the log is valid.  Synchronises `stream` once.  RG_EINVAL: a user whose
 * first row is a bandit row, an index >= P, epsilon outside [0, 1] (nothing is added; d_explored is then unspecified);
 * RG_ENOMEM: a workspace too small.
 */
size_t rg_evolution_workspace_bytes(uint32_t num_products);
int rg_evolution_stats(const rg_ope_eg* eg, const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users,
                       uint32_t num_products, uint8_t* d_explored, int64_t* d_counts, int64_t* d_action_clicks, void* d_workspace,
                       size_t workspace_bytes, void* stream);

/*
 * rg_count_train_online: the train calls evaluate_agent makes, under a filter.  A row is COUNTED when it is a bandit row, not a
 * phantom row, and d_mask (uint8 per row of the log, NULL = all ones) lets it through; session(r) = the organic rows of r's user
 * between that user's previous bandit row (counted or not; else the user's first row) and r.
 *   co_counts += b b^T for every counted r with a non-empty session (b = its view counts); a session no counted row closes — a
 *   user's trailing organic rows, a session in front of a filtered-out or phantom row — is never counted;
 *   pulls[ix][a] += 1, clicks[ix][a] += c for every counted r, ix = last_product_viewed walked over the COUNTED rows in log
 *   order, across users: it moves to the last view of session(r) where that is non-empty, after r's own ix was taken.  Rows that
 *   meet ix = None (-1) add to the whole table row a, as NumPy's pulls_a[None, a] += 1 does; any number of rows may.
 * d_carry[0] (int64, device): in = last_product_viewed before the log (-1 = None), out = after it (written only when pulls is
 * given).  d_workspace: rg_count_online_workspace_bytes(P, n_users) bytes, 8-byte aligned; afterwards its int64 words hold [0]
 * error bits, [1] cell updates the log stands for, [2] global atomics issued for them.  Synchronises `stream` once: the whole log
 * is validated before any table is touched.  RG_EINVAL: P out of range, a half-given pulls / clicks pair, a user whose first
 * row is a bandit row, a row whose index is >= P, d_carry[0] >= P with pulls given (nothing is written in any of these cases);
 * RG_ENOMEM: a workspace too small.
 */
size_t rg_count_online_workspace_bytes(uint32_t num_products, uint64_t n_users);
int rg_count_train_online(const rg_count_tables* tables, const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users,
                          const uint8_t* d_mask, int64_t* d_carry, void* d_workspace, size_t workspace_bytes, void* stream);

/*
 * OrganicMFSquare's training (reference agents/organic_mf.py:80-116 under the offline protocol of bench_agents.py:168-190) from a
 * sorted device log; rows / offsets as rg_count_train, stateless.
 *
 * The train CALLS of a log: one per organic-only user (users 0 .. n_organic_users-1, the session = the user's organic rows), then
 * one per bandit row of every other user, the phantom row included (the session = the organic rows of that user since its previous
 * bandit row); a user's trailing organic rows belong to no call.  Call number k = first_call + 1 + (calls in front of it).  A call
 * with k % mini_batch == 0 is a TRIGGER: one optimiser step over the sessions stored since the previous trigger, its own session
 * is dropped.  A session [v0 .. vm] stands for the PAIRS (v0, v1) .. (v(m-1), vm).
 *
 * rg_omf_pairs writes, in log order: d_pairs = the (i, j) int32 pairs of every stored session, the n_pending pairs of d_pending
 * (carried in from an earlier log: they belong to the first step) in front; d_step_offsets[0 .. n_steps] = the CSR rows of the
 * n_steps triggers of the log (a step without pairs is an empty row), and d_step_offsets[n_steps + 1] = all pairs: the row
 * n_steps is what lies behind the last trigger, the caller's new pending set.  d_out (8 int64, device): [0] error bits (0), [1]
 * calls, [2] n_steps, [3] pairs written, [4] pairs of the pending row.  pairs_capacity >= n_pending + n_rows pairs (2 int32 each),
 * step_capacity >= (first_call % mini_batch + n_rows) / mini_batch + 2; d_workspace: what the workspace function answers for
 * (n_rows, n_pending), 8-byte aligned.  Integer work only: the same bytes on every run.  Synchronises `stream` once: the log is
 * validated before any output is written — RG_EINVAL for a user whose first row is a bandit row, an index >= num_products, an
 * organic-only user without rows or with a bandit row, offsets that descend or leave the n_rows rows, and more than 2^32 - 16 rows; RG_ENOMEM for
 * a capacity or a workspace too small.  d_out is read after the stream's work is done.
 */
size_t rg_omf_pairs_workspace_bytes(uint64_t n_rows, uint64_t n_pending);
int rg_omf_pairs(const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users, uint64_t n_organic_users, uint64_t n_rows,
                 uint32_t num_products, uint64_t first_call, uint32_t mini_batch, const int32_t* d_pending, uint64_t n_pending,
                 int32_t* d_pairs, uint64_t pairs_capacity, int64_t* d_step_offsets, uint64_t step_capacity, int64_t* d_out,
                 void* d_workspace, size_t workspace_bytes, void* stream);

/* The model of rg_omf_steps: float64 device arrays, read and written in place. */
typedef struct rg_omf_model {
    uint32_t num_products;          /* P <= 2048 */
    uint32_t embed_dim;             /* E <= 64 */
    double* emb;                    /* [P][E] nn.Embedding.weight */
    double* w;                      /* [P][E] nn.Linear.weight */
    double* bias;                   /* [P]    nn.Linear.bias */
    double* sq_emb;                 /* RMSprop's square averages of the three */
    double* sq_w;
    double* sq_bias;
} rg_omf_model;

/*
 * rg_omf_steps: every optimiser step of a pair list (d_pairs, d_step_offsets[0 .. n_steps] as rg_omf_pairs writes them) in one
 * launch of one workgroup.  A step with pairs: per distinct input i, logits = w emb[i] + bias, a max-shifted softmax,
 * G[i] = n_i softmax - N[i][.] (N[i][j] = how often the step holds the pair (i, j)); g_emb[i] = G[i] w, g_w = sum_i G[i]^T emb[i],
 * g_bias = sum_i G[i], the sums over i in ascending order; then torch's RMSprop step (no momentum, not centred) on all
 * 2 P E + P parameters: sq = alpha sq + (1 - alpha) g g, p -= lr g / (sqrt(sq) + eps) — a row of emb the step did not see has
 * g = 0.  A step without pairs changes nothing.  float64, no floating-point atomics: the same bits on every run.  The model lives
 * in LDS while P <= lds_max_products of the limits function (228 at E = 5), else in global memory (force_global != 0: there in any
 * case), up to max_products; the global form needs d_workspace of the workspace function's size, 8-byte aligned.  d_out (4 int64,
 * device): [0] error bits, [1] steps taken, [2] steps skipped as empty, [3] pairs consumed.  The list is validated on the device
 * before the model is touched: a pair with an index >= P (bit 2) or offsets that descend or leave n_pairs (bit 4) leave the model
 * as it was.  No synchronisation.  RG_EINVAL: P or E out of range, a null array, alpha outside [0, 1], eps < 0; RG_ENOMEM.
 */
int rg_omf_limits(uint32_t embed_dim, uint32_t* lds_max_products, uint32_t* max_products);
size_t rg_omf_steps_workspace_bytes(uint32_t num_products, uint32_t embed_dim);
int rg_omf_steps(const rg_omf_model* model, double lr, double alpha, double eps, const int32_t* d_pairs, uint64_t n_pairs,
                 const int64_t* d_step_offsets, uint64_t n_steps, uint32_t force_global, int64_t* d_out, void* d_workspace,
                 size_t workspace_bytes, void* stream);

/*
 * BanditMFSquare's training (reference agents/bandit_mf.py:89-126 under the offline protocol of bench_agents.py:168-190) from a
 * sorted device log; rows / offsets as rg_count_train, stateless.
 *
 * The train CALLS and their numbers k are rg_omf_pairs'.  Every call sets the last product viewed to the last view of its
 * session when the session is not empty; a user opens with an organic row (anything else is refused), so at a bandit row it is
 * the nearest organic row in front of it in the same user.  A call with k % mini_batch == 0 is a TRIGGER: one optimiser step over
 * the samples stored since the previous trigger, and it stores nothing itself; every other call with an action (a bandit row)
 * stores the TRIPLE (last product viewed, action, reward 0 / 1).
 *
 * rg_bmf_samples writes, in log order: d_triples = the int32 triples, the n_pending triples of d_pending (carried in from an
 * earlier log: they belong to the first step) in front; d_step_offsets as rg_omf_pairs writes them (rows 0 .. n_steps-1 the steps,
 * row n_steps what lies behind the last trigger).  d_out (8 int64, device): [0] error bits (0), [1] calls, [2] n_steps, [3]
 * triples written, [4] triples of the pending row, [5] the last view at the last call (-1: the log has no call).
 * triples_capacity >= n_pending + n_rows triples (3 int32 each), step_capacity >= (first_call % mini_batch + n_rows) / mini_batch
 * + 2; d_workspace: what the workspace function answers for (n_rows, n_pending), 8-byte aligned.  Integer work only: the same
 * bytes on every run.  Synchronises `stream` once: the log is validated before any output is written — RG_EINVAL for a user whose
 * first row is a bandit row, an index >= num_products (a view or an action), an organic-only user without rows or with a bandit
 * row, offsets that descend or leave the n_rows rows, and more than 2^32 - 16 rows; RG_ENOMEM for a capacity or a workspace too
 * small.  d_out is read after the stream's work is done.
 */
size_t rg_bmf_samples_workspace_bytes(uint64_t n_rows, uint64_t n_pending);
int rg_bmf_samples(const rg_event* d_rows, const int64_t* d_offsets, uint64_t n_users, uint64_t n_organic_users, uint64_t n_rows,
                   uint32_t num_products, uint64_t first_call, uint32_t mini_batch, const int32_t* d_pending, uint64_t n_pending,
                   int32_t* d_triples, uint64_t triples_capacity, int64_t* d_step_offsets, uint64_t step_capacity, int64_t* d_out,
                   void* d_workspace, size_t workspace_bytes, void* stream);

/* The model of rg_bmf_steps: float64 device arrays, read and written in place. */
typedef struct rg_bmf_model {
    uint32_t num_products;          /* P <= 16384 */
    uint32_t embed_dim;             /* E <= 64 */
    double* ep;                     /* [P][E] product_embedding.weight (indexed by the action) */
    double* eu;                     /* [P][E] user_embedding.weight (indexed by the last product viewed) */
    double* sq_ep;                  /* RMSprop's square averages of the two */
    double* sq_eu;
} rg_bmf_model;

/*
 * rg_bmf_steps: every optimiser step of a triple list (d_triples, d_step_offsets[0 .. n_steps] as rg_bmf_samples writes them) in
 * one launch of one workgroup.  A step with n > 0 samples (l_s, a_s, r_s): z_s = <ep[a_s], eu[l_s]>, the loss is the mean of
 * BCEWithLogits(z, r), so d_s = (sigmoid(z_s) - r_s) / n, computed from t = exp(-|z|) without cancellation: sigmoid(|z|) = 1 / (1 + t),
 * sigmoid(-|z|) = t / (1 + t), and sigmoid(z) - 1 = -sigmoid(-z); g_ep[a] = sum_{a_s = a} d_s eu[l_s], g_eu[l] = sum_{l_s = l} d_s ep[a_s], the sums in sample order; then torch's
 * RMSprop step (no momentum, not centred) on all 2 P E parameters: sq = alpha sq + (1 - alpha) g g, p -= lr g / (sqrt(sq) + eps) —
 * a row the step did not touch has g = 0.  A step without samples changes nothing.  float64, no floating-point atomics: the same
 * bits on every run.  The model lives in LDS while P <= lds_max_products of the limits function (245 at E = 5), else in global
 * memory (force_global != 0: there in any case), up to max_products; the global form needs d_workspace of the workspace function's
 * size, 8-byte aligned.  A step holds at most max_step samples (256).  d_out (4 int64, device): [0] error bits, [1] steps taken,
 * [2] steps skipped as empty, [3] samples consumed.  The list is validated on the device before the model is touched: an index
 * >= P (bit 2), offsets that descend or leave n_triples (bit 4), a reward that is not 0 / 1 (bit 64) or a step longer than
 * max_step (bit 128) leave the model as it was.  No synchronisation.  RG_EINVAL: P or E out of range, a null array, alpha outside
 * [0, 1], eps < 0; RG_ENOMEM.
 */
int rg_bmf_limits(uint32_t embed_dim, uint32_t* lds_max_products, uint32_t* max_products, uint32_t* max_step);
size_t rg_bmf_steps_workspace_bytes(uint32_t num_products, uint32_t embed_dim);
int rg_bmf_steps(const rg_bmf_model* model, double lr, double alpha, double eps, const int32_t* d_triples, uint64_t n_triples,
                 const int64_t* d_step_offsets, uint64_t n_steps, uint32_t force_global, int64_t* d_out, void* d_workspace,
                 size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RECOGYM_HIP_H */
