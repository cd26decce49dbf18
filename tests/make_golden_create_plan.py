"""Writes tests/golden/create_plan.json: what rg_sim_create decides — the workspace size and every option rg_sim_get_option
reads back — for a matrix of configurations and RECOGYM_* switches, from the library as it is built now.

    python tests/make_golden_create_plan.py          (host only: needs no GPU)

The file pins the create path for a restructuring: tests/test_create_plan.py replays the same matrix (`cases()` below) and
compares every case.  Layout: `names` (the options read per case, in order: the settable ones, then the read-only ones),
`tuples` (the distinct option tuples, each as [index into `settable`, index into `read_only`]: the distinct values of the two
halves), `errors` (the distinct [return code, rg_last_error text] pairs of refused configurations) and per case, in the order of
`cases()`, [workspace_bytes, index into tuples] or, for a refused configuration, [return code (< 0), index into errors].
`matrix_sha256` is the hash of the cases' descriptions (a matrix edited without regenerating the file shows there),
`generated_at` the commit.  `load()` gives the file back with the tuples spelled out."""
import ctypes as C
import hashlib
import itertools
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OUT = os.path.join(HERE, 'golden', 'create_plan.json')

SETTABLE = ('walk_bias', 'walk_refill', 'walk_handover', 'walk_click_batch', 'walk_search_batch', 'walk_helpers',
            'walk_click_join', 'walk_line64', 'pipe_groups', 'pipe_occ1', 'pipe_occ2', 'pipe_xblocks', 'pipe_min_users',
            'exact_mix', 'exact_tile', 'slices', 'sweep_prefix_off', 'tail_below', 'repack_every', 'run_ahead', 'lr_part_cap',
            'sweep_lds', 'debug')
READ_ONLY = ('sweep_lds_kernel', 'draw_kh', 'draw_n1', 'draw_split', 'draw_kernel', 'draw_pipelined', 'xh_class', 'xh_waves',
             'walk_form', 'walk_occ', 'walk_solo', 'use_cache', 'fin_in_sweep', 'handover_auto', 'draw_smem', 'mfma_smem',
             'xh_smem', 'tp_smem', 'tp_nts', 'tp_cpt', 'draw_threads', 'exact_rows', 'hist_cap', 'repack_min', 'ablate')
NAMES = SETTABLE + READ_ONLY

# every RECOGYM_* variable the library reads -> its legal values, then the out-of-range and junk ones
SWITCHES = {
    'EXACT_TILE': ('1', '0'), 'EXACT_MIX': ('0', '3', '8', '11'), 'SLICES': ('-1', '1', '4'), 'SWEEP_PREFIX_OFF': ('1',),
    'DEBUG': ('1',), 'WALK_HIST': ('1', '0'), 'BF16': ('lean', 'zzz'), 'DRAW': ('f64', 'fp32', 'bf16', 'f16', 'zzz'),
    'FORCE_EXACT': ('1', '0'), 'XH_WAVES': ('4', '8', '6'), 'XH_SMEM_PAD': ('20000',), 'SWEEP_LDS': ('0', '1'),
    'WALK': ('0', '1', '2'), 'WALK_HANDOVER': ('0', '16', '48'), 'WALK_CLICK_BATCH': ('4', '16'), 'WALK_CLICK_JOIN': ('0', '1'),
    'WALK_HELPERS': ('0', '3', '7', '9', '-1'), 'WALK_SEARCH_BATCH': ('12', '0'), 'WALK_REFILL': ('4',), 'WALK_BIAS': ('6', '0'),
    'WALK_SOLO': ('0', '1'), 'PIPE': ('0', '1', '2'), 'PIPE_OCC1': ('1', '2', '3', '9', '0'), 'PIPE_OCC2': ('1', '2', '3', '9', '0'),
    'PIPE_XBLOCKS': ('256', '0'), 'FIN_IN_SWEEP': ('0', '1'), 'PIPE_MIN': ('256', '1000000', '100'), 'TAIL': ('0', '100'),
    'REPACK': ('0', '8'), 'RUN_AHEAD': ('0', '8'), 'LR_PART_CAP': ('1000', '100000000'), 'ABLATE': ('3',), 'LDS_PAD': ('1024',),
    'SORT_PLAIN': ('1',), 'REPACK_MIN': ('500', '0'), 'F16W': ('0', '1'), 'XH': ('0', '1'), 'CACHE': ('0', '1'),
}
PAIRS = (
    {'WALK': '1'}, {'WALK_HELPERS': '0'}, {'WALK_HELPERS': '0', 'WALK_SEARCH_BATCH': '12'}, {'WALK_BIAS': '6', 'WALK_HELPERS': '0'},
    {'DRAW': 'bf16', 'BF16': 'lean'}, {'DRAW': 'f64', 'CACHE': '0'}, {'FORCE_EXACT': '1', 'DRAW': 'f16'},
    {'XH': '0', 'XH_WAVES': '8'}, {'TAIL': '100'}, {'RUN_AHEAD': '8'}, {'REPACK_MIN': '500'}, {'LDS_PAD': '1024'},
    {'XH_SMEM_PAD': '20000'}, {'SWEEP_LDS': '0'},
)


def _c(K=20, P=1000, sigma=0.0, policy=0, n=200000, **fields):
    return dict(K=K, P=P, sigma=sigma, policy=policy, n=n, **fields)


# the configurations every switch is tried on: the walked shapes, k_draw_tp's and k_draw_tpw's drift shapes, the frozen LogReg,
# K = 65, reco-gym-v0, a small population, a table below k_draw_tp's four tiles, a wide K with a cache, the likelihood agent,
# per-user clocks and a sampling LogReg
REDUCED = (
    _c(K=5, policy=0), _c(K=5, policy=1), _c(K=20, P=10000, policy=2), _c(K=20, P=10000, policy=4),
    _c(K=20, P=10000, sigma=0.1), _c(K=40, P=100000, sigma=0.1), _c(K=20, P=10000, policy=5), _c(K=65, P=10000),
    _c(K=1, policy=2, env_kind=1), _c(K=20, P=10000, n=1000), _c(K=8, P=300, sigma=0.1, policy=1), _c(K=32, P=12800),
    _c(K=20, sigma=0.1, policy=6), _c(K=20, P=10000, time_mode=1), _c(K=20, policy=5, lr_select_randomly=1),
)

OUC = dict(K=20, P=1000, policy=2)
SPECIALS = (
    [_c(K=K, P=P, sigma=s, policy=p, time_mode=1) for K, P, s, p in ((20, 10000, 0.0, 0), (20, 10000, 0.1, 2), (5, 1000, 0.0, 5), (40, 100000, 0.1, 1))]
    + [_c(K=1, P=P, policy=p, n=n, env_kind=1) for P in (10, 1000) for p in (0, 1, 2, 3) for n in (1000, 200000)]
    + [_c(sigma=s, change_omega_for_bandits=1) for s in (0.0, 0.1)]
    + [_c(**OUC, ouc_epsilon=0.3), _c(**OUC, ouc_exploit_explore=0), _c(**OUC, ouc_select_randomly=0),
       _c(**OUC, ouc_history_cap=8), _c(**OUC, ouc_history_cap=40000), _c(**OUC, ouc_history_cap=40000, n=1000)]
    + [_c(policy=5, lr_select_randomly=1), _c(policy=5, lr_select_randomly=1, n=1000)]
    # one refused configuration of each kind validate names
    + [dict(null=1, n=1000), _c(P=0), _c(P=1 << 29), _c(K=0), _c(K=1025), _c(K=128), _c(K=102), _c(n=0), _c(n=1 << 31), _c(policy=7),
       _c(time_mode=2), _c(env_kind=2), _c(policy=0, lr_select_randomly=1), _c(P=2000, policy=5, lr_select_randomly=1),
       _c(K=1, env_kind=1, time_mode=1), _c(K=1, env_kind=1, policy=5), _c(K=1, env_kind=1, policy=4), _c(K=1, env_kind=1, policy=6),
       _c(time_mode=1, time_sigma=-1.0), _c(time_mode=1, time_sigma=float('nan')), _c(cdf0=(0.9, 0.5, 1.0)), _c(cdf1=(0.5, 1.5, 1.0)),
       _c(cdf0=(-0.1, 0.5, 1.0))]
)


def cases():
    """-> [(configuration dict, environment dict)] in the order of the file's `cases`."""
    out = []
    for K, P, s, p, n in itertools.product((1, 2, 5, 7, 8, 20, 21, 22, 32, 33, 40, 53, 64, 65, 128),
                                           (10, 300, 1000, 10000, 12800, 100000), (0.0, 0.1), range(7), (1000, 200000)):
        out.append((_c(K=K, P=P, sigma=s, policy=p, n=n), {}))
    out += [(c, {}) for c in SPECIALS]
    for name, values in SWITCHES.items():
        out += [(c, {name: v}) for v in values for c in REDUCED]
    out += [(c, env) for env in PAIRS for c in REDUCED]
    return out


def matrix_sha256():
    return hashlib.sha256(json.dumps(cases(), sort_keys=True).encode()).hexdigest()


def rg_config(c):
    from recogym_amd import _abi
    cfg = _abi.RgConfig()
    cfg.num_products, cfg.K, cfg.seed, cfg.policy_seed = c['P'], c['K'], 1, 1
    for row, key, default in ((0, 'cdf0', (0.9, 0.99, 1.0)), (1, 'cdf1', (0.02, 0.99, 1.0))):
        for j, x in enumerate(c.get(key, default)):
            cfg.trans_cdf[row][j] = x
    cfg.sigma_omega_initial, cfg.sigma_omega, cfg.policy = 1.0, c['sigma'], c['policy']
    cfg.ouc_select_randomly, cfg.ouc_exploit_explore = c.get('ouc_select_randomly', 1), c.get('ouc_exploit_explore', 1)
    cfg.time_sigma = c.get('time_sigma', 1.0)
    for f in ('change_omega_for_bandits', 'ouc_history_cap', 'ouc_epsilon', 'time_mode', 'env_kind', 'lr_select_randomly'):
        setattr(cfg, f, c.get(f, 0))
    return cfg


def observe(lib, c, env, setenv, delenv):
    """One case -> (workspace_bytes, option tuple) or (return code, (return code, error text)).  `setenv` / `delenv` change the
    process environment (os.environ's or monkeypatch's); every variable set is removed again."""
    for k, v in env.items():
        setenv('RECOGYM_' + k, v)
    try:
        ref = None if c.get('null') else C.byref(rg_config(c))
        need = lib.rg_sim_workspace_bytes(ref, c['n'])
        h = C.c_void_p()
        rc = lib.rg_sim_create(C.byref(h), ref, c['n'], C.c_void_p(1 << 20), need)      # (create does not touch the memory)
        if rc != 0:
            assert need == 0 and not h.value, (c, env, need)
            return rc, (rc, lib.rg_last_error().decode())
        v = C.c_int64(0)
        values = []
        for name in NAMES:
            assert lib.rg_sim_get_option(h, name.encode(), C.byref(v)) == 0, name
            values.append(v.value)
        lib.rg_sim_destroy(h)
        return need, tuple(values)
    finally:
        for k in env:
            delenv('RECOGYM_' + k)


def load():
    """-> the file's document with `tuples` as full lists of values, in the order of `names`."""
    doc = json.load(open(OUT))
    doc['tuples'] = [doc['settable'][i] + doc['read_only'][j] for i, j in doc['tuples']]
    return doc


def main():
    import __graft_entry__ as graft
    from recogym_amd import _abi
    graft.build()
    lib = _abi.load()
    for k in [k for k in os.environ if k.startswith('RECOGYM_') and k[8:] in SWITCHES]:
        del os.environ[k]
    all_cases = cases()
    seen = [observe(lib, c, env, os.environ.__setitem__, os.environ.__delitem__) for c, env in all_cases]
    tuples, errors, rows = {}, {}, []
    for first, second in seen:
        table = errors if first < 0 else tuples
        rows.append([first, table.setdefault(second, len(table))])
    # a switch that changes nothing on any of its configurations pins nothing (RECOGYM_SORT_PLAIN, which no option reads back, is
    # listed for completeness)
    plain = {json.dumps(c, sort_keys=True): r for (c, env), r in zip(all_cases, seen) if not env}
    for name in SWITCHES:
        changed = any(r != plain[json.dumps(c, sort_keys=True)] for (c, env), r in zip(all_cases, seen) if list(env) == [name])
        if not changed and name != 'SORT_PLAIN':
            raise SystemExit(f'RECOGYM_{name} changes nothing on the reduced set')
    halves = ({}, {})
    for t in tuples:
        halves[0].setdefault(t[:len(SETTABLE)], len(halves[0]))
        halves[1].setdefault(t[len(SETTABLE):], len(halves[1]))
    head = subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    dirty = subprocess.run(['git', 'status', '--porcelain', '--', 'recogym_amd', 'include'], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    doc = {'generated_at': head + (' + uncommitted changes to the library sources' if dirty else ''),
           'matrix_sha256': matrix_sha256(), 'names': list(NAMES),
           'settable': [list(t) for t in halves[0]], 'read_only': [list(t) for t in halves[1]],
           'tuples': [[halves[0][t[:len(SETTABLE)]], halves[1][t[len(SETTABLE):]]] for t in tuples], 'errors': [list(e) for e in errors], 'cases': rows}
    with open(OUT, 'w') as f:
        f.write('{\n' + ',\n'.join(f'"{k}": ' + json.dumps(v, separators=(',', ':')) for k, v in doc.items()) + '\n}\n')
    print(f'{len(rows)} cases, {len(tuples)} option tuples, {len(errors)} refusals, {os.path.getsize(OUT)} bytes -> {OUT}')


if __name__ == '__main__':
    main()
