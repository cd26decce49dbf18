"""Shared pieces of the adversarial certificate tests (tests/test_hip_parity.py, tests/test_adversarial_inputs.py).

1. The float64 reference of an organic draw whose uniform sits next to a boundary of the user's own cdf
   (reco_env_v1.py:119-128 in numpy float64): logits -> cdf -> a boundary drawn by mass -> u = cdf[b] (1 +- eps), eps from
   1e-9 to 3e-3 -> the float64 decision `want_v` and `margin`, the distance of u to its two neighbouring boundaries relative to u.
2. A restatement of the K -> (KH, N1, split) table of the draw kernels (geom_of, recogym_amd/csrc/rg_common.hpp) and of the
   instantiation tables (`*_kernel_for`), which tests/test_adversarial_inputs.py holds against rg_sim_get_option on the CPU.
3. The launch ledger (rg_sim_get_option 'launched_<family>') read into a dict."""
import ctypes as C
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---------------------------------------------------------------------------------------------------------------------------
# 1. the float64 reference
# ---------------------------------------------------------------------------------------------------------------------------
N_USERS = 4096


@functools.lru_cache(maxsize=None)
def reference(P, K, config_seed, rng_seed, sigma_omega=None, n=N_USERS):
    """(cfg, omega, u, want_v, margin) of n users; computed once per shape and shared (the arrays are read-only)."""
    from recogym_amd.envs.configuration import Configuration
    from recogym_amd.envs.reco_env_v1 import env_1_args
    from recogym_amd.envs.static_params import draw_tables
    over = {'random_seed': config_seed, 'num_products': P, 'K': K}
    if sigma_omega is not None:
        over['sigma_omega'] = sigma_omega
    cfg = Configuration({**env_1_args, **over})
    gamma, mu_o, _, _ = draw_tables(cfg)
    rng = np.random.RandomState(rng_seed)
    omega = rng.standard_normal((n, K))
    # the reference's arithmetic (reco_env_v1.py:119-128) in float64
    logits = omega @ gamma.T + mu_o.reshape(1, -1)
    logits -= logits.max(axis=1, keepdims=True)
    e = np.exp(logits)
    prob = e / e.sum(axis=1, keepdims=True)
    cdf = np.cumsum(prob, axis=1)
    cdf /= cdf[:, -1:]
    # a boundary per user, drawn by mass (so that heavy and light products both occur), then u beside it
    b = np.array([np.searchsorted(cdf[i], rng.random_sample(), 'right') for i in range(n)])
    b = np.clip(b, 0, P - 2)
    eps = 10.0 ** rng.uniform(-9, -2.5, n)
    sign = rng.choice([-1.0, 1.0], n)
    u = np.clip(cdf[np.arange(n), b] * (1.0 + sign * eps), 0.0, np.nextafter(1.0, 0.0))
    want_v = np.array([np.searchsorted(cdf[i], u[i], 'right') for i in range(n)])
    # distance of u to its two neighbouring boundaries, relative to u
    lo = np.where(want_v > 0, cdf[np.arange(n), np.maximum(want_v - 1, 0)], -np.inf)
    hi = np.where(want_v < P - 1, cdf[np.arange(n), np.minimum(want_v, P - 1)], np.inf)     # (no boundary behind the last product)
    margin = np.minimum(u - lo, hi - u) / np.maximum(u, 1e-300)
    for a in (omega, u, want_v, margin):
        a.setflags(write=False)
    return cfg, omega, u, want_v, margin


def lockstep_reference(P, K):
    """The inputs of test_certificate_is_sound_* (one lock-step step, omega drifting: no per-user sum cache)."""
    return reference(P, K, 1234 + P + K, 99)


def walk_reference(P, K):
    """The inputs of test_walk_certificate_is_sound_* (sigma_omega = 0: the user-major walk)."""
    return reference(P, K, 4321 + P + K, 7, sigma_omega=0.0)


def well_posed(margin):
    """What the inputs must offer for the GPU assertions to mean something, from the reference alone."""
    return dict(near=int((margin < 5e-7).sum()), far=int((margin > 1e-3).sum()), clear=float((margin > 1e-12).mean()))


def fp32_documented_band(P, K):
    """Per user of lockstep_reference(P, K): the relative distance from a cdf boundary beyond which k_draw_mfma's certificate
    passes BY ITS DOCUMENTED BUDGET, from float64 quantities alone.  cert_correlated (rg_common.hpp) accepts u S - C[v-1] (and
    C[v] - u S) above delta' (u T + (1 - u) A + a|b) + rho S <= 2 delta' u S + rho S, i.e. margin > 2 delta' + rho / u, with
    delta = (K + 5) 2^-24 Ahat + 3e-5 + 6e-6 n_resc (search_and_emit), Ahat as ahat_of bounds the partial logits (the smaller of
    the per-coordinate bound and the joint Cauchy-Schwarz bound at the grid point at or above |omega|, with the device's
    round-ups), n_resc at most the re-references the logit range allows (one per 57 log2 units above the first chunk's maximum).
    The budget grows with K Ahat: at K = 100 it is ~8e-4, so draws 1e-3 from a boundary are inside the band by design."""
    from recogym_amd.envs.static_params import draw_tables
    cfg, omega, u, want_v, margin = lockstep_reference(P, K)
    gamma, mu_o, _, _ = draw_tables(cfg)
    mu = np.asarray(mu_o, dtype=np.float64).reshape(-1)
    absdot = np.abs(omega) @ np.abs(gamma).max(axis=0)
    r = np.sqrt((omega * omega).sum(axis=1)) * 1.000001
    gnorm = np.sqrt((gamma * gamma).sum(axis=1))
    grid = np.maximum(np.ceil(r * 4.0), 1.0) * 0.25
    joint = (np.abs(mu)[None, :] + gnorm[None, :] * grid[:, None]).max(axis=1) * (1.0 + 1e-6)
    joint = np.minimum(joint, np.abs(mu).max() * (1.0 + 1e-6) + gnorm.max() * (1.0 + 1e-6) * r)
    ahat = np.minimum(np.abs(mu).max() * (1.0 + 1e-6) + absdot, joint) * 1.00001
    logits = omega @ gamma.T + mu[None, :]
    n_resc = np.floor((logits.max(axis=1) - logits[:, :32].max(axis=1)) * 1.4426950408889634 / 57.0)
    delta = (K + 5) * 2.0 ** -24 * ahat + 3.0e-5 + 6.0e-6 * n_resc
    band = 2.0 * delta * (1.0 + 2.0 * delta) + 9.5463e-7 / np.maximum(u, 1e-300)
    band.setflags(write=False)
    return band


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the class tables
# ---------------------------------------------------------------------------------------------------------------------------
KH_OPTS = (4, 10, 16, 32, 64)
BF16_CLASSES = ((1, 1, 1), (2, 1, 1), (3, 2, 1), (4, 3, 2), (6, 4, 2), (12, 8, 4))     # (N1, N2, N3) of the three-way split
SPLIT_NONE, SPLIT_BF16, SPLIT_F16, SPLIT_F16_WIDE = 0, 1, 2, 3
K_MAX = 128
K_VALID = 101        # rg_sim_create refuses K > 101 (the float64 tile kernel's LDS budget): geom_of's classes up to K = 128 end there

# environment of each way to choose the split (geom_of reads RECOGYM_DRAW = bf16 and RECOGYM_BF16 = lean; the other RECOGYM_DRAW
# values choose among the kernels of one geometry)
SETTINGS = {
    'default': {},
    'f16': {'RECOGYM_DRAW': 'f16'},
    'fp32': {'RECOGYM_DRAW': 'fp32'},
    'f64': {'RECOGYM_DRAW': 'f64'},
    'bf16': {'RECOGYM_DRAW': 'bf16'},
    'lean': {'RECOGYM_BF16': 'lean'},
    'lean_bf16': {'RECOGYM_BF16': 'lean', 'RECOGYM_DRAW': 'bf16'},
}
THREE_WAY = ('bf16', 'lean', 'lean_bf16')


def geom(K, setting='default'):
    """(KH, N1, split) as geom_of computes them; (0, 0, 0): K > 128, float64 only."""
    need = (K + 1) // 2
    KH = next((o for o in KH_OPTS if need <= o), 0)
    if not KH:
        return 0, 0, SPLIT_NONE
    n1 = next((c[0] for c in BF16_CLASSES if 3 * K + 3 <= 16 * c[0] and 2 * K <= 16 * c[1] and K <= 16 * c[2]), 0)
    split = SPLIT_BF16 if n1 else SPLIT_NONE
    if setting not in THREE_WAY:
        if 3 * K + 1 <= 64 and KH <= 16:
            n1, split = (3 * K + 1 + 15) // 16, SPLIT_F16
        elif 21 < K <= 64 and KH in (16, 32):
            n1, split = (7 if 3 * K + 1 <= 112 else 10 if 3 * K + 1 <= 160 else 13), SPLIT_F16_WIDE
    return KH, n1, split


def n23(n1):
    return next(c[1:] for c in BF16_CLASSES if c[0] == n1)


@functools.lru_cache(maxsize=None)
def instantiated():
    """{table: set of template-argument tuples} parsed from the RG_CASE lists of the `*_kernel_for` functions; bf16p's two lists
    are 'bf16p_f16' (KH, N1) and 'bf16p' (KH, N1, N2, N3)."""
    csrc = os.path.join(ROOT, 'recogym_amd', 'csrc')
    out = {}
    for unit, names in (('rg_draw_fp32.hip', ('bf16',)), ('rg_draw_pipelined.hip', ('bf16p',)), ('rg_draw_wide.hip', ('f16w',)),
                        ('rg_draw_lds.hip', ('tp', 'pick', 'tpw'))):
        src = open(os.path.join(csrc, unit)).read()
        for name in names:
            body = src[src.index(f'draw_kernel_t {name}_kernel_for('):]
            body = body[:body.index('\n}\n')]
            cases = {tuple(int(x) for x in m.split(',')) for m in re.findall(r'RG_CASE\(([\d, ]+)\)', body)}
            if name == 'bf16p':
                out['bf16p_f16'] = {c for c in cases if len(c) == 2}
                out['bf16p'] = {c for c in cases if len(c) == 4}
            else:
                out[name] = cases
    return out


def tables_serving(KH, n1, split):
    """The (table, class) pairs a K of this geometry can select."""
    if split == SPLIT_BF16:
        c = (KH, n1) + n23(n1)
        return {('bf16', c), ('bf16p', c)}
    if split == SPLIT_F16:
        return {(t, (KH, n1)) for t in ('bf16p_f16', 'tp', 'pick')}
    if split == SPLIT_F16_WIDE:
        return {(t, (KH, n1)) for t in ('f16w', 'tpw', 'pick')}
    return set()


# the K that stands for its class in the GPU tests: one per (KH, N1) class of the 16-bit sweeps, K = 100 for the fp32 kernel's KH = 64
PREFERRED_K = (3, 8, 10, 13, 20, 21, 27, 35, 40, 64, 100)


def classes(setting):
    """{(KH, N1, split): [K, ...]} of the 16-bit classes under a setting, over K = 1..128."""
    out = {}
    for K in range(1, K_MAX + 1):
        g = geom(K, setting)
        if g[2] != SPLIT_NONE:
            out.setdefault(g, []).append(K)
    return out


def representative(ks):
    """The largest K of PREFERRED_K in a class's K range (a table change that empties a range fails here, not silently)."""
    hit = [k for k in PREFERRED_K if k in ks]
    assert hit, f'no preferred K in {ks[0]}..{ks[-1]}'
    return hit[-1]


def class_ks(setting, table):
    """[(K, (KH, N1, split))] — the representative K of every class under `setting` that `table` instantiates, by K."""
    inst = instantiated()[table]
    out = []
    for g, ks in classes(setting).items():
        if any(t == table and c in inst for t, c in tables_serving(*g)):
            out.append((representative(ks), g))
    return sorted(out)


def fp32_ks():
    """The largest preferred K of every KH of the fp32 MFMA kernel."""
    by_kh = {}
    for K in PREFERRED_K:
        by_kh[geom(K)[0]] = K
    return sorted(by_kh.values())


def expected_choice(K, setting):
    """(draw_kernel, draw_pipelined) rg_sim_create must report for K under a setting: 0 float64 only, 1 fp32 MFMA, 2 a 16-bit
    sweep; a RECOGYM_DRAW value that no class serves falls back without a word, which is why the tests read it back."""
    KH, n1, split = geom(K, setting)
    inst = instantiated()
    kernel = pipelined = False
    if split == SPLIT_BF16:
        c = (KH, n1) + n23(n1)
        kernel = c in inst['bf16']
        if 'lean' not in setting and c in inst['bf16p']:
            kernel = pipelined = True
    elif split == SPLIT_F16:
        kernel = pipelined = (KH, n1) in inst['bf16p_f16']
    elif split == SPLIT_F16_WIDE:
        kernel = (KH, n1) in inst['f16w']
    use = 0 if not KH else 2 if kernel and (split in (SPLIT_F16, SPLIT_F16_WIDE) or (n1 <= 4 and KH <= 10)) else 1
    draw = SETTINGS[setting].get('RECOGYM_DRAW')
    if draw == 'f64':
        use = 0
    elif draw == 'fp32' and KH:
        use = 1
    elif draw in ('bf16', 'f16') and kernel:
        use = 2
    return use, int(pipelined)


def tile_sizes(split):
    """P with a ragged last tile over several tiles: 4 x 128 + 33 (the smallest table the LDS-search sweep serves) and 2049;
    the wide classes' tiles hold 64 products: 5 x 64 + 1."""
    return (321, 2049) if split == SPLIT_F16_WIDE else (545, 2049)


def lockstep_cases():
    """[(form, K, P)] of test_certificate_is_sound_for_every_kernel_class: a K per class of every table, in every form that
    reaches it at 4096 users."""
    out = []
    sweeps16 = class_ks('default', 'bf16p_f16') + class_ks('default', 'f16w')
    lds = class_ks('default', 'tp') + class_ks('default', 'tpw')
    for form, ks in (('sliced', sweeps16), ('fused', sweeps16), ('lds', lds), ('bf16', class_ks('bf16', 'bf16p')),
                     ('lean', class_ks('lean_bf16', 'bf16'))):
        out += [(form, K, P) for K, g in ks for P in tile_sizes(g[2])]
    out += [('fp32', K, P) for K in fp32_ks() for P in tile_sizes(SPLIT_NONE)]
    return out


FORM_ENV = {
    'sliced': {},
    'fused': {'RECOGYM_SLICES': '1', 'RECOGYM_SWEEP_LDS': '0'},
    'lds': {'RECOGYM_SLICES': '1'},
    'fp32': {'RECOGYM_DRAW': 'fp32'},
    'bf16': {'RECOGYM_DRAW': 'bf16'},
    'lean': {'RECOGYM_BF16': 'lean', 'RECOGYM_DRAW': 'bf16'},
}

# (walk form, K, P): the walk of every K class it is compiled for.  default: run_walk with k_walk2 (KH <= 16); k_walk: the only walk
# of KH = 32; pipe: run_walk_pipe, whose sweep is k_sweep_xh in its two classes (K = 3: (4, 1, 2), K = 13: (10, 2, 5)), pipe_xh8:
# eight waves per block
WALK_CASES = ([('default', K, P) for K in (3, 10, 13, 21, 27) for P in (640, 545)] +
              [('k_walk', K, P) for K in (40, 64) for P in (640, 545)] +
              [('pipe', K, P) for K in (3, 13) for P in (640, 545)] + [('pipe_xh8', 13, 545)])


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the ledger
# ---------------------------------------------------------------------------------------------------------------------------
FAMILIES = ('draw_f64', 'draw_fp32', 'draw16_fused', 'draw16_sliced', 'search', 'draw_tp', 'pick', 'draw_cached', 'sweep_xh',
            'exact_m', 'exact_tile', 'exact_h', 'walk', 'walk2', 'walk_solo', 'advance', 'advance_run', 'tail', 'repack', 'env0',
            'logreg_screen', 'logreg_acts', 'logreg_sample', 'sort_tiled', 'sort_plain', 'logreg_poly', 'logreg_poly_w', 'bayes_vb',
            'nn_ips')
DESCRIPTORS = ('draw_kh', 'draw_n1', 'draw_split', 'draw_kernel', 'draw_pipelined', 'xh_class', 'xh_waves', 'sweep_lds_kernel')
DRAW_FAMILIES = ('draw_f64', 'draw_fp32', 'draw16_fused', 'draw16_sliced', 'draw_tp', 'draw_cached', 'sweep_xh', 'env0')


def ledger(sim):
    """Launch counts per kernel family since the Simulator was created, and the create-time choice."""
    return {k: sim.get_option(k if k in DESCRIPTORS else 'launched_' + k) for k in FAMILIES + DESCRIPTORS}


def assert_draws_by(led, *families):
    """The organic draws (first sweeps) were launched by exactly these families."""
    for f in DRAW_FAMILIES:
        if f in families:
            assert led[f] > 0, (f, led)
        else:
            assert led[f] == 0, (f, led)


_host_buf = [(C.c_char * 1)()]


def host_sim(lib, cfg, n_users=16, **pol):
    """rg_sim_create on a host buffer (no device: rg_sim_create and rg_sim_get_option are host-only calls).  Returns the handle
    (rg_sim_destroy it), None where the library refuses the configuration.  The buffer is the module's, shared by every handle:
    one handle at a time."""
    from recogym_amd.envs.static_params import make_rg_config
    rc = make_rg_config(cfg, 1, **pol)
    need = lib.rg_sim_workspace_bytes(C.byref(rc), n_users)
    if need == 0:                    # the configuration is refused (rg_last_error says why)
        return None
    if need + 256 > len(_host_buf[0]):           # one buffer for every handle of a test (a fresh one is zero-filled: ~200 MB each time)
        _host_buf[0] = (C.c_char * (need + 256))()
    base = (C.addressof(_host_buf[0]) + 255) // 256 * 256
    h = C.c_void_p()
    assert lib.rg_sim_create(C.byref(h), C.byref(rc), n_users, C.c_void_p(base), need) == 0, lib.rg_last_error()
    return h


def host_option(lib, h, name):
    v = C.c_int64(0)
    assert lib.rg_sim_get_option(h, name.encode(), C.byref(v)) == 0, lib.rg_last_error()
    return v.value
