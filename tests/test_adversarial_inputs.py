"""CPU checks behind the adversarial certificate tests of tests/test_hip_parity.py: the helper's K -> kernel-class table is the
library's (rg_sim_create and rg_sim_get_option are host-only calls), every instantiated class is reached by some K, and the
adversarial inputs of every new shape are well posed from the float64 reference alone — what keeps a GPU test from passing by
leaving cases out."""
import numpy as np
import pytest

import __graft_entry__ as graft
import adversarial_util as au
from recogym_amd import _abi
from recogym_amd.envs.configuration import Configuration
from recogym_amd.envs.reco_env_v1 import env_1_args

# an instantiation no K selects (geom_of): k_draw_bf16<16, 4, 3, 2> — the (4, 3, 2) class needs 3K + 3 <= 64, K <= 20, and every
# K <= 20 has KH <= 10.  Recorded here; the kernel is left alone.
UNREACHABLE = {('bf16', (16, 4, 3, 2))}


@pytest.fixture(scope='module')
def lib():
    graft.build()
    return _abi.load()


def _choice(lib, K, sigma_omega):
    cfg = Configuration({**env_1_args, 'random_seed': 1, 'num_products': 40, 'K': K, 'sigma_omega': sigma_omega})
    h = au.host_sim(lib, cfg)
    if h is None:
        return None
    got = {k: au.host_option(lib, h, k) for k in ('draw_kh', 'draw_n1', 'draw_split', 'draw_kernel', 'draw_pipelined', 'xh_class')}
    lib.rg_sim_destroy(h)
    return got


@pytest.mark.parametrize('setting', list(au.SETTINGS))
def test_kernel_class_table_matches_the_library(lib, setting, monkeypatch):
    """adversarial_util.geom / expected_choice against draw_kh / draw_n1 / draw_split / draw_kernel / draw_pipelined of a handle
    created under the setting's environment, for every K in 1..128 (beyond K = 101 the library refuses the configuration)."""
    for k in ('RECOGYM_DRAW', 'RECOGYM_BF16', 'RECOGYM_F16W', 'RECOGYM_FORCE_EXACT', 'RECOGYM_XH', 'RECOGYM_CACHE'):
        monkeypatch.delenv(k, raising=False)
    for k, v in au.SETTINGS[setting].items():
        monkeypatch.setenv(k, v)
    for K in range(1, au.K_MAX + 1):
        got = _choice(lib, K, 0.01)
        if K > au.K_VALID:           # geom_of has a class for these (KH = 64), validate() refuses them first
            assert got is None and b'LDS budget' in lib.rg_last_error(), K
            continue
        KH, n1, split = au.geom(K, setting)
        use, pipelined = au.expected_choice(K, setting)
        assert (got['draw_kh'], got['draw_n1'], got['draw_split']) == (KH, n1, split), (K, got)
        assert (got['draw_kernel'], got['draw_pipelined']) == (use, pipelined), (K, got)
        assert got['xh_class'] == 0, (K, got)              # (omega drifts: no per-user cache, no k_sweep_xh)
    # the error-free sweep of the walked run (sigma_omega = 0): K <= 8 the (4, 1, 2) class, K <= 20 the (10, 2, 5) class
    for K in (3, 8, 9, 13, 20, 21, 40):
        want = 0
        if au.expected_choice(K, setting) == (2, 1) and au.geom(K, setting)[2] == au.SPLIT_F16 and K <= 20:
            want = 412 if K <= 8 else 1025
        assert _choice(lib, K, 0.0)['xh_class'] == want, (K, setting)


def test_every_instantiated_class_is_reached_by_some_K(lib, monkeypatch):
    """Every template instance in the `*_kernel_for` tables is selected by at least one K in 1..128 under some setting — from what
    the library reports, not from the helper's restatement — except the one recorded in UNREACHABLE."""
    reached = set()
    for setting in ('default', 'bf16'):
        for k in ('RECOGYM_DRAW', 'RECOGYM_BF16', 'RECOGYM_F16W'):
            monkeypatch.delenv(k, raising=False)
        for k, v in au.SETTINGS[setting].items():
            monkeypatch.setenv(k, v)
        for K in range(1, au.K_MAX + 1):
            got = _choice(lib, K, 0.01)
            if got is None:
                continue
            reached |= au.tables_serving(got['draw_kh'], got['draw_n1'], got['draw_split'])
    every = {(t, c) for t, cs in au.instantiated().items() for c in cs}
    assert len(every) == 7 + 6 + 4 + 4 + 5 + 9 + 4
    assert every - reached == UNREACHABLE


def test_ledger_names_are_read_only(lib):
    cfg = Configuration({**env_1_args, 'random_seed': 1, 'num_products': 40, 'K': 5})
    h = au.host_sim(lib, cfg)
    for name in au.FAMILIES:
        assert au.host_option(lib, h, 'launched_' + name) == 0               # nothing launched yet
        assert lib.rg_sim_set_option(h, ('launched_' + name).encode(), 1) == -1 and b'unknown option' in lib.rg_last_error()
    for name in au.DESCRIPTORS:
        assert lib.rg_sim_set_option(h, name.encode(), 1) == -1 and b'unknown option' in lib.rg_last_error()
    lib.rg_sim_destroy(h)


def test_class_representatives_are_the_expected_ones():
    """One K per class, derived from the table: 3, 8, 10, 13, 20, 21 (two-way fp16), 27, 35, 40, 64 (wide), 100 (fp32, KH = 64)."""
    assert [k for k, _ in au.class_ks('default', 'bf16p_f16') + au.class_ks('default', 'f16w')] == [3, 8, 10, 13, 20, 21, 27, 35, 40, 64]
    assert [k for k, _ in au.class_ks('default', 'tp') + au.class_ks('default', 'tpw')] == [3, 8, 10, 13, 20, 27, 35, 40, 64]
    assert [k for k, _ in au.class_ks('bf16', 'bf16p')] == [3, 8, 13, 20]
    assert [k for k, _ in au.class_ks('lean_bf16', 'bf16')] == [3, 8, 13, 20, 27, 40]
    assert au.fp32_ks() == [8, 20, 27, 64, 100]


def _shapes():
    lock = sorted({(P, K) for _, K, P in au.lockstep_cases()})
    walk = sorted({(P, K) for _, K, P in au.WALK_CASES})
    return [('lockstep', P, K) for P, K in lock] + [('walk', P, K) for P, K in walk]


@pytest.mark.parametrize('kind,P,K', _shapes())
def test_adversarial_inputs_are_well_posed(kind, P, K):
    """From the float64 reference alone: enough draws inside the band nothing may be certified in, enough far from every boundary,
    and nearly all clear of the float64 summation-order ambiguity."""
    margin = (au.lockstep_reference if kind == 'lockstep' else au.walk_reference)(P, K)[4]
    w = au.well_posed(margin)
    assert w['near'] >= 200 and w['far'] >= 20 and w['clear'] > 0.95, w
    if kind == 'lockstep' and au.geom(K)[0] == 64:
        # k_draw_mfma<64>: its documented band is wider than 1e-3 (fp32_documented_band); enough draws lie beyond both
        band = au.fp32_documented_band(P, K)
        assert np.median(band) > 1e-3 and ((margin > 1e-3) & (margin > band)).sum() >= 20
