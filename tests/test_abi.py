"""The C-ABI library loads on a CPU-only box and exports every symbol include/recogym_hip.h
declares; without a device the compute entry points fail loudly (no CPU fallback)."""
import ctypes as C
import os
import re

import pytest

import __graft_entry__ as graft
from recogym_amd import _abi
from recogym_amd.envs.configuration import Configuration
from recogym_amd.envs.reco_env_v1 import env_1_args
from recogym_amd.envs.static_params import make_rg_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    graft.build()
    return _abi.load()


def test_every_declared_symbol_is_exported(lib):
    header = open(os.path.join(ROOT, 'include', 'recogym_hip.h')).read()
    body = header[header.index('typedef struct rg_sim rg_sim;'):]
    declared = set(re.findall(r'\b(rg_[a-z_0-9]+)\s*\(', body))
    assert declared, 'no declarations parsed'
    assert declared == set(_abi.SYMBOLS), declared ^ set(_abi.SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.rg_abi_version() == _abi.RG_ABI_VERSION


def test_config_struct_layout_matches_header(lib):
    # sizeof(rg_config): 2*4 + 2*8 + 6*8 + 2*8 + 2*4 + 4*4 + 8 + (2*4 + 2*8: time generator)
    assert C.sizeof(_abi.RgConfig) == 152
    assert C.sizeof(_abi.RgEvent) == 16


def test_integration_stub_declares_the_current_config_struct():
    """The ctypes stub INTEGRATION.md shows a reference maintainer must declare struct rg_config exactly as the header
    (and the package's own mirror) does: same fields, same order, same types, 152 bytes — a short struct would have
    the library read time_mode past its end."""
    md = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    block = md[md.index('class RgConfig(C.Structure)'):]
    block = block[:block.index('lib = C.CDLL')]
    ns = {'C': C}
    exec(block, ns)
    stub = ns['RgConfig']
    assert C.sizeof(stub) == C.sizeof(_abi.RgConfig) == 152
    assert [(n, C.sizeof(t)) for n, t in stub._fields_] == [(n, C.sizeof(t)) for n, t in _abi.RgConfig._fields_]
    assert [getattr(stub, n).offset for n, _ in stub._fields_] == [getattr(_abi.RgConfig, n).offset for n, _ in _abi.RgConfig._fields_]
    header = open(os.path.join(ROOT, 'include', 'recogym_hip.h')).read()
    struct = header[header.index('typedef struct rg_config {'):header.index('} rg_config;')]
    names = re.findall(r'^\s*(?:uint32_t|uint64_t|double)\s+([a-zA-Z_0-9]+)(?:\[\d+\])*;', struct, flags=re.M)
    assert names == [n for n, _ in stub._fields_], names
    m = re.search(r'rg_abi_version\(\) == (\d+)', md)
    assert m and int(m.group(1)) == _abi.RG_ABI_VERSION


def test_workspace_and_validation(lib):
    cfg = make_rg_config(Configuration({**env_1_args, 'random_seed': 1}), 1)
    n = lib.rg_sim_workspace_bytes(C.byref(cfg), 1000)
    assert n > 0 and n % 256 == 0
    bad = make_rg_config(Configuration({**env_1_args, 'random_seed': 1, 'K': 0}), 1)
    assert lib.rg_sim_workspace_bytes(C.byref(bad), 1000) == 0
    assert b'K' in lib.rg_last_error()
    h = C.c_void_p()
    assert lib.rg_sim_create(C.byref(h), C.byref(cfg), 1000, None, 0) == -1   # RG_EINVAL


def test_no_cpu_fallback(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    assert lib.rg_device_count() == 0
    from recogym_amd.sim import Simulator
    with pytest.raises(_abi.RecoGymHipError):
        Simulator(Configuration({**env_1_args, 'random_seed': 1}), 10)
    # the raw ABI refuses too
    cfg = make_rg_config(Configuration({**env_1_args, 'random_seed': 1}), 1)
    need = lib.rg_sim_workspace_bytes(C.byref(cfg), 16)
    buf = (C.c_char * (need + 256))()
    base = (C.addressof(buf) + 255) // 256 * 256
    h = C.c_void_p()
    assert lib.rg_sim_create(C.byref(h), C.byref(cfg), 16, C.c_void_p(base), need) == 0
    assert lib.rg_sim_set_tables(h, C.c_void_p(base), C.c_void_p(base), C.c_void_p(base),
                                 C.c_void_p(base), None) == -2           # RG_ENODEV
    lib.rg_sim_destroy(h)


def test_run_options_are_set_by_name_not_by_the_environment_at_run_time(lib, monkeypatch):
    """rg_sim_create takes the run-path knobs' initial values from the RECOGYM_* environment once; afterwards
    rg_sim_set_option / rg_sim_get_option are the way to them (host-only calls: no device needed)."""
    monkeypatch.setenv('RECOGYM_EXACT_MIX', '6')
    monkeypatch.setenv('RECOGYM_WALK_HANDOVER', '48')
    cfg = make_rg_config(Configuration({**env_1_args, 'random_seed': 1, 'sigma_omega': 0.0}), 1)
    need = lib.rg_sim_workspace_bytes(C.byref(cfg), 16)
    buf = (C.c_char * (need + 256))()
    base = (C.addressof(buf) + 255) // 256 * 256
    h = C.c_void_p()
    assert lib.rg_sim_create(C.byref(h), C.byref(cfg), 16, C.c_void_p(base), need) == 0
    v = C.c_int64(0)
    assert lib.rg_sim_get_option(h, b'exact_mix', C.byref(v)) == 0 and v.value == 6
    assert lib.rg_sim_get_option(h, b'walk_handover', C.byref(v)) == 0 and v.value == 48
    monkeypatch.setenv('RECOGYM_EXACT_MIX', '3')                       # too late: the handle has its options
    assert lib.rg_sim_get_option(h, b'exact_mix', C.byref(v)) == 0 and v.value == 6
    assert lib.rg_sim_set_option(h, b'exact_mix', 4) == 0
    assert lib.rg_sim_get_option(h, b'exact_mix', C.byref(v)) == 0 and v.value == 4
    assert lib.rg_sim_set_option(h, b'pipe_groups', 0) == 0 and lib.rg_sim_set_option(h, b'walk_bias', 6) == 0
    assert lib.rg_sim_set_option(h, b'pipe_groups', 2) == -1 and b'pipe_groups' in lib.rg_last_error()
    assert lib.rg_sim_get_option(h, b'walk_bias', C.byref(v)) == 0 and v.value == 6
    assert lib.rg_sim_set_option(h, b'exact_mix', 9) == -1 and b'exact_mix' in lib.rg_last_error()
    assert lib.rg_sim_set_option(h, b'pipe_occ1', 0) == -1
    assert lib.rg_sim_set_option(h, b'no_such_option', 1) == -1 and b'no_such_option' in lib.rg_last_error()
    # round 4: the rounds of a run to the end (events per user and round; 0 = lock-step) and the LogReg screen's scratch rows
    assert lib.rg_sim_get_option(h, b'run_ahead', C.byref(v)) == 0 and v.value == 32
    assert lib.rg_sim_set_option(h, b'run_ahead', 0) == 0 and lib.rg_sim_get_option(h, b'run_ahead', C.byref(v)) == 0 and v.value == 0
    assert lib.rg_sim_get_option(h, b'lr_part_cap', C.byref(v)) == 0 and v.value == 0          # (not a LogReg policy: no rows)
    assert lib.rg_sim_set_option(h, b'lr_part_cap', 5) == -1 and b'lowered' in lib.rg_last_error()
    lib.rg_sim_destroy(h)
