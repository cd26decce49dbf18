"""OrganicMFSquare without a GPU: the reference's bits through `train` and through the host route of `train_from_log`, its act
table and acts, the float64 restatement of the optimiser step against the reference's weights, the call and pair enumeration
against a plain walk of the log, and the ABI."""
import os
import re

import numpy as np
import pytest
import torch

import organic_mf_util as ou
from recogym_amd import _abi
from recogym_amd.agents import LastViewTableAgent, OrganicMFSquare, organic_mf_square_args
from recogym_amd.agents.organic_mf import log_pairs
from recogym_amd.envs.configuration import Configuration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ou.fixtures()
WEIGHTS = ('emb', 'w', 'b')


def config(meta, **over):
    return Configuration({**organic_mf_square_args, 'num_products': meta['num_products'], 'embed_dim': meta['embed_dim'],
                          'mini_batch_size': meta['mini_batch_size'], **over})


def logs_of(meta, cols):
    out = [(ou.log_columns(cols), meta['n_organic'])]
    if meta['n_users2']:
        out.append((ou.log_columns(cols, 'log2_'), 0))
    return out


def assert_reference_bits(agent, cols):
    for p, k in zip(agent._params(), WEIGHTS):
        assert np.array_equal(p.detach().numpy().view(np.uint32), cols[k].view(np.uint32)), k
    for p, k in zip(agent._params(), ('sq_emb', 'sq_w', 'sq_b')):
        assert np.array_equal(agent.optimizer.state[p]['square_avg'].numpy().view(np.uint32), cols[k].view(np.uint32)), k


def test_the_fixtures_are_the_cases_the_tests_need():
    assert NAMES == ['organic_mf_p10_mb4', 'organic_mf_p10_s0', 'organic_mf_p10_s01', 'organic_mf_p10_s01_org', 'organic_mf_p10_s0_org',
                     'organic_mf_p10_two', 'organic_mf_p40_e8']
    for name in NAMES:
        meta, _ = ou.load(name)
        assert meta['top_two_gap'] >= 100 * ou.TOL_F64_VS_REFERENCE          # the table comparison leaves out no product
    assert ou.load('organic_mf_p10_mb4')[0]['empty_steps'] > 0
    meta, _ = ou.load('organic_mf_p10_two')
    assert meta['n_users2'] and meta['calls'] > 0


# ---- 1. the reference's bits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_train_call_by_call_gives_the_reference_bits(name):
    meta, cols = ou.load(name)
    torch.manual_seed(meta['agent_seed'])
    agent = OrganicMFSquare(config(meta))                    # torch's default initialisation, the reference's construction order
    for p, k in zip(agent._params(), ('emb0', 'w0', 'b0')):
        assert np.array_equal(p.detach().numpy(), cols[k]), k
    for lc, n_org in logs_of(meta, cols):
        for call in ou.observations(lc['u'], lc['t'], lc['is_bandit'], lc['v'], lc['a'], np.nan_to_num(lc['c']), n_org):
            agent.train(*call)
    assert agent.curr_step == meta['calls']
    assert_reference_bits(agent, cols)


@pytest.mark.parametrize('name', NAMES)
def test_train_from_log_host_route_gives_the_reference_bits(name):
    meta, cols = ou.load(name)
    agent = OrganicMFSquare(config(meta), cols['emb0'], cols['w0'], cols['b0'])
    assert not agent.device_route() and not agent.accepts_device_log
    for lc, n_org in logs_of(meta, cols):
        agent.train_from_log(lc, n_org)
    assert agent.curr_step == meta['calls']
    assert_reference_bits(agent, cols)


def test_train_and_train_from_log_continue_each_other():
    meta, cols = ou.load('organic_mf_p10_two')
    agent = OrganicMFSquare(config(meta), cols['emb0'], cols['w0'], cols['b0'])
    (lc1, n_org), (lc2, _) = logs_of(meta, cols)
    for call in ou.observations(lc1['u'], lc1['t'], lc1['is_bandit'], lc1['v'], lc1['a'], np.nan_to_num(lc1['c']), n_org):
        agent.train(*call)
    assert agent.curr_step % agent.batch != 0 and agent.train_data          # the boundary lies inside a mini-batch
    agent.train_from_log(lc2, 0)
    assert_reference_bits(agent, cols)


def test_device_training_without_its_conditions_takes_the_host_route(monkeypatch):
    meta, cols = ou.load('organic_mf_p10_s01')
    from recogym_amd.agents import count_tables as ct
    monkeypatch.setattr(ct, 'device_present', lambda: False)
    agent = OrganicMFSquare(config(meta, device_training=True), cols['emb0'], cols['w0'], cols['b0'])
    assert not agent.device_route()
    agent.train_from_log(ou.log_columns(cols), meta['n_organic'])
    assert_reference_bits(agent, cols)
    other_loss = OrganicMFSquare(config(meta, device_training=True, loss_function=torch.nn.CrossEntropyLoss(reduction='sum')))
    other_opt = OrganicMFSquare(config(meta, device_training=True, optim_function=torch.optim.Adam))
    monkeypatch.setattr(ct, 'device_present', lambda: True)
    assert not other_loss.device_route() and not other_opt.device_route()


# ---- 2. the act table and the acts ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_act_table_and_acts_are_the_reference_s(name):
    from recogym_amd.envs.context import DefaultContext
    from recogym_amd.envs.observation import Observation
    from recogym_amd.envs.session import OrganicSessions
    meta, cols = ou.load(name)
    agent = OrganicMFSquare(config(meta, with_ps_all=True), cols['emb'], cols['w'], cols['b'])
    fz = agent.frozen()
    assert isinstance(fz, LastViewTableAgent) and fz.ps is None
    assert np.array_equal(fz.table, cols['table'])
    assert agent.ope_policy()['kind'] == _abi.RG_POLICY_LAST_VIEW_TABLE and agent.device_policy() is None       # with_ps_all: replay only
    plain = OrganicMFSquare(config(meta), cols['emb'], cols['w'], cols['b'])
    assert plain.device_policy()['policy'] == _abi.RG_POLICY_LAST_VIEW_TABLE and plain.device_policy()['policy_ps'] is None
    # the evaluation run, observation by observation
    u, t, z, v = cols['eval_u'], cols['eval_t'], cols['eval_z'], cols['eval_v']
    sessions, prev, acts = OrganicSessions(), None, 0
    for r in range(len(u)):
        if prev is not None and u[r] != prev:
            sessions = OrganicSessions()
        prev = u[r]
        ctx = DefaultContext(t[r], int(u[r]))
        if z[r] == 0:
            sessions.next(ctx, int(v[r]))
            continue
        act = agent.act(Observation(ctx, sessions), 0, False)
        assert act['a'] == cols['eval_a'][r] and act['ps'] == 1.0 == cols['eval_ps'][r]
        assert np.argmax(act['ps-a']) == cols['eval_psa'][r] and act['ps-a'].sum() == 1.0 and act['ps-a'].max() == 1.0
        sessions = OrganicSessions()
        acts += 1
    assert acts > 100


def test_cached_table_is_dropped_when_weights_change():
    meta, cols = ou.load('organic_mf_p10_s01')
    agent = OrganicMFSquare(config(meta), cols['emb0'], cols['w0'], cols['b0'])
    first = agent.frozen()
    assert agent.frozen() is first
    agent.train_from_log(ou.log_columns(cols), meta['n_organic'])
    assert agent.frozen() is not first and np.array_equal(agent.frozen().table, cols['table'])


# ---- 3. the float64 restatement of the step --------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_float64_restatement_stays_close_to_the_reference(name):
    meta, cols = ou.load(name)
    model, k, pending = ou.NumpyModel(cols['emb0'], cols['w0'], cols['b0']), 0, []
    for lc, n_org in logs_of(meta, cols):
        pairs, off, n_calls = log_pairs(lc['u'], lc['is_bandit'], lc['v'], n_org, k, meta['mini_batch_size'], pending)
        for s in range(len(off) - 2):
            model.step(pairs[off[s]:off[s + 1]], meta['learning_rate'])
        pending = pairs[off[-2]:off[-1]]
        k += n_calls
    dev = max(float(np.abs(x - cols[key]).max()) for x, key in zip(model.arrays(), WEIGHTS + ('sq_emb', 'sq_w', 'sq_b')))
    print(f'{name}: float64 restatement vs reference {dev:.3e} (fixture: {meta["float64_deviation"]:.3e})')
    assert dev <= ou.TOL_F64_VS_REFERENCE
    assert np.array_equal(model.table(), cols['table'])


# ---- 4. the call and pair enumeration ----------------------------------------------------------------------------------------------
def check_enumeration(u, is_b, v, n_org, first_call, mb, pending):
    calls = ou.walk_calls(u, is_b, v, n_org)
    steps, left = ou.walk_steps(calls, first_call, mb, [tuple(p) for p in pending])
    pairs, off, n_calls = log_pairs(u, is_b, v, n_org, first_call, mb, pending)
    assert n_calls == len(calls) and len(off) == len(steps) + 2 and off[0] == 0 and off[-1] == len(pairs)
    for s, want in enumerate(steps):
        assert [tuple(p) for p in pairs[off[s]:off[s + 1]].tolist()] == want, s
    assert [tuple(p) for p in pairs[off[-2]:off[-1]].tolist()] == left
    return len(steps), sum(len(s) == 0 for s in steps)


@pytest.mark.parametrize('name', NAMES)
def test_pair_enumeration_equals_a_walk_of_the_log(name):
    meta, cols = ou.load(name)
    lc, n_org, mb = ou.log_columns(cols), meta['n_organic'], meta['mini_batch_size']
    u, is_b, v = lc['u'], lc['is_bandit'], lc['v']
    n_calls = len(ou.walk_calls(u, is_b, v, n_org))
    pend = [(1, 2), (2, 2), (0, 3)]
    for first_call, pending in ((0, []), (mb - 1, pend), ((-n_calls) % mb, pend), (5 * mb + 3, [])):     # a trigger on the first / the last call
        n_steps, _ = check_enumeration(u, is_b, v, n_org, first_call, mb, pending)
        assert n_steps > 10
    # trailing organic rows: users that lose their last bandit row
    drop = np.zeros(len(u), dtype=bool)
    last = np.flatnonzero(np.r_[u[1:] != u[:-1], True])
    drop[last[n_org::3]] = is_b[last[n_org::3]]
    assert drop.sum() > 3
    check_enumeration(u[~drop], is_b[~drop], v[~drop], n_org, 7, mb, pend)


def test_pair_enumeration_refuses_what_the_protocol_cannot_produce():
    meta, cols = ou.load('organic_mf_p10_s0_org')
    lc = ou.log_columns(cols)
    u, is_b, v = lc['u'], lc['is_bandit'].copy(), lc['v'].copy()
    with pytest.raises(ValueError):
        log_pairs(u, is_b, v, meta['n_organic'] + 1, 0, 32)          # an "organic-only" user with bandit rows
    v2 = v.copy()
    v2[np.flatnonzero(~is_b)[5]] = 10
    with pytest.raises(ValueError):
        log_pairs(u, is_b, v2, meta['n_organic'], 0, 32, num_products=10)
    b2 = is_b.copy()
    b2[0] = True
    with pytest.raises(ValueError):
        log_pairs(u, b2, v, 0, 0, 32)


# ---- 5. the ABI ---------------------------------------------------------------------------------------------------------------------
def test_abi_exports_the_entry_points_and_keeps_its_version():
    import __graft_entry__ as graft
    graft.build()
    lib = _abi.load()
    for name in ('rg_omf_pairs_workspace_bytes', 'rg_omf_pairs', 'rg_omf_limits', 'rg_omf_steps_workspace_bytes', 'rg_omf_steps'):
        assert name in _abi.SYMBOLS and hasattr(lib, name)
    assert _abi.RG_ABI_VERSION == 15 == lib.rg_abi_version()
    header = open(os.path.join(ROOT, 'include', 'recogym_hip.h')).read()
    assert re.search(r'#define RG_ABI_VERSION 15\b', header) and 'v15, additive since: rg_omf_pairs_workspace_bytes' in header
    assert 'rg_organic_mf' in graft.UNITS and '#include "rg_organic_mf.hip"' in open(os.path.join(ROOT, 'recogym_amd', 'csrc', 'recogym_hip.hip')).read()
    import ctypes as C
    lds_max, p_max = C.c_uint32(0), C.c_uint32(0)
    assert lib.rg_omf_limits(5, C.byref(lds_max), C.byref(p_max)) == 0 and (lds_max.value, p_max.value) == (228, 2048)
    assert lib.rg_omf_limits(0, None, None) == -1 and lib.rg_omf_limits(65, None, None) == -1
    assert lib.rg_omf_pairs_workspace_bytes(1000, 10) >= 4 * (2 * 1001 + 1010 + 1) + 1000
    assert C.sizeof(_abi.RgOmfModel) == 56
    # the arguments are checked before a device is looked for
    model = _abi.RgOmfModel(4000, 5, 8, 8, 8, 8, 8, 8)
    assert lib.rg_omf_steps(C.byref(model), 0.01, 0.99, 1e-8, None, 0, C.c_void_p(8), 0, 0, C.c_void_p(8), None, 0, None) == -1
    assert b'num_products' in lib.rg_last_error()


# ---- the update's arithmetic, through a host compiler ------------------------------------------------------------------------------
RMSPROP_PROGRAM = r'''
#include <cstdio>
#include <cstdint>
#include <cstring>
#include "rg_omf_common.hpp"
int main() {
    double p = 0.37, sq = 1e-3;
    for (int i = 0; i < 200; ++i) {
        const double g = (i % 7 == 0) ? 0.0 : 0.05 * ((i * 37) % 11 - 5) + 1e-3 * i;
        rgomf::omf_rmsprop(p, sq, g, 0.01, 0.99, 1e-8);
        uint64_t a, b;
        std::memcpy(&a, &p, 8); std::memcpy(&b, &sq, 8);
        std::printf("%llx %llx\n", (unsigned long long)a, (unsigned long long)b);
    }
    std::printf("fits %d %d %zu\n", (int)rgomf::omf_lds_fits(228, 5), (int)rgomf::omf_lds_fits(229, 5), rgomf::omf_lds_bytes(10, 5, true));
    return 0;
}
'''


def test_rmsprop_update_through_a_host_compiler_equals_numpy(tmp_path):
    import shutil
    import subprocess
    cxx = shutil.which('g++')
    assert cxx, 'the test needs g++'
    src = tmp_path / 'omf_host.cpp'
    src.write_text(RMSPROP_PROGRAM)
    exe = tmp_path / 'omf_host'
    subprocess.check_call([cxx, '-O2', '-mfma', '-ffp-contract=off', '-Wno-unknown-pragmas', '-std=c++17', '-I',
                           os.path.join(ROOT, 'recogym_amd', 'csrc'), '-o', str(exe), str(src)])
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    model = ou.NumpyModel(np.zeros((1, 1)), np.zeros((1, 1)), np.array([0.37]), [np.zeros((1, 1)), np.zeros((1, 1)), np.array([1e-3])])
    p, sq = model.bias, model.sq[2]
    for i in range(200):
        g = np.array([0.0 if i % 7 == 0 else 0.05 * ((i * 37) % 11 - 5) + 1e-3 * i])
        before = p.copy()
        sq *= ou.ALPHA                                     # NumpyModel.step's update, statement for statement
        sq += (1.0 - ou.ALPHA) * g * g
        p -= 0.01 * (g / (np.sqrt(sq) + ou.EPS))
        if g[0] == 0.0:
            assert p[0] == before[0]                       # g = 0: the value stays, the average decays
        a, b = (int(x, 16) for x in lines[i].split())
        assert a == int(p.view(np.uint64)[0]) and b == int(sq.view(np.uint64)[0]), i
    assert lines[200].split() == ['fits', '1', '0', '3368']
