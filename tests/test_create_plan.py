"""What rg_sim_create decides, pinned: the workspace size and every option rg_sim_get_option reads back, for the matrix of
configurations and RECOGYM_* switches of tests/make_golden_create_plan.py, against tests/golden/create_plan.json (recorded
from the create path as it was before it was restructured).  Host only: rg_sim_create does no device work."""
import pytest

import __graft_entry__ as graft
import make_golden_create_plan as plan
from recogym_amd import _abi


@pytest.fixture(scope='module')
def lib():
    graft.build()
    return _abi.load()


def test_rg_sim_create_decides_what_the_recorded_plan_says(lib, monkeypatch):
    golden = plan.load()
    all_cases = plan.cases()
    assert golden['names'] == list(plan.NAMES)
    assert golden['matrix_sha256'] == plan.matrix_sha256(), 'the matrix changed: run tests/make_golden_create_plan.py'
    assert len(golden['cases']) == len(all_cases)
    for name in plan.SWITCHES:
        monkeypatch.delenv('RECOGYM_' + name, raising=False)
    wrong = []
    for (c, env), (first, index) in zip(all_cases, golden['cases']):
        got_first, got = plan.observe(lib, c, env, monkeypatch.setenv, monkeypatch.delenv)
        want = golden['errors' if first < 0 else 'tuples'][index]
        if got_first != first or list(got) != want:
            diff = ('workspace_bytes' if first >= 0 else 'return code', first, got_first) if got_first != first else \
                [(n, w, g) for n, w, g in zip(plan.NAMES if first >= 0 else ('return code', 'error'), want, got) if w != g]
            wrong.append((c, env, diff))
    assert not wrong, f'{len(wrong)} of {len(all_cases)} cases differ (name, recorded, now); the first: {wrong[:5]}'
