"""build()'s dependency list against what the sources include: an edit to any header must rebuild the library."""
import glob
import os
import re

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_quoted_include_is_a_build_dependency():
    csrc = os.path.join(ROOT, 'recogym_amd', 'csrc')
    deps = {os.path.realpath(p) for p in entry.build_deps()}
    assert deps and all(os.path.isfile(p) for p in deps)
    sources = glob.glob(os.path.join(csrc, '*.hip')) + glob.glob(os.path.join(csrc, '*.hpp'))
    assert len(sources) > len(entry.UNITS)
    units = {os.path.realpath(os.path.join(csrc, u + '.hip')) for u in entry.UNITS}      # (recogym_hip.hip, the one-unit build, includes them)
    headers = 0
    for src in sources:
        for name in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(src).read(), flags=re.M):
            resolved = os.path.realpath(os.path.join(os.path.dirname(src), name))
            if resolved in units:            # a source of build()'s own list
                continue
            headers += 1
            assert resolved in deps, f'{os.path.basename(src)} includes "{name}", which build_deps() does not list'
    assert headers >= len(entry.UNITS)       # every unit includes at least one of the shared headers
