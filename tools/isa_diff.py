"""Per-kernel comparison of two builds' device assembly (a refactor that must not change the code of a surviving kernel).
    for u in rg_*.hip: hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC [unit flags] --cuda-device-only -S -o DIR/u.s u.hip
    python tools/isa_diff.py DIR_A DIR_B ['OLD_NAME_REGEX=>NEW' ...]
One line per function (same / DIFF / gone / new), exit status 1 if a function that both builds have differs.  Compared: the
text between the function's label and its .Lfunc_end, without comments and section directives, with the function's index in local labels (.LBB<n>_,
.Lfunc_end<n>: it moves when an instantiation before it disappears) and its own mangled name replaced.  The optional arguments
rename demangled names of DIR_A (a dropped template argument: 'k_draw_f16w<(\\d+), (\\d+), 1>=>k_draw_f16w<\\1, \\2>')."""
import glob, os, re, subprocess, sys


def functions(directory, renames):
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, '*.s'))):
        name, body = None, []
        for line in open(path):
            m = re.match(r'(_Z\w+):', line)
            if m and name is None:
                name, body = m.group(1), []
            elif name and re.match(r'\.Lfunc_end\d+:', line):
                text = '\n'.join(body).replace(name, '@')
                out[(os.path.basename(path), name)] = re.sub(r'\.LBB\d+_', '.LBB_', text)
                name = None
            elif name:
                line = line.split(';')[0].rstrip()
                if line and line.split()[0] not in ('.section', '.text'):      # (a template's comdat section: not code)
                    body.append(line)
    keys = list(out)
    dem = subprocess.run(['c++filt'] + [k[1] for k in keys], capture_output=True, text=True).stdout.split('\n')
    res = {}
    for (unit, _), d in zip(keys, dem):
        d = d.replace('(anonymous namespace)::', '').split('(')[0].replace('void ', '')
        for pat, new in renames:
            d = re.sub(pat, new, d)
        res[(unit, d)] = out[(unit, _)]
    return res


a = functions(sys.argv[1], [r.split('=>') for r in sys.argv[3:]])
b = functions(sys.argv[2], [])
bad = 0
for k in sorted(set(a) | set(b)):
    state = 'gone' if k not in b else 'new' if k not in a else 'same' if a[k] == b[k] else 'DIFF'
    bad += state == 'DIFF'
    print(f'{state:4s} {k[0][:-2]:18s} {k[1]}  ({len((a.get(k) or b[k]).splitlines())} lines)')
sys.exit(1 if bad else 0)
