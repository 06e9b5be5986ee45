"""Compare the device code of two sets of gfx950 assembly files kernel by kernel (developer tool): the check that moving
kernels between translation units changed none of them.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S UNIT.hip -o UNIT.s      # once per unit, both trees
    python tools/kernel_diff.py OLD.s [OLD2.s ...] -- NEW.s [NEW2.s ...]

Kernels are matched by DEMANGLED name (a unit's position-dependent manglings may differ).  Per kernel it compares the
`.amdhsa_*` resource block (VGPRs, AGPR offset, SGPRs, LDS, scratch, ...) and the instruction stream with comments
stripped, symbols demangled and local labels (`.LBB<n>_<m>`: n is the function's index in its unit) renumbered in
order of appearance.  Exit status 0: every old kernel exists exactly once among the new ones, no others, all equal.
"""
import re
import subprocess
import sys


def demangler(texts):
    names = sorted({m for t in texts for m in re.findall(r'\b_Z\w+', t)})
    out = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True, check=True).stdout.split('\n')
    return dict(zip(names, out))


def clean(lines, dem):
    """comments and blank lines dropped, symbols demangled, local labels renumbered by first appearance"""
    labels, out = {}, []
    for line in lines:
        line = line.split(';')[0].strip()
        if not line:
            continue
        line = re.sub(r'\b_Z\w+', lambda m: dem[m.group(0)], line)
        line = re.sub(r'\.L[A-Za-z_]+\d+(?:_\d+)?', lambda m: labels.setdefault(m.group(0), '.L%d' % len(labels)), line)
        out.append(re.sub(r'\s+', ' ', line))
    return out


def kernels(paths):
    """demangled name -> list of (file, resource block, instruction stream), one entry per definition"""
    texts = {p: open(p).read() for p in paths}
    dem = demangler(texts.values())
    found = {}
    for p, text in texts.items():
        lines = text.split('\n')
        for i, line in enumerate(lines):
            m = re.match(r'\s*\.amdhsa_kernel\s+(\S+)', line)
            if not m:
                continue
            sym = m.group(1)
            end = next(j for j in range(i, len(lines)) if lines[j].strip() == '.end_amdhsa_kernel')
            start = next(j for j in range(len(lines)) if lines[j].startswith(sym + ':'))
            stop = next(j for j in range(start, len(lines)) if re.match(r'\s*\.section\b', lines[j]))
            found.setdefault(dem[sym], []).append((p, clean(lines[i + 1:end], dem), clean(lines[start + 1:stop], dem)))
    return found


def main():
    args = sys.argv[1:]
    if '--' not in args:
        sys.exit(__doc__)
    cut = args.index('--')
    old, new = kernels(args[:cut]), kernels(args[cut + 1:])
    n_old, n_new = sum(map(len, old.values())), sum(map(len, new.values()))
    bad = 0
    for name in sorted(set(old) | set(new)):
        o, n = old.get(name, []), new.get(name, [])
        if len(o) != 1 or len(n) != 1:
            print('COUNT   %d old, %d new (%s): %s' % (len(o), len(n), ', '.join(f for f, _, _ in n) or '-', name))
            bad += 1
            continue
        (_, ores, oins), (nfile, nres, nins) = o[0], n[0]
        if ores != nres:
            print('RESOURCE %s [%s]: %s' % (name, nfile, sorted(set(ores) ^ set(nres))))
        if oins != nins:
            at = next((k for k, (x, y) in enumerate(zip(oins, nins)) if x != y), min(len(oins), len(nins)))
            print('CODE    %s [%s]: %d vs %d lines, first difference at line %d: %r vs %r'
                  % (name, nfile, len(oins), len(nins), at, oins[at:at + 1], nins[at:at + 1]))
        bad += ores != nres or oins != nins
    per_file = {}
    for defs in new.values():
        for f, _, ins in defs:
            c = per_file.setdefault(f, [0, 0])
            c[0] += 1
            c[1] += len(ins)
    print('old: %d kernels in %d files, %d instruction-stream lines' % (n_old, cut, sum(len(d[2]) for v in old.values() for d in v)))
    for f, (k, ins) in per_file.items():
        print('new: %s: %d kernels, %d instruction-stream lines' % (f, k, ins))
    print('new: %d kernels in all; %d kernels differ, are missing, extra or duplicated' % (n_new, bad))
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
