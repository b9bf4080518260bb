#!/usr/bin/env python3
"""Are the gfx950 kernels of two trees the same code?  (no GPU needed)

    python tools/kernel_diff.py OLD_TREE [--old pem_kernels.hip] [--new pem_kernels.hip pem_radii.hip pem_stages.hip]

Compiles the named csrc/*.hip files of OLD_TREE (another checkout, e.g. a `git worktree` of the parent commit) and of this tree to
device assembly -- each with its own tree's tools/kernel_stats.py, so with its own headers -- and compares, function by function
(kernels and the out-of-line device functions they call), the instruction stream and the .amdhsa_* resource block.  Only symbol
names, labels and comments are normalised; `--rename 'regex=replacement'` maps demangled names that changed on purpose.
Prints the kernel count and "identical", or the names that differ / exist on one side only; exit status 1 then."""
import argparse
import importlib.util
import re
import sys
from pathlib import Path


def functions(root: Path, files, renames):
    spec = importlib.util.spec_from_file_location(f'kernel_stats_{abs(hash(root))}', root / 'tools' / 'kernel_stats.py')
    ks = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ks)
    out, kernels = {}, set()

    names = {}

    def name_of(sym):
        if sym not in names:
            names[sym] = ks.demangle(sym)
            for pat, to in renames:
                names[sym] = re.sub(pat, to, names[sym])
        return names[sym]
    for f in files or sorted(p.name for p in ks.CSRC.glob('*.hip')):
        asm = ks.assembly(ks.CSRC / f, [])
        asm = re.sub(r'_Z\w+', lambda m: '<' + name_of(m.group(0)) + '>', asm)
        for m in re.finditer(r'^(<[^\n]*>):[^\n]*\n(.*?)^\.Lfunc_end\d+:', asm, re.S | re.M):
            labels = {}
            body = [re.sub(r'\.L\w+', lambda l: labels.setdefault(l.group(0), f'.L{len(labels)}'), line.split(';')[0].rstrip())
                    for line in m.group(2).splitlines()]
            out[m.group(1)] = ['\n'.join(b for b in body if b.strip())]
        for m in re.finditer(r'^\s*\.amdhsa_kernel (<[^\n]*>)\n(.*?)\.end_amdhsa_kernel', asm, re.S | re.M):
            out[m.group(1)].append(m.group(2))
            kernels.add(m.group(1))
    return out, kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('old_tree')
    ap.add_argument('--old', nargs='*', default=[], help='files of csrc/ in the old tree (default: every .hip)')
    ap.add_argument('--new', nargs='*', default=[], help='files of csrc/ in this tree (default: every .hip)')
    ap.add_argument('--rename', action='append', default=[], help="regex=replacement applied to every demangled name")
    args = ap.parse_args()
    renames = [r.split('=', 1) for r in args.rename]
    old, old_k = functions(Path(args.old_tree).resolve(), args.old, renames)
    new, new_k = functions(Path(__file__).resolve().parents[1], args.new, renames)
    lost, added = sorted(old_k - new_k), sorted(new_k - old_k)
    differ = sorted(k for k in old.keys() & new.keys() if old[k] != new[k])
    only = sorted(k for k in old.keys() ^ new.keys() if k not in old_k | new_k)
    print(f'{len(old_k)} kernels before, {len(new_k)} after, {len(old.keys() & new.keys())} functions compared: '
          + ('identical' if not (lost or added or differ or only) else 'DIFFERENT'))
    for title, names in (('kernels lost', lost), ('kernels new', added), ('device functions on one side only', only),
                         ('instructions or resources differ', differ)):
        for n in names:
            print(f'  {title}: {n}')
    return 1 if lost or added or differ or only else 0


if __name__ == '__main__':
    sys.exit(main())
