#!/usr/bin/env python3
"""isa_same.py OLD_DIR NEW_DIR -- are the kernels of two builds the same instructions?

Each directory holds one gfx950 listing per unit (<unit>.s from `hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S`).
A kernel is the text from `<name>:` to `.Lfunc_end`; block labels `.LBB<n>_` become `.LBB_`, `;` comments and blank lines go,
nothing else is normalised.  Prints kernels per unit on both sides, names in more than one unit, names on one side only and the
kernels that differ; exit status 1 unless both sides hold the same names, each in one unit, with the same text.
"""
import glob, os, re, sys


def kernels(directory):
    found, count, twice = {}, {}, []
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        text, unit = open(path).read(), os.path.basename(path)[:-2]
        names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
        count[unit] = len(names)
        for name in names:
            body = text.split("\n" + name + ":", 1)[1].split(".Lfunc_end", 1)[0]
            lines = [re.sub(r"\.LBB\d+_", ".LBB_", line.split(";", 1)[0]).rstrip() for line in body.split("\n")]
            if name in found:
                twice.append(name)
            found[name] = (unit, [line for line in lines if line.strip()])
    return found, count, twice


def main(old_dir, new_dir):
    (old, old_n, old_twice), (new, new_n, new_twice) = kernels(old_dir), kernels(new_dir)
    for side, n in (("before", old_n), ("after", new_n)):
        print(f"{side}: {sum(n.values())} kernels; " + ", ".join(f"{u} {k}" for u, k in n.items()))
    only = sorted(set(old) ^ set(new))
    differ = sorted(k for k in set(old) & set(new) if old[k][1] != new[k][1])
    print(f"in two units: {len(old_twice + new_twice)}", *(old_twice + new_twice))
    print(f"on one side only: {len(only)}", *only)
    print(f"differing: {len(differ)} of {len(set(old) & set(new))}")
    for k in differ:
        print(f"  {k}  ({old[k][0]} -> {new[k][0]}, {len(old[k][1])} -> {len(new[k][1])} lines)")
    return 1 if only or differ or old_twice or new_twice else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
