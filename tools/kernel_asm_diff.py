#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel (a refactor must leave kept kernels alone).

  python tools/kernel_asm_diff.py OLD.s NEW.s [--drop KERNEL:I=V] ...

OLD.s / NEW.s: assembly of one translation unit from two builds (csrc/build/*.dev.s or *.pad.s).
Every kernel of NEW must have a counterpart in OLD with the same instruction stream and the same
.amdhsa_* directives (register counts, LDS and scratch sizes), after the function number in local
labels and the kernel's own symbol are normalised and comments dropped. Kernels are matched by
demangled name and template arguments; --drop gemm_bf16_kernel:6=16 removes template argument 6
(0-based) of OLD's gemm_bf16_kernel instantiations that have 16 there, for a parameter the refactor
fixed at that value and removed (instantiations with another value stay unmatched).
Prints the kernels only OLD has, grouped by name, and exits non-zero on any difference.
"""
import argparse
import collections
import re
import subprocess
import sys

CXXFILT = "c++filt"


def kernels(path):
    """{symbol: (instruction lines, amdhsa directive lines)} for every kernel of an assembly file."""
    lines = open(path).read().split("\n")
    names = [m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))]
    start = {l.split(":")[0]: i for i, l in enumerate(lines) if l[:1] not in ("", "\t", " ", ".", ";") and ":" in l}
    out = {}
    for name in names:
        code, hsa, in_hsa = [], [], False
        for l in lines[start[name] + 1:]:
            if re.match(r"\.Lfunc_end\d+:", l):
                break
            l = l.split(";")[0].rstrip().replace(name, "KERNEL")
            l = re.sub(r"\.LBB\d+_", ".LBB_", l)
            s = l.strip()
            if s.startswith(".amdhsa_kernel"):
                in_hsa = True
            elif s.startswith(".end_amdhsa_kernel"):
                in_hsa = False
            elif in_hsa:
                hsa.append(s)
            elif s and not s.startswith((".section", ".text")):  # (a template's comdat section is not code)
                code.append(l)
        out[name] = (code, hsa)
    return out


def demangle(syms):
    res = subprocess.run([CXXFILT], input="\n".join(syms), capture_output=True, text=True, check=True)
    return dict(zip(syms, res.stdout.split("\n")))


def key(dem, drops):
    """(kernel name, template arguments) of a demangled kernel; the kernels here take ints and bools only."""
    # (a kernel in an unnamed namespace demangles with "(anonymous namespace)::" in its qualified name)
    m = re.match(r"(?:void )?([\w:]+)(?:<([^<>]*)>)?\(", dem.replace("(anonymous namespace)::", ""))
    if not m:  # a symbol the demangler does not know (bf16 template arguments): matched by its mangled name
        return dem, ()
    name = m.group(1).split("::")[-1]
    args = [a.strip() for a in m.group(2).split(",")] if m.group(2) else []
    for i, v in sorted(drops.get(name, ()), reverse=True):
        if i < len(args) and args[i] == v:
            del args[i]
    return name, tuple(args)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--drop", action="append", default=[], metavar="KERNEL:I=V")
    a = ap.parse_args()
    drops = collections.defaultdict(list)
    for d in a.drop:
        k, iv = d.split(":")
        drops[k].append((int(iv.split("=")[0]), iv.split("=")[1]))
    old, new = kernels(a.old), kernels(a.new)
    dold, dnew = demangle(list(old)), demangle(list(new))
    by_key = collections.defaultdict(list)
    for s in old:
        by_key[key(dold[s], drops)].append(s)
    bad, used = 0, set()
    for s in new:
        k = key(dnew[s], {})
        cand = by_key.get(k, [])
        if len(cand) != 1:
            print(f"NO MATCH ({len(cand)} candidates): {dnew[s]}")
            bad += 1
            continue
        used.add(cand[0])
        bad += old[cand[0]] != new[s]
        for what, x, y in zip(("code", "amdhsa"), old[cand[0]], new[s]):
            if x != y:
                first = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
                print(f"DIFF {what}: {dnew[s]}\n  line {first} of {len(x)} / {len(y)}:\n  old: "
                      f"{x[first] if first < len(x) else '<end>'}\n  new: {y[first] if first < len(y) else '<end>'}")
    gone = collections.Counter(key(dold[s], {})[0] for s in old if s not in used)
    print(f"{a.new}: {len(new)} kernels, {len(new) - bad} identical to {a.old} ({len(old)} kernels)")
    for name, n in sorted(gone.items()):
        print(f"  only in old: {n:3d} x {name}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
