#!/usr/bin/env python3
"""Diff the device code of two builds of druggen_amd/csrc, kernel by kernel.

    for f in druggen_amd/csrc/*.hip; do
        hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=fast --cuda-device-only -S $f -o DIR/$(basename $f .hip).s
    done                                             # once per tree (the flags of druggen_amd/build.py)
    python scripts/asm_diff.py OLD_DIR NEW_DIR [--map FILE] [--list]

A kernel that exists in both builds must have the same instruction stream and the same .amdhsa_* resource block
(VGPRs, SGPRs, scratch, LDS) after its own mangled name and the local label numbers are normalised.  --map FILE names
kernels whose template parameter list changed: lines of `<file stem> <old mangled name> <new mangled name>`.
scripts/asm_diff_parent.map is the map for the commit that removed the unreachable instances (against its parent).
Prints the kernel count per file before / after and the kernels only one side has; exit status 1 when a kernel that
both builds have differs.  --list also prints the demangled names of removed / added kernels (needs c++filt).
"""
import argparse
import glob
import os
import re
import subprocess
import sys


def kernels(path):
    """{mangled name: (normalised instruction lines, normalised .amdhsa lines)} of one .s file"""
    text = open(path).read().split("\n")
    names = [m.group(1) for ln in text if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln))]
    out, known = {}, set(names)
    name, body, hsa, state = None, [], [], 0
    for ln in text:
        s = ln.strip()
        if state == 0:
            label = s.split(";")[0].strip()      # `name: ; @name`
            if label.endswith(":") and label[:-1] in known:
                name, body, hsa, state = label[:-1], [], [], 1
        elif state == 1:
            if s.startswith(".amdhsa_kernel"):
                state = 2
            elif s and not s.startswith((";", ".p2align", ".Lfunc_end", ".section", ".size", ".text", ".rodata")):
                body.append(s.split(";")[0].rstrip())
        elif s.startswith(".end_amdhsa_kernel"):
            # local labels carry a function number (.LBB12_3) and the kernel's name appears in symbol arithmetic
            labels = {}
            def norm(t):
                t = t.replace(name, "<self>")
                return re.sub(r"\.L[A-Za-z_]*\d+(_\d+)?", lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), t)
            out[name] = ([norm(t) for t in body], [norm(t) for t in hsa])
            state = 0
        else:
            hsa.append(s)
    return out


def demangle(names):
    if not names:
        return []
    try:
        return subprocess.run(["c++filt"] + list(names), capture_output=True, text=True, check=True).stdout.split("\n")[:len(names)]
    except (OSError, subprocess.CalledProcessError):
        return list(names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--map")
    ap.add_argument("--list", action="store_true")
    args = ap.parse_args()
    renamed = {}
    if args.map:
        for ln in open(args.map):
            f = ln.split()
            if len(f) == 3 and not ln.startswith("#"):
                renamed[(f[0], f[1])] = f[2]
    stems = sorted({os.path.basename(p)[:-2] for d in (args.old, args.new) for p in glob.glob(os.path.join(d, "*.s"))})
    bad = 0
    tot_old = tot_new = 0
    for stem in stems:
        po, pn = os.path.join(args.old, stem + ".s"), os.path.join(args.new, stem + ".s")
        ko = kernels(po) if os.path.exists(po) else {}
        kn = kernels(pn) if os.path.exists(pn) else {}
        tot_old += len(ko)
        tot_new += len(kn)
        pairs = [(o, renamed.get((stem, o), o)) for o in ko]
        pairs = [(o, n) for o, n in pairs if n in kn]
        differ = [(o, n) for o, n in pairs if ko[o] != kn[n]]
        removed = sorted(set(ko) - {o for o, _ in pairs})
        added = sorted(set(kn) - {n for _, n in pairs})
        print(f"{stem:22s} kernels {len(ko):3d} -> {len(kn):3d}   same {len(pairs) - len(differ):3d}   differ {len(differ)}"
              f"   removed {len(removed)}   added {len(added)}")
        for o, n in differ:
            io, ino = ko[o], kn[n]
            what = "instructions" if io[0] != ino[0] else "resources"
            print(f"    DIFFERS ({what}): {demangle([n])[0]}")
        if args.list:
            for tag, lst in (("-", removed), ("+", added)):
                for d in demangle(lst):
                    print(f"    {tag} {d}")
        bad += len(differ)
    print(f"total kernels {tot_old} -> {tot_new}; {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
