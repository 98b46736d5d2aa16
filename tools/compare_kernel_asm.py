#!/usr/bin/env python3
"""Compares the kernels of two device assembly listings (hipcc --cuda-device-only -S) of one source file:
for every kernel of the first listing, its instructions and its kernel descriptor (.amdhsa_ directives:
registers, LDS, scratch) in the second. Basic-block labels carry the function's index in the file, which
shifts when instances are added, so the index is dropped from them; comments and debug directives are
ignored. Prints one line per kernel and a summary; exit status 0 iff every kernel of the first listing is
in the second with identical text.
    compare_kernel_asm.py parent.s new.s [--markdown] [--map FILE]
With --markdown the per-kernel lines are a table, and the kernels only the second listing has are listed
with their VGPR, SGPR and scratch figures.
With --map FILE a kernel of the first listing is looked up in the second under another name: the file has
lines `old_mangled_name new_mangled_name` (a kernel without a line keeps its name). Every mapped kernel's own
name inside its text is rewritten before the comparison, two old names must not share a new one, and a kernel
of the second listing that no kernel of the first accounts for fails the comparison. Under a map the kernels
take other argument structs, so .amdhsa_kernarg_size is left out of the descriptor comparison, and nothing
else is."""
from __future__ import annotations

import re
import sys


def kernels(path):
    """{name: (instructions, descriptor)} of a listing."""
    text = open(path).read().splitlines()
    body, desc, name, out, descs = [], [], None, {}, {}
    label = re.compile(r"\.LBB\d+_")
    for line in text:
        s = line.split(";")[0].strip()
        if not s:
            continue
        m = re.match(r"^(_Z[\w$.]+):", s)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if s.startswith(".amdhsa_kernel "):
            dname, desc = s.split()[1], []
            continue
        if s == ".end_amdhsa_kernel":
            descs[dname] = desc  # the descriptor lies inside the function, before its end label
            continue
        if s.startswith(".amdhsa_"):
            desc.append(s)
            continue
        if name is not None:
            if s.startswith(".Lfunc_end"):
                out[name] = body
                name = None
            elif not s.startswith((".loc", ".file", ".cfi", ".p2align", ".section")):
                body.append(label.sub(".LBB_", s))
    return {k: (v, descs.get(k, [])) for k, v in out.items()}


def figure(desc, key):
    for d in desc:
        if d.startswith(key + " "):
            return d.split()[1]
    return "?"


def read_map(path):
    """{old name: new name} of a map file; a new name taken twice is an error."""
    names = {}
    for line in open(path):
        if line.strip() and not line.startswith("#"):
            old, new = line.split()
            names[old] = new
    if len(set(names.values())) != len(names):
        sys.exit(f"{path}: two kernels map to one name")
    return names


def main(argv):
    md = "--markdown" in argv
    names = {}
    if "--map" in argv:
        i = argv.index("--map")
        names = read_map(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
    a, b = [x for x in argv if not x.startswith("--")]
    old, new = kernels(a), kernels(b)
    if names:
        # a kernel's text names the kernel itself (its kernarg symbol, its end label's size expression)
        old = {names.get(k, k): ([s.replace(k, names.get(k, k)) for s in v[0]], v[1]) for k, v in old.items()}
        drop = lambda desc: [d for d in desc if not d.startswith(".amdhsa_kernarg_size ")]  # noqa: E731
        old = {k: (v[0], drop(v[1])) for k, v in old.items()}
        new = {k: (v[0], drop(v[1])) for k, v in new.items()}
    bad = 0
    if md:
        print("| kernel | instructions | same text | same descriptor |\n|---|---|---|---|")
    for name in sorted(old):
        if name not in new:
            print(f"| `{name}` | {len(old[name][0])} | missing | missing |" if md else f"MISSING {name}")
            bad += 1
            continue
        same, samed = old[name][0] == new[name][0], old[name][1] == new[name][1]
        bad += not (same and samed)
        print(f"| `{name}` | {len(old[name][0])} | {'yes' if same else 'NO'} | {'yes' if samed else 'NO'} |" if md
              else f"{'same' if same and samed else 'DIFFERENT'} {name} ({len(old[name][0])} instructions)")
    added = sorted(set(new) - set(old))
    if md and added:
        print("\n| new kernel | instructions | VGPRs | SGPRs | scratch bytes |\n|---|---|---|---|---|")
    for name in added:
        d = new[name][1]
        row = (len(new[name][0]), figure(d, ".amdhsa_next_free_vgpr"), figure(d, ".amdhsa_next_free_sgpr"),
               figure(d, ".amdhsa_private_segment_fixed_size"))
        print(f"| `{name}` | {row[0]} | {row[1]} | {row[2]} | {row[3]} |" if md else f"new {name}: {row}")
    print(f"\n{len(old)} kernels in the first listing, {len(old) - bad} identical in the second, {bad} different or missing, "
          f"{len(added)} new")
    return 1 if bad or (names and added) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
