#!/usr/bin/env python3
"""Compares the kernels of two device assembly listings (hipcc --cuda-device-only -S) of one source file:
for every kernel of the first listing, its instructions and its kernel descriptor (.amdhsa_ directives:
registers, LDS, scratch) in the second. Basic-block labels carry the function's index in the file, which
shifts when instances are added, so the index is dropped from them; comments and debug directives are
ignored. Prints one line per kernel and a summary; exit status 0 iff every kernel of the first listing is
in the second with identical text.
    compare_kernel_asm.py parent.s new.s [--markdown]
With --markdown the per-kernel lines are a table, and the kernels only the second listing has are listed
with their VGPR, SGPR and scratch figures."""
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
        m = re.match(r"^(_Z\w+):", s)
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


def main(argv):
    md = "--markdown" in argv
    a, b = [x for x in argv if not x.startswith("--")]
    old, new = kernels(a), kernels(b)
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
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
