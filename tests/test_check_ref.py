"""The CPU side of the C++ check programs (csrc/host/*_check.cpp over csrc/host/check_ref.h), without a GPU.

Every check program takes --expected: it generates its requests, computes what its plain reference aligner
expects of the GPU functions (if it has one), prints the 64-bit FNV-1a digests of both as one JSON line and
calls nothing of the libraries. tests/golden/check_expected.json holds those lines for exactly the invocations
the test_cpp_* GPU tests make. Its digests were recorded from the programs of commit 4c30315 (the parent of
the commit that folded their five references into check_ref.h), not from the folded ones: in a scratch copy
of that tree each program got the same digest helper and printed the digests, the expectations of its own
reference copy (gotoh, gotohAlign, fitAlign, bandAlign, endsAlign, bandAtAlign) included, before its first
GPU call. So a line that differs means the programs now give the GPU other requests or compare it with
other results than they did then. The prefixes that extend_check and extend_band_check cut after the
extension's own result depend on the GPU and are in no digest.

bin/sa_ref_check runs the reference aligner against the properties of an alignment (see ref_check.cpp)."""
from __future__ import annotations

import json
import os
import subprocess

import pytest

from conftest import PKG, ROOT

with open(os.path.join(ROOT, "tests", "golden", "check_expected.json")) as f:
    GOLDEN = json.load(f)


def program(name: str) -> str:
    exe = os.path.join(PKG, "bin", name)
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", PKG, "bin/" + name], check=True)
    return exe


@pytest.mark.parametrize("line", GOLDEN, ids=lambda g: "-".join([g["program"]] + g["args"]))
def test_expected_digests_are_the_parents(line):
    out = subprocess.run([program(line["program"]), "--expected"] + line["args"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert json.loads(out.stdout) == line


def test_expected_flag_stands_anywhere():
    line = next(g for g in GOLDEN if g["program"] == "sa_band_at_check")
    out = subprocess.run([program(line["program"])] + line["args"] + ["--expected"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and json.loads(out.stdout) == line, out.stdout + out.stderr


def test_programs_with_a_reference_print_its_digest():
    with_reference = {"sa_score_affine_check", "sa_align_affine_check", "sa_fit_check", "sa_band_check", "sa_ends_check",
                      "sa_band_at_check"}
    assert {g["program"] for g in GOLDEN if g["expected"] is not None} == with_reference
    assert len({g["program"] for g in GOLDEN}) == 13


def test_reference_aligner_properties():
    out = subprocess.run([program("sa_ref_check")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1].startswith("OK ")
