"""The score-only planner with the affine gap model (csrc/sa_score_plan.cpp) on the CPU:
bin/sa_score_plan_check --gap-extend E plans for score_affine_kernel, --gap being the gap-open
penalty. Linear plans come out as before. Each case runs the program once (milliseconds)."""
from __future__ import annotations

import json
import os
import subprocess

import pytest

from conftest import PKG

CHECK = os.path.join(PKG, "bin", "sa_score_plan_check")
SA_ERR_INVALID, SA_ERR_UNSUPPORTED = 1, 4


def plan(*args, cus=256) -> dict:
    if not os.path.exists(CHECK):
        subprocess.run(["make", "-s", "-C", PKG, "bin/sa_score_plan_check"], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SA_")}
    out = subprocess.run([CHECK, "--cus", str(cus)] + [str(a) for a in args], env=env, check=True,
                         capture_output=True, text=True).stdout
    return json.loads(out)


# Two linear plans as the planner printed them before it knew the affine model.
LINEAR = [
    (256, ["--mode", "local", "--alphabet", 23, "--gap", 5, "400x150x3", "1000x512x2"],
     {"mode": 1, "A": 23, "gap": 5, "R": 4, "key_rowbits": 10, "num_cu": 256, "waves_per_simd": 4, "grid": 5,
      "num_pairs": 5, "max_text": 1000, "row_stride": 1088, "input_bytes": 4674, "device_bytes": 31046,
      "padded_cells": 1331200, "cost": [508200, 383588, 304614, 330410], "order": [3, 4, 0, 1, 2]}),
    (64, ["--mode", "global", "--gap", -2, "--rows-per-lane", 2, "100x130", "10x1", "2048x2048x5"],
     {"mode": 0, "A": 4, "gap": -2, "R": 2, "key_rowbits": 12, "num_cu": 64, "waves_per_simd": 7, "grid": 7,
      "num_pairs": 7, "max_text": 2048, "row_stride": 2112, "input_bytes": 20721, "device_bytes": 84573,
      "padded_cells": 20998400, "cost": [6766440, 4401254, 3217688, 2632272], "order": [2, 3, 4, 5, 6, 0, 1]}),
]


@pytest.mark.parametrize("cus,args,want", LINEAR)
def test_linear_plans_are_unchanged(cus, args, want):
    pl = plan(*args, cus=cus)
    assert {k: pl[k] for k in want} == want
    assert pl["affine"] is False and pl["gap_extend"] == 0


def test_affine_plan_reports_its_gap_model():
    pl = plan("--mode", "local", "--gap", 11, "--gap-extend", 2, "100x50", "10x10", "70x70", "100x50")
    assert pl["affine"] is True and pl["gap"] == 11 and pl["gap_extend"] == 2
    assert pl["order"] == [0, 3, 2, 1] and pl["grid"] == 4


def test_affine_row_buffer_holds_two_ints_per_column():
    thin = plan("--mode", "global", "--gap", 11, "--gap-extend", 2, "1024x64x64")
    square = plan("--mode", "global", "--gap", 11, "--gap-extend", 2, "--rows-per-lane", 1, "1024x1024x64")
    assert thin["row_stride"] == 1024 + 64  # still a column count
    # (H, F) per column and wave; descriptors, order and results per pair; score table; counters
    assert thin["device_bytes"] - thin["input_bytes"] == 64 * thin["row_stride"] * 8 + 64 * 52 + 4096 + 256
    assert thin["device_bytes"] - thin["input_bytes"] == square["device_bytes"] - square["input_bytes"]
    linear = plan("--mode", "global", "--gap", 11, "1024x64x64")
    assert thin["device_bytes"] - linear["device_bytes"] == 64 * thin["row_stride"] * 4


@pytest.mark.parametrize("forced,got", [(1, 1), (2, 2), (4, 4), (8, 8), (16, 8), (32, 8)])
def test_affine_forced_rows_per_lane(forced, got):
    """No instance of score_affine_kernel spills, so R = 8 is not capped."""
    pl = plan("--mode", "local", "--gap", 11, "--gap-extend", 2, "--rows-per-lane", forced, "300x300x10")
    assert pl["R"] == got and pl["affine"] is True


def test_affine_rows_per_lane_3_is_invalid():
    assert plan("--mode", "global", "--gap", 11, "--gap-extend", 2, "--rows-per-lane", 3, "300x300")["error"] == SA_ERR_INVALID


def test_affine_limits_use_the_larger_penalty():
    pl = plan("--mode", "global", "--gap", 1, "--gap-extend", 100, "4000000x4000000")
    assert pl["error"] == SA_ERR_UNSUPPORTED and pl["message"] == "scores may exceed the int32 range"
    pl = plan("--mode", "global", "--gap", 100, "--gap-extend", 1, "4000000x4000000")
    assert pl["error"] == SA_ERR_UNSUPPORTED
    pl = plan("--mode", "global", "--gap", 1, "--gap-extend", -100, "4000000x4000000")
    assert pl["error"] == SA_ERR_UNSUPPORTED
    assert "error" not in plan("--mode", "global", "--gap", 1, "--gap-extend", 1, "4000000x4000000")
    # lengths and the local key, as for the linear gap
    pl = plan("--mode", "global", "--gap", 11, "--gap-extend", 2, "16777215x100")
    assert pl["error"] == SA_ERR_UNSUPPORTED and "2^24" in pl["message"]
    pl = plan("--mode", "local", "--gap", 11, "--gap-extend", 2, "16000000x16000000")
    assert pl["message"] == "local scores may exceed the best-cell key range"
    # 10^6 squared: 20-bit rows and columns leave 24 bits for H. 5 * 10^6 fits; a negative penalty makes
    # every step a possible gain, and the bound (max|S| + 11) * (n + m) = 32 * 10^6 does not
    assert "error" not in plan("--mode", "local", "--gap", 11, "--gap-extend", 2, "1000000x1000000")
    pl = plan("--mode", "local", "--gap", 11, "--gap-extend", -3, "1000000x1000000")
    assert pl["error"] == SA_ERR_UNSUPPORTED and pl["message"] == "local scores may exceed the best-cell key range"


def test_affine_grid_is_capped_by_resident_waves():
    """Waves per SIMD from the registers of the instances: 8, 5, 4, 3 at R = 1, 2, 4, 8."""
    for R, waves in ((1, 8), (2, 5), (4, 4), (8, 3)):
        pl = plan("--mode", "local", "--gap", 11, "--gap-extend", 2, "--rows-per-lane", R, "100x50x20000", cus=16)
        assert pl["waves_per_simd"] == waves and pl["grid"] == 16 * 4 * waves


# The automatic rule with the affine step costs: a strip of 64R rows over n columns costs
# (n + 63) * (18 + R * c) instructions, c = 10 per global row and 14 per local row (the steady loop
# of score_affine_kernel): per strip 28 / 38 / 58 / 98 global and 32 / 46 / 74 / 130
# local at R = 1 / 2 / 4 / 8; the cheapest total wins, ties to the smaller R.
AUTO = [
    ("global", "1000x64x100", 1, "exactly one 64-row strip (28)"),
    ("global", "1000x65x100", 2, "two R = 1 strips (2 * 28) cost more than one R = 2 strip (38)"),
    ("global", "1000x256x100", 4, "one R = 4 strip (58) against two R = 2 (76) or one R = 8 (98)"),
    ("global", "1000x512x100", 8, "one R = 8 strip (98) against two R = 4 strips (116)"),
    ("local", "400x150x400", 4, "one R = 4 strip (74) against two R = 2 (92), three R = 1 (96), one R = 8 (130)"),
    ("local", "1000x300x100", 8, "one R = 8 strip (130) against three R = 2 (138), two R = 4 (148), five R = 1 (160)"),
    ("local", "1000x512x20000", 8, "the search shape: one R = 8 strip (130) against two R = 4 strips (148)"),
]


@pytest.mark.parametrize("mode,shape,R,reason", AUTO)
def test_affine_automatic_rows_per_lane(mode, shape, R, reason):
    pl = plan("--mode", mode, "--gap", 11, "--gap-extend", 2, shape)
    assert pl["R"] == R, (reason, pl["cost"])
    assert pl["cost"][[1, 2, 4, 8].index(R)] == min(pl["cost"])
    n, m, count = (int(x) for x in shape.split("x"))
    c = 14 if mode == "local" else 10
    assert pl["cost"] == [(n + 63) * -(-m // (64 * r)) * (18 + r * c) * count for r in (1, 2, 4, 8)]
