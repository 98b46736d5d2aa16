"""The score-only planner (csrc/sa_score_plan.cpp) on the CPU: bin/sa_score_plan_check plans a list of
pair shapes (text length x pattern length) for a CU count and prints the plan as JSON; each case runs
it once (milliseconds). The matrix is +5 / -4, the gap penalty 5."""
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


def test_work_order_is_cells_descending_ties_by_index():
    pl = plan("--mode", "local", "100x50", "10x10", "70x70", "100x50")
    assert pl["order"] == [0, 3, 2, 1]
    assert pl["grid"] == 4 and pl["num_pairs"] == 4 and pl["max_text"] == 100


@pytest.mark.parametrize("forced,got", [(1, 1), (2, 2), (4, 4), (8, 8), (16, 8), (32, 8)])
def test_forced_rows_per_lane(forced, got):
    assert plan("--mode", "global", "--rows-per-lane", forced, "300x300x10")["R"] == got


def test_rows_per_lane_3_is_invalid():
    assert plan("--mode", "global", "--rows-per-lane", 3, "300x300")["error"] == SA_ERR_INVALID


@pytest.mark.parametrize("shape", ["16777215x100", "100x16777215"])
def test_length_limit(shape):
    pl = plan("--mode", "global", shape)
    assert pl["error"] == SA_ERR_UNSUPPORTED and "2^24" in pl["message"]
    assert "error" not in plan("--mode", "global", "--gap", 1, "--match", 1, "--mismatch", -1, "16777214x1")


def test_other_limits_are_the_plans():
    assert plan("--mode", "global", "--gap", 100, "4000000x4000000")["message"] == "scores may exceed the int32 range"
    assert plan("--mode", "local", "16000000x16000000")["message"] == "local scores may exceed the best-cell key range"
    assert plan("--mode", 7, "100x100")["error"] == SA_ERR_INVALID
    assert plan("--mode", "global", "--alphabet", 33, "100x100")["error"] == SA_ERR_INVALID


def test_device_bytes_do_not_depend_on_the_cell_count():
    thin, square = plan("--mode", "global", "1024x64x64"), plan("--mode", "global", "1024x1024x64")
    assert thin["device_bytes"] - thin["input_bytes"] == square["device_bytes"] - square["input_bytes"]
    assert thin["input_bytes"] == 64 * (1024 + 64) and square["input_bytes"] == 64 * 2048
    # one boundary row of max n + padding ints per wave; descriptors, order and results per pair
    assert thin["row_stride"] == 1024 + 64
    assert thin["device_bytes"] - thin["input_bytes"] == 64 * thin["row_stride"] * 4 + 64 * (24 + 4 + 24) + 4096 + 256


def test_grid_is_capped_by_resident_waves():
    pl = plan("--mode", "global", "--rows-per-lane", 1, "100x50x20000", cus=256)
    assert pl["grid"] == 256 * 4 * pl["waves_per_simd"] and pl["waves_per_simd"] == 8
    pl = plan("--mode", "global", "--rows-per-lane", 8, "100x50x20000", cus=16)
    assert pl["grid"] == 16 * 4 * pl["waves_per_simd"] and pl["waves_per_simd"] == 3


# The automatic rule: a strip of 64R rows over n columns costs (n + 63) * (14 + R * c) instructions,
# c = 6 per global row and 10 per local row (the steady loop's instruction count);
# the cheapest total wins, ties to the smaller R.
AUTO = [
    ("global", "1000x50x100", 1, "one strip either way: taller strips only add padded rows"),
    ("global", "1000x64x100", 1, "exactly one 64-row strip"),
    ("global", "1000x65x100", 2, "two R = 1 strips (2 * 20) cost more than one R = 2 strip (26)"),
    ("global", "1000x128x100", 2, "one R = 2 strip (26) against one R = 4 strip (38)"),
    ("global", "1000x256x100", 4, "one R = 4 strip (38) against two R = 2 (52) or one R = 8 (62)"),
    ("global", "1000x512x100", 8, "one R = 8 strip (62) against two R = 4 strips (76)"),
    ("global", "2048x2048x4096", 8, "the batch shape: 4 strips of 62 against 8 of 38"),
    ("local", "400x150x400", 4, "a 150-letter query: one R = 4 strip (54) against two R = 2 (68), three R = 1 (72)"),
    ("local", "1000x512x100", 8, "local rows cost 10: one R = 8 strip (94) against two R = 4 strips (108)"),
    ("local", "1000x300x100", 8, "300 rows: one R = 8 strip (94) against three R = 2 (102) or two R = 4 (108)"),
]


@pytest.mark.parametrize("mode,shape,R,reason", AUTO)
def test_automatic_rows_per_lane(mode, shape, R, reason):
    pl = plan("--mode", mode, shape)
    assert pl["R"] == R, (reason, pl["cost"])
    assert pl["cost"][[1, 2, 4, 8].index(R)] == min(pl["cost"])


def test_automatic_rule_weighs_a_mixed_batch():
    """Many short patterns and a few tall ones: the sum decides, not the tallest pair."""
    pl = plan("--mode", "global", "500x60x1000", "500x2000x2")
    assert pl["R"] == 1 and pl["cost"][0] == min(pl["cost"])
    pl = plan("--mode", "global", "500x60x10", "500x2000x100")
    assert pl["R"] == 8


def test_padded_cells():
    pl = plan("--mode", "global", "--rows-per-lane", 2, "100x130", "10x1")
    assert pl["padded_cells"] == 100 * 256 + 10 * 128
