"""Fit mode (sa_hip.h: SA_FIT = 2, the whole pattern inside the text) in the two planners of the wave
paths, on the CPU: bin/sa_score_plan_check and bin/sa_trace_plan_check with --mode fit. A fit plan is
the global plan of the same shapes but for the step costs that choose R; the limits are the global
ones (a fit result is read from one lane, so no key limits it). Each case runs a program once."""
from __future__ import annotations

import pytest

from conftest import PKG  # noqa: F401  (first: it puts the package on the path)

from test_score_affine_plan import plan as score_plan
from test_trace_plan import plan as trace_plan

SA_ERR_INVALID, SA_ERR_UNSUPPORTED = 1, 4
FIT = 2
SAME_AS_GLOBAL = ("A", "gap", "key_rowbits", "num_cu", "num_pairs", "max_text", "row_stride", "input_bytes", "order",
                  "affine", "gap_extend")


@pytest.mark.parametrize("gap", [["--gap", 5], ["--gap", 11, "--gap-extend", 2]])
def test_fit_plans_through_the_score_planner(gap):
    shapes = ["600x150x3", "1000x512x2", "40x40", "0x7", "9x0"]
    fit = score_plan("--mode", "fit", *gap, *shapes)
    assert "error" not in fit and fit["mode"] == FIT
    glob = score_plan("--mode", "global", *gap, *shapes)
    assert {k: fit[k] for k in SAME_AS_GLOBAL} == {k: glob[k] for k in SAME_AS_GLOBAL}
    assert score_plan("--mode", 2, *gap, *shapes) == fit


@pytest.mark.parametrize("gap", [["--gap", 5], ["--gap", 11, "--gap-extend", 2]])
@pytest.mark.parametrize("forced,got", [(1, 1), (2, 2), (4, 4), (8, 8), (16, 8), (32, 8)])
def test_fit_forced_rows_per_lane(gap, forced, got):
    pl = score_plan("--mode", "fit", *gap, "--rows-per-lane", forced, "600x150x10")
    assert pl["R"] == got and pl["mode"] == FIT
    # the grid is sized as for the other modes: the fit instances need no more registers than the local ones
    loc = score_plan("--mode", "local", *gap, "--rows-per-lane", forced, "600x150x10")
    assert (pl["waves_per_simd"], pl["grid"]) == (loc["waves_per_simd"], loc["grid"])


def test_fit_rows_per_lane_3_is_invalid():
    assert score_plan("--mode", "fit", "--rows-per-lane", 3, "300x300")["error"] == SA_ERR_INVALID


# The automatic rule with the fit step costs: a fit step is the global step of its kernel plus the
# best of row m, 5 + (R - 1) instructions. Per strip, linear (14 + 6 R global):
# 25 / 32 / 46 / 74 at R = 1 / 2 / 4 / 8; affine (18 + 10 R global): 33 / 44 / 66 / 110.
def fit_costs(affine, n, m, count):
    base, row = (18, 10) if affine else (14, 6)
    return [(n + 63) * -(-m // (64 * r)) * (base + r * row + 5 + (r - 1)) * count for r in (1, 2, 4, 8)]


AUTO = [
    (False, "600x64x100", 1, "exactly one 64-row strip (25)"),
    (False, "600x65x100", 2, "two R = 1 strips (50) cost more than one R = 2 strip (32)"),
    (False, "600x150x30000", 4, "the mapping shape: one R = 4 strip (46) against two R = 2 (64), three R = 1 (75), one R = 8 (74)"),
    (False, "1000x512x100", 8, "one R = 8 strip (74) against two R = 4 strips (92)"),
    (True, "600x64x100", 1, "exactly one 64-row strip (33)"),
    (True, "600x150x30000", 4, "one R = 4 strip (66) against two R = 2 (88), three R = 1 (99), one R = 8 (110)"),
    (True, "1000x512x100", 8, "one R = 8 strip (110) against two R = 4 strips (132)"),
]


@pytest.mark.parametrize("affine,shape,R,reason", AUTO)
def test_fit_automatic_rows_per_lane(affine, shape, R, reason):
    gap = ["--gap", 11, "--gap-extend", 2] if affine else ["--gap", 5]
    pl = score_plan("--mode", "fit", *gap, shape)
    assert pl["R"] == R, (reason, pl["cost"])
    n, m, count = (int(x) for x in shape.split("x"))
    assert pl["cost"] == fit_costs(affine, n, m, count)
    assert pl["cost"][[1, 2, 4, 8].index(R)] == min(pl["cost"])
    # dearer than a global step at every R; cheaper than a local one from R = 2 on (at R = 1 the
    # model has 5 for the fit best and 4 for the local row's clamp and best)
    glob = score_plan("--mode", "global", *gap, shape)["cost"]
    loc = score_plan("--mode", "local", *gap, shape)["cost"]
    assert all(g < f for g, f in zip(glob, pl["cost"]))
    assert all(f < l for f, l in zip(pl["cost"][1:], loc[1:]))


def test_fit_limits_are_the_global_ones():
    pl = score_plan("--mode", "fit", "16777215x100")
    assert pl["error"] == SA_ERR_UNSUPPORTED and "2^24" in pl["message"]
    pl = score_plan("--mode", "fit", "--gap", 11, "--gap-extend", 2, "100x16777215")
    assert pl["error"] == SA_ERR_UNSUPPORTED and "2^24" in pl["message"]
    pl = score_plan("--mode", "fit", "--gap", 1000000, "1000x1000")
    assert pl["error"] == SA_ERR_UNSUPPORTED and pl["message"] == "scores may exceed the int32 range"
    pl = score_plan("--mode", "fit", "--gap", 1, "--gap-extend", 100, "4000000x4000000")
    assert pl["error"] == SA_ERR_UNSUPPORTED and pl["message"] == "scores may exceed the int32 range"
    # no key: the shape the local scorer refuses for its best-cell key is planned
    assert score_plan("--mode", "local", "16000000x16000000")["message"] == "local scores may exceed the best-cell key range"
    assert "error" not in score_plan("--mode", "fit", "16000000x16000000")
    for bad in (0, 33):
        assert score_plan("--mode", "fit", "--alphabet", bad, "100x100")["error"] == SA_ERR_INVALID


def test_mode_7_is_still_invalid():
    assert score_plan("--mode", 7, "100x100")["error"] == SA_ERR_INVALID
    assert score_plan("--mode", 3, "--gap", 11, "--gap-extend", 2, "100x100")["error"] == SA_ERR_INVALID
    assert score_plan("--mode", -1, "100x100")["error"] == SA_ERR_INVALID
    assert trace_plan("--mode", 7, "100x100")["error"] == SA_ERR_INVALID
    assert trace_plan("--mode", 3, "100x100")["error"] == SA_ERR_INVALID


def test_fit_plans_through_the_trace_planner():
    shapes = ["600x150x3", "300x513x2", "1x1", "0x5", "5x0"]
    fit = trace_plan("--mode", "fit", *shapes)
    assert "error" not in fit and fit["mode"] == FIT and fit["R"] == 8
    glob = trace_plan("--mode", "global", *shapes)
    for k in fit:
        if k != "mode":
            assert fit[k] == glob[k], k  # direction bytes, slots, chunks, grid: a fit pair is traced as a global one
    assert trace_plan("--mode", 2, *shapes) == fit
    # chunks under a small budget, as for the other modes (300x513: 196608 direction bytes each)
    pl = trace_plan("--mode", "fit", "--budget", 400000, "300x513x5")
    assert pl["num_chunks"] == 3 and pl["chunk_begin"] == [0, 2, 4, 5]
    pl = trace_plan("--mode", "fit", "--budget", 100000, "300x513")
    assert pl["error"] == SA_ERR_UNSUPPORTED and "direction bytes" in pl["message"]
    pl = trace_plan("--mode", "fit", "16777215x100")
    assert pl["error"] == SA_ERR_UNSUPPORTED and "2^24" in pl["message"]
