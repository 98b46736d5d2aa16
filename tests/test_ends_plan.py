"""Ends-free modes (sa_hip.h: SA_ENDS_FREE = 16 or'ed with TB = 1, TE = 2, PB = 4, PE = 8) in the
planners, on the CPU: bin/sa_score_plan_check and bin/sa_trace_plan_check take the mode numbers through
--mode, bin/sa_plan_check refuses them. A mode with a free text end (TE) runs the fit program and is
planned as SA_FIT, any other runs the global program and is planned as SA_GLOBAL; the other free ends
cost nothing per step. Each case runs a program once."""
from __future__ import annotations

import pytest

from conftest import PKG  # noqa: F401  (first: it puts the package on the path)

from test_plan import run_check as engine_plan
from test_score_affine_plan import plan as score_plan
from test_trace_plan import plan as trace_plan

SA_ERR_INVALID, SA_ERR_UNSUPPORTED = 1, 4
GLOBAL, FIT, ENDS, TE = 0, 2, 16, 2
MODES = list(range(16, 32))
GAPS = [["--gap", 5], ["--gap", 11, "--gap-extend", 2]]
DNA_SCHEME = ["--alphabet", "4", "--gap", "5", "--matrix", "blast"]
SHAPES = ["600x150x3", "1000x512x2", "600x65x9", "40x40", "0x7", "9x0"]


@pytest.mark.parametrize("gap", GAPS)
def test_every_ends_free_mode_plans_as_its_program(gap):
    base = {name: score_plan("--mode", name, *gap, *SHAPES) for name in ("global", "fit")}
    for mode in MODES:
        pl = score_plan("--mode", mode, *gap, *SHAPES)
        assert "error" not in pl and pl["mode"] == mode
        want = base["fit" if mode & TE else "global"]
        for k in pl:
            if k != "mode":
                assert pl[k] == want[k], (mode, k)  # cost[], R, grid, order, bytes: everything but the mode
    assert base["fit"]["cost"] != base["global"]["cost"]


@pytest.mark.parametrize("gap", GAPS)
@pytest.mark.parametrize("forced,got", [(1, 1), (2, 2), (4, 4), (8, 8), (16, 8)])
def test_forced_rows_per_lane(gap, forced, got):
    for mode, same in ((ENDS | 15, "fit"), (ENDS | 9, "global")):
        pl = score_plan("--mode", mode, *gap, "--rows-per-lane", forced, "600x150x10")
        base = score_plan("--mode", same, *gap, "--rows-per-lane", forced, "600x150x10")
        assert pl["R"] == got == base["R"]
        assert (pl["waves_per_simd"], pl["grid"], pl["cost"]) == (base["waves_per_simd"], base["grid"], base["cost"])


def test_the_other_mode_numbers_are_invalid():
    for mode in list(range(3, 16)) + [32, 33, 48, 63, -16]:
        for plan, gap in ((score_plan, GAPS[0]), (score_plan, GAPS[1]), (trace_plan, [])):
            pl = plan("--mode", mode, *gap, "100x100")
            assert pl["error"] == SA_ERR_INVALID and "mode" in pl["message"], mode


def test_a_band_with_free_ends_is_unsupported():
    for mode in MODES:
        for plan in (score_plan, trace_plan):
            pl = plan("--mode", mode, "--gap", 11, "--gap-extend", 2, "--band", 5, "100x100")
            assert pl["error"] == SA_ERR_UNSUPPORTED and "SA_ENDS_FREE" in pl["message"] and "band" in pl["message"], mode
    assert "error" not in score_plan("--mode", "global", "--gap", 11, "--gap-extend", 2, "--band", 5, "100x100")


def test_the_plans_refuse_the_modes_and_name_the_functions_that_take_them():
    for mode in (16, 19, 31):
        pl = engine_plan(["--mode", str(mode)] + DNA_SCHEME + ["100x100"], {})
        assert pl["error"] == SA_ERR_UNSUPPORTED, mode
        for name in ("sa_align_pairs_affine", "sa_score_batch", "sa_scorer_create", "sa_search"):
            assert name in pl["message"], (mode, name)
    assert engine_plan(["--mode", "15"] + DNA_SCHEME + ["100x100"], {})["error"] == SA_ERR_INVALID
    assert engine_plan(["--mode", "32"] + DNA_SCHEME + ["100x100"], {})["error"] == SA_ERR_INVALID


def test_the_trace_planner_takes_the_modes_with_the_arena_of_global():
    shapes = ["600x150x3", "300x513x2", "1x1", "0x5", "5x0"]
    glob = trace_plan("--mode", "global", *shapes)
    for mode in MODES:
        pl = trace_plan("--mode", mode, *shapes)
        assert "error" not in pl and pl["mode"] == mode and pl["R"] == 8
        for k in ("arena_bytes", "total_dir_bytes", "num_chunks", "chunk_begin", "pairs", "grid"):
            assert pl[k] == glob[k], (mode, k)  # a pair is traced as a global one: direction bytes, slots, chunks
    pl = trace_plan("--mode", 31, "--budget", 400000, "300x513x5")
    assert pl["num_chunks"] == 3 and pl["chunk_begin"] == [0, 2, 4, 5]
    pl = trace_plan("--mode", 25, "--budget", 100000, "300x513")
    assert pl["error"] == SA_ERR_UNSUPPORTED and "direction bytes" in pl["message"]


def test_the_limits_are_the_global_ones():
    pl = score_plan("--mode", 31, "16777215x100")
    assert pl["error"] == SA_ERR_UNSUPPORTED and "2^24" in pl["message"]
    pl = score_plan("--mode", 24, "--gap", 1000000, "1000x1000")
    assert pl["error"] == SA_ERR_UNSUPPORTED and pl["message"] == "scores may exceed the int32 range"
    # no local key: the result comes from one wave maximum over (value + 2^30, row), inside the int32 limit
    assert score_plan("--mode", "local", "16000000x16000000")["message"] == "local scores may exceed the best-cell key range"
    assert "error" not in score_plan("--mode", 31, "16000000x16000000")
