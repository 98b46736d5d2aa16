"""The planners of the banded path on the CPU, through bin/sa_score_plan_check and bin/sa_trace_plan_check
with --band: band cells, the window of every strip and the direction bytes against a plain Python
count; the unbanded plan where the band admits every cell; the fall of R with the band; the arena
budget; the codes of a negative band and of fit mode; and the sentinel's score limit."""
from __future__ import annotations

import pytest

from test_score_affine_plan import plan as score_plan
from test_trace_plan import plan as trace_plan

SA_ERR_INVALID, SA_ERR_UNSUPPORTED = 1, 4
LENGTHS = [1, 63, 64, 65, 511, 512, 513, 1500]


def limits(n, m, w):
    d = n - m
    return min(0, d) - w, max(0, d) + w


def count_cells(n, m, w):
    lo, hi = limits(n, m, w)
    return sum(1 for i in range(1, m + 1) for j in range(max(1, i + lo), min(n, i + hi) + 1))


def count_windows(n, m, w, rows):
    """Per strip of `rows` rows: the first and last in-band column of any of its rows, and the 64-step
    bodies that hold a step at which some lane meets one of them (lane l meets column j at step
    j + l - 1; lane 0 owns the strip's first rows, the last row lies in a lane up to 63)."""
    lo, hi = limits(n, m, w)
    out = []
    for first in range(1, m + 1, rows):
        last = min(m, first + rows - 1)
        cols = [j for i in range(first, last + 1) for j in (max(1, i + lo), min(n, i + hi))]
        jmin, jmax = min(cols), max(cols)
        assert jmin <= jmax
        out.append([jmin, jmax, (jmin - 1) // 64, (jmax + 62) // 64 + 1])
    return out


SHAPES = [(n, m) for n in LENGTHS for m in LENGTHS]  # n != m both ways, |n - m| above every small w


@pytest.mark.parametrize("w", [0, 1, 31, 64, 200, "max"])
def test_band_cells_windows_and_direction_bytes_against_a_plain_count(w):
    for n, m in SHAPES:
        ww = max(n, m) if w == "max" else w
        for R in (1, 8):
            pl = score_plan("--mode", "global", "--gap", 11, "--gap-extend", 2, "--band", ww, "--rows-per-lane", R, f"{n}x{m}")
            b = pl["bands"][0]
            assert (b["lo"], b["hi"]) == limits(n, m, min(ww, max(n, m))), (n, m, ww)
            want = count_windows(n, m, ww, 64 * R)
            assert b["windows"] == want, (n, m, ww, R)
            assert pl["padded_cells"] == sum((x[1] - x[0] + 1) * 64 * R for x in want), (n, m, ww, R)
            assert pl["cost"][(1, 2, 4, 8).index(R)] == sum(x[1] - x[0] + 64 for x in want) * (18 + 10 * R), (n, m, ww, R)
        if n * m <= 513 * 513 or ww <= 64:
            assert b["cells"] == pl["band_cells"] == count_cells(n, m, ww), (n, m, ww)
        tp = trace_plan("--mode", "global", "--band", ww, f"{n}x{m}")
        want = count_windows(n, m, ww, 512)
        pr = tp["pairs"][0]
        assert pr["windows"] == [x[2:] for x in want], (n, m, ww)
        assert pr["dir_bytes"] == sum(64 * (x[3] - x[2]) * 256 for x in want) == tp["arena_bytes"], (n, m, ww)
        assert pr["strips"] == len(want) and pr["steps"] * 256 == pr["dir_bytes"]


def test_a_band_that_admits_every_cell_plans_as_the_unbanded_call():
    shapes = [f"{n}x{m}" for n, m in SHAPES]
    for mode in ("global", "local"):
        full = score_plan("--mode", mode, "--gap", 11, "--gap-extend", 2, *shapes)
        for w in (1500, 1 << 30):
            band = score_plan("--mode", mode, "--gap", 11, "--gap-extend", 2, "--band", w, *shapes)
            for key in ("R", "cost", "padded_cells", "order", "grid", "device_bytes", "row_stride", "key_rowbits"):
                assert band[key] == full[key], (mode, w, key)
            assert band["band_cells"] == sum(n * m for n, m in SHAPES)
        tfull = trace_plan("--mode", mode, *shapes)
        tband = trace_plan("--mode", mode, "--band", 1500, *shapes)
        for key in ("arena_bytes", "total_dir_bytes", "chunk_begin", "order", "string_bytes"):
            assert tband[key] == tfull[key], (mode, key)
        assert [p["dir_bytes"] for p in tband["pairs"]] == [p["dir_bytes"] for p in tfull["pairs"]]


def test_the_planned_rows_per_lane_fall_with_the_band():
    wide = score_plan("--mode", "global", "--gap", 11, "--gap-extend", 2, "--band", 4096, "4096x4096")
    narrow = score_plan("--mode", "global", "--gap", 11, "--gap-extend", 2, "--band", 16, "4096x4096")
    assert wide["R"] == score_plan("--mode", "global", "--gap", 11, "--gap-extend", 2, "4096x4096")["R"]
    assert narrow["R"] < wide["R"]
    # a 512-row strip at w = 32 steps through 512 + 64 + 63 columns for the 65 its rows hold each
    assert narrow["cost"].index(min(narrow["cost"])) == (1, 2, 4, 8).index(narrow["R"])
    # the work order counts band cells: the long narrow pair after the short wide one
    pl = score_plan("--mode", "global", "--gap", 11, "--gap-extend", 2, "--band", 2, "3000x3000", "300x300")
    assert pl["order"] == [0, 1] and pl["band_cells"] == count_cells(3000, 3000, 2) + count_cells(300, 300, 2)
    pl = score_plan("--mode", "global", "--gap", 11, "--gap-extend", 2, "--band", 2, "3000x3000", "400x100")
    assert pl["order"] == [1, 0]  # 100 rows of 305 columns against 3000 rows of at most 5


def test_a_pair_beyond_the_budget_is_planned_inside_its_band():
    budget = 8 << 20
    full = trace_plan("--mode", "global", "--budget", budget, "6000x6000")
    assert full["error"] == SA_ERR_UNSUPPORTED and "SA_TRACE_ARENA_BYTES" in full["message"]
    band = trace_plan("--mode", "global", "--budget", budget, "--band", 100, "6000x6000")
    assert band["num_chunks"] == 1 and band["arena_bytes"] == sum(64 * (x[3] - x[2]) * 256 for x in count_windows(6000, 6000, 100, 512))
    wide = trace_plan("--mode", "global", "--budget", budget, "--band", 6000, "6000x6000")
    assert wide == full  # the same refusal, the existing message
    # chunks are cut by banded bytes: three such pairs fit the budget, four do not
    four = trace_plan("--mode", "global", "--budget", budget, "--band", 100, "6000x6000x4")
    assert four["chunk_begin"] == [0, 3, 4] and four["arena_bytes"] == 3 * band["arena_bytes"]


def test_a_negative_band_and_fit_mode_are_refused():
    for plan in (score_plan, trace_plan):
        bad = plan("--mode", "global", "--gap", 11, "--gap-extend", 2, "--band", -1, "100x100")
        assert bad["error"] == SA_ERR_INVALID and "band" in bad["message"]
        fit = plan("--mode", "fit", "--gap", 11, "--gap-extend", 2, "--band", 5, "100x100")
        assert fit["error"] == SA_ERR_UNSUPPORTED and "SA_FIT" in fit["message"]
        assert "error" not in plan("--mode", "fit", "--gap", 11, "--gap-extend", 2, "100x100")
    assert score_plan("--mode", "global", "--gap", 5, "--band", 5, "100x100")["error"] == SA_ERR_INVALID  # no gap model


def test_the_sentinel_bound_is_refused_one_past_its_limit():
    # match 5, mismatch -4, gap open G, extend 1: (5 + G) (n + m) + G (n + m) < 2^29 with n + m = 2^10
    # holds up to 2 G + 5 = 2^19 - 1, G = 262141
    args = ("--mode", "global", "--gap-extend", 1, "--band", 3, "512x512")
    assert "error" not in score_plan("--gap", 262141, *args)
    over = score_plan("--gap", 262142, *args)
    assert over["error"] == SA_ERR_UNSUPPORTED and "sentinel" in over["message"]
    assert "error" not in score_plan("--gap", 262142, "--mode", "global", "--gap-extend", 1, "512x512")  # unbanded: 2^30
    assert trace_plan("--gap", 262142, *args)["error"] == SA_ERR_UNSUPPORTED
    assert "error" not in trace_plan("--gap", 262141, *args)
    # negative penalties count by their size
    assert score_plan("--gap", -262142, *args)["error"] == SA_ERR_UNSUPPORTED
