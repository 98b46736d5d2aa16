"""Banded extension (sa_hip.h: sa_score_batch_extend_band, sa_score_batch_seeds_band and their aligners) in the
planners, on the CPU: bin/sa_score_plan_check and bin/sa_trace_plan_check take --width W beside --extend (and
--seeds). A pair, or a seed's half from its own shape, is planned on the band {max(-w, -m), min(w, n)}: the
windows, the band cells and the direction bytes against numbers worked out by hand and against a plain Python
count; a width that admits every cell has the cost structure of the full rectangle; R falls with the width; and
the refusals and limits. Each case runs a program a few times."""
from __future__ import annotations

import pytest

from conftest import PKG  # noqa: F401  (first: it puts the package on the path)

from test_score_affine_plan import plan as score_plan
from test_trace_plan import plan as trace_plan

SA_ERR_INVALID, SA_ERR_UNSUPPORTED = 1, 4
GAP = ["--gap", 11, "--gap-extend", 2]
EXT = ["--mode", "global", *GAP, "--extend", 20]


def band_of_width(n, m, w):
    return max(-w, -m), min(w, n)


def count(n, m, w, rows):
    """(band cells, [jmin, jmax, b0, b1] of every strip of `rows` rows) by looking at every row."""
    lo, hi = band_of_width(n, m, w)
    cells, windows = 0, []
    for s in range((m + rows - 1) // rows):
        cols = []
        for i in range(rows * s + 1, min(m, rows * (s + 1)) + 1):
            a, b = max(1, i + lo), min(n, i + hi)
            if a <= b:
                cols += [a, b]
                cells += b - a + 1
        windows.append([min(cols), max(cols), (min(cols) - 1) // 64, (max(cols) + 62) // 64 + 1] if cols else [1, 0, 0, 0])
    return cells, windows


def dir_bytes(n, m, w):
    """Direction bytes of a traced pair: 512-row strips, 64 steps of 64 dwords per body of a strip's window."""
    return sum(b1 - b0 for _, _, b0, b1 in count(n, m, w, 512)[1]) * 64 * 64 * 4 if n and m else 0


# ---- windows, band cells and direction bytes ----------------------------------------------------------------------------
def test_windows_and_cells_by_hand():
    """300 x 300 at w = 10 in 64-row strips: strip s holds rows 64 s + 1 .. min(300, 64 s + 64), its columns run
    from the first row's i - 10 to the last row's i + 10 inside 1 .. 300, lane 0 meets column jmin at step
    jmin - 1 and lane 63 column jmax at step jmax + 62. The band holds 21 cells a row less the two corners of
    10 + 9 + .. + 1: 6300 - 110. The tall pair (100 columns, 700 rows) has no in-band cell past row 110."""
    pl = score_plan(*EXT, "--width", 10, "--rows-per-lane", 1, "300x300", "100x700")
    assert "error" not in pl and pl["width"] == 10 and pl["extend"] is True and pl["xdrop"] == 20 and pl["R"] == 1
    a, b = pl["bands"]
    assert (a["lo"], a["hi"], a["cells"]) == (-10, 10, 6190)
    assert a["windows"] == [[1, 74, 0, 3], [55, 138, 0, 4], [119, 202, 1, 5], [183, 266, 2, 6], [247, 300, 3, 6]]
    # rows 1 .. 10 hold i + 10 cells, rows 11 .. 90 hold 21, rows 91 .. 110 hold 110 - i + 1
    assert (b["lo"], b["hi"], b["cells"]) == (-10, 10, sum(range(11, 21)) + 80 * 21 + sum(range(1, 21)))
    assert b["windows"] == [[1, 74, 0, 3], [55, 100, 0, 3]] + [[1, 0, 0, 0]] * 9
    assert pl["band_cells"] == a["cells"] + b["cells"]
    assert pl["order"] == [0, 1]  # by band cells: the square pair holds more of them, the tall pair more cells
    # padded_cells: each strip's in-band columns times its 64 rows; an empty strip adds jmax - jmin + 1 = 0
    assert pl["padded_cells"] == 64 * sum(w[1] - w[0] + 1 for w in a["windows"] + b["windows"])
    # the cost of R = 1: the local affine step (18 + 14) for jmax - jmin + 64 steps of every strip with a window
    assert pl["cost"][0] == 32 * sum(w[1] - w[0] + 64 for w in a["windows"] + b["windows"] if w[3] > w[2])


@pytest.mark.parametrize("shape", [(300, 300), (100, 700), (700, 100), (1, 1), (65, 64), (513, 500), (1027, 300)])
@pytest.mark.parametrize("w", [0, 1, 5, 63, 64, 65, 2000])
def test_windows_and_cells_against_a_plain_count(shape, w):
    n, m = shape
    for R in (1, 8):
        pl = score_plan(*EXT, "--width", w, "--rows-per-lane", R, f"{n}x{m}")
        cells, windows = count(n, m, w, 64 * R)
        b = pl["bands"][0]
        assert (b["lo"], b["hi"]) == band_of_width(n, m, w)
        assert b["cells"] == cells == pl["band_cells"] and b["windows"] == windows, (R, b)
    tp = trace_plan(*EXT, "--width", w, f"{n}x{m}")
    assert tp["width"] == w and tp["pairs"][0]["dir_bytes"] == dir_bytes(n, m, w) == tp["arena_bytes"]
    assert tp["pairs"][0]["windows"] == [[b0, b1] for _, _, b0, b1 in count(n, m, w, 512)[1]]


def test_direction_bytes_by_hand():
    """2000 x 2000 at w = 64 in 512-row strips: the windows' bodies are [0, 10), [7, 18), [15, 26) and [23, 33),
    42 bodies of 64 steps of 256 bytes; the full rectangle takes 4 strips of 33 bodies. 6000 x 6000 takes 12
    strips of 95 bodies unbanded, 18.7 MB, and 128 bodies at w = 64, 2.1 MB."""
    pl = trace_plan(*EXT, "--width", 64, "2000x2000", "6000x6000")
    assert pl["pairs"][0]["windows"] == [[0, 10], [7, 18], [15, 26], [23, 33]]
    assert pl["pairs"][0]["dir_bytes"] == 42 * 64 * 256 == 688128
    assert pl["pairs"][1]["dir_bytes"] == 128 * 64 * 256 == 2097152
    full = trace_plan(*EXT, "2000x2000", "6000x6000")
    assert [p["dir_bytes"] for p in full["pairs"]] == [4 * 33 * 64 * 256, 12 * 95 * 64 * 256]
    assert full["pairs"][1]["dir_bytes"] == 18677760
    # under a budget of 8 MiB the big pair is refused unbanded and planned inside its width
    assert trace_plan(*EXT, "--budget", 8 << 20, "6000x6000")["error"] == SA_ERR_UNSUPPORTED
    assert trace_plan(*EXT, "--budget", 8 << 20, "--width", 64, "6000x6000")["arena_bytes"] == 2097152
    # and refused only when the band itself exceeds the budget
    pl = trace_plan(*EXT, "--budget", 2 << 20, "--width", 65, "6000x6000")
    assert pl["error"] == SA_ERR_UNSUPPORTED and "direction bytes" in pl["message"]
    # chunks are cut by the band's bytes: five pairs of 688128 bytes under a budget of 1.5 MB go two by two
    pl = trace_plan(*EXT, "--budget", 1500000, "--width", 64, "2000x2000x5")
    assert pl["num_chunks"] == 3 and pl["chunk_begin"] == [0, 2, 4, 5] and pl["arena_bytes"] == 2 * 688128


# ---- a width that admits every cell ---------------------------------------------------------------------------------------
SHAPES = ["400x150x3", "1000x512x2", "63x70", "1x1", "0x5", "5x0", "129x1000"]
SAME = ("A", "gap", "R", "key_rowbits", "num_cu", "waves_per_simd", "grid", "num_pairs", "max_text", "row_stride", "input_bytes",
        "device_bytes", "padded_cells", "cost", "affine", "gap_extend", "order")


@pytest.mark.parametrize("w", [1000, 1 << 30])
def test_a_width_that_admits_every_cell_costs_the_full_rectangle(w):
    local = score_plan("--mode", "local", *GAP, *SHAPES)
    pl = score_plan(*EXT, "--width", w, *SHAPES)
    for k in SAME:
        assert pl[k] == local[k], k
    assert pl == {**score_plan(*EXT, *SHAPES), "width": w, "band_cells": pl["band_cells"], "bands": pl["bands"]}
    assert pl["band_cells"] == 3 * 400 * 150 + 2 * 1000 * 512 + 63 * 70 + 1 + 129 * 1000
    # the traced plan: the direction bytes of the global pairs
    full, tp = trace_plan(*EXT, *SHAPES), trace_plan(*EXT, "--width", w, *SHAPES)
    for k in ("arena_bytes", "total_dir_bytes", "string_bytes", "num_chunks", "chunk_begin", "grid", "order"):
        assert tp[k] == full[k], k
    assert [p["dir_bytes"] for p in tp["pairs"]] == [p["dir_bytes"] for p in full["pairs"]]


def test_the_instance_is_affine_whatever_the_penalties():
    """gap open == gap extend: the unbanded extension plans the linear instances, the banded one the affine ones
    (W4: the outputs are the linear recurrence's all the same)."""
    lin = ["--gap", 5, "--gap-extend", 5]
    assert score_plan("--mode", "global", *lin, "--extend", 20, *SHAPES)["affine"] is False
    pl = score_plan("--mode", "global", *lin, "--extend", 20, "--width", 1000, *SHAPES)
    local = score_plan("--mode", "local", "--gap", 5, "--gap-extend", 5, *SHAPES)
    assert pl["affine"] is True and local["affine"] is True and pl["gap_extend"] == 5
    for k in SAME:
        assert pl[k] == local[k], k


# ---- R falls with the width -------------------------------------------------------------------------------------------------
def test_rows_per_lane_fall_with_the_width():
    """2048 pairs of 20000 letters: a tall strip under a narrow band mostly steps through out-of-band cells."""
    gap = ["--mode", "global", "--gap", 16, "--gap-extend", 4, "--extend", "none"]
    Rs, costs = [], []
    for w in (0, 16, 64, 500, 4000, 20000):
        pl = score_plan(*gap, "--width", w, "20000x20000x2048")
        Rs.append(pl["R"])
        costs.append(min(pl["cost"]))
    assert Rs == sorted(Rs) and Rs[0] == 1 and Rs[-1] == 8 and len(set(Rs)) >= 3, Rs
    assert costs == sorted(costs)
    full = score_plan(*gap, "20000x20000x2048")
    assert (full["R"], full["cost"]) == (8, score_plan(*gap, "--width", 20000, "20000x20000x2048")["cost"])
    # the band-at global scorer on {-w, w} covers the same cells at the global step cost: same windows, so the
    # two plans' costs are in the ratio of the step costs at every R (local 18 + 14 R, global 18 + 10 R)
    at = score_plan("--mode", "global", "--gap", 16, "--gap-extend", 4, "--band-at", "-64:64", "20000x20000x2048")
    pl = score_plan(*gap, "--width", 64, "20000x20000x2048")
    assert [c * (18 + 10 * R) for c, R in zip(pl["cost"], (1, 2, 4, 8))] == [c * (18 + 14 * R) for c, R in zip(at["cost"], (1, 2, 4, 8))]
    assert pl["band_cells"] == at["band_cells"]


# ---- seeds: the items are planned from their halves' shapes -----------------------------------------------------------------
def test_the_seeds_items_are_planned_from_their_halves():
    """300 x 200 with the seed {100, 50, 10}: the left half is 100 columns x 50 rows, the right half 190 x 140.
    At w = 5 both bands are {-5, 5}; at w = 120 the left half's is {-50, 100}, clipped to its own shape, which
    admits every cell, and the right half's {-120, 120}."""
    args = [*EXT, "--seeds", "100:50:10", "300x200"]
    pl = score_plan(*args, "--width", 5, "--rows-per-lane", 1)
    assert pl["seeds"] is True and pl["width"] == 5 and pl["num_pairs"] == 2 and pl["halves"] == [[0, 1]]
    assert [(it["n"], it["m"], it["dir"]) for it in pl["items"]] == [(100, 50, -1), (190, 140, 1)]
    for b, (n, m) in zip(pl["bands"], ((100, 50), (190, 140))):
        cells, windows = count(n, m, 5, 64)
        assert (b["lo"], b["hi"], b["cells"], b["windows"]) == (-5, 5, cells, windows)
    assert pl["bands"][0]["cells"] == 11 * 50 - 15 and pl["bands"][0]["windows"] == [[1, 55, 0, 2]]
    assert pl["band_cells"] == sum(b["cells"] for b in pl["bands"]) and pl["order"] == [1, 0]
    wide = score_plan(*args, "--width", 120)
    assert [(b["lo"], b["hi"]) for b in wide["bands"]] == [(-50, 100), (-120, 120)]
    assert wide["bands"][0]["cells"] == 100 * 50
    # a width that admits every cell of both halves: the unbanded seeds plan but for the affine instance's name
    full, w1 = score_plan(*args), score_plan(*args, "--width", 190)
    for k in SAME + ("items", "halves"):
        if k != "waves_per_simd":
            assert w1[k] == full[k], k
    # but for the grid's class: the banded instances hold 7, 5, 4, 3 waves per SIMD at R = 1, 2, 4, 8, the affine 8, 5, 4, 3
    assert (full["R"], full["waves_per_simd"], w1["waves_per_simd"]) == (1, 8, 7)
    for R, waves in ((1, 7), (2, 5), (4, 4), (8, 3)):
        assert score_plan(*args, "--width", 5, "--rows-per-lane", R)["waves_per_simd"] == waves
    # the traced plan: two banded rectangles, each from its own shape
    tp = trace_plan(*args, "--width", 5)
    assert tp["width"] == 5 and [it["dir_bytes"] for it in tp["items"]] == [dir_bytes(100, 50, 5), dir_bytes(190, 140, 5)] == [32768, 65536]
    assert tp["arena_bytes"] == 98304 and tp["order"] == [1, 0]
    # the bare centre of 6000 x 6000 under 8 MiB: 2 x 4.7 MB unbanded, 2 x 1.0 MB at w = 64
    big = [*EXT, "--budget", 8 << 20, "--seeds", "3000:3000:0", "6000x6000"]
    refused = trace_plan(*big)
    assert refused["error"] == SA_ERR_UNSUPPORTED and "halves" in refused["message"]
    tp = trace_plan(*big, "--width", 64)
    assert [it["dir_bytes"] for it in tp["items"]] == [dir_bytes(3000, 3000, 64)] * 2 and tp["arena_bytes"] == 2 * dir_bytes(3000, 3000, 64) < 2.4e6
    tp = trace_plan(*EXT, "--budget", 2000000, "--seeds", "3000:3000:0", "--width", 64, "6000x6000")
    assert tp["error"] == SA_ERR_UNSUPPORTED and "halves" in tp["message"]  # only when the two bands exceed the arena


# ---- refusals and limits ------------------------------------------------------------------------------------------------------
def test_refusals_and_limits():
    for plan in (score_plan, trace_plan):
        pl = plan(*EXT, "--width", -1, "300x300")
        assert pl == {"error": SA_ERR_INVALID, "message": "width must be >= 0"}
        pl = plan(*EXT, "--width", -1, "--seeds", "1:1:1", "300x300")
        assert pl == {"error": SA_ERR_INVALID, "message": "width must be >= 0"}
        # a band of either kind beside --extend stays what it was, with or without a width
        for band in (["--band", 3], ["--band-at", "-3:3"]):
            for width in ([], ["--width", 3]):
                for seeds in ([], ["--seeds", "1:1:1"]):
                    pl = plan(*EXT, *band, *width, *seeds, "300x300")
                    assert pl == {"error": SA_ERR_UNSUPPORTED, "message": "extension alignment inside a band (band or bands with xdrop) is not built"}
        # the mode and xdrop rules are extension's
        for mode in ("local", "fit", 16, 31):
            pl = plan("--mode", mode, *GAP, "--extend", 20, "--width", 3, "300x300")
            assert pl["error"] == SA_ERR_INVALID and "SA_GLOBAL" in pl["message"]
        for x in (-2, 1 << 30):
            assert plan("--mode", "global", *GAP, "--extend", x, "--width", 3, "300x300")["error"] == SA_ERR_INVALID
        # the banded score limit: (max|S| + G)(n + m) + G (n + m) with |S| <= 5, n + m = 70 reaches 2^29 at G = 2^22,
        # which the unbanded extension still takes
        big = ["--mode", "global", "--gap", 1 << 22, "--gap-extend", 2, "--extend", 20]
        assert "error" not in plan(*big, "50x20")
        pl = plan(*big, "--width", 3, "50x20")
        assert pl == {"error": SA_ERR_UNSUPPORTED, "message": "scores may reach the band's sentinel"}
        assert plan(*big, "--width", 3, "--seeds", "10:5:3", "50x20") == pl
    # a width without an extension is no call of the library's; the planner refuses the spec
    pl = score_plan("--mode", "global", *GAP, "--width", 3, "300x300")
    assert pl["error"] == SA_ERR_INVALID
    # the best-cell key range is extension's: 2^24 - 2 letters are too many for it at these scores
    pl = score_plan(*EXT, "--width", 3, "16000000x16000000")
    assert pl["error"] == SA_ERR_UNSUPPORTED
