"""The band-at path on the CPU (sa_hip.h: a band lo <= j - i <= hi of the caller's per pair):
sa_band_reachable against a brute-force fill, and the planners through bin/sa_score_plan_check and
bin/sa_trace_plan_check with --band-at LO:HI: band cells, the possibly empty window of every strip and
the direction bytes against a plain Python count; the plan of --band at the band it derives; the
unbanded direction bytes where the band admits every cell; and the refusals."""
from __future__ import annotations

import pytest

from sa_amd import engine
from test_band_plan import count_windows as derived_windows, limits
from test_score_affine_plan import plan as score_plan
from test_trace_plan import plan as trace_plan

SA_ERR_INVALID, SA_ERR_UNSUPPORTED = 1, 4
GLOBAL, LOCAL, FIT, ENDS = 0, 1, 2, 16
TB, TE, PB, PE = 1, 2, 4, 8


# ---- sa_band_reachable ----------------------------------------------------------------------------------------------
def real_cells(n, m, lo, hi, starts):
    """The cells with a real value when `starts` are the real border cells the fill begins from: a border
    cell that costs is real iff the border cell before it is (a gap run from the origin), an interior
    cell iff it is in band and one of its three neighbours is real."""
    inb = lambda i, j: lo <= j - i <= hi  # noqa: E731
    real = [[False] * (n + 1) for _ in range(m + 1)]
    for i in range(m + 1):
        for j in range(n + 1):
            if not inb(i, j):
                continue
            if (i, j) in starts:
                real[i][j] = True
            elif i == 0:
                real[i][j] = j > 0 and real[0][j - 1]
            elif j == 0:
                real[i][j] = real[i - 1][0]
            else:
                real[i][j] = real[i - 1][j - 1] or real[i - 1][j] or real[i][j - 1]
    return real


def reachable_by_fill(flags, n, m, lo, hi, fills):
    """Some candidate, (m, n), row m under TE, column n under PE, is real."""
    origin, row0, col0 = fills
    real = lambda i, j: origin[i][j] or (flags & TB and row0[i][j]) or (flags & PB and col0[i][j])  # noqa: E731
    cand = [(m, n)] + ([(m, j) for j in range(n + 1)] if flags & TE else []) + ([(i, n) for i in range(m + 1)] if flags & PE else [])
    return any(real(i, j) for i, j in cand)


def test_band_reachable_equals_a_brute_force_fill():
    """Every n, m <= 6, -8 <= lo <= hi <= 8 and all 16 flag sets: 119952 cases."""
    seen = {f: [0, 0] for f in range(16)}
    cases = 0
    for n in range(7):
        for m in range(7):
            for lo in range(-8, 9):
                for hi in range(lo, 9):
                    fills = (real_cells(n, m, lo, hi, {(0, 0)}),
                             real_cells(n, m, lo, hi, {(0, j) for j in range(n + 1)}),
                             real_cells(n, m, lo, hi, {(i, 0) for i in range(m + 1)}))
                    for f in range(16):
                        want = reachable_by_fill(f, n, m, lo, hi, fills)
                        assert engine.band_reachable(ENDS | f, n, m, lo, hi) == want, (f, n, m, lo, hi)
                        seen[f][want] += 1
                        cases += 1
                    assert engine.band_reachable(GLOBAL, n, m, lo, hi) == reachable_by_fill(0, n, m, lo, hi, fills)
                    assert engine.band_reachable(FIT, n, m, lo, hi) == reachable_by_fill(TB | TE, n, m, lo, hi, fills)
                    assert engine.band_reachable(LOCAL, n, m, lo, hi)
    assert cases == 119952
    assert all(no > 0 and yes > 0 for no, yes in seen.values()), seen
    assert sum(no for no, _ in seen.values()) == 54600


def test_band_reachable_modes_and_large_values():
    for mode in (3, 15, 32, -1):
        with pytest.raises(engine.SaError):
            engine.band_reachable(mode, 10, 10, 0, 0)
    assert not engine.band_reachable(FIT, 10, 10, 3, 2)  # lo > hi
    assert engine.band_reachable(LOCAL, 10, 10, 3, 2)    # a local pair always: the planner refuses lo > hi itself
    big = (1 << 31) - 1
    assert engine.band_reachable(GLOBAL, 1 << 24, 1 << 24, -big - 1, big)
    assert engine.band_reachable(FIT, 5_000_000, 10_000, 2_000_000, 2_000_100)
    assert not engine.band_reachable(FIT, 5_000_000, 10_000, 4_990_001, big)      # the read would end past the text
    assert engine.band_reachable(ENDS | TB | PE, 5_000_000, 10_000, 4_990_001, big)  # unless its end is free


# ---- the planners ---------------------------------------------------------------------------------------------------
def count_cells(n, m, lo, hi):
    return sum(1 for i in range(1, m + 1) for j in range(max(1, i + lo), min(n, i + hi) + 1))


def count_windows(n, m, lo, hi, rows):
    """Per strip of `rows` rows: the first and last in-band column of any of its rows and the 64-step bodies
    that hold a step at which some lane meets one of them (test_band_plan.count_windows), or
    [1, 0, 0, 0] for a strip without an in-band cell."""
    out = []
    for first in range(1, m + 1, rows):
        last = min(m, first + rows - 1)
        cols = [j for i in range(first, last + 1) for j in range(max(1, i + lo), min(n, i + hi) + 1)]
        out.append([min(cols), max(cols), (min(cols) - 1) // 64, (max(cols) + 62) // 64 + 1] if cols else [1, 0, 0, 0])
    return out


# (n, m, lo, hi, mode): hi < 0 with empty top strips, lo > 0 with empty bottom strips, bands inside the text,
# limits beyond [-m, n]
AT = [(600, 1100, -700, -560, ENDS | PB | PE | TE), (600, 1100, -70, -1, ENDS | PB | PE | TE), (300, 1100, 100, 140, ENDS | TB | PE),
      (300, 1100, 1, 64, ENDS | 15), (450, 150, 125, 135, FIT), (813, 513, 0, 0, FIT), (813, 513, 236, 364, FIT),
      (750, 150, 600, 600, FIT), (65, 64, -1000, 1000, GLOBAL), (200, 1500, -1400, -1300, ENDS | PB | TE),
      (1500, 200, 1290, 1310, ENDS | TB | PE), (1, 1, 0, 0, GLOBAL), (64, 64, -3, 70, LOCAL), (500, 513, 600, 700, LOCAL),
      (500, 513, -900, -600, LOCAL)]


@pytest.mark.parametrize("n,m,lo,hi,mode", AT)
def test_band_cells_windows_and_direction_bytes_against_a_plain_count(n, m, lo, hi, mode):
    assert engine.band_reachable(mode, n, m, lo, hi)
    clo, chi = min(max(lo, -m), n), min(max(hi, -m), n)
    cells = count_cells(n, m, lo, hi)
    for R in (1, 2, 8):
        pl = score_plan("--mode", mode, "--gap", 11, "--gap-extend", 2, "--band-at", f"{lo}:{hi}", "--rows-per-lane", R, f"{n}x{m}")
        b = pl["bands"][0]
        assert (b["lo"], b["hi"]) == (clo, chi) and pl["band"] == -1
        want = count_windows(n, m, lo, hi, 64 * R)
        assert b["windows"] == want, R
        assert pl["padded_cells"] == sum((x[1] - x[0] + 1) * 64 * R for x in want), R
        fit = mode == FIT or (mode >= ENDS and mode & TE)
        per_step = (18 + (4 if fit else 0)) + R * ((14 if mode == LOCAL else 10) + (1 if fit else 0))
        assert pl["cost"][(1, 2, 4, 8).index(R)] == sum(x[1] - x[0] + 64 for x in want if x[3] > x[2]) * per_step, R
        assert b["cells"] == pl["band_cells"] == cells
    tp = trace_plan("--mode", mode, "--band-at", f"{lo}:{hi}", f"{n}x{m}", f"{n}x{m}")
    want = count_windows(n, m, lo, hi, 512)
    for pr in tp["pairs"]:
        assert pr["dir_bytes"] == sum(64 * (x[3] - x[2]) * 256 for x in want)
        assert pr["windows"] == ([x[2:] for x in want] if pr["dir_bytes"] else [])  # a pair without directions lists no strips
        assert pr["strips"] == (len(want) if pr["dir_bytes"] else 0) and pr["steps"] * 256 == pr["dir_bytes"]
    assert tp["arena_bytes"] == 2 * tp["pairs"][0]["dir_bytes"] and tp["pairs"][1]["dir_off"] == tp["pairs"][0]["dir_bytes"]


def test_the_cases_hold_empty_top_and_bottom_strips():
    assert count_windows(600, 1100, -700, -560, 512)[0] == [1, 0, 0, 0]
    assert [w == [1, 0, 0, 0] for w in count_windows(600, 1100, -700, -560, 64)[:9]] == [True] * 8 + [False]
    assert count_windows(300, 1100, 100, 140, 512)[1:] == [[1, 0, 0, 0]] * 2
    assert count_windows(300, 1100, 1, 64, 64)[5:] == [[1, 0, 0, 0]] * 13


def test_the_derived_band_plans_as_the_banded_call():
    lengths = [1, 63, 65, 513, 1500]
    for mode in ("global", "local"):
        for w in (0, 1, 64, 200):
            for n in lengths:
                for m in lengths:
                    lo, hi = limits(n, m, w)
                    a = score_plan("--mode", mode, "--gap", 11, "--gap-extend", 2, "--band", w, f"{n}x{m}x3")
                    b = score_plan("--mode", mode, "--gap", 11, "--gap-extend", 2, "--band-at", f"{lo}:{hi}", f"{n}x{m}x3")
                    assert a["device_bytes"] + 3 * 8 == b["device_bytes"]  # the pairs' bands
                    assert (a["band"], b["band"]) == (w, -1)
                    # --band prints the limits its half-width derives, --band-at its own clipped to [-m, n]
                    assert [(x["lo"], x["hi"]) for x in b["bands"]] == [(max(lo, -m), min(hi, n))] * 3
                    for x in a["bands"] + b["bands"]:
                        x["lo"] = x["hi"] = None
                    a["band"] = b["band"] = a["device_bytes"] = b["device_bytes"] = None
                    assert a == b, (mode, w, n, m)
            ta = trace_plan("--mode", mode, "--band", w, "1500x513", "64x1500", "513x513")
            td = [trace_plan("--mode", mode, "--band-at", "%d:%d" % limits(n, m, w), f"{n}x{m}")["pairs"][0]
                  for n, m in ((1500, 513), (64, 1500), (513, 513))]
            assert [(p["dir_bytes"], p["windows"]) for p in ta["pairs"]] == [(p["dir_bytes"], p["windows"]) for p in td]
    assert derived_windows(1500, 513, 64, 512) == count_windows(1500, 513, *limits(1500, 513, 64), 512)


def test_the_whole_rectangle_plans_the_unbanded_direction_bytes():
    shapes = ["1x1", "63x64", "513x1500", "1500x513", "64x1", "700x700"]
    for mode in ("global", "local", "fit", 16, 31, 25):
        full = trace_plan("--mode", mode, *shapes)
        for n, m in ((1, 1), (63, 64), (513, 1500), (1500, 513), (64, 1), (700, 700)):
            k = shapes.index(f"{n}x{m}")
            for lo, hi in ((-m, n), (-(1 << 31), (1 << 31) - 1)):
                at = trace_plan("--mode", mode, "--band-at", f"{lo}:{hi}", f"{n}x{m}")
                assert at["pairs"][0]["dir_bytes"] == full["pairs"][k]["dir_bytes"] == at["arena_bytes"], (mode, n, m)
                sp = score_plan("--mode", mode, "--gap", 11, "--gap-extend", 2, "--band-at", f"{lo}:{hi}", f"{n}x{m}")
                un = score_plan("--mode", mode, "--gap", 11, "--gap-extend", 2, f"{n}x{m}")
                for key in ("R", "cost", "padded_cells", "order", "grid", "row_stride", "key_rowbits"):
                    assert sp[key] == un[key], (mode, n, m, key)
                assert sp["band_cells"] == n * m


def test_refusals():
    for plan in (score_plan, trace_plan):
        bad = plan("--mode", "fit", "--gap", 11, "--gap-extend", 2, "--band-at", "5:4", "100x100")
        assert bad["error"] == SA_ERR_INVALID and "lo > hi" in bad["message"] and "pair 0" in bad["message"]
        # an unreachable pair: the second shape cannot end a fit on diagonals 150 .. 160
        un = plan("--mode", "fit", "--gap", 11, "--gap-extend", 2, "--band-at", "150:160", "400x100", "200x100", "400x100")
        assert un["error"] == SA_ERR_INVALID and "pair 1" in un["message"] and "[150, 160]" in un["message"]
        assert "error" not in plan("--mode", "fit", "--gap", 11, "--gap-extend", 2, "--band-at", "150:160", "400x100", "260x100")
        # global needs the origin and (m, n)
        assert plan("--mode", "global", "--gap", 11, "--gap-extend", 2, "--band-at", "1:300", "400x100")["error"] == SA_ERR_INVALID
        assert "error" not in plan("--mode", "global", "--gap", 11, "--gap-extend", 2, "--band-at", "0:300", "400x100")
        assert "error" not in plan("--mode", "local", "--gap", 11, "--gap-extend", 2, "--band-at", "900:901", "400x100")
        # --band keeps its meaning and its refusals
        fit = plan("--mode", "fit", "--gap", 11, "--gap-extend", 2, "--band", 5, "100x100")
        assert fit["error"] == SA_ERR_UNSUPPORTED and "SA_FIT" in fit["message"]
        both = plan("--mode", "global", "--gap", 11, "--gap-extend", 2, "--band", 5, "--band-at", "-5:5", "100x100")
        assert both["error"] == SA_ERR_INVALID
    assert score_plan("--mode", "fit", "--gap", 5, "--band-at", "0:5", "100x100")["error"] == SA_ERR_INVALID  # no gap model
    # the score limit is the banded one
    args = ("--mode", "fit", "--gap-extend", 1, "--band-at", "0:3", "512x512")
    assert "error" not in score_plan("--gap", 262141, *args)
    over = score_plan("--gap", 262142, *args)
    assert over["error"] == SA_ERR_UNSUPPORTED and "sentinel" in over["message"]
    assert trace_plan("--gap", 262142, *args)["error"] == SA_ERR_UNSUPPORTED


def test_a_fit_pair_beyond_the_budget_is_planned_inside_its_band():
    budget = 8 << 20
    full = trace_plan("--mode", "fit", "--budget", budget, "40000x6000")
    assert full["error"] == SA_ERR_UNSUPPORTED and "SA_TRACE_ARENA_BYTES" in full["message"]
    band = trace_plan("--mode", "fit", "--budget", budget, "--band-at", "20900:21100", "40000x6000")
    assert band["num_chunks"] == 1
    assert band["arena_bytes"] == sum(64 * (x[3] - x[2]) * 256 for x in count_windows(40000, 6000, 20900, 21100, 512)) < budget
