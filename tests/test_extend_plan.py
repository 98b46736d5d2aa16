"""Extension alignment (sa_hip.h: sa_score_batch_extend, sa_scorer_create_extend, sa_align_pairs_extend) in
the planners, on the CPU: bin/sa_score_plan_check and bin/sa_trace_plan_check take --extend X, "none" for
SA_NO_XDROP. An extension runs the local program on the global borders: it is planned as a local scorer of
its penalties, the linear one when gap open equals gap extend, and traced with the arena of a global pair;
the X-drop changes no plan, as the stop rows are not known beforehand. Each case runs a program once."""
from __future__ import annotations

import pytest

from conftest import PKG  # noqa: F401  (first: it puts the package on the path)

from test_ends_plan import SHAPES
from test_score_affine_plan import plan as score_plan
from test_trace_plan import plan as trace_plan

SA_ERR_INVALID, SA_ERR_UNSUPPORTED = 1, 4
# (the extension's penalties, the local scorer it plans as)
GAPS = [(["--gap", 5, "--gap-extend", 5], ["--gap", 5]), (["--gap", 11, "--gap-extend", 2], ["--gap", 11, "--gap-extend", 2])]
XDROPS = [0, 20, "none"]
SAME = ("A", "gap", "R", "key_rowbits", "num_cu", "waves_per_simd", "grid", "num_pairs", "max_text", "row_stride", "input_bytes",
        "device_bytes", "padded_cells", "cost", "affine", "gap_extend", "order")


@pytest.mark.parametrize("ext,loc", GAPS)
def test_the_extend_plan_is_the_local_plan_whatever_the_xdrop(ext, loc):
    local = score_plan("--mode", "local", *loc, *SHAPES)
    assert "error" not in local
    for x in XDROPS:
        pl = score_plan("--mode", "global", *ext, "--extend", x, *SHAPES)
        assert "error" not in pl and pl["mode"] == 0 and pl["extend"] is True
        assert pl["xdrop"] == (-1 if x == "none" else x)
        for k in SAME:
            assert pl[k] == local[k], (x, k)  # cost[], R, grid, order, bytes: the local program's
    # not the global plan: the step of a best-cell program costs more
    assert local["cost"] != score_plan("--mode", "global", *loc, *SHAPES)["cost"]
    assert local["affine"] is (len(loc) == 4)


@pytest.mark.parametrize("ext,loc", GAPS)
@pytest.mark.parametrize("forced,got", [(1, 1), (2, 2), (4, 4), (8, 8), (16, 8)])
def test_forced_rows_per_lane(ext, loc, forced, got):
    pl = score_plan("--mode", "global", *ext, "--extend", 20, "--rows-per-lane", forced, "600x150x10")
    base = score_plan("--mode", "local", *loc, "--rows-per-lane", forced, "600x150x10")
    assert pl["R"] == got == base["R"]
    assert (pl["waves_per_simd"], pl["grid"], pl["cost"]) == (base["waves_per_simd"], base["grid"], base["cost"])


def test_the_trace_plan_is_the_global_one():
    shapes = ["600x150x3", "300x513x2", "1x1", "0x5", "5x0"]
    for gap in (["--gap", 11, "--gap-extend", 2], ["--gap", 5, "--gap-extend", 5]):
        glob = trace_plan("--mode", "global", *gap, *shapes)
        for x in XDROPS:
            pl = trace_plan("--mode", "global", *gap, "--extend", x, *shapes)
            assert "error" not in pl and pl["mode"] == 0 and pl["R"] == 8
            for k in ("arena_bytes", "total_dir_bytes", "string_bytes", "num_chunks", "chunk_begin", "pairs", "grid", "order"):
                assert pl[k] == glob[k], (x, k)  # a pair is traced as a global one: direction bytes, slots, chunks
    pl = trace_plan("--mode", "global", "--extend", 20, "--budget", 400000, "300x513x5")
    assert pl["num_chunks"] == 3 and pl["chunk_begin"] == [0, 2, 4, 5]
    pl = trace_plan("--mode", "global", "--extend", 20, "--budget", 100000, "300x513")
    assert pl["error"] == SA_ERR_UNSUPPORTED and "direction bytes" in pl["message"]


def test_refusals():
    gap = ["--gap", 11, "--gap-extend", 2]
    for plan in (score_plan, trace_plan):
        # a band of either kind with extend: not built, and the message says which combination
        for band in (["--band", 5], ["--band-at", "-5:5"]):
            pl = plan("--mode", "global", *gap, "--extend", 20, *band, "100x100")
            assert pl["error"] == SA_ERR_UNSUPPORTED and "band" in pl["message"] and "exten" in pl["message"], band
        for x in (-2, 1 << 30, -100):
            pl = plan("--mode", "global", *gap, "--extend", x, "100x100")
            assert pl["error"] == SA_ERR_INVALID and "xdrop" in pl["message"], x
        assert "error" not in plan("--mode", "global", *gap, "--extend", (1 << 30) - 1, "100x100")
        for mode in ("local", "fit", 16, 31, 3):
            pl = plan("--mode", mode, *gap, "--extend", 20, "100x100")
            assert pl["error"] == SA_ERR_INVALID and "SA_GLOBAL" in pl["message"], mode
    # the linear scorer has no extension: the penalties are part of the call
    pl = score_plan("--mode", "global", "--gap", 5, "--extend", 20, "100x100")
    assert pl["error"] == SA_ERR_INVALID


def test_the_limits_are_the_int32_one_and_the_key_range():
    pl = score_plan("--mode", "global", "--gap", 1000000, "--gap-extend", 2, "--extend", 20, "1000x1000")
    assert pl["error"] == SA_ERR_UNSUPPORTED and pl["message"] == "scores may exceed the int32 range"
    # inside the int32 limit, beyond the key: global takes the shape, local and the extension do not
    big = "16000000x16000000"
    assert "error" not in score_plan("--mode", "global", "--gap", 5, "--gap-extend", 5, big)
    want = score_plan("--mode", "local", big)["message"]
    assert "key range" in want
    pl = score_plan("--mode", "global", "--gap", 5, "--gap-extend", 5, "--extend", "none", big)
    assert pl["error"] == SA_ERR_UNSUPPORTED and pl["message"] == want
    pl = score_plan("--mode", "global", "--extend", 20, "16777215x100")
    assert pl["error"] in (SA_ERR_INVALID, SA_ERR_UNSUPPORTED)  # no penalties given, or the length limit
    pl = score_plan("--mode", "global", "--gap", 5, "--gap-extend", 5, "--extend", 20, "16777215x100")
    assert pl["error"] == SA_ERR_UNSUPPORTED and "2^24" in pl["message"]
