"""Seed extension (sa_hip.h: sa_score_batch_seeds, sa_scorer_create_seeds, sa_align_pairs_seeds) in the
planners, on the CPU: bin/sa_score_plan_check and bin/sa_trace_plan_check take --seeds TS:PS:L, once for
all pairs or once per shape argument. A pair becomes up to two work items, its left half read backwards
and its right half read forwards, each planned as an extension pair of its shape; an empty half is no
item. The trace plan counts the direction bytes of the two rectangles, never of n x m, and keeps a pair's
halves in one chunk. Each case runs a program once."""
from __future__ import annotations

import itertools

from conftest import PKG  # noqa: F401  (first: it puts the package on the path)

from test_score_affine_plan import plan as score_plan
from test_trace_plan import plan as trace_plan

SA_ERR_INVALID, SA_ERR_UNSUPPORTED = 1, 4
GAP = ["--gap", 11, "--gap-extend", 2]


def dir_bytes(n, m):
    """sa_trace_plan.h trace_dir_bytes, by hand: ceil(m / 512) strips of 64 * floor((n + 126) / 64) steps of
    256 bytes; an empty side has none."""
    return 0 if n == 0 or m == 0 else -(-m // 512) * 64 * ((n + 126) // 64) * 256


def items_of(pl):
    return [(it["pair"], it["dir"], it["text_off"], it["pattern_off"], it["n"], it["m"]) for it in pl["items"]]


def test_the_items_of_a_seed_in_the_middle():
    # pair 0: text 300 at 0, pattern 200 at 0; pair 1: text at 300, pattern at 200
    pl = score_plan("--mode", "global", *GAP, "--extend", 20, "--seeds", "100:50:10", "300x200x2")
    assert "error" not in pl and pl["seeds"] is True and pl["extend"] is True and pl["xdrop"] == 20
    # the left half is read backwards from the letter before the seed, the right half forwards from its end
    assert items_of(pl) == [(0, -1, 99, 49, 100, 50), (0, 1, 110, 60, 190, 140),
                            (1, -1, 399, 249, 100, 50), (1, 1, 410, 260, 190, 140)]
    assert pl["halves"] == [[0, 1], [2, 3]] and pl["num_seed_pairs"] == 2
    assert pl["num_pairs"] == 4 and pl["grid"] == 4  # the items: one launch, a wave each
    assert pl["order"] == [1, 3, 0, 2]  # by cells, ties by index
    assert pl["input_bytes"] == 1000 and pl["max_text"] == 190  # the whole pairs' letters; the longest half


def test_seeds_at_the_corners_and_empty_halves():
    for seed, want, halves in (("0:0:0", [(0, 1, 0, 0, 300, 200)], [-1, 0]),
                               ("300:200:0", [(0, -1, 299, 199, 300, 200)], [0, -1]),
                               ("0:50:10", [(0, 1, 10, 60, 290, 140)], [-1, 0]),          # ts = 0 with ps > 0
                               ("100:0:10", [(0, 1, 110, 10, 190, 190)], [-1, 0]),        # ps = 0 with ts > 0
                               ("290:100:10", [(0, -1, 289, 99, 290, 100)], [0, -1]),     # the seed reaches the text's end
                               ("100:190:10", [(0, -1, 99, 189, 100, 190)], [0, -1]),     # and the pattern's
                               ("0:0:200", [], [-1, -1]),                                 # L covers the pattern
                               ("100:0:200", [], [-1, -1]),
                               ("150:100:0", [(0, -1, 149, 99, 150, 100), (0, 1, 150, 100, 150, 100)], [0, 1])):  # a bare anchor
        pl = score_plan("--mode", "global", *GAP, "--seeds", seed, "300x200")
        assert "error" not in pl, seed
        assert items_of(pl) == want and pl["halves"] == [halves], seed
        assert pl["num_pairs"] == len(want) == pl["grid"] and pl["xdrop"] == -1, seed
    pl = score_plan("--mode", "global", *GAP, "--seeds", "0:0:300", "300x300")  # L covers both sides
    assert pl["items"] == [] and pl["order"] == [] and pl["grid"] == 0


def test_one_seed_per_shape_and_the_order_by_cells():
    pl = score_plan("--mode", "global", *GAP, "--seeds", "10:10:5", "--seeds", "500:400:20", "--seeds", "0:0:0",
                    "100x100x2", "1000x900", "40x30")
    assert pl["halves"] == [[0, 1], [2, 3], [4, 5], [-1, 6]]
    cells = [it["n"] * it["m"] for it in pl["items"]]
    assert cells == [100, 85 * 85, 100, 85 * 85, 500 * 400, 480 * 480, 40 * 30]
    assert pl["order"] == [5, 4, 1, 3, 6, 0, 2]
    assert [cells[k] for k in pl["order"]] == sorted(cells, reverse=True)


def test_the_items_are_planned_as_extension_pairs():
    """R, cost, grid, the boundary rows and the order are those of the extension scorer on the halves'
    shapes; the bytes add 8 per item (a 32-byte descriptor) and an 88-byte seed and result per pair."""
    for gap in (GAP, ["--gap", 5, "--gap-extend", 5]):
        seeded = score_plan("--mode", "global", *gap, "--extend", 20, "--seeds", "100:50:10", "300x200x3")
        halves = score_plan("--mode", "global", *gap, "--extend", 20, "100x50", "190x140", "100x50", "190x140", "100x50", "190x140")
        for k in ("R", "cost", "grid", "row_stride", "order", "key_rowbits", "waves_per_simd", "padded_cells", "affine", "gap", "gap_extend"):
            assert seeded[k] == halves[k], k
        assert seeded["affine"] is (gap is GAP)  # (S4): open == extend plans the linear kernels
        assert seeded["input_bytes"] == 1500 and halves["input_bytes"] == 3 * (150 + 330)
        assert seeded["device_bytes"] == halves["device_bytes"] + (1500 - 1440) + 6 * 8 + 3 * (48 + 40)
    for forced in (1, 2, 4, 8):
        pl = score_plan("--mode", "global", *GAP, "--seeds", "100:50:10", "--rows-per-lane", forced, "300x200x3")
        assert pl["R"] == forced


def test_the_trace_plan_counts_the_two_rectangles():
    pl = trace_plan("--mode", "global", *GAP, "--extend", 20, "--seeds", "100:50:10", "300x200x2", "1000x1000")
    assert "error" not in pl and pl["seeds"] is True and pl["R"] == 8 and pl["xdrop"] == 20
    assert pl["num_pairs"] == 3 and pl["num_items"] == 6
    want = [dir_bytes(100, 50), dir_bytes(190, 140)] * 2 + [dir_bytes(100, 50), dir_bytes(890, 940)]
    assert [it["dir_bytes"] for it in pl["items"]] == want
    assert pl["total_dir_bytes"] == pl["arena_bytes"] == sum(want)
    assert want[4] + want[5] < dir_bytes(1000, 1000)  # not the n x m rectangle
    assert pl["string_bytes"] == 500 + 500 + 2000 and [p["slot_off"] for p in pl["pairs"]] == [0, 500, 1000]
    assert pl["num_chunks"] == 1 and pl["chunk_begin"] == [0, 6] and pl["pair_chunk_begin"] == [0, 3]
    assert pl["pair_order"] == [2, 0, 1]  # by the cells of both halves
    assert pl["order"] == [5, 1, 3, 4, 0, 2]  # the chunk's items by cells, ties by index
    # the offsets follow the pair order, left before right
    offs = {k: it["dir_off"] for k, it in enumerate(pl["items"])}
    assert [offs[k] for k in (4, 5, 0, 1, 2, 3)] == [0] + list(itertools.accumulate([want[k] for k in (4, 5, 0, 1, 2)]))
    # empty halves: no item, no bytes
    pl = trace_plan("--mode", "global", *GAP, "--seeds", "0:0:200", "300x200")
    assert pl["num_items"] == 0 and pl["arena_bytes"] == 0 and pl["num_chunks"] == 1 and pl["chunk_begin"] == [0, 0]
    assert pl["pairs"] == [{"left": -1, "right": -1, "slot_off": 0}]


def test_a_seeded_pair_plans_under_a_budget_that_refuses_the_unseeded_pair():
    full, half = dir_bytes(3000, 3000), dir_bytes(1500, 1500)
    budget = 3000000
    assert 2 * half <= budget < full
    pl = trace_plan("--mode", "global", *GAP, "--extend", "none", "--budget", budget, "3000x3000")
    assert pl["error"] == SA_ERR_UNSUPPORTED and "direction bytes" in pl["message"]
    pl = trace_plan("--mode", "global", *GAP, "--seeds", "1500:1500:0", "--budget", budget, "3000x3000")
    assert "error" not in pl and pl["arena_bytes"] == 2 * half and pl["num_chunks"] == 1
    # the two halves together exceed the budget: refused, the message names the pair
    pl = trace_plan("--mode", "global", *GAP, "--seeds", "5:5:0", "--seeds", "1500:1500:0", "--budget", 2 * half - 1, "10x10", "3000x3000")
    assert pl["error"] == SA_ERR_UNSUPPORTED and "pair 1" in pl["message"] and "halves" in pl["message"]
    # one half alone may fill the budget
    pl = trace_plan("--mode", "global", *GAP, "--seeds", "0:0:0", "--budget", dir_bytes(1500, 1500), "1500x1500")
    assert "error" not in pl


def test_both_halves_of_a_pair_share_a_chunk():
    left, right = dir_bytes(300, 513), dir_bytes(290, 477)
    per_pair = left + right
    # five equal pairs, a budget of two and a half: two pairs a chunk, never a pair's halves apart
    pl = trace_plan("--mode", "global", *GAP, "--seeds", "300:513:10", "--budget", 2 * per_pair + left, "600x1000x5")
    assert "error" not in pl and pl["num_chunks"] == 3
    assert pl["pair_chunk_begin"] == [0, 2, 4, 5] and pl["chunk_begin"] == [0, 4, 8, 10]
    assert pl["arena_bytes"] == 2 * per_pair
    for c in range(3):
        items = pl["order"][pl["chunk_begin"][c]:pl["chunk_begin"][c + 1]]
        pairs = pl["pair_order"][pl["pair_chunk_begin"][c]:pl["pair_chunk_begin"][c + 1]]
        assert sorted(pl["items"][k]["pair"] for k in items) == sorted(pairs * 2), c
        cells = [pl["items"][k]["n"] * pl["items"][k]["m"] for k in items]
        assert cells == sorted(cells, reverse=True), c  # by cells inside the chunk
        # the chunk's items lie apart in the arena, from offset 0
        spans = sorted((pl["items"][k]["dir_off"], pl["items"][k]["dir_bytes"]) for k in items)
        assert spans[0][0] == 0 and all(a + b == c2 for (a, b), (c2, _) in zip(spans, spans[1:])), c
        assert spans[-1][0] + spans[-1][1] <= pl["budget"]


def test_refusals():
    for plan in (score_plan, trace_plan):
        # a seed that does not lie inside its pair: the first such pair is named
        for seed in ("291:0:10", "0:191:10", "301:0:0", "0:201:0", "0:0:201", "100:100:101", "18446744073709551615:0:2"):
            pl = plan("--mode", "global", *GAP, "--seeds", "0:0:0", "--seeds", seed, "50x50x2", "300x200")
            assert pl["error"] == SA_ERR_INVALID and "pair 2" in pl["message"] and "seed" in pl["message"], seed
        assert "error" not in plan("--mode", "global", *GAP, "--seeds", "290:190:10", "300x200")
        # the mode and the xdrop, as the extension functions have them
        for mode in ("local", "fit", 16, 31, 3):
            pl = plan("--mode", mode, *GAP, "--extend", 20, "--seeds", "0:0:0", "100x100")
            assert pl["error"] == SA_ERR_INVALID and "SA_GLOBAL" in pl["message"], mode
        for x in (-2, 1 << 30, -100):
            pl = plan("--mode", "global", *GAP, "--extend", x, "--seeds", "0:0:0", "100x100")
            assert pl["error"] == SA_ERR_INVALID and "xdrop" in pl["message"], x
        assert "error" not in plan("--mode", "global", *GAP, "--extend", (1 << 30) - 1, "--seeds", "0:0:0", "100x100")
        # a band of either kind stays refused exactly as with --extend
        for band in (["--band", 5], ["--band-at", "-5:5"]):
            a = plan("--mode", "global", *GAP, "--extend", 20, "--seeds", "10:10:5", *band, "100x100")
            b = plan("--mode", "global", *GAP, "--extend", 20, *band, "100x100")
            assert a == b and a["error"] == SA_ERR_UNSUPPORTED and "band" in a["message"], band
    # the linear scorer has no seeds: the penalties are part of the call
    assert score_plan("--mode", "global", "--gap", 5, "--seeds", "0:0:0", "100x100")["error"] == SA_ERR_INVALID


def test_the_limits_are_the_whole_pairs():
    # the halves alone would pass the int32 limit, the pair does not: the limit covers the sum
    ok = score_plan("--mode", "global", "--gap", 100000, "--gap-extend", 2, "--extend", 20, "2600x2600")
    assert "error" not in ok
    whole = score_plan("--mode", "global", "--gap", 100000, "--gap-extend", 2, "--extend", 20, "5300x5300")
    assert whole["error"] == SA_ERR_UNSUPPORTED and whole["message"] == "scores may exceed the int32 range"
    pl = score_plan("--mode", "global", "--gap", 100000, "--gap-extend", 2, "--seeds", "2650:2650:0", "5300x5300")
    assert pl["error"] == SA_ERR_UNSUPPORTED and pl["message"] == whole["message"]
    pl = score_plan("--mode", "global", "--gap", 5, "--gap-extend", 5, "--seeds", "5:5:5", "16777215x100")
    assert pl["error"] == SA_ERR_UNSUPPORTED and "2^24" in pl["message"]
