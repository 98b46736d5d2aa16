"""Chained seeds (sa_hip.h: sa_score_batch_chains, sa_scorer_create_chains, sa_align_pairs_chains) in the
planners, on the CPU: bin/sa_score_plan_check and bin/sa_trace_plan_check take --chain TS:PS:L,TS:PS:L,...,
once for all pairs or once per shape argument. A pair becomes its two end items (the seeds scorer's halves of
its first and its last seed) and one gap item per rectangle between two consecutive seeds; a piece with an empty
side is no item, and an empty-side gap's closed-form score and length go into the pair's record. Each launch
has a plan of its own. The trace plan counts the direction bytes of the pieces, never of n x m, and keeps a
pair's pieces in one chunk. Each case runs a program once."""
from __future__ import annotations

import ctypes
import os

from conftest import PKG  # noqa: F401  (first: it puts the package on the path)

from test_score_affine_plan import plan as score_plan
from test_seeds_plan import dir_bytes
from test_trace_plan import plan as trace_plan

SA_ERR_INVALID, SA_ERR_UNSUPPORTED = 1, 4
GAP = ["--gap", 11, "--gap-extend", 2]


def items_of(items):
    return [(it["pair"], it["dir"], it["text_off"], it["pattern_off"], it["n"], it["m"]) for it in items]


def test_the_library_exports_the_three_functions():
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libsa_hip.so"))
    for name in ("sa_score_batch_chains", "sa_scorer_create_chains", "sa_align_pairs_chains"):
        assert getattr(lib, name) is not None


def test_three_seeds_in_the_middle_of_a_pair():
    # pair 0: text 300 at 0, pattern 200 at 0; pair 1: text at 300, pattern at 200
    pl = score_plan("--mode", "global", *GAP, "--extend", 20, "--chain", "50:30:10,100:80:10,150:100:20", "300x200x2")
    assert "error" not in pl and pl["chains_call"] is True and pl["xdrop"] == 20
    # the ends are the halves of seed 0 and of seed 2; the gaps lie between the end of a seed and the next seed
    assert items_of(pl["ends"]) == [(0, -1, 49, 29, 50, 30), (0, 1, 170, 120, 130, 80),
                                    (1, -1, 349, 229, 50, 30), (1, 1, 470, 320, 130, 80)]
    assert items_of(pl["gaps"]) == [(0, 1, 60, 40, 40, 40), (0, 1, 110, 90, 40, 10),
                                    (1, 1, 360, 240, 40, 40), (1, 1, 410, 290, 40, 10)]
    assert pl["chains"][0] == {"left": 0, "right": 1, "seeds": [0, 3], "gap_items": [0, 2], "closed_score": 0, "closed_cols": 0,
                               "begin": [50, 30], "end": [170, 120], "gap_of_seed": [0, 1, -1]}
    assert pl["chains"][1]["seeds"] == [3, 6] and pl["chains"][1]["gap_items"] == [2, 4] and pl["chains"][1]["gap_of_seed"] == [2, 3, -1]
    # two work orders, each by cells with ties by index, each launch with its own R and grid
    assert pl["ends_plan"]["order"] == [1, 3, 0, 2] and pl["gaps_plan"]["order"] == [0, 2, 1, 3]
    assert pl["ends_plan"]["extend"] is True and pl["gaps_plan"]["extend"] is False
    assert pl["ends_plan"]["num_items"] == 4 == pl["ends_plan"]["grid"] and pl["gaps_plan"]["num_items"] == 4 == pl["gaps_plan"]["grid"]
    assert pl["ends_plan"]["max_text"] == 130 and pl["gaps_plan"]["max_text"] == 40
    assert pl["input_bytes"] == 1000


def test_each_launch_is_planned_on_its_own_items():
    """The ends as the extension scorer plans pairs of their shapes, the gaps as the global affine scorer does:
    R, cost, grid, boundary rows."""
    chained = score_plan("--mode", "global", *GAP, "--extend", 20, "--chain", "50:30:10,100:80:10,150:100:20", "300x200x2")
    ends = score_plan("--mode", "global", *GAP, "--extend", 20, "50x30", "130x80", "50x30", "130x80")
    gaps = score_plan("--mode", "global", *GAP, "40x40", "40x10", "40x40", "40x10")
    for name, alone in (("ends_plan", ends), ("gaps_plan", gaps)):
        for k in ("R", "cost", "grid", "row_stride", "order", "affine", "gap", "gap_extend"):
            assert chained[name][k] == alone[k], (name, k)
    # (C5): open == extend plans the linear instances for both launches
    lin = score_plan("--mode", "global", "--gap", 5, "--gap-extend", 5, "--chain", "50:30:10,100:80:10", "300x200")
    assert lin["ends_plan"]["affine"] is False and lin["gaps_plan"]["affine"] is False and lin["gaps_plan"]["gap"] == 5
    for forced in (1, 2, 4, 8):
        pl = score_plan("--mode", "global", *GAP, "--chain", "50:30:10,100:80:10", "--rows-per-lane", forced, "300x200")
        assert pl["ends_plan"]["R"] == forced == pl["gaps_plan"]["R"]
    # many small gaps and two larger ends: the launches choose their own rows per lane
    chain = ",".join(f"{2000 + 40 * k}:{2000 + 40 * k}:15" for k in range(50))
    pl = score_plan("--mode", "global", *GAP, "--chain", chain, "6000x6000")
    assert pl["gaps_plan"]["R"] == 1 and pl["ends_plan"]["R"] == 8 and pl["gaps_plan"]["num_items"] == 49


def test_adjacent_seeds_have_no_gap_item():
    pl = score_plan("--mode", "global", *GAP, "--chain", "50:30:10,60:40:10,70:50:0,70:50:5", "300x200")
    assert pl["gaps"] == [] and pl["gaps_plan"]["num_items"] == 0 and pl["gaps_plan"]["grid"] == 0
    assert pl["chains"][0]["gap_of_seed"] == [-1, -1, -1, -1] and pl["chains"][0]["closed_score"] == 0 and pl["chains"][0]["closed_cols"] == 0
    assert items_of(pl["ends"]) == [(0, -1, 49, 29, 50, 30), (0, 1, 75, 55, 225, 145)]


def test_an_empty_side_gap_is_closed_form():
    # seed 0 ends at (60, 40); seed 1 at (67, 40): 7 text letters against nothing; seed 2: 3 pattern letters
    pl = score_plan("--mode", "global", *GAP, "--chain", "50:30:10,67:40:5,72:48:5,80:60:1", "300x200")
    assert items_of(pl["gaps"]) == [(0, 1, 77, 53, 3, 7)]
    assert pl["chains"][0]["gap_of_seed"] == [-1, -1, 0, -1]
    assert pl["chains"][0]["closed_score"] == -(11 + 6 * 2) - (11 + 2 * 2) and pl["chains"][0]["closed_cols"] == 10
    pl = score_plan("--mode", "global", "--gap", 3, "--gap-extend", 3, "--chain", "0:0:1,1:5:1", "10x10")
    assert pl["chains"][0]["closed_score"] == -12 and pl["chains"][0]["closed_cols"] == 4


def test_a_chain_of_one_has_the_items_of_the_seed():
    for seed in ("100:50:10", "0:0:0", "300:200:0", "0:50:10", "290:100:10", "0:0:200", "150:100:0"):
        one = score_plan("--mode", "global", *GAP, "--extend", 20, "--chain", seed, "300x200x2")
        seeded = score_plan("--mode", "global", *GAP, "--extend", 20, "--seeds", seed, "300x200x2")
        assert one["ends"] == seeded["items"] and one["gaps"] == [], seed
        assert [[c["left"], c["right"]] for c in one["chains"]] == seeded["halves"], seed
        for k in ("R", "cost", "grid", "row_stride", "order", "affine"):
            assert one["ends_plan"][k] == seeded[k], (seed, k)


def test_seeds_at_both_corners():
    pl = score_plan("--mode", "global", *GAP, "--chain", "0:0:10,100:80:10,290:190:10", "300x200")
    assert pl["ends"] == [] and pl["ends_plan"]["grid"] == 0 and pl["chains"][0]["left"] == -1 == pl["chains"][0]["right"]
    assert items_of(pl["gaps"]) == [(0, 1, 10, 10, 90, 70), (0, 1, 110, 90, 180, 100)]
    assert pl["chains"][0]["begin"] == [0, 0] and pl["chains"][0]["end"] == [300, 200]
    # only one end empty
    pl = score_plan("--mode", "global", *GAP, "--chain", "0:0:10,100:80:10", "300x200")
    assert items_of(pl["ends"]) == [(0, 1, 110, 90, 190, 110)] and [pl["chains"][0]["left"], pl["chains"][0]["right"]] == [-1, 0]
    pl = score_plan("--mode", "global", *GAP, "--chain", "5:0:10,100:80:120", "300x200")  # ps = 0; the last seed reaches the pattern's end
    assert pl["ends"] == [] and items_of(pl["gaps"]) == [(0, 1, 15, 10, 85, 70)]


def test_one_chain_per_shape():
    pl = score_plan("--mode", "global", *GAP, "--chain", "10:10:5", "--chain", "100:100:20,500:400:20", "100x100x2", "1000x900")
    assert [c["seeds"] for c in pl["chains"]] == [[0, 1], [1, 2], [2, 4]]
    assert items_of(pl["gaps"]) == [(2, 1, 200 + 120, 200 + 120, 380, 280)]
    assert [c["gap_items"] for c in pl["chains"]] == [[0, 0], [0, 0], [0, 1]]


def test_refusals():
    for plan in (score_plan, trace_plan):
        base = ("--mode", "global", *GAP)
        # null arguments with pairs
        pl = plan(*base, "--chain", "null", "100x100")
        assert pl["error"] == SA_ERR_INVALID and "seeds is null" in pl["message"]
        pl = plan(*base, "--chain", "10:10:5", "--chain-off", "null", "100x100")
        assert pl["error"] == SA_ERR_INVALID and "chain_off is null" in pl["message"]
        # chain_off
        pl = plan(*base, "--chain", "10:10:5", "--chain-off", "1,2,3", "100x100x2")
        assert pl["error"] == SA_ERR_INVALID and "chain_off[0]" in pl["message"] and "pair 0" in pl["message"]
        pl = plan(*base, "--chain", "10:10:5", "--chain", "20:20:5", "--chain-off", "0,2,1", "100x100", "100x100")  # pair 0 takes both seeds
        assert pl["error"] == SA_ERR_INVALID and "pair 1" in pl["message"] and "decreases" in pl["message"]
        # a pair without a seed
        pl = plan(*base, "--chain", "10:10:5", "--chain", "", "100x100", "50x50")
        assert pl["error"] == SA_ERR_INVALID and "pair 1" in pl["message"] and "no seed" in pl["message"]
        # a seed out of range: the pair and the seed's index in its chain
        for bad in ("291:0:10", "0:191:10", "301:0:0", "0:0:201", "18446744073709551615:0:2"):
            pl = plan(*base, "--chain", "0:0:0", "--chain", "0:0:0", "--chain", "0:0:1,5:5:5," + bad, "50x50", "50x50", "300x200")
            assert pl["error"] == SA_ERR_INVALID and "pair 2, seed 2" in pl["message"] and "does not lie inside" in pl["message"], bad
        # out of order on either side, or overlapping
        for bad in ("50:30:10,40:60:5", "50:30:10,70:20:5", "50:30:10,59:60:5", "50:30:10,70:39:5", "50:30:10,60:40:5,64:50:5"):
            pl = plan(*base, "--chain", "0:0:0", "--chain", bad, "50x50", "300x200")
            which = bad.count(",")
            assert pl["error"] == SA_ERR_INVALID and f"pair 1, seed {which}" in pl["message"] and "begins before the end" in pl["message"], bad
        assert "error" not in plan(*base, "--chain", "50:30:10,60:40:5,65:45:0,65:45:135", "300x200")
        # the mode and the xdrop, as the seeds functions have them
        for mode in ("local", "fit", 16, 31, 3):
            pl = plan("--mode", mode, *GAP, "--extend", 20, "--chain", "0:0:0", "100x100")
            assert pl["error"] == SA_ERR_INVALID and "SA_GLOBAL" in pl["message"], mode
        for x in (-2, 1 << 30):
            pl = plan(*base, "--extend", x, "--chain", "0:0:0", "100x100")
            assert pl["error"] == SA_ERR_INVALID and "xdrop" in pl["message"], x
        # no band of any kind
        for band in (["--band", 5], ["--band-at", "-5:5"], ["--width", 5]):
            pl = plan(*base, "--extend", 20, "--chain", "10:10:5", *band, "100x100")
            assert pl["error"] == SA_ERR_UNSUPPORTED and "band" in pl["message"], band
    # the linear scorer has no chains: the penalties are part of the call
    assert score_plan("--mode", "global", "--gap", 5, "--chain", "0:0:0", "100x100")["error"] == SA_ERR_INVALID


def test_the_limits_are_the_whole_pairs():
    whole = score_plan("--mode", "global", "--gap", 100000, "--gap-extend", 2, "--extend", 20, "5300x5300")
    assert whole["error"] == SA_ERR_UNSUPPORTED and whole["message"] == "scores may exceed the int32 range"
    pl = score_plan("--mode", "global", "--gap", 100000, "--gap-extend", 2, "--chain", "1000:1000:10,2650:2650:0,4000:4000:10", "5300x5300")
    assert pl["error"] == SA_ERR_UNSUPPORTED and pl["message"] == whole["message"]


def test_existing_arguments_print_what_they_printed():
    """--chain adds a branch: a call without it goes the way it went (the keys of the seeds and the plain plans)."""
    pl = score_plan("--mode", "global", *GAP, "--extend", 20, "--seeds", "100:50:10", "300x200")
    assert "chains_call" not in pl and pl["seeds"] is True
    pl = trace_plan("--mode", "global", *GAP, "--extend", 20, "--seeds", "100:50:10", "300x200")
    assert "chains_call" not in pl and pl["seeds"] is True


# ---- the trace plan -------------------------------------------------------------------------------------
def test_the_trace_plan_counts_the_pieces():
    pl = trace_plan("--mode", "global", *GAP, "--extend", 20, "--chain", "50:30:10,100:80:10,150:100:20", "300x200x2", "1000x1000")
    assert "error" not in pl and pl["chains_call"] is True and pl["R"] == 8 == pl["gap_R"] and pl["xdrop"] == 20
    assert pl["affine"] is True and pl["gap_affine"] is True and pl["num_pairs"] == 3
    want_ends = [dir_bytes(50, 30), dir_bytes(130, 80)] * 2 + [dir_bytes(50, 30), dir_bytes(830, 880)]
    want_gaps = [dir_bytes(40, 40), dir_bytes(40, 10)] * 3
    assert [it["dir_bytes"] for it in pl["ends"]] == want_ends and [it["dir_bytes"] for it in pl["gaps"]] == want_gaps
    assert pl["total_dir_bytes"] == pl["arena_bytes"] == sum(want_ends) + sum(want_gaps)
    assert pl["string_bytes"] == 500 + 500 + 2000 and pl["slots"] == [0, 500, 1000]
    assert pl["num_chunks"] == 1 and pl["chunk_begin"] == [0, 6] and pl["gap_chunk_begin"] == [0, 6] and pl["pair_chunk_begin"] == [0, 3]
    assert pl["pair_order"] == [2, 0, 1]  # by the cells of all pieces
    assert pl["order"] == [5, 1, 3, 4, 0, 2] and pl["gap_order"] == [4, 0, 2, 5, 1, 3]  # each launch by cells, ties in the pair order
    # the offsets follow the pair order; in a pair the ends, then the gaps
    spans = sorted([(it["dir_off"], it["dir_bytes"]) for it in pl["ends"] + pl["gaps"]])
    assert spans[0][0] == 0 and all(a + b == c for (a, b), (c, _) in zip(spans, spans[1:]))
    by_pair = [min(it["dir_off"] for it in pl["ends"] + pl["gaps"] if it["pair"] == p) for p in range(3)]
    assert by_pair[2] < by_pair[0] < by_pair[1]
    # open == extend: the traced instances are affine whatever the penalties
    pl = trace_plan("--mode", "global", "--gap", 5, "--gap-extend", 5, "--chain", "50:30:10,100:80:10", "300x200")
    assert pl["affine"] is True and pl["gap_affine"] is True
    # nothing but seeds and closed-form gaps: no item, no bytes
    pl = trace_plan("--mode", "global", *GAP, "--chain", "0:0:100,100:150:50", "150x200")
    assert pl["ends"] == [] and pl["gaps"] == [] and pl["arena_bytes"] == 0 and pl["num_chunks"] == 1
    assert pl["chains"][0]["closed_cols"] == 50


def chain_of(count, step, first, length=15):
    return ",".join(f"{first + step * k}:{first + step * k}:{length}" for k in range(count))


def test_a_long_pair_plans_under_a_budget_that_refuses_its_rectangle():
    budget = 8 << 20
    assert dir_bytes(6000, 6000) > budget
    pl = trace_plan("--mode", "global", *GAP, "--extend", "none", "--budget", budget, "6000x6000")
    assert pl["error"] == SA_ERR_UNSUPPORTED and "direction bytes" in pl["message"]
    # one seed is no help: its two halves are still most of the rectangle
    pl = trace_plan("--mode", "global", *GAP, "--seeds", "100:100:15", "--budget", budget, "6000x6000")
    assert pl["error"] == SA_ERR_UNSUPPORTED
    pl = trace_plan("--mode", "global", *GAP, "--chain", chain_of(60, 98, 100), "--budget", budget, "6000x6000")
    assert "error" not in pl and pl["num_chunks"] == 1 and pl["chunk_begin"] == [0, 2] and pl["gap_chunk_begin"] == [0, 59]
    want = dir_bytes(100, 100) + 59 * dir_bytes(83, 83) + dir_bytes(6000 - 100 - 59 * 98 - 15, 6000 - 100 - 59 * 98 - 15)
    assert pl["arena_bytes"] == pl["total_dir_bytes"] == want <= budget
    # the pieces together exceed the budget: refused, the message names the pair
    pl = trace_plan("--mode", "global", *GAP, "--chain", "5:5:0", "--chain", chain_of(60, 98, 100), "--budget", want - 1, "10x10", "6000x6000")
    assert pl["error"] == SA_ERR_UNSUPPORTED and "pair 1" in pl["message"] and "pieces" in pl["message"]


def test_the_pieces_of_a_pair_share_a_chunk():
    chain = chain_of(4, 100, 100)
    one = trace_plan("--mode", "global", *GAP, "--chain", chain, "600x600")
    per_pair = one["total_dir_bytes"]
    pl = trace_plan("--mode", "global", *GAP, "--chain", chain, "--budget", 2 * per_pair + per_pair // 2, "600x600x5")
    assert "error" not in pl and pl["num_chunks"] == 3 and pl["pair_chunk_begin"] == [0, 2, 4, 5]
    assert pl["chunk_begin"] == [0, 4, 8, 10] and pl["gap_chunk_begin"] == [0, 6, 12, 15] and pl["arena_bytes"] == 2 * per_pair
    for c in range(3):
        pairs = sorted(pl["pair_order"][pl["pair_chunk_begin"][c]:pl["pair_chunk_begin"][c + 1]])
        ends = [pl["ends"][k] for k in pl["order"][pl["chunk_begin"][c]:pl["chunk_begin"][c + 1]]]
        gaps = [pl["gaps"][k] for k in pl["gap_order"][pl["gap_chunk_begin"][c]:pl["gap_chunk_begin"][c + 1]]]
        assert sorted(it["pair"] for it in ends) == sorted(pairs * 2) and sorted(it["pair"] for it in gaps) == sorted(pairs * 3), c
        for items in (ends, gaps):
            cells = [it["n"] * it["m"] for it in items]
            assert cells == sorted(cells, reverse=True), c
        spans = sorted((it["dir_off"], it["dir_bytes"]) for it in ends + gaps)
        assert spans[0][0] == 0 and all(a + b == c2 for (a, b), (c2, _) in zip(spans, spans[1:])), c
        assert spans[-1][0] + spans[-1][1] <= pl["budget"]
