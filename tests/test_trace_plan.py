"""The planner of the affine alignment path (csrc/sa_trace_plan.cpp) on the CPU, through
bin/sa_trace_plan_check: direction bytes and string slots per pair, the chunks of the work order, the
budget, and the limits, which are make_score_plan's for the affine gap model. Each case runs the
program once (milliseconds)."""
from __future__ import annotations

import json
import os
import subprocess

import pytest

from conftest import PKG
from test_score_affine_plan import plan as score_plan

CHECK = os.path.join(PKG, "bin", "sa_trace_plan_check")
SA_ERR_INVALID, SA_ERR_UNSUPPORTED = 1, 4


def plan(*args, env_budget=None, env_waves=None) -> dict:
    if not os.path.exists(CHECK):
        subprocess.run(["make", "-s", "-C", PKG, "bin/sa_trace_plan_check"], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SA_")}
    if env_budget is not None:
        env["SA_TRACE_ARENA_BYTES"] = str(env_budget)
    if env_waves is not None:
        env["SA_SCORE_WAVES"] = str(env_waves)
    out = subprocess.run([CHECK] + [str(a) for a in args], env=env, check=True, capture_output=True, text=True).stdout
    return json.loads(out)


# By hand: a strip is 64 lanes x 8 rows = 512 rows; a pair runs steps 0 .. n + 62 in whole 64-step
# bodies, (n + 126) // 64 of them (n = 1: one body, n = 2 .. 65: two, n = 66: three, n = 300: 363 steps
# in six); a step of a strip is 64 dwords.
STRIPS = {1: 1, 512: 1, 513: 2}
STEPS = {1: 64, 2: 128, 3: 128, 64: 128, 65: 128, 66: 192, 300: 384}


def test_direction_bytes_and_slots_of_hand_derived_shapes():
    shapes = [(n, m) for m in STRIPS for n in STEPS]
    pl = plan("--mode", "global", *[f"{n}x{m}" for n, m in shapes])
    assert pl["num_pairs"] == len(shapes) == 21 and pl["R"] == 8
    slot = 0
    for (n, m), pr in zip(shapes, pl["pairs"]):
        assert (pr["strips"], pr["steps"]) == (STRIPS[m], STEPS[n]), (n, m)
        assert pr["dir_bytes"] == STRIPS[m] * STEPS[n] * 256, (n, m)
        assert pr["slot_off"] == slot, (n, m)
        slot += n + m
    assert pl["string_bytes"] == slot
    assert pl["total_dir_bytes"] == sum(pr["dir_bytes"] for pr in pl["pairs"]) == pl["arena_bytes"]
    assert pl["budget"] == 2 << 30 and pl["num_chunks"] == 1 and pl["chunk_begin"] == [0, 21]
    # the pairs of the one chunk lie one after another in the work order
    off = 0
    for k in pl["order"]:
        assert pl["pairs"][k]["dir_off"] == off
        off += pl["pairs"][k]["dir_bytes"]


def test_chunks_split_five_pairs_two_two_one():
    # 300x513: 2 strips x 384 steps x 256 B = 196608 B each; two fit 400000 B, three do not
    pl = plan("--mode", "local", "--budget", 400000, "300x513x5")
    assert pl["num_chunks"] == 3 and pl["chunk_begin"] == [0, 2, 4, 5]
    assert pl["arena_bytes"] == 2 * 196608 and pl["total_dir_bytes"] == 5 * 196608
    assert [pr["dir_off"] for pr in pl["pairs"]] == [0, 196608, 0, 196608, 0]
    assert [pr["slot_off"] for pr in pl["pairs"]] == [813 * k for k in range(5)]
    # chunks follow the work order (most cells first), not the pair order
    pl = plan("--mode", "local", "--budget", 400000, "1x1", "300x513x2", "64x512", "300x513")
    assert pl["order"] == [1, 2, 4, 3, 0] and pl["chunk_begin"] == [0, 2, 5]
    assert [pr["dir_off"] for pr in pl["pairs"]] == [196608 + 32768, 0, 196608, 196608, 0]
    assert pl["arena_bytes"] == 2 * 196608


def test_budget_from_the_environment():
    assert plan("--mode", "local", "300x513x5", env_budget=400000)["chunk_begin"] == [0, 2, 4, 5]
    assert plan("--mode", "local", "300x513x5")["chunk_begin"] == [0, 5]


def test_a_pair_above_the_budget_is_refused():
    pl = plan("--mode", "global", "--budget", 196607, "1x1", "300x513")
    assert pl["error"] == SA_ERR_UNSUPPORTED
    assert pl["message"] == "pair 1 needs 196608 direction bytes, the arena budget is 196607 (SA_TRACE_ARENA_BYTES)"
    assert "error" not in plan("--mode", "global", "--budget", 196608, "1x1", "300x513")


LIMITS = [
    ["--mode", "global", "--gap", 1, "--gap-extend", 100, "4000000x4000000"],
    ["--mode", "global", "--gap", 100, "--gap-extend", 1, "4000000x4000000"],
    ["--mode", "global", "--gap", 1, "--gap-extend", -100, "4000000x4000000"],
    ["--mode", "global", "--gap", 11, "--gap-extend", 2, "16777215x100"],
    ["--mode", "local", "--gap", 11, "--gap-extend", 2, "16000000x16000000"],
    ["--mode", "local", "--gap", 11, "--gap-extend", -3, "1000000x1000000"],
    ["--mode", 7, "--gap", 11, "--gap-extend", 2, "10x10"],
    ["--mode", "global", "--alphabet", 33, "--gap", 11, "--gap-extend", 2, "10x10"],
]


@pytest.mark.parametrize("args", LIMITS)
def test_limits_are_the_affine_scorers(args):
    """Refused exactly where make_score_plan refuses, with its code and message (a huge budget, so
    that the arena is not what refuses)."""
    want = score_plan(*args)
    got = plan("--budget", 1 << 62, *args)
    assert "error" in want and (got["error"], got["message"]) == (want["error"], want["message"])


def test_accepted_where_the_scorer_accepts():
    args = ["--mode", "global", "--gap", 1, "--gap-extend", 1, "40000x40000"]
    assert "error" not in score_plan(*args)
    pl = plan("--budget", 1 << 62, *args)
    assert pl["pairs"][0]["dir_bytes"] == 79 * 40064 * 256 and pl["gap"] == 1 and pl["gap_extend"] == 1


def test_zero_pairs_and_empty_sides():
    pl = plan("--mode", "global")
    assert (pl["num_pairs"], pl["num_chunks"], pl["chunk_begin"], pl["arena_bytes"], pl["string_bytes"]) == (0, 0, [0], 0, 0)
    # an empty side has no cells: no directions, and a slot for the run of gaps
    pl = plan("--mode", "global", "0x0", "5x0", "0x5", "1x1")
    assert [pr["dir_bytes"] for pr in pl["pairs"]] == [0, 0, 0, 64 * 256]
    assert [pr["slot_off"] for pr in pl["pairs"]] == [0, 0, 5, 10] and pl["string_bytes"] == 12
    assert pl["num_chunks"] == 1 and pl["arena_bytes"] == 64 * 256


def test_grid_is_sized_for_two_waves_per_simd():
    """The traced instances take up to 226 VGPRs: two resident waves per SIMD."""
    assert plan("--mode", "local", "--cus", 16, "100x50x20000")["grid"] == 16 * 4 * 2
    assert plan("--mode", "local", "--cus", 16, "100x50x7")["grid"] == 7


def test_the_scorers_waves_knob_lowers_the_grid_but_does_not_raise_it():
    """SA_SCORE_WAVES is tuned for the untraced kernels (up to 8 waves per SIMD); no more than two
    traced waves fit."""
    assert plan("--mode", "local", "--cus", 16, "100x50x20000", env_waves=8)["grid"] == 16 * 4 * 2
    assert plan("--mode", "local", "--cus", 16, "100x50x20000", env_waves=1)["grid"] == 16 * 4 * 1
