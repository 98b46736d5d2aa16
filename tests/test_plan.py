"""The host planner (csrc/sa_plan.cpp) on the CPU: bin/sa_plan_check plans a list of pair shapes for
a CU count under a knob set and prints the plan as JSON; each case runs it once (milliseconds).

HAND holds expectations derived by hand from the planning rules; RECORDED holds the whole output of
the planner as it was when it moved out of the engine unchanged (the parent's plan_create and
sa_plan_fill arithmetic, verbatim, behind the same program), so any later reshaping of the planner
is checked against the behaviour it started from. The structural tests read the descriptors
themselves (--strips). One GPU test compares plans the engine creates with the program's, for the
device's CU count."""
from __future__ import annotations

import json
import os
import subprocess

import pytest

from conftest import PKG, ROOT

CHECK = os.path.join(PKG, "bin", "sa_plan_check")
MATRICES = os.path.join(ROOT, "tests", "golden", "matrices.json")
kArr, kArr8, kPair, kArr8A = 2, 3, 4, 5  # sa_layout.h ScoreKind
kHasPrev, kHasNext = 1, 2

DNA = ["--mode", "global", "--alphabet", "4", "--gap", "5", "--matrix", "blast"]
DNA_LOCAL = ["--mode", "local", "--alphabet", "4", "--gap", "5", "--matrix", "blast"]
PROTEIN = ["--mode", "global", "--alphabet", "23", "--gap", "5", "--matrix", "blosum50"]

# name: (arguments, knobs); 256 CUs unless the arguments say otherwise
CASES = {
    # ---- hand-derived (HAND) ----
    "headline": (DNA + ["32768x32768"], {}),
    "dna8k": (DNA + ["8192x8192"], {}),
    "protein4k": (PROTEIN + ["4096x4096"], {}),
    "persistent_band3": (DNA + ["2048x4096"], {"SA_MAX_CUS": "16", "SA_BAND_R": "3"}),
    "four_pairs_two_row": (DNA + ["2100x256", "2100x512", "2100x768", "2100x1024"], {}),
    "four_pairs_three_row": (DNA + ["2100x384", "2100x768", "2100x1152", "2100x1536"], {}),
    "local_negative_gap": (["--mode", "local", "--alphabet", "4", "--gap", "-3", "--matrix", "blast", "4500x450"], {}),
    "headline_no_band": (DNA + ["32768x32768"], {"SA_BAND": "0"}),
    "headline_two_row": (DNA + ["32768x32768"], {"SA_BAND_R": "2"}),
    # ---- recorded: batch planning ----
    "batch": (DNA + ["2048x2048x4096"], {}),
    "batch_shard512": (DNA + ["2048x2048x512"], {}),
    "batch_shard1024": (DNA + ["2048x2048x1024"], {}),
    "batch_2048": (DNA + ["2048x2048x2048"], {}),
    # KNOWN GAP (second finding): choose_R lowers R to the pair-chain height 8, the LDS
    # condition then refuses the pair chains (7 rows of 8192 columns, 236 KiB) and the plan runs
    # generic one-wave chains at R = 8 instead of one R = 32 strip per pair. The fix changes this row.
    "advice_gap": (DNA + ["8192x4096x512"], {}),
    "batch_odd": (DNA + ["2048x2048x511"], {}),
    "batch_other_shape": (DNA + ["2048x2048x511", "2048x1024"], {}),
    "batch_no_pair16": (DNA + ["2048x2048x512"], {"SA_NO_PAIR16": "1"}),
    "local_headline": (DNA_LOCAL + ["32768x32768"], {}),
    "empty_text": (DNA + ["0x100"], {}),
    "empty_pattern": (DNA + ["100x0"], {}),
    "no_pairs": (DNA, {}),
    # ---- recorded: limits (code and message) ----
    "limit_length": (DNA + ["16777215x100"], {}),
    "limit_score_range": (["--mode", "global", "--alphabet", "4", "--gap", "100", "--matrix", "blast", "4000000x4000000"], {}),
    "limit_local_key": (DNA_LOCAL + ["16000000x16000000"], {}),
    "limit_alphabet_0": (["--mode", "global", "--alphabet", "0", "--gap", "5", "--matrix", "unit", "100x100"], {}),
    "limit_alphabet_33": (["--mode", "global", "--alphabet", "33", "--gap", "5", "--matrix", "unit", "100x100"], {}),
    "limit_mode": (["--mode", "7", "--alphabet", "4", "--gap", "5", "--matrix", "blast", "100x100"], {}),
    # ---- structural (--strips): two pairs, m <= 1100 ----
    "small_strips": (DNA + ["700x1100", "700x960"], {"SA_BAND": "0"}),
    "small_two_row": (DNA + ["700x1100", "700x960"], {"SA_BAND_R": "2"}),
    "small_three_row": (DNA + ["700x1100", "700x960"], {}),
}

HAND = {
    "headline": dict(fill_kind="band3", num_strips=512, num_bands=170, R=1,
                     launch=dict(num_band_groups=43, num_groups=171, grid=214, band3=1, sk=kArr8)),
    "dna8k": dict(fill_kind="band3", num_strips=128, num_bands=42, launch=dict(num_band_groups=11, num_groups=43)),
    "protein4k": dict(fill_kind="band", num_strips=64, num_bands=31, sk=kArr8,
                      launch=dict(num_band_groups=8, num_groups=16, sk=kArr8A, band3=0)),
    "persistent_band3": dict(fill_kind="band3", num_bands=21, num_cu=16,
                             launch=dict(num_band_groups=6, num_groups=22, band_wgs=5, grid=16)),
    "four_pairs_two_row": dict(fill_kind="band", band_r=2),
    "four_pairs_three_row": dict(fill_kind="band3", band_r=3),
    "local_negative_gap": dict(fill_kind="strips", sk=kArr),
    "headline_no_band": dict(fill_kind="strips", chain_solo=1, num_bands=0),
    "headline_two_row": dict(fill_kind="band", band_r=2),
}

RECORDED = {
    "headline": {"mode": 0, "A": 4, "gap": 5, "R": 1, "U": 16, "W": 4, "key_bits": 12, "key_rowbits": 16, "sk": 3,
        "chain": 1, "chain_solo": 0, "band": 1, "band_r": 3, "strip_w": 3, "num_cu": 256, "fill_kind": "band3",
        "num_pairs": 1, "num_strips": 512, "num_bands": 170, "tb_groups": 32, "tb_slots": 512, "max_recs": 32768,
        "code_bytes": 132352, "mask_entries": 16809984, "granules": 5571920, "out_bytes": 65552, "rec_words":
        32832, "hash": "7ad9f98a695a669f", "launch": {"W": 4, "sk": 3, "band3": 1, "num_groups": 171, "num_bands":
        170, "num_band_groups": 43, "band_wgs": 43, "strip_w": 3, "grid": 214, "chain_lds": 98304,
        "pair_text_len": 0}},
    "dna8k": {"mode": 0, "A": 4, "gap": 5, "R": 1, "U": 16, "W": 4, "key_bits": 12, "key_rowbits": 14, "sk": 3,
        "chain": 1, "chain_solo": 0, "band": 1, "band_r": 3, "strip_w": 3, "num_cu": 256, "fill_kind": "band3",
        "num_pairs": 1, "num_strips": 128, "num_bands": 42, "tb_groups": 8, "tb_slots": 128, "max_recs": 8192,
        "code_bytes": 34048, "mask_entries": 1056768, "granules": 344400, "out_bytes": 16400, "rec_words": 8256,
        "hash": "e3619e46efb856d8", "launch": {"W": 4, "sk": 3, "band3": 1, "num_groups": 43, "num_bands": 42,
        "num_band_groups": 11, "band_wgs": 11, "strip_w": 3, "grid": 54, "chain_lds": 98304, "pair_text_len": 0}},
    "protein4k": {"mode": 0, "A": 23, "gap": 5, "R": 1, "U": 16, "W": 4, "key_bits": 12, "key_rowbits": 13, "sk":
        3, "chain": 1, "chain_solo": 0, "band": 1, "band_r": 2, "strip_w": 4, "num_cu": 256, "fill_kind": "band",
        "num_pairs": 1, "num_strips": 64, "num_bands": 31, "tb_groups": 4, "tb_slots": 64, "max_recs": 4096,
        "code_bytes": 101568, "mask_entries": 266240, "granules": 127224, "out_bytes": 8208, "rec_words": 4160,
        "hash": "d8cbf6e8e3dfe5b5", "launch": {"W": 4, "sk": 5, "band3": 0, "num_groups": 16, "num_bands": 31,
        "num_band_groups": 8, "band_wgs": 8, "strip_w": 4, "grid": 24, "chain_lds": 98304, "pair_text_len": 0}},
    "persistent_band3": {"mode": 0, "A": 4, "gap": 5, "R": 1, "U": 16, "W": 4, "key_bits": 12, "key_rowbits": 13,
        "sk": 3, "chain": 1, "chain_solo": 0, "band": 1, "band_r": 3, "strip_w": 3, "num_cu": 16, "fill_kind":
        "band3", "num_pairs": 1, "num_strips": 64, "num_bands": 21, "tb_groups": 4, "tb_slots": 64, "max_recs":
        4096, "code_bytes": 9472, "mask_entries": 135168, "granules": 43176, "out_bytes": 6160, "rec_words": 4160,
        "hash": "e859f33aa0b10457", "launch": {"W": 4, "sk": 3, "band3": 1, "num_groups": 22, "num_bands": 21,
        "num_band_groups": 6, "band_wgs": 5, "strip_w": 3, "grid": 16, "chain_lds": 98304, "pair_text_len": 0}},
    "four_pairs_two_row": {"mode": 0, "A": 4, "gap": 5, "R": 1, "U": 16, "W": 4, "key_bits": 12, "key_rowbits":
        12, "sk": 3, "chain": 1, "chain_solo": 0, "band": 1, "band_r": 2, "strip_w": 4, "num_cu": 256,
        "fill_kind": "band", "num_pairs": 4, "num_strips": 40, "num_bands": 16, "tb_groups": 3, "tb_slots": 36,
        "max_recs": 1024, "code_bytes": 38720, "mask_entries": 87040, "granules": 33728, "out_bytes": 11024,
        "rec_words": 8656, "hash": "16c4eff8a35448a1", "launch": {"W": 4, "sk": 3, "band3": 0, "num_groups": 10,
        "num_bands": 16, "num_band_groups": 4, "band_wgs": 4, "strip_w": 4, "grid": 14, "chain_lds": 98304,
        "pair_text_len": 0}},
    "four_pairs_three_row": {"mode": 0, "A": 4, "gap": 5, "R": 1, "U": 16, "W": 4, "key_bits": 12, "key_rowbits":
        12, "sk": 3, "chain": 1, "chain_solo": 0, "band": 1, "band_r": 3, "strip_w": 3, "num_cu": 256,
        "fill_kind": "band3", "num_pairs": 4, "num_strips": 60, "num_bands": 16, "tb_groups": 5, "tb_slots": 54,
        "max_recs": 1536, "code_bytes": 38720, "mask_entries": 130560, "granules": 33728, "out_bytes": 12304,
        "rec_words": 8656, "hash": "f608ef0cb6229c90", "launch": {"W": 4, "sk": 3, "band3": 1, "num_groups": 20,
        "num_bands": 16, "num_band_groups": 4, "band_wgs": 4, "strip_w": 3, "grid": 24, "chain_lds": 98304,
        "pair_text_len": 0}},
    "local_negative_gap": {"mode": 1, "A": 4, "gap": -3, "R": 1, "U": 16, "W": 4, "key_bits": 12, "key_rowbits":
        13, "sk": 2, "chain": 1, "chain_solo": 1, "band": 0, "band_r": 2, "strip_w": 1, "num_cu": 256,
        "fill_kind": "strips", "num_pairs": 1, "num_strips": 8, "num_bands": 0, "tb_groups": 1, "tb_slots": 8,
        "max_recs": 450, "code_bytes": 19280, "mask_entries": 36608, "granules": 31556, "out_bytes": 4966,
        "rec_words": 4564, "hash": "4e89d290d58fb1d2", "launch": {"W": 4, "sk": 2, "band3": 0, "num_groups": 2,
        "num_bands": 0, "num_band_groups": 0, "band_wgs": 0, "strip_w": 0, "grid": 2, "chain_lds": 98304,
        "pair_text_len": 0}},
    "headline_no_band": {"mode": 0, "A": 4, "gap": 5, "R": 1, "U": 16, "W": 4, "key_bits": 12, "key_rowbits": 16,
        "sk": 3, "chain": 1, "chain_solo": 1, "band": 0, "band_r": 2, "strip_w": 1, "num_cu": 256, "fill_kind":
        "strips", "num_pairs": 1, "num_strips": 512, "num_bands": 0, "tb_groups": 32, "tb_slots": 512, "max_recs":
        32768, "code_bytes": 132352, "mask_entries": 16809984, "granules": 16748536, "out_bytes": 65552,
        "rec_words": 32832, "hash": "9551f95c6fc89021", "launch": {"W": 4, "sk": 3, "band3": 0, "num_groups": 128,
        "num_bands": 0, "num_band_groups": 0, "band_wgs": 0, "strip_w": 0, "grid": 128, "chain_lds": 98304,
        "pair_text_len": 0}},
    "headline_two_row": {"mode": 0, "A": 4, "gap": 5, "R": 1, "U": 16, "W": 4, "key_bits": 12, "key_rowbits": 16,
        "sk": 3, "chain": 1, "chain_solo": 0, "band": 1, "band_r": 2, "strip_w": 4, "num_cu": 256, "fill_kind":
        "band", "num_pairs": 1, "num_strips": 512, "num_bands": 255, "tb_groups": 32, "tb_slots": 512, "max_recs":
        32768, "code_bytes": 132352, "mask_entries": 16809984, "granules": 8357880, "out_bytes": 65552,
        "rec_words": 32832, "hash": "a46e8368eaf642ff", "launch": {"W": 4, "sk": 3, "band3": 0, "num_groups": 128,
        "num_bands": 255, "num_band_groups": 64, "band_wgs": 64, "strip_w": 4, "grid": 192, "chain_lds": 98304,
        "pair_text_len": 0}},
    "batch": {"mode": 0, "A": 4, "gap": 5, "R": 32, "U": 4, "W": 4, "key_bits": 12, "key_rowbits": 12, "sk": 4,
        "chain": 0, "chain_solo": 0, "band": 0, "band_r": 2, "strip_w": 1, "num_cu": 256, "fill_kind": "pair",
        "num_pairs": 4096, "num_strips": 4096, "num_bands": 0, "tb_groups": 0, "tb_slots": 0, "max_recs": 2048,
        "code_bytes": 19398656, "mask_entries": 276824064, "granules": 0, "out_bytes": 16842752, "rec_words":
        8650752, "hash": "d3394ae18faf7a05", "launch": {"W": 4, "sk": 4, "band3": 0, "num_groups": 512,
        "num_bands": 0, "num_band_groups": 0, "band_wgs": 0, "strip_w": 0, "grid": 512, "chain_lds": 0,
        "pair_text_len": 0}},
    "batch_shard512": {"mode": 0, "A": 4, "gap": 5, "R": 8, "U": 4, "W": 4, "key_bits": 12, "key_rowbits": 12,
        "sk": 4, "chain": 1, "chain_solo": 0, "band": 0, "band_r": 2, "strip_w": 1, "num_cu": 256, "fill_kind":
        "pair_chain", "num_pairs": 512, "num_strips": 2048, "num_bands": 0, "tb_groups": 0, "tb_slots": 0,
        "max_recs": 2048, "code_bytes": 2424832, "mask_entries": 34603008, "granules": 0, "out_bytes": 2105344,
        "rec_words": 1081344, "hash": "96d9ed1ef332f148", "launch": {"W": 4, "sk": 4, "band3": 0, "num_groups":
        256, "num_bands": 0, "num_band_groups": 0, "band_wgs": 0, "strip_w": 0, "grid": 256, "chain_lds": 0,
        "pair_text_len": 2048}},
    "batch_shard1024": {"mode": 0, "A": 4, "gap": 5, "R": 8, "U": 4, "W": 4, "key_bits": 12, "key_rowbits": 12,
        "sk": 4, "chain": 1, "chain_solo": 0, "band": 0, "band_r": 2, "strip_w": 1, "num_cu": 256, "fill_kind":
        "pair_chain", "num_pairs": 1024, "num_strips": 4096, "num_bands": 0, "tb_groups": 0, "tb_slots": 0,
        "max_recs": 2048, "code_bytes": 4849664, "mask_entries": 69206016, "granules": 0, "out_bytes": 4210688,
        "rec_words": 2162688, "hash": "523735649f7e3e19", "launch": {"W": 4, "sk": 4, "band3": 0, "num_groups":
        512, "num_bands": 0, "num_band_groups": 0, "band_wgs": 0, "strip_w": 0, "grid": 512, "chain_lds": 0,
        "pair_text_len": 2048}},
    "batch_2048": {"mode": 0, "A": 4, "gap": 5, "R": 32, "U": 4, "W": 4, "key_bits": 12, "key_rowbits": 12, "sk":
        4, "chain": 0, "chain_solo": 0, "band": 0, "band_r": 2, "strip_w": 1, "num_cu": 256, "fill_kind": "pair",
        "num_pairs": 2048, "num_strips": 2048, "num_bands": 0, "tb_groups": 0, "tb_slots": 0, "max_recs": 2048,
        "code_bytes": 9699328, "mask_entries": 138412032, "granules": 0, "out_bytes": 8421376, "rec_words":
        4325376, "hash": "12c6f96068252fb9", "launch": {"W": 4, "sk": 4, "band3": 0, "num_groups": 256,
        "num_bands": 0, "num_band_groups": 0, "band_wgs": 0, "strip_w": 0, "grid": 256, "chain_lds": 0,
        "pair_text_len": 0}},
    "advice_gap": {"mode": 0, "A": 4, "gap": 5, "R": 8, "U": 4, "W": 4, "key_bits": 12, "key_rowbits": 14, "sk":
        0, "chain": 1, "chain_solo": 0, "band": 0, "band_r": 2, "strip_w": 1, "num_cu": 256, "fill_kind":
        "strips", "num_pairs": 512, "num_strips": 4096, "num_bands": 0, "tb_groups": 0, "tb_slots": 0, "max_recs":
        8192, "code_bytes": 8716288, "mask_entries": 270532608, "granules": 29388800, "out_bytes": 6299648,
        "rec_words": 4227072, "hash": "af8d3b65cccff9c4", "launch": {"W": 4, "sk": 0, "band3": 0, "num_groups":
        1024, "num_bands": 0, "num_band_groups": 0, "band_wgs": 0, "strip_w": 0, "grid": 512, "chain_lds": 0,
        "pair_text_len": 0}},
    "batch_odd": {"mode": 0, "A": 4, "gap": 5, "R": 32, "U": 4, "W": 4, "key_bits": 12, "key_rowbits": 12, "sk":
        0, "chain": 0, "chain_solo": 0, "band": 0, "band_r": 2, "strip_w": 1, "num_cu": 256, "fill_kind":
        "strips", "num_pairs": 511, "num_strips": 511, "num_bands": 0, "tb_groups": 0, "tb_slots": 0, "max_recs":
        2048, "code_bytes": 2420096, "mask_entries": 34535424, "granules": 0, "out_bytes": 2101232, "rec_words":
        1079232, "hash": "3a5a1dbc50c72425", "launch": {"W": 4, "sk": 0, "band3": 0, "num_groups": 128,
        "num_bands": 0, "num_band_groups": 0, "band_wgs": 0, "strip_w": 0, "grid": 128, "chain_lds": 0,
        "pair_text_len": 0}},
    "batch_other_shape": {"mode": 0, "A": 4, "gap": 5, "R": 32, "U": 4, "W": 4, "key_bits": 12, "key_rowbits": 12,
        "sk": 0, "chain": 0, "chain_solo": 0, "band": 0, "band_r": 2, "strip_w": 1, "num_cu": 256, "fill_kind":
        "strips", "num_pairs": 512, "num_strips": 512, "num_bands": 0, "tb_groups": 0, "tb_slots": 0, "max_recs":
        2048, "code_bytes": 2424832, "mask_entries": 34603008, "granules": 0, "out_bytes": 2104320, "rec_words":
        1081344, "hash": "bbfb6233b021add5", "launch": {"W": 4, "sk": 0, "band3": 0, "num_groups": 128,
        "num_bands": 0, "num_band_groups": 0, "band_wgs": 0, "strip_w": 0, "grid": 128, "chain_lds": 0,
        "pair_text_len": 0}},
    "batch_no_pair16": {"mode": 0, "A": 4, "gap": 5, "R": 32, "U": 4, "W": 4, "key_bits": 12, "key_rowbits": 12,
        "sk": 0, "chain": 0, "chain_solo": 0, "band": 0, "band_r": 2, "strip_w": 1, "num_cu": 256, "fill_kind":
        "strips", "num_pairs": 512, "num_strips": 512, "num_bands": 0, "tb_groups": 0, "tb_slots": 0, "max_recs":
        2048, "code_bytes": 2424832, "mask_entries": 34603008, "granules": 0, "out_bytes": 2105344, "rec_words":
        1081344, "hash": "dc4d8173509d45d1", "launch": {"W": 4, "sk": 0, "band3": 0, "num_groups": 128,
        "num_bands": 0, "num_band_groups": 0, "band_wgs": 0, "strip_w": 0, "grid": 128, "chain_lds": 0,
        "pair_text_len": 0}},
    "local_headline": {"mode": 1, "A": 4, "gap": 5, "R": 1, "U": 16, "W": 4, "key_bits": 12, "key_rowbits": 16,
        "sk": 3, "chain": 1, "chain_solo": 0, "band": 1, "band_r": 3, "strip_w": 3, "num_cu": 256, "fill_kind":
        "band3", "num_pairs": 1, "num_strips": 512, "num_bands": 170, "tb_groups": 32, "tb_slots": 512,
        "max_recs": 32768, "code_bytes": 132352, "mask_entries": 16809984, "granules": 5571920, "out_bytes":
        65552, "rec_words": 32832, "hash": "7ad9f98a695a669f", "launch": {"W": 4, "sk": 3, "band3": 1,
        "num_groups": 171, "num_bands": 170, "num_band_groups": 43, "band_wgs": 43, "strip_w": 3, "grid": 214,
        "chain_lds": 98304, "pair_text_len": 0}},
    "empty_text": {"mode": 0, "A": 4, "gap": 5, "R": 1, "U": 16, "W": 4, "key_bits": 12, "key_rowbits": 7, "sk":
        3, "chain": 0, "chain_solo": 0, "band": 0, "band_r": 2, "strip_w": 1, "num_cu": 256, "fill_kind":
        "strips", "num_pairs": 1, "num_strips": 0, "num_bands": 0, "tb_groups": 0, "tb_slots": 0, "max_recs": 100,
        "code_bytes": 1280, "mask_entries": 0, "granules": 0, "out_bytes": 116, "rec_words": 164, "hash":
        "1a7de12188713166", "launch": {"W": 1, "sk": 3, "band3": 0, "num_groups": 0, "num_bands": 0,
        "num_band_groups": 0, "band_wgs": 0, "strip_w": 0, "grid": 0, "chain_lds": 0, "pair_text_len": 0}},
    "empty_pattern": {"mode": 0, "A": 4, "gap": 5, "R": 1, "U": 16, "W": 4, "key_bits": 12, "key_rowbits": 7,
        "sk": 3, "chain": 0, "chain_solo": 0, "band": 0, "band_r": 2, "strip_w": 1, "num_cu": 256, "fill_kind":
        "strips", "num_pairs": 1, "num_strips": 0, "num_bands": 0, "tb_groups": 0, "tb_slots": 0, "max_recs": 1,
        "code_bytes": 1680, "mask_entries": 0, "granules": 0, "out_bytes": 116, "rec_words": 164, "hash":
        "9351e6977e97ba0a", "launch": {"W": 1, "sk": 3, "band3": 0, "num_groups": 0, "num_bands": 0,
        "num_band_groups": 0, "band_wgs": 0, "strip_w": 0, "grid": 0, "chain_lds": 0, "pair_text_len": 0}},
    "no_pairs": {"mode": 0, "A": 4, "gap": 5, "R": 1, "U": 16, "W": 4, "key_bits": 12, "key_rowbits": 1, "sk": 3,
        "chain": 0, "chain_solo": 0, "band": 0, "band_r": 2, "strip_w": 1, "num_cu": 256, "fill_kind": "strips",
        "num_pairs": 0, "num_strips": 0, "num_bands": 0, "tb_groups": 0, "tb_slots": 0, "max_recs": 1,
        "code_bytes": 0, "mask_entries": 0, "granules": 0, "out_bytes": 0, "rec_words": 0, "hash":
        "cbf29ce484222325", "launch": {"W": 1, "sk": 3, "band3": 0, "num_groups": 0, "num_bands": 0,
        "num_band_groups": 0, "band_wgs": 0, "strip_w": 0, "grid": 0, "chain_lds": 0, "pair_text_len": 0}},
    "limit_length": {"error": 4, "message": "sequence longer than 2^24-2 letters"},
    "limit_score_range": {"error": 4, "message": "scores may exceed the int32 range"},
    "limit_local_key": {"error": 4, "message": "local scores may exceed the best-cell key range"},
    "limit_alphabet_0": {"error": 1, "message": "alphabet_size must be 1..32"},
    "limit_alphabet_33": {"error": 1, "message": "alphabet_size must be 1..32"},
    "limit_mode": {"error": 1, "message": "mode must be SA_GLOBAL or SA_LOCAL"},
    "small_strips": {"mode": 0, "A": 4, "gap": 5, "R": 1, "U": 16, "W": 4, "key_bits": 12, "key_rowbits": 11,
        "sk": 3, "chain": 1, "chain_solo": 1, "band": 0, "band_r": 2, "strip_w": 1, "num_cu": 256, "fill_kind":
        "strips", "num_pairs": 2, "num_strips": 33, "num_bands": 0, "tb_groups": 3, "tb_slots": 33, "max_recs":
        1100, "code_bytes": 8160, "mask_entries": 25344, "granules": 21948, "out_bytes": 3492, "rec_words": 2188,
        "hash": "1dd0445eda517f64", "launch": {"W": 4, "sk": 3, "band3": 0, "num_groups": 9, "num_bands": 0,
        "num_band_groups": 0, "band_wgs": 0, "strip_w": 0, "grid": 9, "chain_lds": 98304, "pair_text_len": 0}},
    "small_two_row": {"mode": 0, "A": 4, "gap": 5, "R": 1, "U": 16, "W": 4, "key_bits": 12, "key_rowbits": 11,
        "sk": 3, "chain": 1, "chain_solo": 0, "band": 1, "band_r": 2, "strip_w": 4, "num_cu": 256, "fill_kind":
        "band", "num_pairs": 2, "num_strips": 33, "num_bands": 15, "tb_groups": 3, "tb_slots": 33, "max_recs":
        1100, "code_bytes": 8160, "mask_entries": 25344, "granules": 10620, "out_bytes": 3492, "rec_words": 2188,
        "hash": "a874e32573164a74", "launch": {"W": 4, "sk": 3, "band3": 0, "num_groups": 9, "num_bands": 15,
        "num_band_groups": 4, "band_wgs": 4, "strip_w": 4, "grid": 13, "chain_lds": 98304, "pair_text_len": 0}},
    "small_three_row": {"mode": 0, "A": 4, "gap": 5, "R": 1, "U": 16, "W": 4, "key_bits": 12, "key_rowbits": 11,
        "sk": 3, "chain": 1, "chain_solo": 0, "band": 1, "band_r": 3, "strip_w": 3, "num_cu": 256, "fill_kind":
        "band3", "num_pairs": 2, "num_strips": 33, "num_bands": 9, "tb_groups": 3, "tb_slots": 33, "max_recs":
        1100, "code_bytes": 8160, "mask_entries": 25344, "granules": 6372, "out_bytes": 3492, "rec_words": 2188,
        "hash": "56d320065865a8ad", "launch": {"W": 4, "sk": 3, "band3": 1, "num_groups": 11, "num_bands": 9,
        "num_band_groups": 3, "band_wgs": 3, "strip_w": 3, "grid": 14, "chain_lds": 98304, "pair_text_len": 0}},
}


def plan(name: str, strips: bool = False, cus: int = 256) -> dict:
    args, knobs = CASES[name]
    return run_check(args, knobs, strips, cus)


def run_check(args, knobs, strips=False, cus=256) -> dict:
    if not os.path.exists(CHECK):
        subprocess.run(["make", "-s", "-C", PKG, "bin/sa_plan_check"], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SA_")}
    env.update(knobs)
    out = subprocess.run([CHECK, "--matrices", MATRICES, "--cus", str(cus)] + (["--strips"] if strips else []) + args,
                         env=env, check=True, capture_output=True, text=True).stdout
    return json.loads(out)


def subset_differences(got: dict, exp: dict, where: str = "") -> list:
    bad = []
    for k, v in exp.items():
        if isinstance(v, dict):
            bad += subset_differences(got.get(k, {}), v, where + k + ".")
        elif got.get(k) != v:
            bad.append((where + k, got.get(k), v))
    return bad


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_derived_plans(name):
    assert not subset_differences(plan(name), HAND[name])


def test_four_pairs_first_strips():
    """Pattern lengths 256 .. 1024 start their pairs at strips 0, 4, 12, 24 (no multiple of three
    throughout: two-row bands); 384 .. 1536 at 0, 6, 18, 36."""
    assert [p["first_strip"] for p in plan("four_pairs_two_row", strips=True)["pairs"]] == [0, 4, 12, 24]
    assert [p["first_strip"] for p in plan("four_pairs_three_row", strips=True)["pairs"]] == [0, 6, 18, 36]


def test_every_case_is_recorded():
    assert sorted(RECORDED) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_matches_recorded(name):
    """The whole plan (scalars, sizes, launch geometry and the hash of the descriptor arrays) is
    what the planner gave when it left the engine."""
    assert plan(name) == RECORDED[name]


def test_known_gap_row():
    """The ADVICE.md case as it stands today: R = 8 chosen for pair chains that the LDS condition
    refuses, so generic chains at R = 8 (see CASES["advice_gap"])."""
    got = plan("advice_gap")
    assert (got["R"], got["fill_kind"], got["sk"] != kPair, got["chain"]) == (8, "strips", True, 1)


def ranges_overlap(ranges) -> bool:
    ranges = sorted(r for r in ranges if r[1] > r[0])
    return any(a[1] > b[0] for a, b in zip(ranges, ranges[1:]))


@pytest.mark.parametrize("name,kind,SW,BR", [("small_strips", "strips", 0, 0), ("small_two_row", "band", 4, 2),
                                             ("small_three_row", "band3", 3, 3)])
def test_structure(name, kind, SW, BR):
    pl = plan(name, strips=True)
    assert pl["fill_kind"] == kind and pl["R"] == 1
    strips, bands, pairs = pl["strips"], pl["bands"], pl["pairs"]
    assert len(strips) == 18 + 15 and all(p["pattern_len"] <= 1100 for p in pairs)
    n_of = lambda d: pairs[d["pair"]]["text_len"]  # noqa: E731
    # who publishes granules: the bands of a band plan, else every strip with a successor
    producers = bands if bands else [s for s in strips if s["flags"] & kHasNext]
    assert all(b["flags"] & kHasNext for b in bands)
    out_of = {(d["pair"], d["bnd_out"]) for d in producers}
    assert not ranges_overlap([(d["bnd_out"], d["bnd_out"] + n_of(d) + 8) for d in producers])
    assert pl["granules"] == sum(n_of(d) + 8 for d in producers)
    # who reads granules: a band with a band above; a strip with a strip above (a band plan: at a group start)
    for i, s in enumerate(strips):
        if s["flags"] & kHasPrev and (not bands or i % SW == 0):
            assert (s["pair"], s["bnd_in"]) in out_of, (i, s)
    for b in bands:
        if b["flags"] & kHasPrev:
            assert (b["pair"], b["bnd_in"]) in out_of, b
    if bands:
        by_out = {b["bnd_out"]: b for b in bands}
        for i, s in enumerate(strips):
            first = pairs[s["pair"]]["first_strip"]
            assert first % BR == 0 and s["bnd_out"] == 0
            if (i + 1) % SW == 0:
                assert not s["flags"] & kHasNext, (i, s)  # a group's last strip publishes nothing
            if i % SW == 0 and i > first:
                # the first strip of a group reads the band that ends on the row above it
                b = by_out[s["bnd_in"]]
                assert b["pair"] == s["pair"] and b["row0"] + 64 * BR == s["row0"], (i, s, b)
        assert pl["launch"]["strip_w"] == SW and pl["band_r"] == BR
    assert not ranges_overlap([(s["mask_off"], s["mask_off"] + s["nsteps"] * pl["R"]) for s in strips])
    assert pl["mask_entries"] == sum(s["nsteps"] * pl["R"] for s in strips)


# (text length, pattern length, count) of shapes test_band_fill.py, test_band3_fill.py and
# test_batch_golden.py fill; here the plans are only created
GPU_SHAPES = [(DNA, 700, 193, 1), (DNA, 2100, 769, 1), (DNA, 700, 1100, 1), (DNA, 4500, 2900, 1),
              (PROTEIN, 2100, 769, 1), (DNA, 2048, 2048, 256)]


@pytest.mark.gpu
def test_engine_plans_match_plan_check(eng):
    """Plan creation only (no fill): the engine's fill kind, strip count and R are the stand-alone
    planner's for the device's CU count."""
    import torch
    from conftest import matrix
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    knobs = {k: v for k, v in os.environ.items() if k.startswith("SA_")}
    for args, n, m, count in GPU_SHAPES:
        A = int(args[3])
        S = matrix("blast" if A == 4 else "blosum50", A)
        p = eng.Plan(0, S, 5, [(i * n, n, i * m, m) for i in range(count)])
        info = p.info()
        p.close()
        exp = run_check(args + [f"{n}x{m}x{count}"], knobs, cus=cus)
        assert (info["fill_kernel"], info["num_strips"], info["rows_per_lane"], info["mask_bytes"]) == (
            exp["fill_kind"], exp["num_strips"], exp["R"], 16 * exp["mask_entries"]), (n, m, count, info, exp)
