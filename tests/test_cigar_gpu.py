"""CIGAR output on the device (sa_hip.h: sa_align_pairs_cigar): in every case the expected ops and counts are
test_cigar_plan.cigar_ref of the two strings that align_pairs_affine returns for the same arguments in the same
test (identity G1), and every field of sa_result must be that call's too. The cases are those at which the encoder
kernel can go wrong: every variant's string layout (a tail piece, a head and a tail piece, joined pieces), empty
sides and empty results, runs that cross a 64-column step or the head/tail junction, 64 run ends in one step, more
than one chunk of the work order, and the offsets of the pairs' ops in the call's op array."""
from __future__ import annotations

import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, matrix  # first: it puts oracle/ and the package on the path

from sa_amd import synthetic
from test_chains_gpu import random_chain
from test_cigar_plan import COUNTS, D, EQ, I, X, cigar_ref, cigar_text
from test_extend_gpu import random_small_pairs

gpu = pytest.mark.gpu

GLOBAL, LOCAL, FIT, OVERLAP = 0, 1, 2, 31
GAPS = [(11, 2), (5, 5)]
SCALARS = ("score", "num_bytes", "start_text", "start_pattern")
CHUNK_BUDGET = 256 << 10


def dna_pairs(count=24, seed=92100, nmax=200):
    """`count` random DNA pairs of 1 to nmax letters a side, three of them with an empty side or two."""
    pairs = [(t, p) for A, t, p in random_small_pairs(2 * count, seed, nmax) if A == 4][:count]
    empty = np.zeros(0, np.int8)
    pairs[3] = (empty, pairs[3][1])
    pairs[7] = (pairs[7][0], empty)
    pairs[11] = (empty, empty)
    return [t for t, _ in pairs], [p for _, p in pairs]


def variant_keywords(name, texts, patterns, seed=92200):
    """(mode, keywords) of the named variant for these pairs."""
    rng = np.random.default_rng(seed)
    shapes = [(len(t), len(p)) for t, p in zip(texts, patterns)]
    seeds = []
    for n, m in shapes:
        ts, ps = int(rng.integers(0, n + 1)), int(rng.integers(0, m + 1))
        seeds.append((ts, ps, int(rng.integers(0, min(n - ts, m - ps, 12) + 1))))
    if name in ("global", "local", "fit", "overlap"):
        return {"global": GLOBAL, "local": LOCAL, "fit": FIT, "overlap": OVERLAP}[name], {}
    if name == "band":
        return GLOBAL, {"band": 8}
    if name == "bands":
        return FIT, {"bands": [(-m - 2, n + 2) if k % 2 else (min(0, n - m) - 6, max(0, n - m) + 6) for k, (n, m) in enumerate(shapes)]}
    if name == "xdrop":
        return GLOBAL, {"xdrop": 30}
    if name == "seeds":
        return GLOBAL, {"xdrop": 30, "seeds": seeds}
    if name == "width":
        return GLOBAL, {"xdrop": 30, "width": 8}
    if name == "width_seeds":
        return GLOBAL, {"xdrop": 30, "width": 8, "seeds": seeds}
    assert name == "chains"
    return GLOBAL, {"xdrop": 30, "chains": [random_chain(rng, n, m, 1 + k % 5) for k, (n, m) in enumerate(shapes)]}


VARIANTS = ("global", "local", "fit", "overlap", "band", "bands", "xdrop", "seeds", "width", "width_seeds", "chains")


def check(eng, mode, texts, patterns, S, go, ge, what, flags=(True, False), **kw):
    """align_pairs_cigar against cigar_ref of align_pairs_affine's strings, under both flags: the ops, their text, the
    counts, the offsets, the totals and every field of sa_result. Returns the strings call's and the EQX results."""
    want = eng.align_pairs_affine(mode, texts, patterns, S, go, ge, **kw)
    out = None
    for eqx in flags:
        got = eng.align_pairs_cigar(mode, texts, patterns, S, go, ge, eqx=eqx, **kw)
        assert len(got) == len(want)
        off = 0
        for k, (g, w) in enumerate(zip(got, want)):
            ops, counts = cigar_ref(w["aligned_text"], w["aligned_pattern"], "-", eqx)
            where = (what, eqx, go, ge, k, len(texts[k]), len(patterns[k]))
            assert {f: g[f] for f in SCALARS} == {f: w[f] for f in SCALARS}, where
            assert g["cigar"].dtype == np.uint32 and g["cigar"].tolist() == ops, (where, g["cigar_string"], cigar_text(ops))
            assert g["cigar_string"] == cigar_text(ops) and g["num_ops"] == len(ops), where
            assert {f: g[f] for f in COUNTS} == counts, where
            assert g["matches"] + g["mismatches"] + g["text_gap_letters"] + g["pattern_gap_letters"] == g["num_bytes"], where
            assert g["ops_off"] == off, where  # the exclusive sum of num_ops in pair order
            off += g["num_ops"]
        assert eng.cigar_last_stats()["ops_bytes"] == 4 * off
        out = out or got
    return want, out


# ---- 1. every variant -------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("go,ge", GAPS)
@pytest.mark.parametrize("name", VARIANTS)
def test_variants(eng, name, go, ge):
    texts, patterns = dna_pairs()
    assert sum(len(t) == 0 for t in texts) == 2 and sum(len(p) == 0 for p in patterns) == 2 and max(map(len, texts)) > 128
    mode, kw = variant_keywords(name, texts, patterns)
    want, got = check(eng, mode, texts, patterns, matrix("blast", 4), go, ge, name, **kw)
    assert sum(g["num_ops"] for g in got) > len(got)  # the case is not trivial
    st = eng.cigar_last_stats()
    assert st["string_bytes_not_copied"] == 2 * sum(len(t) + len(p) for t, p in zip(texts, patterns)) and st["encode_ms"] > 0


# ---- 2. step boundaries -----------------------------------------------------------------------------------------------
@gpu
def test_identical_pairs_are_one_run(eng):
    lens = (63, 64, 65, 128, 129, 300)
    texts = [synthetic.random_sequence(92300 + n, n, 4) for n in lens]
    for mode in (GLOBAL, LOCAL):
        _, got = check(eng, mode, texts, texts, matrix("blast", 4), 11, 2, "identical")
        assert [g["cigar_string"] for g in got] == [f"{n}=" for n in lens]
        assert [g["matches"] for g in got] == list(lens) and all(g["gap_opens"] == 0 for g in got)
    got = eng.align_pairs_cigar(GLOBAL, texts, texts, matrix("blast", 4), 11, 2, eqx=False)
    assert [g["cigar_string"] for g in got] == [f"{n}M" for n in lens]


@gpu
def test_one_insertion_run_across_three_steps(eng):
    t = synthetic.random_sequence(92400, 300, 4)
    extra = synthetic.random_sequence(92401, 150, 4)
    p = np.concatenate([t[:150], extra, t[150:]]).astype(np.int8)
    _, got = check(eng, GLOBAL, [t], [p], matrix("blast", 4), 16, 1, "insertion")
    g = got[0]
    runs = [op >> 4 for op in g["cigar"].tolist() if op & 15 == I]
    assert runs == [150] and g["text_gap_letters"] == 150 and g["gap_opens"] == 1 and g["matches"] == 300, g["cigar_string"]
    # and the deletion: the same pair the other way round
    _, got = check(eng, GLOBAL, [p], [t], matrix("blast", 4), 16, 1, "deletion")
    assert [op >> 4 for op in got[0]["cigar"].tolist() if op & 15 == D] == [150] and got[0]["pattern_gap_letters"] == 150


@gpu
def test_two_hundred_runs_of_one_column(eng):
    """Every second letter substituted, a mismatch at -1 and gaps at 16/4: 200 ops of length 1, so that every step
    but the last ends 64 runs and the op index is carried across the steps."""
    S = np.full((4, 4), -1, dtype=np.int32)
    np.fill_diagonal(S, 5)
    t = synthetic.random_sequence(92500, 200, 4)
    p = t.copy()
    p[1::2] = (p[1::2] + 1) % 4
    _, got = check(eng, GLOBAL, [t], [p], S, 16, 4, "alternating")
    g = got[0]
    assert g["cigar"].tolist() == [1 << 4 | (X if k % 2 else EQ) for k in range(200)]
    assert g["matches"] == 100 and g["mismatches"] == 100 and g["gap_opens"] == 0
    got = eng.align_pairs_cigar(GLOBAL, [t], [p], S, 16, 4, eqx=False)
    assert got[0]["cigar_string"] == "200M" and got[0]["mismatches"] == 100  # counted from the letters under M too


# ---- 3. the head/tail junction of a seeded pair --------------------------------------------------------------------------
@gpu
def test_a_run_merges_across_the_junction_and_the_seed(eng):
    t = synthetic.random_sequence(92600, 150, 4)
    u = synthetic.random_sequence(92601, 77, 4)
    texts = [t, t, t, t, t, u, u]
    seeds = [(50, 50, 20), (70, 70, 0), (0, 0, 0), (150, 150, 0), (0, 0, 150), (13, 13, 64), (64, 64, 13)]
    for kw in ({}, {"width": 8}):
        _, got = check(eng, GLOBAL, texts, texts, matrix("blast", 4), 11, 2, "junction", xdrop=eng.NO_XDROP, seeds=seeds, **kw)
        assert [g["cigar_string"] for g in got] == [f"{len(x)}=" for x in texts]
    # mismatching seed letters are scored and encoded as they are: X columns between the two halves' = runs
    p = t.copy()
    p[60:63] = (p[60:63] + 1) % 4
    _, got = check(eng, GLOBAL, [t], [p], matrix("blast", 4), 11, 2, "seed of mismatches", xdrop=eng.NO_XDROP, seeds=[(60, 60, 3)])
    assert got[0]["cigar_string"] == "60=3X87="


@gpu
def test_an_empty_result_has_no_ops_and_a_null_op_array(eng):
    a, c = np.zeros(6, np.int8), np.full(6, 2, np.int8)
    want, got = check(eng, GLOBAL, [a, a], [c, c], matrix("blast", 4), 11, 2, "empty", xdrop=eng.NO_XDROP, seeds=[(3, 3, 0), (0, 6, 0)])
    assert [w["num_bytes"] for w in want] == [0, 0]
    assert [(g["num_ops"], g["cigar_string"], g["start_text"], g["start_pattern"]) for g in got] == [(0, "", 3, 3), (0, "", 0, 6)]
    # through the C ABI: the handle exists, holds 0 ops and gives no address
    S = np.ascontiguousarray(matrix("blast", 4), dtype=np.int32)
    params = eng.SaParams(GLOBAL, 4, 0, 0, S.ctypes.data, b"ATCG-")
    sd = np.array([3, 3, 0], dtype=np.uint64)
    spec = eng.SaAlignSpec(11, 2, -1, eng.NO_XDROP, -1, 1, None, sd.ctypes.data, None)
    hp = (eng.SaHostPair * 1)(eng.SaHostPair(a.ctypes.data, 6, c.ctypes.data, 6))
    res = (eng.SaCigarResult * 1)()
    handle = ctypes.c_void_p()
    assert eng.lib.sa_align_pairs_cigar(ctypes.byref(params), ctypes.byref(spec), eng.CIGAR_EQX, hp, 1, 0, res, ctypes.byref(handle)) == 0
    assert handle.value is not None and eng.lib.sa_cigars_num_ops(handle) == 0 and eng.lib.sa_cigars_ops(handle) is None
    assert (res[0].num_ops, res[0].num_alignment_bytes, res[0].ops_off, res[0].start_text) == (0, 0, 0, 3)
    assert eng.lib.sa_cigars_destroy(handle) == 0
    # no pairs at all
    assert eng.align_pairs_cigar(GLOBAL, [], [], matrix("blast", 4), 11, 2) == []


# ---- 4. many pieces ---------------------------------------------------------------------------------------------------
@gpu
def test_a_chain_of_more_than_64_seeds_and_one_with_empty_sided_gaps(eng):
    rng = np.random.default_rng(92700)
    t = synthetic.random_sequence(92701, 700, 4)
    p = synthetic.mutate(t, 92702, 4)
    long_chain = random_chain(rng, len(t), len(p), 75)
    assert len(long_chain) >= 70  # 151 pieces: the join's third batch of 64
    u = synthetic.random_sequence(92703, 60, 4)
    empty_sides = [(5, 5, 4), (20, 9, 3), (23, 30, 2)]  # a gap of 11 text letters against none, then none against 18
    for go, ge in GAPS:
        _, got = check(eng, GLOBAL, [t, u], [p, u], matrix("blast", 4), go, ge, "long chain", xdrop=eng.NO_XDROP, chains=[long_chain, empty_sides])
        runs = got[1]["cigar"].tolist()
        assert 11 << 4 | D in runs and 18 << 4 | I in runs


# ---- 5. more than one chunk ---------------------------------------------------------------------------------------------
def chunk_calls(engine):
    """The variants case as the affine and as the chains aligner, under EQX at 11/2: what the parent and the child
    of the chunks test both run."""
    texts, patterns = dna_pairs()
    out = {}
    for name in ("global", "chains"):
        mode, kw = variant_keywords(name, texts, patterns)
        got = engine.align_pairs_cigar(mode, texts, patterns, matrix("blast", 4), 11, 2, **kw)
        out[name] = {"cigars": [g["cigar_string"] for g in got], "ops_off": [g["ops_off"] for g in got],
                     "counts": [[g[f] for f in COUNTS] for g in got], "scalars": [[g[f] for f in SCALARS] for g in got],
                     "num_chunks": engine.affine_last_stats()["num_chunks"]}
    return out


@gpu
def test_three_chunks_give_the_ops_of_one(eng):
    """In a process of its own (the budget is read once per process): the string arenas hold the whole call, so the
    encoder finds the pairs of every chunk after the last chunk's walk."""
    env = dict(os.environ, SA_TRACE_ARENA_BYTES=str(CHUNK_BUDGET))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "chunks"], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    child = json.loads(out.stdout.strip().splitlines()[-1])
    mine = chunk_calls(eng)
    for name in ("global", "chains"):
        assert mine[name]["num_chunks"] == 1 and child[name]["num_chunks"] >= 3, (name, child[name]["num_chunks"])
        for f in ("cigars", "ops_off", "counts", "scalars"):
            assert child[name][f] == mine[name][f], (name, f)


# ---- 6. the C++ function -------------------------------------------------------------------------------------------------
@gpu
def test_cpp_cigar_check():
    out = subprocess.run([os.path.join(PKG, "bin", "sa_cigar_check"), "400", "64"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1] == "OK 64"


if __name__ == "__main__" and sys.argv[1:] == ["chunks"]:
    # the child of test_three_chunks_give_the_ops_of_one
    from sa_amd import engine as engine_
    print(json.dumps(chunk_calls(engine_)))
