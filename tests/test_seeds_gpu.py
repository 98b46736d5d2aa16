"""Seed extension (sa_hip.h: sa_score_batch_seeds, sa_scorer_create_seeds, sa_scorer_fetch_seeds,
sa_align_pairs_seeds): every pair carries a seed {ts, ps, L}; the right half t[ts + L:], p[ps + L:] and the
left half reverse(t[:ts]), reverse(p[:ps]) are extension alignments, and one call returns their sum with the
seed's score, the covered intervals and the joined strings. The engine reads the left halves backwards in
place. The reference of this file is seeds_ref: identity (S1), the composition of test_extend_gpu's extend_ref
on sliced and reversed numpy arrays. It is pinned on the CPU by (S2), by the mirror identity (S3) and by
re-scoring its strings; the GPU is then compared with it exactly, every field and both strings, at every
forced rows_per_lane of the scorer, through the linear kernels, and in the aligner."""
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
from test_align_affine_gpu import KEYS, alphabet_of, pick, rescore
from test_extend_gpu import GAPS, NONE, SMALL_GAPS, SMALL_X, extend_ref, random_small_pairs, xd
from test_score_gpu import related_pair

gpu = pytest.mark.gpu

GLOBAL, LOCAL, FIT, ENDS = 0, 1, 2, 16
FIELDS = ("score", "begin_text", "begin_pattern", "end_text", "end_pattern")


# ---- the reference of this file ------------------------------------------------------------------------
def seeds_ref(t, p, seed, S, go, ge, xdrop, alphabet=None, key=None):
    """(S1): the keys of align_pairs_affine, the fields of sa_seed_result, and the halves' stop rows."""
    t, p = np.asarray(t, dtype=np.int64), np.asarray(p, dtype=np.int64)
    ts, ps, L = (int(v) for v in seed)
    assert ts + L <= len(t) and ps + L <= len(p)
    alphabet = alphabet or alphabet_of(S)
    left = extend_ref(t[:ts][::-1], p[:ps][::-1], S, go, ge, xdrop, alphabet, key=(key, ts, ps, L, "left") if key else None)
    right = extend_ref(t[ts + L:], p[ps + L:], S, go, ge, xdrop, alphabet, key=(key, ts, ps, L, "right") if key else None)
    mid = sum(int(S[p[ps + q]][t[ts + q]]) for q in range(L))
    res = {"score": left["score"] + mid + right["score"],
           "begin_text": ts - left["end_text"], "begin_pattern": ps - left["end_pattern"],
           "end_text": ts + L + right["end_text"], "end_pattern": ps + L + right["end_pattern"],
           "aligned_text": left["aligned_text"][::-1] + "".join(alphabet[c] for c in t[ts:ts + L]) + right["aligned_text"],
           "aligned_pattern": left["aligned_pattern"][::-1] + "".join(alphabet[c] for c in p[ps:ps + L]) + right["aligned_pattern"],
           "left_stop": left["stop_row"], "right_stop": right["stop_row"], "left": left, "right": right}
    res["num_bytes"] = len(res["aligned_text"])
    res["start_text"], res["start_pattern"] = res["begin_text"], res["begin_pattern"]
    assert res["num_bytes"] == left["num_bytes"] + L + right["num_bytes"] == len(res["aligned_pattern"])
    return res


_REFS = {}  # key -> seeds_ref: the big pairs' references are computed once per process


def cached_ref(key, t, p, seed, S, go, ge, xdrop):
    k = (key, tuple(seed), go, ge, xdrop)
    if k not in _REFS:
        _REFS[k] = seeds_ref(t, p, seed, S, go, ge, xdrop, key=key)
    return _REFS[k]


def fields(r):
    return tuple(int(r[k]) for k in FIELDS)


def mirror(t, p, seed):
    ts, ps, L = seed
    return t[::-1].copy(), p[::-1].copy(), (len(t) - ts - L, len(p) - ps - L, L)


def mirrored(res, n, m):
    """What (S3) says the mirrored pair returns, from this pair's result."""
    return {"score": res["score"], "begin_text": n - res["end_text"], "begin_pattern": m - res["end_pattern"],
            "end_text": n - res["begin_text"], "end_pattern": m - res["begin_pattern"], "num_bytes": res["num_bytes"],
            "start_text": n - res["end_text"], "start_pattern": m - res["end_pattern"],
            "aligned_text": res["aligned_text"][::-1], "aligned_pattern": res["aligned_pattern"][::-1]}


def random_seed(rng, n, m, lmax=None):
    ts, ps = int(rng.integers(0, n + 1)), int(rng.integers(0, m + 1))
    room = min(n - ts, m - ps)
    return ts, ps, int(rng.integers(0, min(room, lmax if lmax is not None else room) + 1))


def check(eng, texts, patterns, seeds, S, go, ge, xdrop, wants, what, Rs=(1, 2, 4, 8)):
    """Every forced rows_per_lane of the seeds scorer (the linear kernels too when go == ge, through
    gap_extend=None), and the seeds aligner: every field and both strings."""
    x = xd(eng, xdrop)
    for R in Rs:
        got = eng.score_batch(GLOBAL, texts, patterns, S, go, rows_per_lane=R, gap_extend=ge, xdrop=x, seeds=seeds)
        assert got.dtype == eng.SEED_DTYPE and (got["status"] == 0).all()
        assert [fields(g) for g in got] == [fields(w) for w in wants], (what, "score", go, ge, xdrop, R)
        if go == ge:
            got = eng.score_batch(GLOBAL, texts, patterns, S, go, rows_per_lane=R, xdrop=x, seeds=seeds)
            assert [fields(g) for g in got] == [fields(w) for w in wants], (what, "score, gap_extend=None", go, xdrop, R)
    got = eng.align_pairs_affine(GLOBAL, texts, patterns, S, go, ge, xdrop=x, seeds=seeds)
    for k, (g, w) in enumerate(zip(got, wants)):
        assert pick(g) == pick(w), (what, "align", go, ge, xdrop, k, seeds[k], len(patterns[k]), len(texts[k]))
    return got


# ---- 1. the reference of this file is sound (CPU) ------------------------------------------------------
def small_cases(count=60, seed=71100):
    rng = np.random.default_rng(seed)
    out = []
    for k, (A, t, p) in enumerate(random_small_pairs(count, seed)):
        out.append((A, t, p, random_seed(rng, len(t), len(p), lmax=None if k % 4 else 0)))
    return out


def test_s2_the_seed_at_the_origin_is_the_extension():
    for k, (A, t, p, _) in enumerate(small_cases()):
        S = matrix("blast" if A == 4 else "blosum50", A)
        for go, ge in SMALL_GAPS:
            for x in SMALL_X:
                want = extend_ref(t, p, S, go, ge, x)
                got = seeds_ref(t, p, (0, 0, 0), S, go, ge, x)
                assert pick(got) == pick(want), (k, go, ge, x)
                assert fields(got) == (want["score"], 0, 0, want["end_text"], want["end_pattern"]), (k, go, ge, x)
                assert got["left_stop"] == 1 and got["right_stop"] == want["stop_row"]


def test_s3_the_mirrored_pair_mirrors_every_output():
    for k, (A, t, p, sd) in enumerate(small_cases()):
        S = matrix("blast" if A == 4 else "blosum50", A)
        mt, mp, msd = mirror(t, p, sd)
        for go, ge in SMALL_GAPS:
            for x in SMALL_X:
                a, b = seeds_ref(t, p, sd, S, go, ge, x), seeds_ref(mt, mp, msd, S, go, ge, x)
                want = mirrored(a, len(t), len(p))
                assert {f: b[f] for f in want} == want, (k, sd, go, ge, x)
                # its left half is literally this pair's right half
                assert pick(b["left"]) == pick(a["right"]) and b["left_stop"] == a["right_stop"]


def test_the_strings_of_the_reference_rescore_and_cover_their_intervals():
    for k, (A, t, p, sd) in enumerate(small_cases()):
        S = matrix("blast" if A == 4 else "blosum50", A)
        alpha = alphabet_of(S)
        for go, ge in SMALL_GAPS:
            for x in SMALL_X:
                res = seeds_ref(t, p, sd, S, go, ge, x)
                assert res["aligned_text"].replace("-", "") == "".join(alpha[c] for c in t[res["begin_text"]:res["end_text"]])
                assert res["aligned_pattern"].replace("-", "") == "".join(alpha[c] for c in p[res["begin_pattern"]:res["end_pattern"]])
                assert res["begin_text"] <= sd[0] and sd[0] + sd[2] <= res["end_text"]
                if not 0 <= ge <= go:
                    continue  # rescore reads a run of gap letters as one gap: the recurrence's reading for these only
                # with L = 0 a gap next to the anchor in the left half and one next to it in the right half, on the
                # same side, are two gaps to the definition and one run to rescore, which then charges ge for go
                # (the halves' own strings start at their origins: their first letters are the ones next to the seed)
                la, ra = res["left"], res["right"]
                first_l = (la["aligned_text"][:1], la["aligned_pattern"][:1])
                first_r = (ra["aligned_text"][:1], ra["aligned_pattern"][:1])
                joined = sd[2] == 0 and any(a == "-" and b == "-" for a, b in zip(first_l, first_r))
                if joined:
                    assert rescore(res, S, go, ge, alpha) == res["score"] + go - ge, (k, sd, go, ge, x)
                else:
                    assert rescore(res, S, go, ge, alpha) == res["score"], (k, sd, go, ge, x)


# ---- 2. edge halves ------------------------------------------------------------------------------------
HALF = (0, 1, 7, 63, 64, 65, 129)
SEED_L = (0, 1, 15, 64)


def edge_cases(A, count=36, seed=72200):
    """Half shapes (rows x columns) drawn from HALF on each side and L from SEED_L, and two pairs whose left
    and whose right half is 513 rows x 300 columns: across a 512-row traced strip and a 64 R-row score strip
    at every R."""
    rng = np.random.default_rng(seed + A)
    shapes = [tuple(int(rng.choice(HALF)) for _ in range(4)) + (int(rng.choice(SEED_L)),) for _ in range(count)]
    shapes += [(0, 0, 0, 0, 0), (0, 0, 0, 0, 15), (129, 0, 0, 129, 1), (0, 129, 129, 0, 64)]  # nothing but a seed; crossed empties
    shapes += [(513, 300, 65, 64, 15), (64, 65, 513, 300, 1)]
    out = []
    for k, (ml, nl, mr, nr, L) in enumerate(shapes):
        n, m = nl + L + nr, ml + L + mr
        letters = 20 if A == 23 else A
        t = synthetic.random_sequence(seed + 7 * k + A, n, letters).astype(np.int8)
        # the pattern's halves are the text's halves mutated away from the seed, so that both extensions run
        # along related letters; a half with an empty side gets random letters
        left = synthetic.mutate(np.resize(t[:nl][::-1], max(ml, 1)), seed + k, letters, ml)[::-1] if nl else synthetic.random_sequence(seed + k, ml, letters)
        right = synthetic.mutate(np.resize(t[nl + L:], max(mr, 1)), seed + k + 1, letters, mr) if nr else synthetic.random_sequence(seed + k + 1, mr, letters)
        p = np.concatenate([left, t[nl:nl + L], right]).astype(np.int8)
        if k % 3 == 0 and L:
            p[ml + L // 2] = (p[ml + L // 2] + 1) % 4  # a seed's letters need not match
        assert (len(t), len(p)) == (n, m)
        out.append((t, p, (nl, ml, L)))
    return out


def test_the_edge_cases_have_their_shapes():
    cases = edge_cases(4)
    assert any(sd[1] == 513 and sd[0] == 300 for _, _, sd in cases)
    assert any(len(p) - sd[1] - sd[2] == 513 and len(t) - sd[0] - sd[2] == 300 for t, p, sd in cases)
    for t, p, (ts, ps, L) in cases:
        assert ts + L <= len(t) and ps + L <= len(p)


@gpu
@pytest.mark.parametrize("go,ge", GAPS)
@pytest.mark.parametrize("A,mat", [(4, "blast"), (23, "blosum50")])
def test_edge_halves(eng, A, mat, go, ge):
    S = matrix(mat, A)
    cases = edge_cases(A)
    texts, patterns, seeds = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    for x in (NONE, 20):
        wants = [cached_ref(("edge", A, k), t, p, sd, S, go, ge, x) for k, (t, p, sd) in enumerate(cases)]
        check(eng, texts, patterns, seeds, S, go, ge, x, wants, "edge halves")


# ---- 3. packed arenas ----------------------------------------------------------------------------------
def packed_cases():
    """Pairs that align from corner to corner, so that one letter more on either side would be a match: the
    byte before a pair's first letter and the byte after its last are its neighbours' in the packed arenas,
    and every pair's text and pattern end (and begin) in the same letter."""
    out = []
    for k, n in enumerate((70, 1, 64, 129, 65, 200, 63, 7)):
        X = synthetic.random_sequence(7300 + k, n, 4).astype(np.int8)
        Y = synthetic.random_sequence(7400 + k, 20 + k, 4).astype(np.int8)
        Y[-1] = (X[0] + 1) % 4  # no match across the junction of Y and X
        Y[0] = X[0]             # the pair's two first letters are one letter, with Y in front too
        which = k % 4
        if which == 0:
            out.append((X, X.copy(), (n // 2, n // 2, min(3, n - n // 2))))
        elif which == 1:
            out.append((X, np.concatenate([Y, X]), (0, len(Y), 0)))              # ts = 0 with ps > 0
        elif which == 2:
            out.append((np.concatenate([Y, X]), X, (len(Y), 0, min(1, n))))      # ps = 0 with ts > 0
        else:
            out.append((X, X.copy(), (n, n, 0)))                                  # the seed at the far corner
    return out


def test_the_packed_pairs_reach_their_corners():
    S = matrix("blast", 4)
    cases = packed_cases()
    texts, patterns = np.concatenate([c[0] for c in cases]), np.concatenate([c[1] for c in cases])
    to = np.concatenate([[0], np.cumsum([len(c[0]) for c in cases])])
    po = np.concatenate([[0], np.cumsum([len(c[1]) for c in cases])])
    for k, (t, p, sd) in enumerate(cases):
        w = seeds_ref(t, p, sd, S, 11, 2, NONE)
        assert (w["end_text"], w["end_pattern"]) == (len(t), len(p)), k  # the right half runs to the pair's end
        assert w["begin_text"] == 0 or w["begin_pattern"] == 0, k
        if sd[0] and sd[1]:
            assert (w["begin_text"], w["begin_pattern"]) == (0, 0), k    # the left half to its first letters
        if k + 1 < len(cases):
            assert texts[to[k + 1]] == patterns[po[k + 1]]   # the byte after this pair's last, on both sides: a match
        if k:
            assert texts[to[k] - 1] == patterns[po[k] - 1]   # the byte before its first


@gpu
@pytest.mark.parametrize("go,ge", GAPS)
def test_packed_arenas(eng, go, ge):
    import torch
    S = matrix("blast", 4)
    cases = packed_cases()
    to = np.concatenate([[0], np.cumsum([len(c[0]) for c in cases])])
    po = np.concatenate([[0], np.cumsum([len(c[1]) for c in cases])])
    dt = torch.from_numpy(np.concatenate([c[0] for c in cases])).cuda()
    dp = torch.from_numpy(np.concatenate([c[1] for c in cases])).cuda()
    pairs = [(int(to[k]), len(c[0]), int(po[k]), len(c[1])) for k, c in enumerate(cases)]
    seeds = [c[2] for c in cases]
    for x in (NONE, 20):
        wants = [seeds_ref(t, p, sd, S, go, ge, x) for t, p, sd in cases]
        for R in (1, 2, 4, 8):
            for lin in ((False, True) if go == ge else (False,)):
                sc = eng.Scorer(GLOBAL, S, go, pairs, rows_per_lane=R, gap_extend=None if lin else ge, xdrop=xd(eng, x), seeds=seeds)
                assert sc.info()["rows_per_lane"] == R
                sc.run(dt.data_ptr(), dp.data_ptr())
                got = sc.results()
                ends = sc.score_results()
                sc.close()
                assert [fields(g) for g in got] == [fields(w) for w in wants], (x, R, lin)
                # sa_scorer_fetch on a seeds scorer: the score with the absolute end cell
                assert [(int(e["score"]), int(e["end_text"]), int(e["end_pattern"])) for e in ends] == \
                       [(w["score"], w["end_text"], w["end_pattern"]) for w in wants]


# ---- 4. the X-drop on each side --------------------------------------------------------------------------
XGAP, XDROP = (16, 4), 20


def xdrop_cases():
    """Related for 40 letters on either side of the seed, random beyond."""
    out = []
    for k, (n, m, ts, ps, L) in enumerate(((300, 300, 130, 130, 20), (400, 260, 250, 100, 15), (200, 330, 90, 200, 0), (500, 500, 100, 380, 64))):
        t = synthetic.random_sequence(7500 + k, n, 4).astype(np.int8)
        p = synthetic.random_sequence(7600 + k, m, 4).astype(np.int8)
        a, b = min(40, ts, ps), min(40, n - ts - L, m - ps - L)
        p[ps - a:ps + L + b] = t[ts - a:ts + L + b]
        out.append((t, p, (ts, ps, L)))
    return out


def test_the_xdrop_cases_stop_inside_their_halves():
    S = matrix("blast", 4)
    left = right = 0
    for t, p, sd in xdrop_cases():
        w = seeds_ref(t, p, sd, S, *XGAP, XDROP)
        left += w["left_stop"] <= sd[1]                          # a stop row inside the left half's ps rows
        right += w["right_stop"] <= len(p) - sd[1] - sd[2]        # and inside the right half's
        assert w["score"] >= 5 * (sd[2] + 60)
    assert left >= 1 and right >= 1, (left, right)


@gpu
def test_the_xdrop_on_each_side(eng):
    S = matrix("blast", 4)
    cases = xdrop_cases()
    texts, patterns, seeds = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    wants = [cached_ref(("xdrop", k), t, p, sd, S, *XGAP, XDROP) for k, (t, p, sd) in enumerate(cases)]
    assert sum(w["left_stop"] <= sd[1] for w, sd in zip(wants, seeds)) >= 1
    assert sum(w["right_stop"] <= len(p) - sd[1] - sd[2] for w, p, sd in zip(wants, patterns, seeds)) >= 1
    check(eng, texts, patterns, seeds, S, *XGAP, XDROP, wants, "xdrop")
    nodrop = [cached_ref(("xdrop", k), t, p, sd, S, *XGAP, NONE) for k, (t, p, sd) in enumerate(cases)]
    check(eng, texts, patterns, seeds, S, *XGAP, NONE, nodrop, "xdrop, none")


# ---- 5. (S1) against the library itself, (S2) and (S3) on the device ----------------------------------------
def library_cases(count=100, seed=73300, nmax=96):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        n, m = int(rng.integers(1, nmax + 1)), int(rng.integers(1, nmax + 1))
        t, p = related_pair(seed + 10 * k, n, m, 4)
        out.append((t.astype(np.int8), p.astype(np.int8), random_seed(rng, n, m, lmax=None if k % 3 else 0)))
    return out


@gpu
@pytest.mark.parametrize("go,ge", GAPS)
def test_s1_against_the_extension_functions(eng, go, ge):
    S = matrix("blast", 4)
    cases = library_cases()
    texts, patterns, seeds = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    lt = [np.ascontiguousarray(t[:ts][::-1]) for t, _, (ts, ps, L) in cases]
    lp = [np.ascontiguousarray(p[:ps][::-1]) for _, p, (ts, ps, L) in cases]
    rt = [np.ascontiguousarray(t[ts + L:]) for t, _, (ts, ps, L) in cases]
    rp = [np.ascontiguousarray(p[ps + L:]) for _, p, (ts, ps, L) in cases]
    for x in (20, eng.NO_XDROP):
        ls = eng.score_batch(GLOBAL, lt, lp, S, go, gap_extend=ge, xdrop=x)
        rs = eng.score_batch(GLOBAL, rt, rp, S, go, gap_extend=ge, xdrop=x)
        la = eng.align_pairs_affine(GLOBAL, lt, lp, S, go, ge, xdrop=x)
        ra = eng.align_pairs_affine(GLOBAL, rt, rp, S, go, ge, xdrop=x)
        got = eng.score_batch(GLOBAL, texts, patterns, S, go, gap_extend=ge, xdrop=x, seeds=seeds)
        al = eng.align_pairs_affine(GLOBAL, texts, patterns, S, go, ge, xdrop=x, seeds=seeds)
        for k, (t, p, (ts, ps, L)) in enumerate(cases):
            mid = sum(int(S[p[ps + q]][t[ts + q]]) for q in range(L))
            want = (int(ls[k]["score"]) + mid + int(rs[k]["score"]), ts - int(ls[k]["end_text"]), ps - int(ls[k]["end_pattern"]),
                    ts + L + int(rs[k]["end_text"]), ps + L + int(rs[k]["end_pattern"]))
            assert fields(got[k]) == want, (x, k)
            assert al[k]["aligned_text"] == la[k]["aligned_text"][::-1] + "".join("ATCG"[c] for c in t[ts:ts + L]) + ra[k]["aligned_text"], (x, k)
            assert al[k]["aligned_pattern"] == la[k]["aligned_pattern"][::-1] + "".join("ATCG"[c] for c in p[ps:ps + L]) + ra[k]["aligned_pattern"], (x, k)
            assert (al[k]["score"], al[k]["start_text"], al[k]["start_pattern"], al[k]["num_bytes"]) == \
                   (want[0], want[1], want[2], la[k]["num_bytes"] + L + ra[k]["num_bytes"]), (x, k)
        # (S2): the seed {0, 0, 0} is the extension function
        zero = [(0, 0, 0)] * len(cases)
        ext = eng.score_batch(GLOBAL, texts, patterns, S, go, gap_extend=ge, xdrop=x)
        got = eng.score_batch(GLOBAL, texts, patterns, S, go, gap_extend=ge, xdrop=x, seeds=zero)
        assert [fields(g) for g in got] == [(int(e["score"]), 0, 0, int(e["end_text"]), int(e["end_pattern"])) for e in ext]
        assert eng.align_pairs_affine(GLOBAL, texts, patterns, S, go, ge, xdrop=x, seeds=zero) == \
               eng.align_pairs_affine(GLOBAL, texts, patterns, S, go, ge, xdrop=x)


@gpu
@pytest.mark.parametrize("A,mat", [(4, "blast"), (23, "blosum50")])
def test_s3_on_the_device(eng, A, mat):
    S = matrix(mat, A)
    cases = edge_cases(A)
    texts, patterns, seeds = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    mir = [mirror(*c) for c in cases]
    for go, ge in GAPS:
        for x in (20, eng.NO_XDROP):
            a = eng.score_batch(GLOBAL, texts, patterns, S, go, gap_extend=ge, xdrop=x, seeds=seeds)
            b = eng.score_batch(GLOBAL, [c[0] for c in mir], [c[1] for c in mir], S, go, gap_extend=ge, xdrop=x, seeds=[c[2] for c in mir])
            aa = eng.align_pairs_affine(GLOBAL, texts, patterns, S, go, ge, xdrop=x, seeds=seeds)
            bb = eng.align_pairs_affine(GLOBAL, [c[0] for c in mir], [c[1] for c in mir], S, go, ge, xdrop=x, seeds=[c[2] for c in mir])
            for k, (t, p, _) in enumerate(cases):
                n, m = len(t), len(p)
                assert fields(b[k]) == (int(a[k]["score"]), n - int(a[k]["end_text"]), m - int(a[k]["end_pattern"]),
                                        n - int(a[k]["begin_text"]), m - int(a[k]["begin_pattern"])), (go, ge, x, k)
                assert (bb[k]["aligned_text"], bb[k]["aligned_pattern"]) == (aa[k]["aligned_text"][::-1], aa[k]["aligned_pattern"][::-1]), (go, ge, x, k)
                assert (bb[k]["start_text"], bb[k]["start_pattern"]) == (n - int(a[k]["end_text"]), m - int(a[k]["end_pattern"]))


# ---- 6. beyond the arena budget ------------------------------------------------------------------------------
BIG, BIG_L, BIG_BUDGET = 6000, 1000, 8 << 20
BIG_SEED = ((BIG - BIG_L) // 2, (BIG - BIG_L) // 2, BIG_L)   # centred: both halves are 2500 x 2500, 3.2 MiB of directions each
BIG_BARE = (BIG // 2, BIG // 2, 0)                           # the bare centre: two halves of 3000 x 3000, 4.5 MiB each, 9 MiB together


def big_pair():
    t = synthetic.random_sequence(171, BIG, 4).astype(np.int8)
    return t, synthetic.mutate(t, 172, 4, BIG).astype(np.int8)


@gpu
def test_a_seeded_pair_beyond_the_arena_budget_aligns():
    """In a process of its own (the budget is read once per process): 6000 x 6000 needs 18 MiB of directions,
    the budget is 8 MiB. Seeded at its centre with 1000 letters its halves take 6.4 MiB together and the pair
    aligns; the unseeded extension is refused; so is the bare centre point, whose halves take 9 MiB."""
    env = dict(os.environ, SA_TRACE_ARENA_BYTES=str(BIG_BUDGET))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "big"], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    child = json.loads(out.stdout.strip().splitlines()[-1])
    assert child["unseeded_error"] == 4 and child["bare_error"] == 4  # SA_ERR_UNSUPPORTED
    assert "halves" in child["bare_message"]
    plan = subprocess.run([os.path.join(PKG, "bin", "sa_trace_plan_check"), "--mode", "global", "--gap", "11", "--gap-extend", "2",
                           "--budget", str(BIG_BUDGET), "--seeds", "%d:%d:%d" % BIG_SEED, f"{BIG}x{BIG}"], capture_output=True, text=True, check=True)
    plan = json.loads(plan.stdout)
    assert child["arena_bytes"] == plan["arena_bytes"] == sum(it["dir_bytes"] for it in plan["items"]) < BIG_BUDGET
    assert child["num_chunks"] == 1
    t, p = big_pair()
    want = cached_ref("big", t, p, BIG_SEED, matrix("blast", 4), 11, 2, NONE)
    assert child["result"] == pick(want)
    assert child["score"] == list(fields(want))
    assert want["num_bytes"] > 5000  # both halves were walked a long way


# ---- 7. reruns, empties, refusals ---------------------------------------------------------------------------------
@gpu
def test_a_scorer_runs_again_on_new_arena_contents(eng):
    import torch
    S = matrix("blast", 4)
    cases = library_cases(40, 74400)
    seeds = [c[2] for c in cases]
    to = np.concatenate([[0], np.cumsum([len(c[0]) for c in cases])])
    po = np.concatenate([[0], np.cumsum([len(c[1]) for c in cases])])
    pairs = [(int(to[k]), len(c[0]), int(po[k]), len(c[1])) for k, c in enumerate(cases)]
    sc = eng.Scorer(GLOBAL, S, 11, pairs, gap_extend=2, xdrop=20, seeds=seeds)
    ht, hp = np.concatenate([c[0] for c in cases]), np.concatenate([c[1] for c in cases])
    dt, dp = torch.from_numpy(ht).cuda(), torch.from_numpy(hp).cuda()
    sc.run(dt.data_ptr(), dp.data_ptr())
    first = sc.results().copy()
    assert [fields(g) for g in first] == [fields(seeds_ref(t, p, sd, S, 11, 2, 20)) for t, p, sd in cases]
    # new contents in the same arenas: the same shapes and seeds, other letters
    ht2 = synthetic.random_sequence(7, len(ht), 4).astype(np.int8)
    hp2 = np.concatenate([synthetic.mutate(np.resize(ht2[to[k]:to[k + 1]], int(po[k + 1] - po[k])), 7700 + k, 4, int(po[k + 1] - po[k]))
                          for k in range(len(cases))]).astype(np.int8)
    dt.copy_(torch.from_numpy(ht2))
    dp.copy_(torch.from_numpy(hp2))
    sc.run(dt.data_ptr(), dp.data_ptr())
    second = sc.results().copy()
    sc.run(dt.data_ptr(), dp.data_ptr())
    third = sc.results().copy()
    sc.close()
    want = [fields(seeds_ref(ht2[to[k]:to[k + 1]], hp2[po[k]:po[k + 1]], sd, S, 11, 2, 20)) for k, sd in enumerate(seeds)]
    assert [fields(g) for g in second] == want and second.tobytes() == third.tobytes()
    assert first.tobytes() != second.tobytes()


@gpu
def test_empty_calls_and_empty_sides(eng):
    S = matrix("blast", 4)
    x, none = synthetic.random_sequence(1, 50, 4).astype(np.int8), np.zeros(0, dtype=np.int8)
    for xdrop in (eng.NO_XDROP, 0, 20):
        assert eng.align_pairs_affine(GLOBAL, [], [], S, 11, 2, xdrop=xdrop, seeds=[]) == []
        got = eng.score_batch(GLOBAL, [], [], S, 11, gap_extend=2, xdrop=xdrop, seeds=[])
        assert len(got) == 0 and got.dtype == eng.SEED_DTYPE
        sc = eng.Scorer(GLOBAL, S, 11, [], gap_extend=2, xdrop=xdrop, seeds=[])
        sc.run(0, 0)
        assert len(sc.results()) == 0 and len(sc.score_results()) == 0
        sc.close()
    texts = [none, x[:5], none, x, x, x]
    patterns = [none, none, x[:5], x[:20], x[:20], x]
    seeds = [(0, 0, 0), (3, 0, 0), (0, 2, 0), (50, 20, 0), (0, 0, 20), (0, 0, 50)]
    for go, ge in GAPS + [(-3, 1)]:
        for xdrop in (NONE, 0, 20):
            wants = [seeds_ref(t, p, sd, S, go, ge, xdrop) for t, p, sd in zip(texts, patterns, seeds)]
            assert [fields(w) for w in wants[:3]] == [(0, 0, 0, 0, 0), (0, 3, 0, 3, 0), (0, 0, 2, 0, 2)]
            assert fields(wants[5]) == (250, 0, 0, 50, 50) and wants[5]["aligned_text"] == wants[5]["aligned_pattern"]
            got = check(eng, texts, patterns, seeds, S, go, ge, xdrop, wants, "empty")
            # an empty result has start = (ts, ps)
            assert [(g["num_bytes"], g["start_text"], g["start_pattern"], g["aligned_text"]) for g in got[:3]] == \
                   [(0, 0, 0, ""), (0, 3, 0, ""), (0, 0, 2, "")]
    got = eng.align_pairs_affine(GLOBAL, [x], [x[:40]], S, 11, 2, strings=False, xdrop=20, seeds=[(10, 10, 5)])[0]
    want = seeds_ref(x, x[:40], (10, 10, 5), S, 11, 2, 20)
    assert got == {k: want[k] for k in KEYS[:4]}
    stats = eng.affine_last_stats()
    # two halves of one strip each, 10 and 35 columns: 64 * floor((n + 126) / 64) = 128 steps of 256 bytes
    assert stats["num_chunks"] == 1 and stats["arena_bytes"] == 2 * 128 * 256


@gpu
def test_refusals(eng):
    S = matrix("blast", 4)
    x = synthetic.random_sequence(1, 50, 4).astype(np.int8)
    y = x[:20]
    sd = [(10, 5, 3)]
    scorer = lambda mode, **kw: eng.Scorer(mode, S, 11, [(0, 50, 0, 20)], gap_extend=2, **kw)  # noqa: E731
    # a band of either kind, and seeds without an xdrop: ValueError in the binding
    for kw in ({"band": 3, "xdrop": 20}, {"bands": [(0, 30)], "xdrop": 20}, {"band": 3}, {"bands": [(0, 30)]}, {}):
        for call in (lambda: eng.score_batch(GLOBAL, [x], [y], S, 11, gap_extend=2, seeds=sd, **kw),
                     lambda: scorer(GLOBAL, seeds=sd, **kw),
                     lambda: eng.align_pairs_affine(GLOBAL, [x], [y], S, 11, 2, seeds=sd, **kw)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        eng.score_batch(GLOBAL, [x], [y], S, 11, gap_extend=2, xdrop=20, seeds=sd * 2)
    # a bad xdrop, and a mode other than global
    for mode, xdrop in ((GLOBAL, -2), (GLOBAL, 1 << 30), (LOCAL, 20), (FIT, 20), (ENDS, 20), (ENDS | 15, eng.NO_XDROP), (3, 20)):
        for call in (lambda: eng.score_batch(mode, [x], [y], S, 11, gap_extend=2, xdrop=xdrop, seeds=sd),
                     lambda: eng.score_batch(mode, [x], [y], S, 5, xdrop=xdrop, seeds=sd),
                     lambda: scorer(mode, xdrop=xdrop, seeds=sd),
                     lambda: eng.align_pairs_affine(mode, [x], [y], S, 11, 2, xdrop=xdrop, seeds=sd)):
            with pytest.raises(eng.SaError) as e:
                call()
            assert e.value.code == 1, (mode, xdrop)
    # a seed outside its pair: the first such pair's index is in the message
    for bad in ((48, 0, 3), (0, 18, 3), (51, 0, 0), (0, 21, 0), (0, 0, 21), (1 << 40, 0, 0)):
        for call in (lambda: eng.score_batch(GLOBAL, [x, x, x], [y, y, y], S, 11, gap_extend=2, xdrop=20, seeds=[(0, 0, 0), bad, bad]),
                     lambda: eng.Scorer(GLOBAL, S, 11, [(0, 50, 0, 20)] * 3, gap_extend=2, xdrop=20, seeds=[(0, 0, 0), bad, bad]),
                     lambda: eng.align_pairs_affine(GLOBAL, [x, x, x], [y, y, y], S, 11, 2, xdrop=20, seeds=[(0, 0, 0), bad, bad])):
            with pytest.raises(eng.SaError) as e:
                call()
            assert e.value.code == 1 and "pair 1" in str(e.value), bad
    assert fields(eng.score_batch(GLOBAL, [x], [y], S, 11, gap_extend=2, xdrop=20, seeds=[(47, 17, 3)])[0]) == \
        fields(seeds_ref(x, y, (47, 17, 3), S, 11, 2, 20))
    # over the score limit of the whole pair
    for call in (lambda: eng.score_batch(GLOBAL, [x], [y], S, 1 << 23, gap_extend=2, xdrop=20, seeds=sd),
                 lambda: eng.align_pairs_affine(GLOBAL, [x], [y], S, 1 << 23, 2, xdrop=20, seeds=sd)):
        with pytest.raises(eng.SaError) as e:
            call()
        assert e.value.code == 4  # SA_ERR_UNSUPPORTED
    # an out-of-alphabet byte in the left half, inside the seed and in the right half, on either side
    for where in (3, 11, 30):
        bad = x.copy()
        bad[where] = 4
        for tt, pp, s2 in (([bad, x], [y, y], [(10, 5, 3), (10, 5, 3)]), ([x, x], [y, bad[:40]], [(10, 5, 3), (20, where - 1, 3)])):
            for call in (lambda: eng.score_batch(GLOBAL, tt, pp, S, 11, gap_extend=2, xdrop=eng.NO_XDROP, seeds=s2),
                         lambda: eng.score_batch(GLOBAL, tt, pp, S, 5, xdrop=eng.NO_XDROP, seeds=s2),
                         lambda: eng.align_pairs_affine(GLOBAL, tt, pp, S, 11, 2, xdrop=eng.NO_XDROP, seeds=s2)):
                with pytest.raises(eng.SaError) as e:
                    call()
                assert e.value.code == 1, where
    # null arguments
    p, S_keep, alpha_keep = eng._params(GLOBAL, S, 0, None, 0)
    res = (eng.SaResult * 1)()
    out = np.zeros(1, eng.SEED_DTYPE)
    hp = (eng.SaHostPair * 1)(eng.SaHostPair(x.ctypes.data, 50, y.ctypes.data, 20))
    dpair = (eng.SaPair * 1)(eng.SaPair(0, 50, 0, 20))
    s1 = np.array([[10, 5, 3]], dtype=np.uint64)
    buf = ctypes.create_string_buffer(100)
    one = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    h = ctypes.c_void_p()
    L = eng.lib
    P = ctypes.byref(p)
    assert L.sa_align_pairs_seeds(P, 11, 2, 20, s1.ctypes.data, hp, 1, 0, res, None, None) == 0
    assert L.sa_align_pairs_seeds(None, 11, 2, 20, s1.ctypes.data, hp, 1, 0, res, None, None) == 1
    assert L.sa_align_pairs_seeds(P, 11, 2, 20, None, hp, 1, 0, res, None, None) == 1
    assert "seeds" in L.sa_last_error().decode()
    assert L.sa_align_pairs_seeds(P, 11, 2, 20, s1.ctypes.data, None, 1, 0, res, None, None) == 1
    assert L.sa_align_pairs_seeds(P, 11, 2, 20, s1.ctypes.data, hp, 1, 0, None, None, None) == 1
    assert L.sa_align_pairs_seeds(P, 11, 2, 20, s1.ctypes.data, hp, 1, 0, res, one, None) == 1
    assert L.sa_align_pairs_seeds(P, 11, 2, 20, s1.ctypes.data, hp, -1, 0, res, None, None) == 1
    assert L.sa_align_pairs_seeds(P, 11, 2, 20, None, None, 0, 0, None, None, None) == 0  # zero pairs read nothing
    assert L.sa_score_batch_seeds(P, 11, 2, 20, s1.ctypes.data, hp, 1, 0, out.ctypes.data) == 0
    assert L.sa_score_batch_seeds(None, 11, 2, 20, s1.ctypes.data, hp, 1, 0, out.ctypes.data) == 1
    assert L.sa_score_batch_seeds(P, 11, 2, 20, None, hp, 1, 0, out.ctypes.data) == 1
    assert L.sa_score_batch_seeds(P, 11, 2, 20, s1.ctypes.data, None, 1, 0, out.ctypes.data) == 1
    assert L.sa_score_batch_seeds(P, 11, 2, 20, s1.ctypes.data, hp, 1, 0, None) == 1
    assert L.sa_score_batch_seeds(P, 11, 2, 20, s1.ctypes.data, hp, -1, 0, out.ctypes.data) == 1
    assert L.sa_score_batch_seeds(P, 11, 2, 20, None, None, 0, 0, None) == 0
    assert L.sa_scorer_create_seeds(P, 11, 2, 20, None, dpair, 1, 0, ctypes.byref(h)) == 1
    assert L.sa_scorer_create_seeds(P, 11, 2, 20, s1.ctypes.data, None, 1, 0, ctypes.byref(h)) == 1
    assert L.sa_scorer_create_seeds(P, 11, 2, 20, s1.ctypes.data, dpair, 1, 0, None) == 1
    assert L.sa_scorer_create_seeds(None, 11, 2, 20, s1.ctypes.data, dpair, 1, 0, ctypes.byref(h)) == 1
    # sa_scorer_fetch_seeds: a seeds scorer that has run, and no other scorer
    assert L.sa_scorer_create_seeds(P, 11, 2, 20, s1.ctypes.data, dpair, 1, 0, ctypes.byref(h)) == 0
    assert L.sa_scorer_fetch_seeds(h, out.ctypes.data, None) == 1  # not run yet
    assert L.sa_scorer_destroy(h) == 0
    assert L.sa_scorer_fetch_seeds(None, out.ctypes.data, None) == 1
    other = eng.Scorer(GLOBAL, S, 11, [(0, 50, 0, 20)], gap_extend=2, xdrop=20)
    assert L.sa_scorer_fetch_seeds(other.handle, out.ctypes.data, None) == 1
    other.close()


# ---- 8. the C++ functions ---------------------------------------------------------------------------------------------
@gpu
def test_cpp_seeds_check():
    out = subprocess.run([os.path.join(PKG, "bin", "sa_seeds_check"), "700", "96"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1] == "OK 96"


if __name__ == "__main__" and sys.argv[1:] == ["big"]:
    # the child of test_a_seeded_pair_beyond_the_arena_budget_aligns
    from sa_amd import engine as eng

    S = matrix("blast", 4)
    t, p = big_pair()
    errors = {}
    for name, kw in (("unseeded", {}), ("bare", {"seeds": [BIG_BARE]})):
        try:
            eng.align_pairs_affine(GLOBAL, [t], [p], S, 11, 2, xdrop=eng.NO_XDROP, **kw)
            errors[name] = (0, "")
        except eng.SaError as e:
            errors[name] = (e.code, str(e))
    got = eng.align_pairs_affine(GLOBAL, [t], [p], S, 11, 2, xdrop=eng.NO_XDROP, seeds=[BIG_SEED])[0]
    stats = eng.affine_last_stats()
    sc = eng.score_batch(GLOBAL, [t], [p], S, 11, gap_extend=2, xdrop=eng.NO_XDROP, seeds=[BIG_SEED])[0]
    print(json.dumps({"unseeded_error": errors["unseeded"][0], "bare_error": errors["bare"][0], "bare_message": errors["bare"][1],
                      "result": pick(got), "score": [int(sc[f]) for f in FIELDS], "arena_bytes": stats["arena_bytes"],
                      "num_chunks": stats["num_chunks"]}))
