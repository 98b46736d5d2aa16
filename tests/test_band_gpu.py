"""Banded alignment (sa_hip.h: sa_score_batch_banded, sa_scorer_create_banded, sa_align_pairs_banded, and
the C++ functions over them): Gotoh's recurrence inside the diagonal band lo <= j - i <= hi,
lo = min(0, n - m) - w, hi = max(0, n - m) + w, every other cell minus infinity in H, E and F.
The reference of this file is band_ref: a banded fill by anti-diagonals in numpy (int64, out-of-band
cells forced to a far minus infinity) with the walk of test_align_affine_gpu. It is pinned on the CPU
against a plain double loop, against affine_ref where the band admits every cell, and by re-scoring its
strings; the GPU is then compared with it: score, end cell, result fields and both strings."""
from __future__ import annotations

import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, encode, matrix  # first: it puts oracle/ and the package on the path

from sa_amd import synthetic
from test_align_affine_gpu import (DIAG, EDGE_SHAPES, EEXT, FEXT, KEYS, LEFT, NEG, STOP, TOP, affine_ref, alphabet_of,
                                   gap_runs, many_pairs, pick, rescore, walk, with_blocks)
from test_score_gpu import related_pair

gpu = pytest.mark.gpu

GLOBAL, LOCAL, FIT = 0, 1, 2
GAPS = [(11, 2), (3, 1), (5, 5)]
SCHEMES = [(4, "blast"), (23, "blosum50")]


# ---- the reference of this file ------------------------------------------------------------------------
def band_limits(n, m, w):
    d = n - m
    return min(0, d) - w, max(0, d) + w


def band_fill_by_diagonals(mode, t, p, S, go, ge, w):
    """(H, D) of the banded recurrence swept by anti-diagonals, only over the in-band cells of each;
    every out-of-band cell, border cells included, is NEG in H, E and F. D as
    test_align_affine_gpu.nibbles_by_diagonals has it."""
    t, p, S = np.asarray(t, dtype=np.int64), np.asarray(p, dtype=np.int64), np.asarray(S, dtype=np.int64)
    n, m = len(t), len(p)
    lo, hi = band_limits(n, m, w)
    local = mode == LOCAL
    H = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    E = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    F = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    D = np.zeros((m + 1, n + 1), dtype=np.uint8)
    H[0, 0] = 0
    jb, ib = np.arange(1, min(n, hi) + 1), np.arange(1, min(m, -lo) + 1)  # the in-band border cells
    H[0, jb] = 0 if local else -(go + (jb - 1) * ge)
    H[ib, 0] = 0 if local else -(go + (ib - 1) * ge)
    for d in range(2, n + m + 1):
        # i + j = d and lo <= j - i <= hi: (d - hi) / 2 <= i <= (d - lo) / 2
        i = np.arange(max(1, d - n, -((hi - d) // 2)), min(m, d - 1, (d - lo) // 2) + 1)
        if len(i) == 0:
            continue
        j = d - i
        ee, eo = E[i, j - 1] - ge, H[i, j - 1] - go
        fe, fo = F[i - 1, j] - ge, H[i - 1, j] - go
        e, f = np.maximum(ee, eo), np.maximum(fe, fo)
        dg = H[i - 1, j - 1] + S[p[i - 1], t[j - 1]]
        h = np.maximum(dg, np.maximum(e, f))
        src = np.where(dg > np.maximum(e, f), DIAG, np.where(e >= f, LEFT, TOP))
        if local:
            src = np.where(h <= 0, STOP, src)
            h = np.maximum(h, 0)
        D[i, j] = src + EEXT * (ee > eo) + FEXT * (fe > fo)
        H[i, j], E[i, j], F[i, j] = h, e, f
    return H, D


def band_fill_by_loops(mode, t, p, S, go, ge, w):
    """The same as a plain double loop over all cells, the band a test per cell."""
    n, m = len(t), len(p)
    lo, hi = band_limits(n, m, w)
    local = mode == LOCAL
    inb = lambda i, j: lo <= j - i <= hi  # noqa: E731
    H = [[NEG] * (n + 1) for _ in range(m + 1)]
    E = [[NEG] * (n + 1) for _ in range(m + 1)]
    F = [[NEG] * (n + 1) for _ in range(m + 1)]
    D = [[0] * (n + 1) for _ in range(m + 1)]
    H[0][0] = 0
    for j in range(1, n + 1):
        if inb(0, j):
            H[0][j] = 0 if local else -(go + (j - 1) * ge)
    for i in range(1, m + 1):
        if inb(i, 0):
            H[i][0] = 0 if local else -(go + (i - 1) * ge)
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            if not inb(i, j):
                continue
            ee, eo, fe, fo = E[i][j - 1] - ge, H[i][j - 1] - go, F[i - 1][j] - ge, H[i - 1][j] - go
            E[i][j], F[i][j] = max(ee, eo), max(fe, fo)
            dg = H[i - 1][j - 1] + int(S[p[i - 1]][t[j - 1]])
            h = max(dg, E[i][j], F[i][j])
            src = DIAG if dg > max(E[i][j], F[i][j]) else LEFT if E[i][j] >= F[i][j] else TOP
            if local and h <= 0:
                src = STOP
            D[i][j] = src + (EEXT if ee > eo else 0) + (FEXT if fe > fo else 0)
            H[i][j] = max(h, 0) if local else h
    return np.array(H, dtype=np.int64), np.array(D, dtype=np.uint8)


def band_ref(mode, t, p, S, go, ge, w, alphabet=None):
    """The banded alignment: the keys of align_pairs_affine plus end_text and end_pattern of the scorers
    and `inside`, whether every cell of the walk lies in the band."""
    t, p = np.asarray(t, dtype=np.int64), np.asarray(p, dtype=np.int64)
    n, m = len(t), len(p)
    H, D = band_fill_by_diagonals(mode, t, p, S, go, ge, w)
    res, _ = walk(mode, t, p, H, D, go, ge, alphabet or alphabet_of(S))
    if mode == LOCAL:
        i, j = (0, 0) if H.max() <= 0 else (int(v) for v in np.unravel_index(int(H.argmax()), H.shape))
    else:
        i, j = m, n
    res["end_pattern"], res["end_text"] = i, j
    # the cells of the walk, read back from the strings
    lo, hi = band_limits(n, m, w)
    inside = lo <= j - i <= hi
    for a, b in zip(reversed(res["aligned_text"]), reversed(res["aligned_pattern"])):
        j, i = j - (a != "-"), i - (b != "-")
        inside = inside and lo <= j - i <= hi
    res["inside"] = inside
    return res


_REF = {}


def ref_cached(key, *args):
    """band_ref once per case, shared by the tests that meet the case again, and never changed."""
    if key not in _REF:
        _REF[key] = band_ref(*args)
    return _REF[key]


def cell(r):
    return (int(r["score"]), int(r["end_pattern"]), int(r["end_text"]))


def check(eng, mode, texts, patterns, S, go, ge, w, wants, what, Rs=(1, 2, 4, 8)):
    """Every forced rows_per_lane of the banded scorer, and the banded aligner."""
    for R in Rs:
        got = eng.score_batch(mode, texts, patterns, S, go, rows_per_lane=R, gap_extend=ge, band=w)
        assert [cell(g) for g in got] == [cell(x) for x in wants], (what, "score", mode, w, R)
    got = eng.align_pairs_affine(mode, texts, patterns, S, go, ge, band=w)
    for k, (g, x) in enumerate(zip(got, wants)):
        assert pick(g) == pick(x), (what, "align", mode, w, k, len(patterns[k]), len(texts[k]))


# ---- 1. the reference of this file is sound (CPU) ------------------------------------------------------
def random_small_pairs(count, seed, nmax=40):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        A = 4 if k % 2 else 23
        n, m = int(rng.integers(1, nmax + 1)), int(rng.integers(1, nmax + 1))
        out.append((A,) + related_pair(seed + 10 * k, n, m, A))
    return out


def test_band_ref_equals_the_plain_loops():
    for k, (A, t, p) in enumerate(random_small_pairs(60, 5100)):
        S = matrix("blast" if A == 4 else "blosum50", A)
        go, ge = ((11, 1), (5, 5), (4, 0), (3, 7), (-2, -1))[k % 5]
        for w in (0, 1, 3, 9):
            for mode in (GLOBAL, LOCAL):
                H1, D1 = band_fill_by_diagonals(mode, t, p, S, go, ge, w)
                H2, D2 = band_fill_by_loops(mode, t, p, S, go, ge, w)
                assert (H1 == H2).all() and (D1 == D2).all(), (k, w, mode)
                lo, hi = band_limits(len(t), len(p), w)
                jj, ii = np.meshgrid(np.arange(len(t) + 1), np.arange(len(p) + 1))
                out = (jj - ii < lo) | (jj - ii > hi)
                assert (H1[out] == NEG).all() and (H1[~out] > NEG // 2).all(), (k, w, mode)
                assert not out[0, 0] and not out[len(p), len(t)] and not out[1:, 1:].all(axis=1).any()


def test_band_ref_equals_affine_ref_when_the_band_admits_every_cell():
    for k, (A, t, p) in enumerate(random_small_pairs(40, 6200)):
        S = matrix("blast" if A == 4 else "blosum50", A)
        go, ge = ((11, 1), (5, 5), (4, 0), (0, 0), (-2, -2))[k % 5]
        for mode in (GLOBAL, LOCAL):
            for w in (max(len(t), len(p)), 1000):
                assert pick(band_ref(mode, t, p, S, go, ge, w)) == affine_ref(mode, t, p, S, go, ge), (k, mode, w)


def test_band_ref_strings_rescore_and_stay_inside_the_band():
    for k, (A, t, p) in enumerate(random_small_pairs(40, 7300)):
        S = matrix("blast" if A == 4 else "blosum50", A)
        alpha = alphabet_of(S)
        for go, ge in ((11, 1), (5, 5), (4, 0)):
            for w in (0, 2, 7):
                for mode in (GLOBAL, LOCAL):
                    res = band_ref(mode, t, p, S, go, ge, w)
                    assert rescore(res, S, go, ge, alpha) == res["score"], (k, go, ge, w, mode)
                    assert res["inside"], (k, go, ge, w, mode)
                    assert res["score"] <= affine_ref(mode, t, p, S, go, ge)["score"], (k, go, ge, w, mode)


def test_band_ref_empty_sides():
    S = matrix("blast", 4)
    x, none = synthetic.random_sequence(5, 5, 4), np.zeros(0, dtype=np.int8)
    for w in (0, 3):
        for t, p in ((none, none), (x, none), (none, x)):
            for mode in (GLOBAL, LOCAL):
                assert pick(band_ref(mode, t, p, S, 11, 2, w)) == affine_ref(mode, t, p, S, 11, 2)
    assert cell(band_ref(GLOBAL, x, none, S, 11, 2, 0)) == (-(11 + 4 * 2), 0, 5)


# ---- 2. strip, lane and body edges ---------------------------------------------------------------------------
# (m, n): the shapes of the affine tests, and m = 64 R - 1 and 64 R + 1 for every R beside texts of about that length
SHAPES = EDGE_SHAPES + [(63, 70), (65, 60), (127, 140), (129, 120), (255, 260), (257, 250), (511, 520), (513, 500)]
WIDTHS = [0, 1, 63, 64, 65]


@gpu
@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("go,ge", GAPS)
@pytest.mark.parametrize("A,mat", SCHEMES)
def test_strip_lane_and_body_edges(eng, A, mat, go, ge, w):
    S = matrix(mat, A)
    pairs = [related_pair(9000 + 3 * m + 5 * n + A, n, m, A) for m, n in SHAPES]
    texts, patterns = [t for t, _ in pairs], [p for _, p in pairs]
    for mode in (GLOBAL, LOCAL):
        wants = [ref_cached(("edges", A, mode, go, ge, w) + SHAPES[k], mode, t, p, S, go, ge, w) for k, (t, p) in enumerate(pairs)]
        check(eng, mode, texts, patterns, S, go, ge, w, wants, "edges")


# ---- 3. windows that start past body 0 and end before n ---------------------------------------------------------
WINDOW_SHAPES = [(1500, 1500), (1500, 1300), (1300, 1500)]  # (m, n)


def window_pairs():
    out = []
    for m, n in WINDOW_SHAPES:
        t = synthetic.random_sequence(400 + m + n, max(n, m), 4)
        p = synthetic.mutate(t, 401 + m + n, 4, m)
        out.append((t[:n].astype(np.int8), p.astype(np.int8)))
    return out


@gpu
@pytest.mark.parametrize("mode", [GLOBAL, LOCAL])
def test_windows_inside_the_text(eng, mode):
    S = matrix("blast", 4)
    pairs = window_pairs()
    texts, patterns = [t for t, _ in pairs], [p for _, p in pairs]
    wants = [ref_cached(("windows", mode) + WINDOW_SHAPES[k], mode, t, p, S, 11, 2, 16) for k, (t, p) in enumerate(pairs)]
    check(eng, mode, texts, patterns, S, 11, 2, 16, wants, "windows", Rs=(1, 8))
    # w = 200: at R = 1 and 2 the middle bodies of a window lie wholly in the band and run the plain step
    wants200 = [ref_cached(("windows 200", mode) + WINDOW_SHAPES[k], mode, t, p, S, 11, 2, 200) for k, (t, p) in enumerate(pairs)]
    check(eng, mode, texts, patterns, S, 11, 2, 200, wants200, "windows, plain bodies", Rs=(1, 2))
    # one pair at a time as well: a wave's row buffer then holds nothing of another pair
    for k in range(len(pairs)):
        check(eng, mode, texts[k:k + 1], patterns[k:k + 1], S, 11, 2, 16, wants[k:k + 1], "windows, alone", Rs=(1, 8))


@gpu
@pytest.mark.parametrize("mode", [GLOBAL, LOCAL])
def test_a_band_that_admits_every_cell_is_the_unbanded_call(eng, mode):
    S = matrix("blast", 4)
    pairs = window_pairs()
    texts, patterns = [t for t, _ in pairs], [p for _, p in pairs]
    for R in (1, 8):
        full = eng.score_batch(mode, texts, patterns, S, 11, rows_per_lane=R, gap_extend=2)
        assert eng.score_batch(mode, texts, patterns, S, 11, rows_per_lane=R, gap_extend=2, band=2000).tobytes() == full.tobytes()
    assert eng.align_pairs_affine(mode, texts, patterns, S, 11, 2, band=2000) == eng.align_pairs_affine(mode, texts, patterns, S, 11, 2)
    # a linear caller passes its penalty twice: band without gap_extend
    lin = eng.score_batch(mode, texts, patterns, S, 5, band=2000)
    assert lin.tobytes() == eng.score_batch(mode, texts, patterns, S, 5).tobytes()


# ---- 4. stale boundary rows: more pairs than waves, wide pairs between narrow-band ones ---------------------
def mixed_pairs():
    """9000 short pairs (many_pairs three times over, more than any device's resident waves) with, every
    25th, a pair of 700 to 1500 letters: under a band of 8 a wave's row buffer holds a long pair's rows,
    far right of what the next short pair's band admits."""
    texts, patterns = many_pairs()
    texts, patterns = list(texts) * 3, list(patterns) * 3
    rng = np.random.default_rng(99)
    for k in range(0, len(texts), 25):
        n = int(rng.integers(700, 1501))
        t = synthetic.random_sequence(7000 + k, n, 4)
        m = n + int(rng.integers(-6, 7))
        texts[k], patterns[k] = t.astype(np.int8), synthetic.mutate(np.resize(t, m), 7001 + k, 4, m).astype(np.int8)
    return texts, patterns


def digest(rows):
    return hashlib.sha256(json.dumps(rows).encode()).hexdigest()


@gpu
@pytest.mark.parametrize("mode", [GLOBAL, LOCAL])
def test_pairs_outnumber_waves_and_reruns(eng, mode):
    import torch
    S = matrix("blast", 4)
    go, ge, w = 9, 1, 8
    texts, patterns = mixed_pairs()
    to = np.concatenate([[0], np.cumsum([len(t) for t in texts])])
    po = np.concatenate([[0], np.cumsum([len(p) for p in patterns])])
    dt, dp = torch.from_numpy(np.concatenate(texts)).cuda(), torch.from_numpy(np.concatenate(patterns)).cuda()
    sc = eng.Scorer(mode, S, go, [(int(to[k]), len(texts[k]), int(po[k]), len(patterns[k])) for k in range(len(texts))],
                    gap_extend=ge, band=w)
    assert sc.info()["num_waves"] < len(texts)
    sc.run(dt.data_ptr(), dp.data_ptr())
    first = sc.results().copy()
    sc.run(dt.data_ptr(), dp.data_ptr())
    second = sc.results().copy()
    sc.close()
    assert digest(first.tolist()) == digest(second.tolist())
    assert first.tolist() == eng.score_batch(mode, texts, patterns, S, go, gap_extend=ge, band=w).tolist()
    got = eng.align_pairs_affine(mode, texts, patterns, S, go, ge, band=w)
    assert [g["score"] for g in got] == first["score"].tolist()
    rng = np.random.default_rng(4)
    for k in list(range(0, len(texts), 375)) + rng.choice(len(texts), 120, replace=False).tolist():
        want = band_ref(mode, texts[k], patterns[k], S, go, ge, w)
        assert cell(first[k]) == cell(want) and pick(got[k]) == pick(want), int(k)
    again = eng.align_pairs_affine(mode, texts, patterns, S, go, ge, band=w)
    assert digest([[r[k] for k in KEYS] for r in again]) == digest([[r[k] for k in KEYS] for r in got])


# ---- 5. the band binds ------------------------------------------------------------------------------------------
def test_the_global_pair_needs_more_than_its_band():
    """The premise of the next test, on the CPU: the unbanded optimum takes a 40-letter insertion and
    later a 40-letter deletion; at w = 16 the banded optimum is strictly lower."""
    S = matrix("blosum50", 23)
    t, p = with_blocks(150, 300, row_cut=80, col_cut=200)
    assert len(t) == len(p) == 340
    full = affine_ref(GLOBAL, t, p, S, 11, 1)
    banded = ref_cached(("binds", GLOBAL), GLOBAL, t, p, S, 11, 1, 16)
    assert gap_runs(full) == [40, 40]
    assert banded["score"] < full["score"] and banded["inside"]
    assert pick(band_ref(GLOBAL, t, p, S, 11, 1, 40)) == full  # the detour is 40 diagonals wide


@gpu
def test_the_band_binds_global(eng):
    S = matrix("blosum50", 23)
    t, p = with_blocks(150, 300, row_cut=80, col_cut=200)
    banded = ref_cached(("binds", GLOBAL), GLOBAL, t, p, S, 11, 1, 16)
    assert banded["score"] < affine_ref(GLOBAL, t, p, S, 11, 1)["score"]
    check(eng, GLOBAL, [t], [p], S, 11, 1, 16, [banded], "binds")
    wide = eng.align_pairs_affine(GLOBAL, [t], [p], S, 11, 1, band=40)[0]
    assert pick(wide) == affine_ref(GLOBAL, t, p, S, 11, 1)  # the detour is 40 diagonals wide


def local_pair_off_the_diagonal():
    """A 60-letter match far off the main diagonal (text letters 150.., pattern letters 20..: diagonal 130)
    and a 25-letter one on diagonal 5, in junk that matches nothing."""
    big, small = synthetic.random_sequence(31, 60, 2), synthetic.random_sequence(32, 25, 2)  # letters 0, 1
    t, p = np.full(300, 2, dtype=np.int8), np.full(300, 3, dtype=np.int8)
    t[150:210], p[20:80] = big, big
    t[105:130], p[100:125] = small, small
    return t, p


def test_the_local_best_cell_lies_outside_the_band():
    S = matrix("blast", 4)
    t, p = local_pair_off_the_diagonal()
    full = affine_ref(LOCAL, t, p, S, 11, 2)
    banded = ref_cached(("binds", LOCAL), LOCAL, t, p, S, 11, 2, 16)
    assert full["score"] == 5 * 60 and banded["score"] == 5 * 25 < full["score"]
    assert (banded["end_pattern"], banded["end_text"]) == (125, 130) and banded["inside"]


@gpu
def test_the_band_binds_local(eng):
    S = matrix("blast", 4)
    t, p = local_pair_off_the_diagonal()
    banded = ref_cached(("binds", LOCAL), LOCAL, t, p, S, 11, 2, 16)
    assert banded["score"] < affine_ref(LOCAL, t, p, S, 11, 2)["score"]
    check(eng, LOCAL, [t], [p], S, 11, 2, 16, [banded], "binds")
    # two equal in-band maxima: the earlier row wins, as without a band
    t2, p2 = t.copy(), p.copy()
    t2[205:230], p2[200:225] = t[105:130], p[100:125]
    want = band_ref(LOCAL, t2, p2, S, 11, 2, 16)
    assert (want["score"], want["end_pattern"], want["end_text"]) == (125, 125, 130)
    check(eng, LOCAL, [t2], [p2], S, 11, 2, 16, [want], "two maxima")
    # no positive in-band cell: the only matches lie outside
    t3, p3 = t.copy(), p.copy()
    t3[105:130] = 2
    want = band_ref(LOCAL, t3, p3, S, 11, 2, 16)
    assert cell(want) == (0, 0, 0) and want["num_bytes"] == 0
    check(eng, LOCAL, [t3], [p3], S, 11, 2, 16, [want], "nothing positive")


# ---- 6. negative and zero penalties -------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("go,ge", [(3, 7), (0, 0), (-2, -2), (-2, -1), (4, 0)])
def test_negative_and_zero_penalties(eng, go, ge):
    S = matrix("blast", 4)
    shapes = [(9, 65), (64, 70), (129, 120), (513, 500), (300, 700)]
    pairs = [related_pair(1200 + 3 * m + 5 * n, n, m, 4) for m, n in shapes]
    texts, patterns = [t for t, _ in pairs], [p for _, p in pairs]
    for w in (0, 5, 64):
        for mode in (GLOBAL, LOCAL):
            wants = [band_ref(mode, t, p, S, go, ge, w) for t, p in pairs]
            check(eng, mode, texts, patterns, S, go, ge, w, wants, "penalties")


# ---- 7. beyond the arena budget -----------------------------------------------------------------------------------
BIG, BIG_W, BIG_BUDGET = 6000, 100, 8 << 20


def big_pair():
    t = synthetic.random_sequence(61, BIG, 4)
    return t.astype(np.int8), synthetic.mutate(t, 62, 4, BIG).astype(np.int8)


def planned_bytes(n, m, w, budget):
    out = subprocess.run([os.path.join(PKG, "bin", "sa_trace_plan_check"), "--mode", "global", "--gap", "11", "--gap-extend", "2",
                          "--budget", str(budget), "--band", str(w), f"{n}x{m}"], capture_output=True, text=True, check=True)
    return json.loads(out.stdout)


@gpu
def test_a_pair_beyond_the_arena_budget_aligns_inside_its_band():
    """In a process of its own (the budget is read once per process): 6000 x 6000 needs 18 MiB of
    directions, the budget is 8 MiB, the band of half-width 100 takes 2.5 MiB."""
    env = dict(os.environ, SA_TRACE_ARENA_BYTES=str(BIG_BUDGET))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "big"], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    child = json.loads(out.stdout.strip().splitlines()[-1])
    assert child["unbanded_error"] == 4  # SA_ERR_UNSUPPORTED
    plan = planned_bytes(BIG, BIG, BIG_W, BIG_BUDGET)
    assert child["arena_bytes"] == plan["arena_bytes"] == plan["pairs"][0]["dir_bytes"] < BIG_BUDGET
    assert child["num_chunks"] == 1
    t, p = big_pair()
    want = band_ref(GLOBAL, t, p, matrix("blast", 4), 11, 2, BIG_W)
    assert child["result"] == pick(want)
    assert child["score"] == [want["score"], BIG, BIG]


# ---- 8. bad input ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("side", ["text", "pattern"])
@pytest.mark.parametrize("A", [4, 23])
def test_out_of_alphabet_byte_is_rejected(eng, side, A):
    S = matrix("blast" if A == 4 else "blosum50", A)
    t, p = related_pair(11, 150, 90, A)
    (t if side == "text" else p)[70] = A
    for call in (lambda: eng.score_batch(GLOBAL, [t, t[:10]], [p, p[:10]], S, 11, gap_extend=2, band=70),
                 lambda: eng.align_pairs_affine(LOCAL, [t, t[:10]], [p, p[:10]], S, 11, 2, band=70)):
        with pytest.raises(eng.SaError) as e:
            call()
        assert e.value.code == 1  # SA_ERR_INVALID


@gpu
def test_limits_modes_and_null_arguments(eng):
    S = matrix("blast", 4)
    x = synthetic.random_sequence(1, 50, 4)
    for call in (lambda: eng.score_batch(GLOBAL, [x], [x], S, 11, gap_extend=2, band=-1),
                 lambda: eng.align_pairs_affine(GLOBAL, [x], [x], S, 11, 2, band=-1)):
        with pytest.raises(eng.SaError) as e:
            call()
        assert e.value.code == 1  # SA_ERR_INVALID
    for call in (lambda: eng.score_batch(FIT, [x], [x], S, 11, gap_extend=2, band=5),
                 lambda: eng.Scorer(FIT, S, 11, [(0, 50, 0, 50)], gap_extend=2, band=5),
                 lambda: eng.align_pairs_affine(FIT, [x], [x], S, 11, 2, band=5),
                 lambda: eng.align_pairs_affine(GLOBAL, [x], [x], S, 1 << 24, 2, band=5),   # reaches 2^30
                 lambda: eng.align_pairs_affine(GLOBAL, [x], [x], S, 1 << 22, 2, band=5)):  # reaches 2^29: the band's limit
        with pytest.raises(eng.SaError) as e:
            call()
        assert e.value.code == 4  # SA_ERR_UNSUPPORTED
    assert eng.align_pairs_affine(GLOBAL, [x], [x], S, 1 << 22, 2)[0]["score"] == 250  # the unbanded limit is 2^30
    p, S_keep, alpha_keep = eng._params(GLOBAL, S, 0, None, 0)
    res = (eng.SaResult * 1)()
    out = (eng.SaScoreResult * 1)()
    hp = (eng.SaHostPair * 1)(eng.SaHostPair(x.ctypes.data, 50, x.ctypes.data, 50))
    buf = ctypes.create_string_buffer(100)
    one = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    h = ctypes.c_void_p()
    assert eng.lib.sa_align_pairs_banded(None, 11, 2, 5, hp, 1, 0, res, None, None) == 1
    assert eng.lib.sa_align_pairs_banded(ctypes.byref(p), 11, 2, 5, None, 1, 0, res, None, None) == 1
    assert eng.lib.sa_align_pairs_banded(ctypes.byref(p), 11, 2, 5, hp, 1, 0, None, None, None) == 1
    assert eng.lib.sa_align_pairs_banded(ctypes.byref(p), 11, 2, 5, hp, 1, 0, res, one, None) == 1  # one string side only
    assert eng.lib.sa_align_pairs_banded(ctypes.byref(p), 11, 2, 5, hp, -1, 0, res, None, None) == 1
    assert eng.lib.sa_score_batch_banded(None, 11, 2, 5, hp, 1, 0, out) == 1
    assert eng.lib.sa_score_batch_banded(ctypes.byref(p), 11, 2, 5, None, 1, 0, out) == 1
    assert eng.lib.sa_score_batch_banded(ctypes.byref(p), 11, 2, 5, hp, 1, 0, None) == 1
    assert eng.lib.sa_scorer_create_banded(ctypes.byref(p), 11, 2, 5, None, 1, 0, ctypes.byref(h)) == 1
    assert eng.lib.sa_scorer_create_banded(ctypes.byref(p), 11, 2, 5, None, 0, 0, None) == 1
    hp[0].text = None
    assert eng.lib.sa_align_pairs_banded(ctypes.byref(p), 11, 2, 5, hp, 1, 0, res, None, None) == 1
    assert eng.lib.sa_score_batch_banded(ctypes.byref(p), 11, 2, 5, hp, 1, 0, out) == 1
    # a sequence over the length limit
    with pytest.raises(eng.SaError) as e:
        eng.Scorer(GLOBAL, S, 11, [(0, 1 << 24, 0, 50)], gap_extend=2, band=5)
    assert e.value.code == 4
    # zero pairs, empty sides, and results without strings
    assert eng.align_pairs_affine(GLOBAL, [], [], S, 11, 2, band=3) == []
    assert len(eng.score_batch(GLOBAL, [], [], S, 11, gap_extend=2, band=3)) == 0
    none = np.zeros(0, dtype=np.int8)
    for mode in (GLOBAL, LOCAL):
        texts, patterns = [none, x[:5], none, x[:1]], [none, none, x[:5], x[1:2]]
        wants = [band_ref(mode, t, q, S, 11, 2, 0) for t, q in zip(texts, patterns)]
        check(eng, mode, texts, patterns, S, 11, 2, 0, wants, "empty")
    got = eng.align_pairs_affine(GLOBAL, [x], [x[:40]], S, 11, 2, strings=False, band=4)[0]
    want = band_ref(GLOBAL, x, x[:40], S, 11, 2, 4)
    assert got == {k: want[k] for k in KEYS[:4]}


# ---- 9. the C++ functions --------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["global", "local"])
def test_cpp_band_check(mode):
    out = subprocess.run([os.path.join(PKG, "bin", "sa_band_check"), mode, "700", "96"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1] == "OK 96"


if __name__ == "__main__" and sys.argv[1:] == ["big"]:
    # the child of test_a_pair_beyond_the_arena_budget_aligns_inside_its_band
    from sa_amd import engine
    S_ = matrix("blast", 4)
    t_, p_ = big_pair()
    try:
        engine.align_pairs_affine(GLOBAL, [t_], [p_], S_, 11, 2)
        code = 0
    except engine.SaError as err:
        code = err.code
    res_ = engine.align_pairs_affine(GLOBAL, [t_], [p_], S_, 11, 2, band=BIG_W)[0]
    stats = engine.affine_last_stats()
    sc_ = engine.score_batch(GLOBAL, [t_], [p_], S_, 11, gap_extend=2, band=BIG_W)[0]
    print(json.dumps({"unbanded_error": code, "result": pick(res_), "arena_bytes": stats["arena_bytes"],
                      "num_chunks": stats["num_chunks"], "score": [int(sc_["score"]), int(sc_["end_pattern"]), int(sc_["end_text"])]}))
