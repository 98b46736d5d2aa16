"""Extension alignment (sa_hip.h: sa_score_batch_extend, sa_scorer_create_extend, sa_align_pairs_extend):
the alignment starts at the origin, ends at the best interior cell of the rows before the stop row i*, and
i* is the first row whose best lies more than xdrop below the best of the rows before it (B(0) = 0).
The reference of this file is extend_ref: test_align_affine_gpu's numpy fill by anti-diagonals in global
mode, the row maxima, B and i* read from the whole matrix, the first maximum in row-major order over rows
< i*, and test_align_affine_gpu's walk on the prefixes the result cell cuts. It is pinned on the CPU against
a plain double loop that computes r, B and i* row by row, by re-scoring its strings and by the identities of
sa_hip.h; the GPU is then compared with it, every forced rows_per_lane of the scorer and the aligner."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, matrix  # first: it puts oracle/ and the package on the path

from sa_amd import synthetic
from test_align_affine_gpu import (EDGE_SHAPES, KEYS, NEG, alphabet_of, many_pairs, nibbles_by_diagonals, pick, rescore,
                                   walk)
from test_band_gpu import digest
from test_ends_gpu import ends_ref
from test_fit_gpu import cell
from test_score_gpu import related_pair

gpu = pytest.mark.gpu

GLOBAL, LOCAL, FIT = 0, 1, 2
ENDS, TE, PE = 16, 2, 8
NONE = None  # no X-drop: engine.NO_XDROP
GAPS = [(11, 2), (5, 5)]


# ---- the reference of this file ------------------------------------------------------------------------
_FILLS = {}  # (key, go, ge) -> (H, D): the newest few are kept; the fill does not depend on the X-drop


def global_fill(t, p, S, go, ge, key=None):
    fk = (key, go, ge)
    if key is None or fk not in _FILLS:
        H, D = nibbles_by_diagonals(GLOBAL, t, p, S, go, ge)
        if key is None:
            return H, D
        while len(_FILLS) >= 12:
            _FILLS.pop(next(iter(_FILLS)))
        _FILLS[fk] = (H, D)
    return _FILLS[fk]


def stop_row(H, xdrop):
    """i* of sa_hip.h from the whole matrix: the smallest i with B(i - 1) - r(i) > xdrop, else m + 1."""
    m = H.shape[0] - 1
    if xdrop is NONE or H.shape[1] < 2:
        return m + 1
    r = H[1:, 1:].max(axis=1)
    B = np.maximum.accumulate(np.concatenate([[0], r]))  # B[i], i = 0..m
    drops = np.nonzero(B[:-1] - r > xdrop)[0]
    return int(drops[0]) + 1 if len(drops) else m + 1


def extend_ref(t, p, S, go, ge, xdrop, alphabet=None, key=None):
    """The keys of align_pairs_affine plus end_pattern and end_text of the scorers and stop_row."""
    t, p = np.asarray(t, dtype=np.int64), np.asarray(p, dtype=np.int64)
    n, m = len(t), len(p)
    alphabet = alphabet or alphabet_of(S)
    bi = bj = 0
    istar = m + 1
    if n and m:
        H, D = global_fill(t, p, S, go, ge, key)
        istar = stop_row(H, xdrop)
        sub = H[1:istar, 1:]
        if sub.size and sub.max() > 0:
            bi, bj = (int(v) + 1 for v in np.unravel_index(int(sub.argmax()), sub.shape))  # first maximum, row-major
    else:
        H, D = np.zeros((m + 1, n + 1), dtype=np.int64), np.zeros((m + 1, n + 1), dtype=np.uint8)
    # the global walk of the prefixes: from (bi, bj) in state H to the origin; the fill of a prefix pair is
    # the corner of the whole fill
    res, ended = walk(GLOBAL, t[:bj], p[:bi], H[:bi + 1, :bj + 1], D[:bi + 1, :bj + 1], go, ge, alphabet)
    assert ended == "origin"
    res["start_text"] = res["start_pattern"] = 0  # no quirks
    res["end_pattern"], res["end_text"], res["stop_row"] = bi, bj, istar
    assert res["score"] == (int(H[bi, bj]) if bi else 0)
    return res


def extend_by_loops(t, p, S, go, ge, xdrop):
    """(score, end_pattern, end_text, i*) by a plain double loop, r, B and i* row by row; the rows from i* on
    are not even computed."""
    n, m = len(t), len(p)
    if n == 0 or m == 0:
        return 0, 0, 0, m + 1
    Hup = [0] + [-(go + (j - 1) * ge) for j in range(1, n + 1)]
    F = [NEG] * (n + 1)
    B, best, bi, bj = 0, 0, 0, 0
    for i in range(1, m + 1):
        Hrow = [-(go + (i - 1) * ge)] + [0] * n
        E = NEG
        for j in range(1, n + 1):
            E = max(E - ge, Hrow[j - 1] - go)
            F[j] = max(F[j] - ge, Hup[j] - go)
            Hrow[j] = max(Hup[j - 1] + int(S[p[i - 1]][t[j - 1]]), E, F[j])
        r = max(Hrow[1:])
        if xdrop is not NONE and B - r > xdrop:
            return best, bi, bj, i
        B = max(B, r)
        if r > best:  # strictly greater: the earlier row keeps a tie; the first column of the row's maximum
            best, bi, bj = r, i, 1 + Hrow[1:].index(r)
        Hup = Hrow
    return best, bi, bj, m + 1


def xd(eng, xdrop):
    return eng.NO_XDROP if xdrop is NONE else xdrop


def check(eng, texts, patterns, S, go, ge, xdrop, wants, what, Rs=(1, 2, 4, 8)):
    """Every forced rows_per_lane of the extension scorer (the linear kernels too when go == ge through
    gap_extend=None), and the extension aligner."""
    for R in Rs:
        got = eng.score_batch(GLOBAL, texts, patterns, S, go, rows_per_lane=R, gap_extend=ge, xdrop=xd(eng, xdrop))
        assert [cell(g) for g in got] == [cell(x) for x in wants], (what, "score", go, ge, xdrop, R)
        if go == ge:
            got = eng.score_batch(GLOBAL, texts, patterns, S, go, rows_per_lane=R, xdrop=xd(eng, xdrop))
            assert [cell(g) for g in got] == [cell(x) for x in wants], (what, "score, gap_extend=None", go, xdrop, R)
    got = eng.align_pairs_affine(GLOBAL, texts, patterns, S, go, ge, xdrop=xd(eng, xdrop))
    for k, (g, x) in enumerate(zip(got, wants)):
        assert pick(g) == pick(x), (what, "align", go, ge, xdrop, k, len(patterns[k]), len(texts[k]))
    return got


# ---- 1. the reference of this file is sound (CPU) ------------------------------------------------------
SMALL_GAPS = ((11, 1), (5, 5), (4, 0), (3, 7), (-2, -1))
SMALL_X = (0, 3, 20, NONE)


def random_small_pairs(count=60, seed=51100, nmax=40):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        A = 4 if k % 2 else 23
        n, m = int(rng.integers(1, nmax + 1)), int(rng.integers(1, nmax + 1))
        t, p = related_pair(seed + 10 * k, n, m, A)
        if k % 3 == 0:
            # a tail of unrelated letters: the chimeric read an X-drop is for
            cut = int(rng.integers(0, m + 1))
            p = np.concatenate([p[:cut], synthetic.random_sequence(seed + 10 * k + 5, m - cut, 20 if A == 23 else A)]).astype(p.dtype)
        out.append((A, t, p))
    return out


def test_the_diagonal_fill_equals_the_plain_loops():
    for k, (A, t, p) in enumerate(random_small_pairs()):
        S = matrix("blast" if A == 4 else "blosum50", A)
        for go, ge in SMALL_GAPS:
            for x in SMALL_X:
                want = extend_by_loops(t, p, S, go, ge, x)
                got = extend_ref(t, p, S, go, ge, x)
                assert cell(got) + (got["stop_row"],) == want, (k, go, ge, x)


def test_identities_1_and_2_on_the_reference():
    from test_align_affine_gpu import affine_ref
    stopped = changed = cases = 0
    for k, (A, t, p) in enumerate(random_small_pairs()):
        S = matrix("blast" if A == 4 else "blosum50", A)
        alpha = alphabet_of(S)
        for go, ge in SMALL_GAPS:
            full = extend_ref(t, p, S, go, ge, NONE)
            last = None
            for x in SMALL_X:
                res = extend_ref(t, p, S, go, ge, x)
                # the strings re-score to the score where rescore's reading of them is the recurrence's: a run
                # of k gap letters is one gap (extending is no dearer than opening anew, penalties >= 0)
                if 0 <= ge <= go:
                    assert rescore(res, S, go, ge, alpha) == res["score"], (k, go, ge, x)
                # the walk ended at the origin: the strings hold the prefixes the end cell cuts
                assert res["aligned_text"].replace("-", "") == "".join(alpha[c] for c in t[:res["end_text"]])
                assert res["aligned_pattern"].replace("-", "") == "".join(alpha[c] for c in p[:res["end_pattern"]])
                assert (res["start_text"], res["start_pattern"]) == (0, 0)
                # I1: the global alignment of the prefixes
                g = affine_ref(GLOBAL, t[:res["end_text"]], p[:res["end_pattern"]], S, go, ge)
                assert (g["score"], g["aligned_text"], g["aligned_pattern"]) == (res["score"], res["aligned_text"], res["aligned_pattern"])
                # I2: non-decreasing in X
                assert last is None or res["score"] >= last, (k, go, ge, x)
                last = res["score"]
                if x is not NONE:
                    cases += 1
                    stopped += res["stop_row"] <= len(p)
                    changed += res["score"] != full["score"]
            assert extend_ref(t, p, S, go, ge, (1 << 30) - 1) == full
    # the drop is exercised: the cases are not all runs to the last row with the result of no drop
    assert 3 * stopped >= cases and changed >= 20, (stopped, changed, cases)


def test_identities_3_and_4_on_the_reference():
    for k, (A, t, p) in enumerate(random_small_pairs(30, 52200)):
        S = matrix("blast" if A == 4 else "blosum50", A)
        for go, ge in ((11, 1), (5, 5), (4, 0), (0, 0)):
            # I3: the best cell anywhere is no worse than the best of row m and column n, nor than 0
            assert extend_ref(t, p, S, go, ge, NONE)["score"] >= max(0, ends_ref(t, p, S, go, ge, TE | PE)["score"]), (k, go, ge)
        # I4: open == extend is the linear recurrence: a plain linear fill
        g = 5
        n, m = len(t), len(p)
        H = np.zeros((m + 1, n + 1), dtype=np.int64)
        H[0, :], H[:, 0] = -g * np.arange(n + 1), -g * np.arange(m + 1)
        for i in range(1, m + 1):
            for j in range(1, n + 1):
                H[i, j] = max(H[i - 1, j - 1] + int(S[p[i - 1]][t[j - 1]]), H[i, j - 1] - g, H[i - 1, j] - g)
        want = extend_ref(t, p, S, g, g, NONE)
        sub = H[1:, 1:]
        assert want["score"] == max(0, int(sub.max()))
        if want["score"]:
            assert (want["end_pattern"] - 1, want["end_text"] - 1) == np.unravel_index(int(sub.argmax()), sub.shape)


# ---- the constructed pairs: a second copy of the text after junk, the stop row at strip edges ---------------------
STOP_LS = [58, 59, 122, 506, 507, 1018]  # stop rows L + 6 = 64, 65, 128, 512, 513, 1024 at X = 20


def chimeric_pair(L, junk=40):
    """The text has letters 0 and 1 only. The pattern is its first L letters, `junk` letters 2, and the
    text again from letter L + junk to letter L + 340."""
    t = synthetic.random_sequence(7 + L, L + 400, 2).astype(np.int8)
    p = np.concatenate([t[:L], np.full(junk, 2, dtype=np.int8), t[L + junk:L + 340]]).astype(np.int8)
    return t, p


def chimeric_ref(L, go, ge, xdrop, junk=40):
    t, p = chimeric_pair(L, junk)
    return extend_ref(t, p, matrix("blast", 4), go, ge, xdrop, key=("chimeric", L, junk))


@pytest.mark.parametrize("L", STOP_LS)
def test_the_constructed_pairs_stop_where_they_should(L):
    for go, ge in GAPS:
        # junk row k lies min(4 k, go + (k - 1) ge) below 5 L: 21 or 24 at k = 6, the first above 20
        want = chimeric_ref(L, go, ge, 20)
        assert want["stop_row"] == L + 6 and cell(want) == (5 * L, L, L), (L, go, ge)
        full = chimeric_ref(L, go, ge, NONE)
        assert full["stop_row"] == len(chimeric_pair(L)[1]) + 1 and full["score"] == 5 * L + 1340 != want["score"], (L, go, ge)
        # a dip of three junk letters stays within X = 20: no stop, the result of no drop
        dip, nodrop = chimeric_ref(L, go, ge, 20, junk=3), chimeric_ref(L, go, ge, NONE, junk=3)
        assert dip == nodrop and dip["stop_row"] == L + 340 + 1 and dip["score"] > 5 * L, (L, go, ge)


def test_the_drop_is_strict():
    """Under (11, 2) junk row k lies 9 + 2 k below the best for k >= 5: 23 at k = 7, 25 at k = 8. X = 22 stops
    at row L + 7; X = 23 does not (23 is not > 23) and stops at L + 8; so does X = 24 (25 > 24). The two X
    on either side of the strict comparison differ in stop row; 23 and 24 share theirs."""
    L = 122
    rows = [chimeric_ref(L, 11, 2, x)["stop_row"] for x in (22, 23, 24)]
    assert rows == [L + 7, L + 8, L + 8]
    assert all(cell(chimeric_ref(L, 11, 2, x)) == (5 * L, L, L) for x in (22, 23, 24))


# ---- 2. strip, lane and body edges -------------------------------------------------------------------------------
SHAPES = EDGE_SHAPES + [(63, 70), (65, 60), (511, 520), (513, 500), (1100, 600)]  # (m, n)


def shape_pairs(A, seed=61000):
    pairs = [related_pair(seed + 3 * m + 5 * n + A, n, m, A) for m, n in SHAPES]
    return [t for t, _ in pairs], [p for _, p in pairs]


def shape_wants(A, S, texts, patterns, go, ge, xdrop):
    return [extend_ref(t, p, S, go, ge, xdrop, key=("shape", A, k)) for k, (t, p) in enumerate(zip(texts, patterns))]


@gpu
@pytest.mark.parametrize("go,ge", GAPS)
@pytest.mark.parametrize("A,mat", [(4, "blast"), (23, "blosum50")])
def test_strip_lane_and_body_edges(eng, A, mat, go, ge):
    S = matrix(mat, A)
    texts, patterns = shape_pairs(A)
    stops = 0
    for x in (NONE, 20):
        wants = shape_wants(A, S, texts, patterns, go, ge, x)
        stops += sum(w["stop_row"] <= len(p) for w, p in zip(wants, patterns))
        check(eng, texts, patterns, S, go, ge, x, wants, "edges")
    assert stops >= 3  # some of the related pairs drop at X = 20


@gpu
@pytest.mark.parametrize("go,ge", GAPS)
def test_stop_rows_at_strip_edges(eng, go, ge):
    S = matrix("blast", 4)
    pairs = [chimeric_pair(L) for L in STOP_LS]
    texts, patterns = [t for t, _ in pairs], [p for _, p in pairs]
    wants = [chimeric_ref(L, go, ge, 20) for L in STOP_LS]
    assert [cell(w) for w in wants] == [(5 * L, L, L) for L in STOP_LS]
    assert [w["stop_row"] for w in wants] == [64, 65, 128, 512, 513, 1024]
    check(eng, texts, patterns, S, go, ge, 20, wants, "stop rows")
    full = [chimeric_ref(L, go, ge, NONE) for L in STOP_LS]
    assert all(cell(f) != cell(w) and f["score"] == w["score"] + 1340 for f, w in zip(full, wants))  # the second copy wins
    check(eng, texts, patterns, S, go, ge, NONE, full, "stop rows, no drop")


@gpu
def test_the_drop_is_strict_on_the_device(eng):
    S = matrix("blast", 4)
    t, p = chimeric_pair(122)
    for x in (22, 23, 24):
        check(eng, [t], [p], S, 11, 2, x, [chimeric_ref(122, 11, 2, x)], "strict")


@gpu
@pytest.mark.parametrize("go,ge", GAPS)
def test_a_dip_that_stays_within_x(eng, go, ge):
    S = matrix("blast", 4)
    pairs = [chimeric_pair(L, junk=3) for L in STOP_LS]
    texts, patterns = [t for t, _ in pairs], [p for _, p in pairs]
    wants = [chimeric_ref(L, go, ge, 20, junk=3) for L in STOP_LS]
    assert wants == [chimeric_ref(L, go, ge, NONE, junk=3) for L in STOP_LS]
    check(eng, texts, patterns, S, go, ge, 20, wants, "dip")


# ---- 3. ties ---------------------------------------------------------------------------------------------------------
def tie_pairs():
    pairs = [related_pair(7100 + 3 * m + 5 * n, n, m, 4) for m, n in ((9, 65), (129, 120), (513, 500))]
    # a pattern X against a text X, junk, X: row m holds its maximum twice, the leftmost wins
    X = synthetic.random_sequence(74, 70, 2).astype(np.int8)
    pairs.append((np.concatenate([X, np.full(30, 3, dtype=np.int8), X]).astype(np.int8), X))
    return pairs


def test_the_tie_pairs_hold_ties():
    S = matrix("blast", 4)
    pairs = tie_pairs()
    t, p = pairs[-1]
    want = extend_ref(t, p, S, 0, 0, NONE)
    H, _ = global_fill(t, p, S, 0, 0)
    assert cell(want) == (350, 70, 70) and int(H[70, 170]) == 350  # with free gaps the second copy ties in row m
    # under (0, 0) the maximum, once reached, fills every row after it: rows of different R = 1 strips
    two_strips = 0
    for t, p in pairs[:3]:
        H, _ = global_fill(t, p, S, 0, 0)
        rows = 1 + np.nonzero(H[1:, 1:].max(axis=1) == H[1:, 1:].max())[0]
        want = extend_ref(t, p, S, 0, 0, NONE)
        assert want["end_pattern"] == rows[0]  # the earlier row wins
        two_strips += (rows[0] - 1) // 64 != (rows[-1] - 1) // 64
    assert two_strips >= 1


@gpu
@pytest.mark.parametrize("go,ge", [(0, 0), (4, 0), (11, 2)])
def test_ties(eng, go, ge):
    S = matrix("blast", 4)
    pairs = tie_pairs()
    texts, patterns = [t for t, _ in pairs], [p for _, p in pairs]
    for x in (NONE, 20):
        wants = [extend_ref(t, p, S, go, ge, x, key=("tie", k)) for k, (t, p) in enumerate(pairs)]
        check(eng, texts, patterns, S, go, ge, x, wants, "ties")


# ---- 4. score 0 ---------------------------------------------------------------------------------------------------------
def late_pair():
    """Only rows >= i* hold positive cells at X = 0: the pattern's first letter is not in the text, so row 1
    lies 4 below B(0) = 0 and is the stop row; its other letters are the text's."""
    t = synthetic.random_sequence(81, 90, 2).astype(np.int8)
    return t, np.concatenate([[2], t[:80]]).astype(np.int8)


def test_the_late_pair_scores_0_only_under_the_drop():
    S = matrix("blast", 4)
    t, p = late_pair()
    assert cell(extend_ref(t, p, S, 11, 2, 0)) == (0, 0, 0) and extend_ref(t, p, S, 11, 2, 0)["stop_row"] == 1
    assert extend_ref(t, p, S, 11, 2, NONE)["score"] > 100


@gpu
def test_score_0(eng):
    S4 = np.full((4, 4), -4, dtype=np.int32)
    shapes = [(1, 70), (70, 1), (65, 64), (130, 513)]  # (m, n)
    texts = [synthetic.random_sequence(900 + k, n, 4).astype(np.int8) for k, (m, n) in enumerate(shapes)]
    patterns = [synthetic.random_sequence(950 + k, m, 4).astype(np.int8) for k, (m, n) in enumerate(shapes)]
    for go, ge in GAPS:
        for x in (NONE, 0, 20):
            wants = [extend_ref(t, p, S4, go, ge, x) for t, p in zip(texts, patterns)]
            assert all(cell(w) == (0, 0, 0) for w in wants)
            got = check(eng, texts, patterns, S4, go, ge, x, wants, "all -4")
            for g in got:
                assert (g["num_bytes"], g["start_text"], g["start_pattern"], g["aligned_text"], g["aligned_pattern"]) == (0, 0, 0, "", "")
    S = matrix("blast", 4)
    t, p = late_pair()
    for go, ge in GAPS:
        check(eng, [t], [p], S, go, ge, 0, [extend_ref(t, p, S, go, ge, 0)], "late")
        check(eng, [t], [p], S, go, ge, NONE, [extend_ref(t, p, S, go, ge, NONE)], "late, no drop")
        assert cell(extend_ref(t, p, S, go, ge, 0)) == (0, 0, 0)


# ---- 5. negative and zero penalties -------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("go,ge", [(3, 7), (0, 0), (-2, -1), (4, 0)])
def test_negative_and_zero_penalties(eng, go, ge):
    S = matrix("blast", 4)
    pairs = [related_pair(1300 + 3 * m + 5 * n, n, m, 4) for m, n in ((64, 70), (129, 120), (513, 500))]
    texts, patterns = [t for t, _ in pairs], [p for _, p in pairs]
    for x in (5, NONE):
        wants = [extend_ref(t, p, S, go, ge, x, key=("penalties", k)) for k, (t, p) in enumerate(pairs)]
        check(eng, texts, patterns, S, go, ge, x, wants, "penalties")


# ---- 6. pairs outnumber waves, early and late exits share waves and boundary rows ---------------------------------
def mixed_pairs():
    """many_pairs three times over with a constructed pair in every 25th place."""
    texts, patterns = many_pairs()
    texts, patterns = list(texts) * 3, list(patterns) * 3
    for k in range(0, len(texts), 25):
        texts[k], patterns[k] = chimeric_pair(STOP_LS[(k // 25) % len(STOP_LS)])
    return texts, patterns


@gpu
def test_pairs_outnumber_waves_and_reruns(eng):
    import torch
    S = matrix("blast", 4)
    go, ge = 11, 2
    texts, patterns = mixed_pairs()
    to = np.concatenate([[0], np.cumsum([len(t) for t in texts])])
    po = np.concatenate([[0], np.cumsum([len(p) for p in patterns])])
    dt, dp = torch.from_numpy(np.concatenate(texts)).cuda(), torch.from_numpy(np.concatenate(patterns)).cuda()
    sc = eng.Scorer(GLOBAL, S, go, [(int(to[k]), len(texts[k]), int(po[k]), len(patterns[k])) for k in range(len(texts))],
                    gap_extend=ge, xdrop=20)
    assert sc.info()["num_waves"] < len(texts)
    sc.run(dt.data_ptr(), dp.data_ptr())
    first = sc.results().copy()
    sc.run(dt.data_ptr(), dp.data_ptr())
    second = sc.results().copy()
    sc.close()
    assert digest(first.tolist()) == digest(second.tolist())
    assert first.tolist() == eng.score_batch(GLOBAL, texts, patterns, S, go, gap_extend=ge, xdrop=20).tolist()
    got = eng.align_pairs_affine(GLOBAL, texts, patterns, S, go, ge, xdrop=20)
    assert [g["score"] for g in got] == first["score"].tolist()
    rng = np.random.default_rng(5)
    for k in list(range(0, 25 * len(STOP_LS), 25)) + rng.choice(len(texts), 120, replace=False).tolist():
        if k % 25 == 0:
            want = chimeric_ref(STOP_LS[(k // 25) % len(STOP_LS)], go, ge, 20)
        else:
            want = extend_ref(texts[k], patterns[k], S, go, ge, 20)
        assert cell(first[k]) == cell(want) and pick(got[k]) == pick(want), int(k)
    again = eng.align_pairs_affine(GLOBAL, texts, patterns, S, go, ge, xdrop=20)
    assert digest([[r[k] for k in KEYS] for r in again]) == digest([[r[k] for k in KEYS] for r in got])


# ---- 7. the identities of sa_hip.h on the device -------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("go,ge", GAPS)
def test_identity_1_on_the_device(eng, go, ge):
    S = matrix("blast", 4)
    texts, patterns = shape_pairs(4)
    for L in STOP_LS:
        t, p = chimeric_pair(L)
        texts.append(t), patterns.append(p)
    for x in (20, NONE):
        got = eng.align_pairs_affine(GLOBAL, texts, patterns, S, go, ge, xdrop=xd(eng, x))
        ends = eng.score_batch(GLOBAL, texts, patterns, S, go, gap_extend=ge, xdrop=xd(eng, x))
        pt = [t[:int(e["end_text"])] for t, e in zip(texts, ends)]
        pp = [p[:int(e["end_pattern"])] for p, e in zip(patterns, ends)]
        pre = eng.align_pairs_affine(GLOBAL, pt, pp, S, go, ge)
        for k, (g, a) in enumerate(zip(got, pre)):
            assert (g["score"], g["aligned_text"], g["aligned_pattern"]) == (a["score"], a["aligned_text"], a["aligned_pattern"]), (x, k)
            assert g["aligned_text"].replace("-", "") == "".join("ATCG"[c] for c in pt[k])
            assert g["aligned_pattern"].replace("-", "") == "".join("ATCG"[c] for c in pp[k])
            assert (g["start_text"], g["start_pattern"]) == (0, 0)


@gpu
@pytest.mark.parametrize("A,mat", [(4, "blast"), (23, "blosum50")])
def test_identities_2_and_3_on_the_device(eng, A, mat):
    S = matrix(mat, A)
    texts, patterns = shape_pairs(A)
    for go, ge in GAPS:
        for R in (1, 2, 4, 8):
            a = eng.score_batch(GLOBAL, texts, patterns, S, go, rows_per_lane=R, gap_extend=ge, xdrop=eng.NO_XDROP)
            b = eng.score_batch(GLOBAL, texts, patterns, S, go, rows_per_lane=R, gap_extend=ge, xdrop=(1 << 30) - 1)
            assert a.tobytes() == b.tobytes(), (go, ge, R)
        assert (eng.align_pairs_affine(GLOBAL, texts, patterns, S, go, ge, xdrop=eng.NO_XDROP) ==
                eng.align_pairs_affine(GLOBAL, texts, patterns, S, go, ge, xdrop=(1 << 30) - 1))
        free = eng.score_batch(ENDS | TE | PE, texts, patterns, S, go, gap_extend=ge)
        last = None
        for x in (0, 5, 20, 100, eng.NO_XDROP):
            s = eng.score_batch(GLOBAL, texts, patterns, S, go, gap_extend=ge, xdrop=x)["score"]
            assert last is None or (s >= last).all(), (go, ge, x)  # non-decreasing in X
            last = s
        assert (last >= np.maximum(0, free["score"])).all(), (go, ge)


# ---- 8. empty sides, zero pairs, refusals -----------------------------------------------------------------------------
@gpu
def test_empty_sides_and_zero_pairs(eng):
    S = matrix("blast", 4)
    x, none = synthetic.random_sequence(1, 50, 4).astype(np.int8), np.zeros(0, dtype=np.int8)
    for xdrop in (eng.NO_XDROP, 0, 20):
        assert eng.align_pairs_affine(GLOBAL, [], [], S, 11, 2, xdrop=xdrop) == []
        assert len(eng.score_batch(GLOBAL, [], [], S, 11, gap_extend=2, xdrop=xdrop)) == 0
        assert len(eng.score_batch(GLOBAL, [], [], S, 5, xdrop=xdrop)) == 0
    texts, patterns = [none, x[:5], none, x], [none, none, x[:5], x[:20]]
    for go, ge in GAPS + [(-3, 1)]:
        for xdrop in (NONE, 0, 20):
            wants = [extend_ref(t, p, S, go, ge, xdrop) for t, p in zip(texts, patterns)]
            assert [cell(w) for w in wants[:3]] == [(0, 0, 0)] * 3
            got = check(eng, texts, patterns, S, go, ge, xdrop, wants, "empty")
            assert all(g["aligned_text"] == "" and g["num_bytes"] == 0 for g in got[:3])
    got = eng.align_pairs_affine(GLOBAL, [x], [x[:40]], S, 11, 2, strings=False, xdrop=20)[0]
    want = extend_ref(x, x[:40], S, 11, 2, 20)
    assert got == {k: want[k] for k in KEYS[:4]}


@gpu
def test_refusals(eng):
    S = matrix("blast", 4)
    x = synthetic.random_sequence(1, 50, 4).astype(np.int8)
    y = x[:20]
    scorer = lambda mode, **kw: eng.Scorer(mode, S, 11, [(0, 50, 0, 20)], gap_extend=2, **kw)  # noqa: E731
    # a band of either kind with xdrop
    for kw in ({"band": 3}, {"bands": [(0, 30)]}):
        for call in (lambda: eng.score_batch(GLOBAL, [x], [y], S, 11, gap_extend=2, xdrop=20, **kw),
                     lambda: scorer(GLOBAL, xdrop=20, **kw),
                     lambda: eng.align_pairs_affine(GLOBAL, [x], [y], S, 11, 2, xdrop=20, **kw)):
            with pytest.raises(ValueError):
                call()
    # a bad xdrop, and a mode other than global
    stats = eng.align_pairs_affine(GLOBAL, [x], [y], S, 11, 2, xdrop=20) and eng.affine_last_stats()
    assert stats["num_chunks"] == 1 and stats["arena_bytes"] > 0
    for mode, xdrop in ((GLOBAL, -2), (GLOBAL, 1 << 30), (LOCAL, 20), (FIT, 20), (ENDS, 20), (ENDS | 15, eng.NO_XDROP), (3, 20)):
        for call in (lambda: eng.score_batch(mode, [x], [y], S, 11, gap_extend=2, xdrop=xdrop),
                     lambda: eng.score_batch(mode, [x], [y], S, 5, xdrop=xdrop),
                     lambda: scorer(mode, xdrop=xdrop),
                     lambda: eng.align_pairs_affine(mode, [x], [y], S, 11, 2, xdrop=xdrop)):
            with pytest.raises(eng.SaError) as e:
                call()
            assert e.value.code == 1, (mode, xdrop)
    # over the score limit, the unbanded one: (max|S| + G)(n + m) + G (n + m) >= 2^30 at G = 2^23, n + m = 70
    for call in (lambda: eng.score_batch(GLOBAL, [x], [y], S, 1 << 23, gap_extend=2, xdrop=20),
                 lambda: eng.align_pairs_affine(GLOBAL, [x], [y], S, 1 << 23, 2, xdrop=20)):
        with pytest.raises(eng.SaError) as e:
            call()
        assert e.value.code == 4  # SA_ERR_UNSUPPORTED
    # an out-of-alphabet byte
    bad = x.copy()
    bad[10] = 4
    for call in (lambda: eng.score_batch(GLOBAL, [bad, x], [y, y], S, 11, gap_extend=2, xdrop=eng.NO_XDROP),
                 lambda: eng.score_batch(GLOBAL, [bad, x], [y, y], S, 5, xdrop=eng.NO_XDROP),
                 lambda: eng.align_pairs_affine(GLOBAL, [bad, x], [y, y], S, 11, 2, xdrop=eng.NO_XDROP)):
        with pytest.raises(eng.SaError) as e:
            call()
        assert e.value.code == 1
    # null arguments
    p, S_keep, alpha_keep = eng._params(GLOBAL, S, 0, None, 0)
    res = (eng.SaResult * 1)()
    out = (eng.SaScoreResult * 1)()
    hp = (eng.SaHostPair * 1)(eng.SaHostPair(x.ctypes.data, 50, y.ctypes.data, 20))
    dpair = (eng.SaPair * 1)(eng.SaPair(0, 50, 0, 20))
    buf = ctypes.create_string_buffer(100)
    one = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    h = ctypes.c_void_p()
    L = eng.lib
    assert L.sa_align_pairs_extend(ctypes.byref(p), 11, 2, 20, hp, 1, 0, res, None, None) == 0
    assert L.sa_align_pairs_extend(None, 11, 2, 20, hp, 1, 0, res, None, None) == 1
    assert L.sa_align_pairs_extend(ctypes.byref(p), 11, 2, 20, None, 1, 0, res, None, None) == 1
    assert L.sa_align_pairs_extend(ctypes.byref(p), 11, 2, 20, hp, 1, 0, None, None, None) == 1
    assert L.sa_align_pairs_extend(ctypes.byref(p), 11, 2, 20, hp, 1, 0, res, one, None) == 1
    assert L.sa_align_pairs_extend(ctypes.byref(p), 11, 2, 20, hp, -1, 0, res, None, None) == 1
    assert L.sa_align_pairs_extend(ctypes.byref(p), 11, 2, 20, None, 0, 0, None, None, None) == 0  # zero pairs read nothing
    assert L.sa_score_batch_extend(ctypes.byref(p), 11, 2, 20, hp, 1, 0, out) == 0
    assert L.sa_score_batch_extend(None, 11, 2, 20, hp, 1, 0, out) == 1
    assert L.sa_score_batch_extend(ctypes.byref(p), 11, 2, 20, None, 1, 0, out) == 1
    assert L.sa_score_batch_extend(ctypes.byref(p), 11, 2, 20, hp, 1, 0, None) == 1
    assert L.sa_score_batch_extend(ctypes.byref(p), 11, 2, 20, hp, -1, 0, out) == 1
    assert L.sa_score_batch_extend(ctypes.byref(p), 11, 2, 20, None, 0, 0, None) == 0
    assert L.sa_scorer_create_extend(ctypes.byref(p), 11, 2, 20, None, 1, 0, ctypes.byref(h)) == 1
    assert L.sa_scorer_create_extend(ctypes.byref(p), 11, 2, 20, dpair, 1, 0, None) == 1
    assert L.sa_scorer_create_extend(None, 11, 2, 20, dpair, 1, 0, ctypes.byref(h)) == 1
    p.mode = 3
    assert L.sa_score_batch_extend(ctypes.byref(p), 11, 2, 20, hp, 1, 0, out) == 1
    # the mode numbers stay what they were: no extension mode
    for mode in (3, 15, 32):
        with pytest.raises(eng.SaError) as e:
            eng.score_batch(mode, [x], [y], S, 11, gap_extend=2)
        assert e.value.code == 1


# ---- 9. the C++ functions -------------------------------------------------------------------------------------------------
@gpu
def test_cpp_extend_check():
    out = subprocess.run([os.path.join(PKG, "bin", "sa_extend_check"), "700", "96"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1] == "OK 96"
