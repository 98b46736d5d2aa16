"""Ends-free alignment, sa_hip.h SA_ENDS_FREE = 16 with the flags TB = 1, TE = 2, PB = 4, PE = 8 (free
text begin, text end, pattern begin, pattern end; all four: SA_OVERLAP), on the score-only and traced
wave paths (sa_score_batch*, sa_scorer_*, sa_search*, sa_align_pairs_affine and the C++ functions over
them). The reference has no such mode, so parity is pinned as for fit mode: ends_ref below, a numpy fill
by anti-diagonals with a plain Python pick of the result cell and a plain walk, is checked on the CPU
against a plain double loop, against fit_ref and the oracle where the modes coincide, against the
reference's own global recurrence over every permitted trim of the two sequences, by its symmetries and
by re-scoring its strings; the GPU is then compared with ends_ref."""
from __future__ import annotations

import hashlib
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, encode, matrix  # first: it puts oracle/ and the package on the path

import oracle
from sa_amd import synthetic
from test_align_affine_gpu import (DIAG, EDGE_SHAPES, EEXT, FEXT, KEYS, LEFT, LONG_GAPS, NEG, TOP, alphabet_of, many_pairs,
                                   pick, rescore)
from test_fit_gpu import cell, fit_ref, random_small_pairs
from test_score_affine_gpu import gotoh_ref
from test_score_gpu import related_pair

gpu = pytest.mark.gpu

GLOBAL, LOCAL, FIT = 0, 1, 2
ENDS, TB, TE, PB, PE = 16, 1, 2, 4, 8
OVERLAP = ENDS | 15
FLAGS = list(range(16))
GAPS = [(11, 2), (3, 1), (5, 5)]
SCHEMES = [(4, "blast"), (23, "blosum50")]


# ---- the reference of this file ------------------------------------------------------------------------
def gap_cost(k, go, ge):
    return go + (k - 1) * ge


def ends_fill_by_diagonals(t, p, S, go, ge, tb, pb):
    """(H, D) of the recurrence swept by anti-diagonals: row 0 is 0 under TB and one gap run otherwise,
    column 0 likewise under PB, E and F of the borders minus infinity; D as
    test_align_affine_gpu.nibbles_by_diagonals has it."""
    t, p, S = np.asarray(t, dtype=np.int64), np.asarray(p, dtype=np.int64), np.asarray(S, dtype=np.int64)
    n, m = len(t), len(p)
    H = np.zeros((m + 1, n + 1), dtype=np.int64)
    if not tb:
        H[0, 1:] = -(go + np.arange(n) * ge)
    if not pb:
        H[1:, 0] = -(go + np.arange(m) * ge)
    E = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    F = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    D = np.zeros((m + 1, n + 1), dtype=np.uint8)
    for d in range(2, n + m + 1):
        i = np.arange(max(1, d - n), min(m, d - 1) + 1)
        j = d - i
        ee, eo = E[i, j - 1] - ge, H[i, j - 1] - go
        fe, fo = F[i - 1, j] - ge, H[i - 1, j] - go
        e, f = np.maximum(ee, eo), np.maximum(fe, fo)
        dg = H[i - 1, j - 1] + S[p[i - 1], t[j - 1]]
        src = np.where(dg > np.maximum(e, f), DIAG, np.where(e >= f, LEFT, TOP))
        D[i, j] = src + EEXT * (ee > eo) + FEXT * (fe > fo)
        H[i, j], E[i, j], F[i, j] = np.maximum(dg, np.maximum(e, f)), e, f
    return H, D


def ends_fill_by_loops(t, p, S, go, ge, tb, pb):
    """The same as a plain double loop over the cells."""
    n, m = len(t), len(p)
    H = [[0] * (n + 1) for _ in range(m + 1)]
    D = [[0] * (n + 1) for _ in range(m + 1)]
    for j in range(1, n + 1):
        H[0][j] = 0 if tb else -gap_cost(j, go, ge)
    for i in range(1, m + 1):
        H[i][0] = 0 if pb else -gap_cost(i, go, ge)
    F = [NEG] * (n + 1)
    for i in range(1, m + 1):
        E = NEG
        for j in range(1, n + 1):
            ee, eo, fe, fo = E - ge, H[i][j - 1] - go, F[j] - ge, H[i - 1][j] - go
            E, F[j] = max(ee, eo), max(fe, fo)
            dg = H[i - 1][j - 1] + int(S[p[i - 1]][t[j - 1]])
            src = DIAG if dg > max(E, F[j]) else LEFT if E >= F[j] else TOP
            D[i][j] = src + (EEXT if ee > eo else 0) + (FEXT if fe > fo else 0)
            H[i][j] = max(dg, E, F[j])
    return np.array(H, dtype=np.int64), np.array(D, dtype=np.uint8)


def ends_end(H, flags):
    """(score, end_pattern, end_text): the maximum of H over the candidates, (m, n), row m under TE and
    column n under PE. An interior candidate beats a border candidate of the same value; within each
    kind the first in row-major order wins."""
    m, n = H.shape[0] - 1, H.shape[1] - 1
    cand = {(m, n)}
    if flags & TE:
        cand |= {(m, j) for j in range(n + 1)}
    if flags & PE:
        cand |= {(i, n) for i in range(m + 1)}
    best = {}
    for i, j in sorted(cand):  # row-major
        kind = "interior" if i >= 1 and j >= 1 else "border"
        if kind not in best or H[i, j] > best[kind][0]:
            best[kind] = (int(H[i, j]), i, j)
    if "interior" in best and ("border" not in best or best["interior"][0] >= best["border"][0]):
        return best["interior"]
    return best["border"]


def ends_walk(t, p, H, D, flags, alphabet):
    """From the result cell in state H until a free begin or the origin: it ends at (i, j) when
    i == 0 and (TB or j == 0), or j == 0 and (PB or i == 0); else column 0 forces TOP, row 0 LEFT."""
    score, i, j = ends_end(H, flags)
    end = (i, j)
    gapc = alphabet[-1]
    state, at, ap = DIAG, [], []
    while not ((i == 0 and (flags & TB or j == 0)) or (j == 0 and (flags & PB or i == 0))):
        nxt = DIAG
        if j == 0:
            d = TOP
        elif i == 0:
            d = LEFT
        else:
            nib = int(D[i, j])
            d = (nib & 3) if state == DIAG else state
            if d == LEFT:
                nxt = LEFT if nib & EEXT else DIAG
            if d == TOP:
                nxt = TOP if nib & FEXT else DIAG
        tt, tp = d in (DIAG, LEFT), d in (DIAG, TOP)
        at.append(alphabet[t[j - 1]] if tt else gapc)
        ap.append(alphabet[p[i - 1]] if tp else gapc)
        j, i, state = j - tt, i - tp, nxt
    return {"score": score, "num_bytes": len(at), "start_text": j, "start_pattern": i,
            "aligned_text": "".join(reversed(at)), "aligned_pattern": "".join(reversed(ap)), "end_text": end[1],
            "end_pattern": end[0]}


_FILLS = {}  # (key, go, ge, TB, PB) -> (H, D): the fill depends on the begin flags only; the newest few are kept


def ends_ref(t, p, S, go, ge, flags, key=None, alphabet=None):
    """The ends-free alignment of text t and pattern p under gap open go / gap extend ge (go == ge: the
    linear gap) with the free ends `flags`: the keys of align_pairs_affine plus end_text and
    end_pattern of the scorers. With `key` (naming the pair and the scheme) the fill is shared by the
    flag sets with the same free begins."""
    t, p = np.asarray(t, dtype=np.int64), np.asarray(p, dtype=np.int64)
    tb, pb = bool(flags & TB), bool(flags & PB)
    fk = (key, go, ge, tb, pb)
    if key is None or fk not in _FILLS:
        H, D = ends_fill_by_diagonals(t, p, S, go, ge, tb, pb)
        if key is not None:
            while len(_FILLS) >= 8:
                _FILLS.pop(next(iter(_FILLS)))
            _FILLS[fk] = (H, D)
    else:
        H, D = _FILLS[fk]
    return ends_walk(t, p, H, D, flags, alphabet or alphabet_of(S))


_REF = {}


def ref_all_flags(key, t, p, S, go, ge):
    """ends_ref of a case for all 16 flag sets (four fills), once, shared by the tests that meet it again."""
    k = (key, go, ge)
    if k not in _REF:
        _REF[k] = [None] * 16
        for f in sorted(FLAGS, key=lambda f: f & (TB | PB)):
            _REF[k][f] = ends_ref(t, p, S, go, ge, f, key=key)
    return _REF[k]


def check_scores(eng, mode, texts, patterns, S, go, ge, wants, what, Rs=(1, 2, 4, 8)):
    """Every forced rows_per_lane of the affine scorer, and of the linear one when go == ge."""
    for R in Rs:
        got = eng.score_batch(mode, texts, patterns, S, go, rows_per_lane=R, gap_extend=ge)
        assert [cell(g) for g in got] == [cell(w) for w in wants], (what, mode, "affine", R)
        if go == ge:
            got = eng.score_batch(mode, texts, patterns, S, go, rows_per_lane=R)
            assert [cell(g) for g in got] == [cell(w) for w in wants], (what, mode, "linear", R)


def check_alignments(eng, mode, texts, patterns, S, go, ge, wants, what):
    got = eng.align_pairs_affine(mode, texts, patterns, S, go, ge)
    for k, (g, w) in enumerate(zip(got, wants)):
        assert pick(g) == pick(w), (what, mode, k, len(patterns[k]), len(texts[k]))


def check_both(eng, mode, texts, patterns, S, go, ge, wants, what, Rs=(1, 2, 4, 8)):
    check_scores(eng, mode, texts, patterns, S, go, ge, wants, what, Rs)
    check_alignments(eng, mode, texts, patterns, S, go, ge, wants, what)


# ---- 1. the reference of this file is sound (CPU) ------------------------------------------------------
def scheme(A):
    return matrix("blast" if A == 4 else "blosum50", A)


def test_ends_ref_equals_the_plain_loops():
    for k, (A, t, p) in enumerate(random_small_pairs(40, 17100)):
        S = scheme(A)
        go, ge = ((11, 1), (5, 5), (4, 0), (3, 7), (-2, -1))[k % 5]
        for tb, pb in itertools.product((False, True), repeat=2):
            H1, D1 = ends_fill_by_diagonals(t, p, S, go, ge, tb, pb)
            H2, D2 = ends_fill_by_loops(t, p, S, go, ge, tb, pb)
            assert (H1 == H2).all() and (D1 == D2).all(), (k, tb, pb)
            assert H1[0, len(t)] == (0 if tb else -gap_cost(len(t), go, ge)) and H1[len(p), 0] == (0 if pb else -gap_cost(len(p), go, ge))


def test_ends_ref_equals_fit_ref_and_the_global_references():
    for k, (A, t, p) in enumerate(random_small_pairs(30, 18200)):
        S = scheme(A)
        for go, ge in ((11, 1), (5, 5), (4, 0), (3, 7), (-2, -1)):
            assert ends_ref(t, p, S, go, ge, TB | TE) == fit_ref(t, p, S, go, ge), (k, go, ge)
            res = ends_ref(t, p, S, go, ge, 0)
            assert cell(res) == gotoh_ref(GLOBAL, t, p, S, go, ge), (k, go, ge)
            if go == ge:
                assert pick(res) == oracle.align(GLOBAL, t, p, S, go), (k, go)
    none, x = np.zeros(0, dtype=np.int8), synthetic.random_sequence(5, 5, 4)
    S = matrix("blast", 4)
    for t, p in ((none, x), (x, none), (x[:1], x[:1])):
        assert pick(ends_ref(t, p, S, 3, 3, 0)) == oracle.align(GLOBAL, t, p, S, 3)
        assert ends_ref(t, p, S, 11, 2, TB | TE) == fit_ref(t, p, S, 11, 2)
    # both sides empty: global keeps the reference's (uint64)-1 starts, ends-free reports 0
    both = ends_ref(none, none, S, 3, 3, 0)
    assert (both["score"], both["num_bytes"], both["start_text"], both["start_pattern"]) == (0, 0, 0, 0)
    assert oracle.align(GLOBAL, none, none, S, 3)["start_text"] == (1 << 64) - 1


def test_ends_ref_is_the_best_global_alignment_of_a_permitted_trim():
    """go == ge == g, n, m <= 8: the score is the maximum of the reference's global score of t[a:b]
    against p[c:d] over the trims the flags permit (a > 0 needs TB, b < n TE, c > 0 PB, d < m PE) with
    (a == 0 or c == 0) and (b == n or d == m): an alignment cannot skip the begins, or the ends, of
    both sequences."""
    rng = np.random.default_rng(77)
    for k in range(8):
        A = 4 if k % 2 else 23
        n, m = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        t, p = related_pair(19300 + 10 * k, n, m, A)
        S = scheme(A)
        for g in (0, 2, 5):
            glob = {(a, b, c, d): oracle.align(GLOBAL, t[a:b], p[c:d], S, g)["score"]
                    for a in range(n + 1) for b in range(a, n + 1) for c in range(m + 1) for d in range(c, m + 1)
                    if (a == 0 or c == 0) and (b == n or d == m)}
            for f in FLAGS:
                best = max(v for (a, b, c, d), v in glob.items() if (a == 0 or f & TB) and (b == n or f & TE) and
                           (c == 0 or f & PB) and (d == m or f & PE))
                res = ends_ref(t, p, S, g, g, f, key=("trim", k))
                assert res["score"] == best, (k, g, f)
                assert glob[(res["start_text"], res["end_text"], res["start_pattern"], res["end_pattern"])] == best, (k, g, f)


def swap_flags(f):
    return (PB if f & TB else 0) | (PE if f & TE else 0) | (TB if f & PB else 0) | (TE if f & PE else 0)


def test_ends_ref_swap_symmetry():
    for k, (A, t, p) in enumerate(random_small_pairs(20, 20400)):
        S = scheme(A).copy()
        S[0, 1] += 3  # not symmetric: the transpose matters
        S[2, 0] -= 2
        for go, ge in ((11, 1), (5, 5), (4, 0), (-2, -1)):
            for f in FLAGS:
                a = ends_ref(t, p, S, go, ge, f, key=("swap", k))
                b = ends_ref(p, t, S.T, go, ge, swap_flags(f), key=("swapped", k))
                assert a["score"] == b["score"], (k, go, ge, f)


def test_ends_ref_flags_never_lower_the_score_and_overlap_is_at_most_local():
    for k, (A, t, p) in enumerate(random_small_pairs(20, 21500)):
        S = scheme(A)
        for go, ge in ((11, 1), (5, 5), (4, 0), (0, 0)):
            sc = [ends_ref(t, p, S, go, ge, f, key=("mono", k))["score"] for f in FLAGS]
            for f in FLAGS:
                for bit in (TB, TE, PB, PE):
                    assert sc[f | bit] >= sc[f], (k, go, ge, f, bit)
            assert sc[15] <= gotoh_ref(LOCAL, t, p, S, go, ge)[0], (k, go, ge)


def test_ends_ref_strings_rescore_and_strip_to_the_windows():
    for k, (A, t, p) in enumerate(random_small_pairs(20, 22600)):
        S = scheme(A)
        alpha = alphabet_of(S)
        for go, ge in ((11, 1), (5, 5), (4, 0)):
            for f in FLAGS:
                res = ends_ref(t, p, S, go, ge, f, key=("strings", k))
                assert rescore(res, S, go, ge, alpha) == res["score"], (k, go, ge, f)
                assert res["aligned_text"].replace("-", "") == "".join(alpha[c] for c in t[res["start_text"]:res["end_text"]])
                assert res["aligned_pattern"].replace("-", "") == "".join(alpha[c] for c in p[res["start_pattern"]:res["end_pattern"]])
                assert res["start_text"] == 0 or f & TB
                assert res["start_pattern"] == 0 or f & PB
                assert res["end_text"] == len(t) or f & TE
                assert res["end_pattern"] == len(p) or f & PE
                assert res["start_text"] == 0 or res["start_pattern"] == 0
                assert res["end_text"] == len(t) or res["end_pattern"] == len(p)


def empty_side_want(k, go, ge, zero, anywhere):
    """(score, cell) along a border of cells 0..k: its value is 0 at cell 0 and everywhere under `zero`,
    else minus one gap run; the result is cell k, or under `anywhere` the first maximum."""
    vals = [0] + [0 if zero else -gap_cost(c, go, ge) for c in range(1, k + 1)]
    c = vals.index(max(vals)) if anywhere else k
    return vals[c], c


def test_ends_ref_empty_sides():
    S = matrix("blast", 4)
    x, none = synthetic.random_sequence(5, 5, 4), np.zeros(0, dtype=np.int8)
    for go, ge in ((11, 2), (3, 3), (4, 0), (-2, -1), (-3, 1), (2, -1)):
        for f in FLAGS:
            res = ends_ref(none, x, S, go, ge, f)  # n == 0: the cells (i, 0)
            v, c = empty_side_want(5, go, ge, f & PB, f & PE)
            assert cell(res) == (v, c, 0), (go, ge, f)
            assert (res["num_bytes"], res["start_text"]) == (0 if f & PB else c, 0) and res["aligned_text"] == "-" * res["num_bytes"]
            res = ends_ref(x, none, S, go, ge, f)  # m == 0: the cells (0, j)
            v, c = empty_side_want(5, go, ge, f & TB, f & TE)
            assert cell(res) == (v, 0, c), (go, ge, f)
            assert (res["num_bytes"], res["start_pattern"]) == (0 if f & TB else c, 0)
            assert cell(ends_ref(none, none, S, go, ge, f)) == (0, 0, 0)
    assert cell(ends_ref(none, x, S, 11, 2, PE)) == (0, 0, 0) and cell(ends_ref(none, x, S, 11, 2, TE)) == (-19, 5, 0)
    assert cell(ends_ref(none, x, S, -2, -1, PE)) == (6, 5, 0)       # every further gap letter pays: the whole run
    assert cell(ends_ref(none, x, S, -3, 1, PE)) == (3, 1, 0)        # the opening pays, the extensions cost
    assert cell(ends_ref(x, none, S, 2, -1, TE)) == (2, 0, 5)        # -2, -1, 0, 1, 2: cell 5 beats cell 0
    assert cell(ends_ref(x, none, S, 4, 0, TB | TE)) == (0, 0, 0)


# ---- 2. strip, lane and body edges ---------------------------------------------------------------------------
# (m, n): forced R = 1, 2 and 4 cross their strips
SHAPES = EDGE_SHAPES + [(64, 70), (65, 70), (128, 1), (129, 200), (256, 70), (257, 70)]


def edge_pairs(A, seed=9000):
    pairs = [related_pair(seed + 3 * m + 5 * n + A, n, m, A) for m, n in SHAPES]
    return pairs, [t for t, _ in pairs], [p for _, p in pairs]


def edge_wants(A, go, ge, pairs, S):
    """wants[f][k]: flag set f, shape k"""
    per_pair = [ref_all_flags(("edges", A) + SHAPES[k], t, p, S, go, ge) for k, (t, p) in enumerate(pairs)]
    return [[per_pair[k][f] for k in range(len(pairs))] for f in FLAGS]


@gpu
@pytest.mark.parametrize("go,ge", GAPS)
@pytest.mark.parametrize("A,mat", SCHEMES)
def test_strip_lane_and_body_edges(eng, A, mat, go, ge):
    S = matrix(mat, A)
    pairs, texts, patterns = edge_pairs(A)
    wants = edge_wants(A, go, ge, pairs, S)
    for f in FLAGS:
        check_both(eng, ENDS | f, texts, patterns, S, go, ge, wants[f], "edges")


# ---- 3. where the best of the last column, and of row m, lies ---------------------------------------------------
M3, N3 = 600, 700
LS = [1, 8, 9, 64, 65, 128, 129, 256, 257, 512, 513, M3 - 1, M3]  # the row after each lane and strip edge at every R


def head_at_the_text_end(L):
    """The text ends with the pattern's first L letters; the rest of both is junk that matches nothing."""
    p = np.full(M3, 2, dtype=np.int8)
    p[:L] = synthetic.random_sequence(700 + L, L, 2)  # letters 0, 1
    t = np.full(N3, 3, dtype=np.int8)
    t[N3 - L:] = p[:L]
    return t, p


def tail_at_the_text_begin(L):
    """The mirror: the pattern's last L letters start the text."""
    p = np.full(M3, 2, dtype=np.int8)
    p[M3 - L:] = synthetic.random_sequence(800 + L, L, 2)
    t = np.full(N3, 3, dtype=np.int8)
    t[:L] = p[M3 - L:]
    return t, p


@gpu
@pytest.mark.parametrize("go,ge", [(11, 2), (5, 5)])
def test_the_best_row_of_the_last_column(eng, go, ge):
    S = matrix("blast", 4)
    pairs = [head_at_the_text_end(L) for L in LS]
    texts, patterns = [t for t, _ in pairs], [p for _, p in pairs]
    wants = [ends_ref(t, p, S, go, ge, TB | PE) for t, p in pairs]
    for L, w in zip(LS, wants):
        assert (w["score"], w["end_pattern"], w["end_text"], w["start_pattern"], w["start_text"]) == (5 * L, L, N3, 0, N3 - L), L
    check_both(eng, ENDS | TB | PE, texts, patterns, S, go, ge, wants, "last column")
    got = eng.align_pairs_affine(ENDS | TB | PE, texts, patterns, S, go, ge)
    sc = eng.score_batch(ENDS | TB | PE, texts, patterns, S, go, gap_extend=ge)
    for L, g, s in zip(LS, got, sc):
        assert (int(s["end_pattern"]), int(s["end_text"]), g["start_pattern"], g["start_text"]) == (L, N3, 0, N3 - L), L


@gpu
@pytest.mark.parametrize("go,ge", [(11, 2), (5, 5)])
def test_the_best_column_of_row_m_and_a_walk_into_column_0(eng, go, ge):
    S = matrix("blast", 4)
    pairs = [tail_at_the_text_begin(L) for L in LS]
    texts, patterns = [t for t, _ in pairs], [p for _, p in pairs]
    wants = [ends_ref(t, p, S, go, ge, PB | TE) for t, p in pairs]
    for L, w in zip(LS, wants):
        assert (w["score"], w["end_pattern"], w["end_text"], w["start_pattern"], w["start_text"]) == (5 * L, M3, L, M3 - L, 0), L
    check_both(eng, ENDS | PB | TE, texts, patterns, S, go, ge, wants, "row m")
    got = eng.align_pairs_affine(ENDS | PB | TE, texts, patterns, S, go, ge)
    sc = eng.score_batch(ENDS | PB | TE, texts, patterns, S, go, gap_extend=ge)
    for L, g, s in zip(LS, got, sc):
        assert (int(s["end_pattern"]), int(s["end_text"]), g["start_pattern"], g["start_text"]) == (M3, L, M3 - L, 0), L


# ---- 4. ties ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("r1,r2,L", [(500, 520, 10), (3, 6, 2), (11, 15, 3), (512, 513, 1), (300, 420, 70)])
def test_two_equal_maxima_in_the_last_column_the_lower_row_wins(eng, r1, r2, L):
    """The text is X; the pattern holds X ending at row r1 and again at row r2, junk elsewhere: both
    copies run from column 0 to column n. (500, 520) straddles the strip edge at R = 8; (3, 6) and
    (11, 15) sit inside one lane at R = 8."""
    S = matrix("blast", 4)
    m = 600
    t = synthetic.random_sequence(71, L, 2).astype(np.int8)  # letters 0, 1
    p = np.full(m, 2, dtype=np.int8)
    p[r1 - L:r1] = t
    p[r2 - L:r2] = t
    for go, ge in ((11, 2), (5, 5)):
        for f in (PB | PE, OVERLAP & 15):
            want = ends_ref(t, p, S, go, ge, f, key=("two rows", r1, r2))
            H, _ = _FILLS[(("two rows", r1, r2), go, ge, bool(f & TB), True)]
            assert H[r1, L] == H[r2, L] == 5 * L == H[:, L].max()
            assert (cell(want), want["start_pattern"], want["start_text"]) == ((5 * L, r1, L), r1 - L, 0)
            check_both(eng, ENDS | f, [t], [p], S, go, ge, [want], "two rows")


@gpu
@pytest.mark.parametrize("m,n,L", [(40, 70, 8), (600, 300, 65), (1100, 1030, 513)])
def test_a_last_column_cell_equal_to_a_row_m_cell_wins(eng, m, n, L):
    """The text is X, junk, Y and the pattern Y, junk, X, all four pieces L letters: Y against Y runs from
    row 0 to (L, n), X against X from column 0 to (m, L); both score 5 L and (L, n) comes first."""
    S = matrix("blast", 4)
    X, Y = synthetic.random_sequence(72, L, 2), synthetic.random_sequence(73, L, 2)
    p = np.full(m, 2, dtype=np.int8)
    p[:L], p[m - L:] = Y, X
    t = np.full(n, 3, dtype=np.int8)
    t[:L], t[n - L:] = X, Y
    for go, ge in ((11, 2), (5, 5)):
        want = ends_ref(t, p, S, go, ge, 15, key=("column first", m, n))
        H, _ = _FILLS[(("column first", m, n), go, ge, True, True)]
        assert H[L, n] == H[m, L] == 5 * L == max(H[:, n].max(), H[m].max())
        assert (cell(want), want["start_pattern"], want["start_text"]) == ((5 * L, L, n), 0, n - L)
        check_both(eng, OVERLAP, [t], [p], S, go, ge, [want], "column first")
        # without PE the leftmost of row m, without TE the lowest row of column n
        for f, end in ((TB | PB | TE, (m, L)), (TB | PB | PE, (L, n))):
            w = ends_ref(t, p, S, go, ge, f, key=("column first", m, n))
            assert cell(w) == (5 * L,) + end
            check_both(eng, ENDS | f, [t], [p], S, go, ge, [w], "column first")


@gpu
@pytest.mark.parametrize("n", [70, 130])
def test_an_interior_candidate_equal_to_the_border_candidate_wins(eng, n):
    """m = 1, every substitution -4, gap 1 (as test_fit_gpu.test_a_flat_row_reports_column_1): under
    TB | TE H[1][j] = -1 for every j >= 1 and the border candidate H[1][0] is -1 too: (1, 1) wins. With PB
    as well H[1][0] is 0, strictly greater: the border cell wins."""
    S = np.full((4, 4), -4, dtype=np.int32)
    t, p = synthetic.random_sequence(3, n, 4), synthetic.random_sequence(4, 1, 4)
    for go, ge in ((1, 1), (1, 3)):
        want = ends_ref(t, p, S, go, ge, TB | TE)
        assert cell(want) == (-1, 1, 1)
        check_both(eng, ENDS | TB | TE, [t], [p], S, go, ge, [want], "flat")
        want = ends_ref(t, p, S, go, ge, TB | TE | PB)
        assert cell(want) == (0, 1, 0) and want["num_bytes"] == 0 and want["start_pattern"] == 1
        check_both(eng, ENDS | TB | TE | PB, [t], [p], S, go, ge, [want], "flat")
        # column n: H[1][n] = -1 is interior, the border candidate H[0][n] is 0 under TB
        want = ends_ref(t, p, S, go, ge, TB | PE)
        assert cell(want) == (0, 0, n) and want["start_text"] == n
        check_both(eng, ENDS | TB | PE, [t], [p], S, go, ge, [want], "flat")


@gpu
def test_all_mismatch_pairs_under_overlap_are_empty_at_a_border_cell(eng):
    S = matrix("blast", 4)
    shapes = [(30, 70), (70, 30), (513, 200), (100, 1), (1, 100), (1, 1)]
    texts = [encode("A" * n, 4) for _, n in shapes]
    patterns = [encode("T" * m, 4) for m, _ in shapes]
    for go, ge in GAPS:
        wants = [ends_ref(t, p, S, go, ge, 15) for t, p in zip(texts, patterns)]
        for (m, n), w in zip(shapes, wants):  # (0, n) is the first border candidate in row-major order
            assert (cell(w), w["num_bytes"], w["start_text"], w["start_pattern"]) == ((0, 0, n), 0, n, 0)
        check_both(eng, OVERLAP, texts, patterns, S, go, ge, wants, "all mismatch")


# ---- 5. identities on the device ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("A,mat", SCHEMES)
def test_identities_with_fit_and_global(eng, A, mat):
    S = matrix(mat, A)
    _, texts, patterns = edge_pairs(A)
    for go, ge in GAPS:
        for mode, same in ((ENDS | TB | TE, FIT), (ENDS, GLOBAL)):
            for R in (1, 2, 4, 8):
                a = eng.score_batch(mode, texts, patterns, S, go, rows_per_lane=R, gap_extend=ge)
                b = eng.score_batch(same, texts, patterns, S, go, rows_per_lane=R, gap_extend=ge)
                assert a.tolist() == b.tolist(), (mode, go, ge, R)
                if go == ge:
                    lin = eng.score_batch(mode, texts, patterns, S, go, rows_per_lane=R)
                    assert lin.tolist() == a.tolist() == eng.score_batch(same, texts, patterns, S, go, rows_per_lane=R).tolist()
            a = eng.align_pairs_affine(mode, texts, patterns, S, go, ge)
            b = eng.align_pairs_affine(same, texts, patterns, S, go, ge)
            assert [pick(x) for x in a] == [pick(x) for x in b], (mode, go, ge)


@gpu
@pytest.mark.parametrize("A,mat", SCHEMES)
def test_linear_and_affine_scorers_agree_when_open_equals_extend(eng, A, mat):
    S = matrix(mat, A)
    pairs, texts, patterns = edge_pairs(A, seed=12000)
    for g in (0, 2):
        for f in FLAGS:
            lin = eng.score_batch(ENDS | f, texts, patterns, S, g)
            aff = eng.score_batch(ENDS | f, texts, patterns, S, g, gap_extend=g)
            assert lin.tolist() == aff.tolist(), (g, f)
    wants = [ref_all_flags(("linear", A) + SHAPES[k], t, p, S, 2, 2) for k, (t, p) in enumerate(pairs)]
    for f in (15, TB | PE, PB | TE, PE):
        assert [cell(r) for r in eng.score_batch(ENDS | f, texts, patterns, S, 2)] == [cell(w[f]) for w in wants], f


# ---- 6. robustness -------------------------------------------------------------------------------------------------
@gpu
def test_negative_scores_throughout(eng):
    S = matrix("blast", 4)
    shapes = [(30, 70), (70, 30), (513, 200), (100, 1)]
    texts = [encode("A" * n, 4) for _, n in shapes]
    patterns = [encode("T" * m, 4) for m, _ in shapes]
    for go, ge in GAPS:
        for f in (0, TE, PE, TE | PE, TB, PB):  # no free begin on both sides: every candidate is negative
            wants = [ends_ref(t, p, S, go, ge, f, key=("negative", k)) for k, (t, p) in enumerate(zip(texts, patterns))]
            assert all(w["score"] < 0 for w in wants)
            check_both(eng, ENDS | f, texts, patterns, S, go, ge, wants, "negative")


@gpu
def test_empty_sides_and_tiny_pairs(eng):
    S = matrix("blast", 4)
    x, none = synthetic.random_sequence(5, 5, 4), np.zeros(0, dtype=np.int8)
    texts, patterns = [none, x, none, x[:1], x[:1]], [none, none, x, x[1:2], x[:1]]  # (m, n) = (0,0), (0,5), (5,0), (1,1) x 2
    for go, ge in GAPS + [(4, 0), (-2, -1), (-3, 1), (2, -1)]:
        for f in FLAGS:
            wants = [ends_ref(t, p, S, go, ge, f) for t, p in zip(texts, patterns)]
            check_both(eng, ENDS | f, texts, patterns, S, go, ge, wants, "empty", Rs=(1, 8))
    sc = eng.score_batch(ENDS | PE, texts, patterns, S, -3, gap_extend=1)
    assert [cell(s) for s in sc[:3]] == [(0, 0, 0), (-1, 0, 5), (3, 1, 0)]
    got = eng.align_pairs_affine(OVERLAP, texts, patterns, S, 11, 2)
    assert [(g["score"], g["num_bytes"], g["start_text"], g["start_pattern"]) for g in got[:3]] == [(0, 0, 0, 0)] * 3


@gpu
def test_long_gaps_under_overlap(eng):
    S = matrix("blosum50", 23)
    names = list(LONG_GAPS)
    texts, patterns = [LONG_GAPS[k][0] for k in names], [LONG_GAPS[k][1] for k in names]
    wants = [ends_ref(t, p, S, 11, 1, 15) for t, p in zip(texts, patterns)]
    check_both(eng, OVERLAP, texts, patterns, S, 11, 1, wants, "long gaps")


# ---- 7. more pairs than waves, reruns -------------------------------------------------------------------------------
MANY_GAP = (9, 1)


def digest(results):
    return hashlib.sha256(json.dumps([[r[k] for k in KEYS] for r in results]).encode()).hexdigest()


@gpu
def test_pairs_outnumber_waves_and_reruns(eng):
    S = matrix("blast", 4)
    texts, patterns = many_pairs()
    assert len(texts) == 3000
    got = eng.align_pairs_affine(OVERLAP, texts, patterns, S, *MANY_GAP)
    scores = eng.score_batch(OVERLAP, texts, patterns, S, MANY_GAP[0], gap_extend=MANY_GAP[1])
    rng = np.random.default_rng(3)
    for k in rng.choice(len(texts), 150, replace=False):
        want = ends_ref(texts[k], patterns[k], S, *MANY_GAP, 15)
        assert pick(got[k]) == pick(want), int(k)
        assert cell(scores[k]) == cell(want), int(k)
    assert [g["score"] for g in got] == scores["score"].tolist()
    assert digest(eng.align_pairs_affine(OVERLAP, texts, patterns, S, *MANY_GAP)) == digest(got)
    assert eng.score_batch(OVERLAP, texts, patterns, S, MANY_GAP[0], gap_extend=MANY_GAP[1]).tolist() == scores.tolist()


# ---- 8. search -------------------------------------------------------------------------------------------------------
@gpu
def test_search_for_texts_that_end_with_the_head_of_the_query(eng):
    rng = np.random.default_rng(29)
    S = matrix("blast", 4)
    K, mode = 10, ENDS | TB | PE
    q = synthetic.random_sequence(901, 150, 4)
    texts = []
    for k in range(300):
        n = int(rng.integers(100, 301))
        t = synthetic.random_sequence(4000 + k, n, 4).copy()
        if k % 4 == 0:  # some texts end with a mutated copy of the query's first letters
            L = int(rng.integers(40, 100))
            t[n - L:] = synthetic.mutate(q[:L], 2000 + k, 4, L)
        texts.append(t.astype(np.int8))
    # texts 8 and 40 end with the query's first 120 letters themselves: the top two ranks tie, the lower index first
    texts[8] = np.concatenate([synthetic.random_sequence(43, 60, 4), q[:120]]).astype(np.int8)
    texts[40] = texts[8].copy()
    for gap, ge in ((5, None), (11, 2)):
        go, gx = (gap, gap) if ge is None else (gap, ge)
        scores, hits = eng.search(mode, q, texts, S, gap, K, gap_extend=ge)
        assert scores.tolist() == eng.score_batch(mode, texts, [q] * 300, S, gap, gap_extend=ge).tolist(), ge
        rank = sorted(range(300), key=lambda i: (-int(scores["score"][i]), i))
        assert [h["index"] for h in hits] == rank[:K], ge
        assert rank[:2] == [8, 40] and scores[8] == scores[40] and cell(scores[8]) == (5 * 120, 120, 180)
        assert all(i % 4 == 0 for i in rank[2:K])  # then the texts that end with a mutated head
        wants = {}
        for h in hits:
            wants[h["index"]] = want = ends_ref(texts[h["index"]], q, S, go, gx, TB | PE)
            assert pick(h) == pick(want), (ge, h["index"])
            assert cell(scores[h["index"]]) == cell(want), (ge, h["index"])
        assert (hits[0]["start_text"], hits[0]["start_pattern"], hits[0]["aligned_pattern"]) == (60, 0, "".join("ATCG"[c] for c in q[:120]))
        # k = 0: scores only; k beyond the texts: every text
        s0, h0 = eng.search(mode, q, texts[:9], S, gap, 0, gap_extend=ge)
        assert h0 == [] and s0.tolist() == scores[:9].tolist()
        s9, h9 = eng.search(mode, q, texts[:9], S, gap, 12, gap_extend=ge)
        assert [h["index"] for h in h9] == sorted(range(9), key=lambda i: (-int(scores["score"][i]), i))
        for h in h9:
            assert pick(h) == pick(ends_ref(texts[h["index"]], q, S, go, gx, TB | PE)), (ge, h["index"])


# ---- 9. errors ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("side", ["text", "pattern"])
@pytest.mark.parametrize("A", [4, 23])
def test_out_of_alphabet_byte_is_rejected(eng, side, A):
    S = scheme(A)
    t, p = related_pair(11, 150, 90, A)
    (t if side == "text" else p)[70] = A
    for mode in (OVERLAP, ENDS | TB | PE, ENDS):
        calls = [lambda: eng.score_batch(mode, [t, t[:10]], [p, p[:10]], S, 5),
                 lambda: eng.score_batch(mode, [t, t[:10]], [p, p[:10]], S, 11, gap_extend=2),
                 lambda: eng.align_pairs_affine(mode, [t, t[:10]], [p, p[:10]], S, 11, 2),
                 lambda: eng.search(mode, p, [t, t[:10]], S, 5, 2),
                 lambda: eng.search(mode, p, [t, t[:10]], S, 11, 2, gap_extend=2)]
        for call in calls:
            with pytest.raises(eng.SaError) as e:
                call()
            assert e.value.code == 1  # SA_ERR_INVALID


@gpu
def test_the_plans_and_the_band_answer_unsupported(eng):
    S = matrix("blast", 4)
    x = synthetic.random_sequence(1, 50, 4)
    for mode in (ENDS, ENDS | TB | PE, OVERLAP):
        calls = [lambda: eng.Plan(mode, S, 5, [(0, 50, 0, 50)]),
                 lambda: eng.align_pair(mode, x, x, S, 5),
                 lambda: eng.align_batch(mode, [x], [x], S, 5)]
        for call in calls:
            with pytest.raises(eng.SaError) as e:
                call()
            assert e.value.code == 4  # SA_ERR_UNSUPPORTED
            assert "sa_align_pairs_affine" in str(e.value) and "sa_search" in str(e.value) and "sa_score_batch" in str(e.value)
        banded = [lambda: eng.score_batch(mode, [x], [x], S, 11, gap_extend=2, band=8),
                  lambda: eng.score_batch(mode, [x], [x], S, 5, band=8),
                  lambda: eng.Scorer(mode, S, 11, [(0, 50, 0, 50)], gap_extend=2, band=8),
                  lambda: eng.align_pairs_affine(mode, [x], [x], S, 11, 2, band=8)]
        for call in banded:
            with pytest.raises(eng.SaError) as e:
                call()
            assert e.value.code == 4
    for bad in (15, 32, 3, 48):  # any other mode is still a bad argument
        for call in (lambda: eng.score_batch(bad, [x], [x], S, 5), lambda: eng.score_batch(bad, [x], [x], S, 11, gap_extend=2),
                     lambda: eng.align_pairs_affine(bad, [x], [x], S, 11, 2), lambda: eng.search(bad, x, [x], S, 5, 1)):
            with pytest.raises(eng.SaError) as e:
                call()
            assert e.value.code == 1


@gpu
def test_the_python_names(eng):
    assert (eng.ENDS_FREE, eng.FREE_TEXT_BEGIN, eng.FREE_TEXT_END, eng.FREE_PATTERN_BEGIN, eng.FREE_PATTERN_END) == (16, 1, 2, 4, 8)
    assert eng.OVERLAP == 31 == eng.ends_free(True, True, True, True) and eng.ends_free() == 16
    assert eng.ends_free(text_begin=True, pattern_end=True) == ENDS | TB | PE
    assert eng.ends_free(pattern_begin=True, text_end=True) == ENDS | PB | TE


# ---- 10. the C++ functions -----------------------------------------------------------------------------------------
@gpu
def test_cpp_ends_check():
    out = subprocess.run([os.path.join(PKG, "bin", "sa_ends_check"), "300", "96"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1] == "OK 96"
