"""GPU: the score-only path under affine gap penalties (sa_score_batch_affine, sa_scorer_create_affine,
scoreSequencesGPUAffine). The reference has no affine code, so parity is pinned at three points: with
gap_open == gap_extend the recurrence is the reference's linear one and its 894 recorded results
apply; the general case is checked against gotoh_ref below, an independent numpy restatement; and
gotoh_ref is itself checked against a naive triple loop and against the oracle."""
from __future__ import annotations

import itertools
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, encode, matrix
from sa_amd import synthetic
from test_score_gpu import golden_groups, oracle_score, related_pair  # noqa: F401  (golden_groups: a fixture)

pytestmark = pytest.mark.gpu

GLOBAL, LOCAL = 0, 1
NEG = -(1 << 40)  # minus infinity: no score comes near it


def gotoh_ref(mode, t, p, S, go, ge):
    """(score, end_pattern, end_text) of Gotoh's recurrence, swept by anti-diagonals: a cell needs only
    the two diagonals before its own, so each diagonal is a handful of array operations. H, E and F
    are indexed by the row i; E of column 0 and F of row 0 are minus infinity. Global: H[m][n] at
    (m, n). Local: the maximum of H at its first cell in row-major order, (0, 0) when it is 0."""
    t, p = np.asarray(t, dtype=np.int64), np.asarray(p, dtype=np.int64)
    S = np.asarray(S, dtype=np.int64)
    n, m = len(t), len(p)
    local = mode == LOCAL
    if n == 0 or m == 0:
        k = max(n, m)
        return (0, 0, 0) if local else (-(go + (k - 1) * ge) if k else 0, m, n)

    def border(k):  # H[0][k] = H[k][0]
        return 0 if local or k == 0 else -(go + (k - 1) * ge)

    H2 = np.full(m + 1, NEG, dtype=np.int64)  # diagonal d - 2
    H1, E1, F1 = H2.copy(), H2.copy(), H2.copy()  # diagonal d - 1
    H2[0] = 0
    H1[0] = H1[1] = border(1)
    best, bi, bj = 0, 0, 0
    h = None
    for d in range(2, n + m + 1):
        lo, hi = max(1, d - n), min(m, d - 1)  # rows of the diagonal's inner cells, columns j = d - i
        i = np.arange(lo, hi + 1)
        e = np.maximum(E1[lo:hi + 1] - ge, H1[lo:hi + 1] - go)
        f = np.maximum(F1[lo - 1:hi] - ge, H1[lo - 1:hi] - go)
        h = np.maximum(H2[lo - 1:hi] + S[p[i - 1], t[d - i - 1]], np.maximum(e, f))
        if local:
            h = np.maximum(h, 0)
            k = int(h.argmax())  # the first maximum: the smallest row of this diagonal
            hk, ik = int(h[k]), lo + k
            if hk > best or (hk == best and hk > 0 and (ik, d - ik) < (bi, bj)):
                best, bi, bj = hk, ik, d - ik
        Hn, En, Fn = (np.full(m + 1, NEG, dtype=np.int64) for _ in range(3))
        Hn[lo:hi + 1], En[lo:hi + 1], Fn[lo:hi + 1] = h, e, f
        if d <= n:
            Hn[0] = border(d)
        if d <= m:
            Hn[d] = border(d)
        H2, H1, E1, F1 = H1, Hn, En, Fn
    return (best, bi, bj) if local else (int(h[0]), m, n)


def gotoh_matrix(mode, t, p, S, go, ge):
    """H of the same recurrence as a plain double loop over the cells (for the tests that need every cell)."""
    n, m = len(t), len(p)
    local = mode == LOCAL
    H = np.zeros((m + 1, n + 1), dtype=np.int64)
    if not local:
        H[0, 1:] = [-(go + (j - 1) * ge) for j in range(1, n + 1)]
        H[1:, 0] = [-(go + (i - 1) * ge) for i in range(1, m + 1)]
    F = [NEG] * (n + 1)
    for i in range(1, m + 1):
        E, row, prev, Sr = NEG, H[i], H[i - 1], S[p[i - 1]]
        for j in range(1, n + 1):
            E = max(E - ge, int(row[j - 1]) - go)
            F[j] = max(F[j] - ge, int(prev[j]) - go)
            v = max(int(prev[j - 1]) + int(Sr[t[j - 1]]), E, F[j])
            row[j] = max(v, 0) if local else v
    return H


def gotoh_naive(mode, t, p, S, go, ge):
    """The textbook statement without E and F: a cell is the diagonal step or a gap of any length k
    that ends in it, gap_open + (k - 1) gap_extend from the cell it leaves. A triple loop."""
    n, m = len(t), len(p)
    local = mode == LOCAL
    H = [[0] * (n + 1) for _ in range(m + 1)]
    if not local:
        for j in range(1, n + 1):
            H[0][j] = -(go + (j - 1) * ge)
        for i in range(1, m + 1):
            H[i][0] = -(go + (i - 1) * ge)
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            v = H[i - 1][j - 1] + int(S[p[i - 1]][t[j - 1]])
            v = max(v, max(H[i][j - k] - (go + (k - 1) * ge) for k in range(1, j + 1)))
            v = max(v, max(H[i - k][j] - (go + (k - 1) * ge) for k in range(1, i + 1)))
            H[i][j] = max(v, 0) if local else v
    return np.array(H, dtype=np.int64)


def scored_cell(mode, H):
    """(score, end_pattern, end_text) of a full H matrix, by the rule of sa_score_result."""
    if mode == GLOBAL:
        return int(H[-1, -1]), H.shape[0] - 1, H.shape[1] - 1
    if H.max() <= 0:
        return 0, 0, 0
    i, j = np.unravel_index(int(H.argmax()), H.shape)  # the first maximum in row-major order
    return int(H[i, j]), int(i), int(j)


def triple(r):
    return int(r["score"]), int(r["end_pattern"]), int(r["end_text"])


_REF = {}


def ref_cached(key, mode, t, p, S, go, ge):
    """gotoh_ref once per case, shared by the parametrised tests that meet the case again."""
    if key not in _REF:
        _REF[key] = gotoh_ref(mode, t, p, S, go, ge)
    return _REF[key]


# ---- 1. the reference of this file is sound (CPU) --------------------------------------------------
def test_gotoh_ref_equals_the_naive_loops_and_the_oracle():
    rng = np.random.default_rng(31)
    S = matrix("blast", 4)
    pairs = []
    for k in range(20):
        n, m = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        t = synthetic.random_sequence(100 + k, n, 4)
        p = synthetic.mutate(np.resize(t, m), 200 + k, 4, m) if k % 2 else synthetic.random_sequence(300 + k, m, 4)
        pairs.append((t, p))
    for mode in (GLOBAL, LOCAL):
        for t, p in pairs:
            for go, ge in ((10, 1), (12, 2), (3, 7), (0, 0), (-2, -2)):
                want = scored_cell(mode, gotoh_naive(mode, t, p, S, go, ge))
                assert gotoh_ref(mode, t, p, S, go, ge) == want, (mode, len(t), len(p), go, ge)
                assert scored_cell(mode, gotoh_matrix(mode, t, p, S, go, ge)) == want, (mode, len(t), len(p), go, ge)
            assert gotoh_ref(mode, t, p, S, 5, 5) == oracle_score(mode, t, p, S, 5), (mode, len(t), len(p))


# ---- 2. gap_open == gap_extend is the linear gap: the reference's recorded pairs -------------------------
@pytest.mark.parametrize("rows_per_lane", [0, 1, 4, 8])
def test_degenerate_affine_equals_the_reference_goldens(eng, golden_groups, rows_per_lane):  # noqa: F811
    checked = 0
    for mode, S, gap, texts, patterns, scores in golden_groups:
        got = eng.score_batch(mode, texts, patterns, S, gap, rows_per_lane=rows_per_lane, gap_extend=gap)
        assert got["score"].tolist() == scores, (mode, S.shape, gap)
        assert (got["status"] == 0).all()
        checked += len(scores)
    assert checked == 894


# ---- 3. strip and body edges ---------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_strip_and_body_edges(eng, R):
    """First and last lanes, partial strips, the row buffer reused by a third strip, and the body
    boundaries at 64 and 128 columns, at the smallest shapes that have them."""
    ms = [1, 63, 64, 65, 64 * R, 64 * R + 1, 2 * 64 * R + 3]
    ns = [1, 63, 64, 65, 129, 300]
    go, ge = 11, 2
    for A, mat in ((4, "blast"), (23, "blosum50")):
        S = matrix(mat, A)
        shapes = list(itertools.product(ms, ns))
        pairs = [related_pair(7000 + 3 * m + 5 * n + A, n, m, A) for m, n in shapes]  # the same pair at every R
        texts, patterns = [t for t, _ in pairs], [p for _, p in pairs]
        for mode in (GLOBAL, LOCAL):
            got = eng.score_batch(mode, texts, patterns, S, go, rows_per_lane=R, gap_extend=ge)
            for k, (t, p) in enumerate(pairs):
                want = ref_cached(("edges", A, mode) + shapes[k], mode, t, p, S, go, ge)
                assert triple(got[k]) == want, (A, mode, len(p), len(t))


# ---- 4. affine really differs from linear ----------------------------------------------------------------
@pytest.mark.parametrize("longer", ["text", "pattern"])
def test_one_long_gap_is_one_event(eng, longer):
    """200 letters against the same with a block of 20 left out, +5 / -4. Any alignment of 180 letters
    to 200 has at least 20 gap cells: open 12 / extend 1 pays 31 for the block (at least 900 - 31),
    a linear 12 pays 240 (at most 900 - 240). longer = "text": the gap runs along the row (E);
    longer = "pattern": down the column (F)."""
    S = matrix("blast", 4)
    texts, patterns = [], []
    for k, cut in enumerate([0, 10, 37, 64, 90, 128, 155, 180]):
        full = synthetic.random_sequence(900 + k, 200, 4)
        short = np.concatenate([full[:cut], full[cut + 20:]])
        texts.append(full if longer == "text" else short)
        patterns.append(short if longer == "text" else full)
    for go, ge in ((12, 1), (12, 12)):
        want = [gotoh_ref(GLOBAL, t, p, S, go, ge) for t, p in zip(texts, patterns)]
        if ge == 1:
            assert all(w[0] >= 869 for w in want), want
        else:
            assert all(w[0] <= 660 for w in want), want
        got = eng.score_batch(GLOBAL, texts, patterns, S, go, gap_extend=ge)
        assert [triple(r) for r in got] == want, (go, ge)


# ---- 5. local ties ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(60, 200), (200, 200), (300, 150)])
@pytest.mark.parametrize("R", [0, 1, 2, 8])
def test_local_ties_take_the_first_cell_in_row_major_order(eng, m, n, R):
    S = matrix("blast", 4)
    x1, x2 = "ATCGACTG", "GGAACCTT"
    t = encode(x2 + "A" * (n - 16) + x1, 4)
    p = encode(x1 + "T" * (m - 16) + x2, 4)
    go, ge = 10, 1
    if R == 0:  # the premise, once per shape: two cells hold the maximum 40, the earlier row wins
        H = gotoh_matrix(LOCAL, t, p, S, go, ge)
        assert H.max() == 40 and sorted(zip(*np.nonzero(H == 40))) == sorted([(8, n), (m, 8)])
    assert ref_cached(("ties", m, n), LOCAL, t, p, S, go, ge) == (40, 8, n)
    got = eng.score_batch(LOCAL, [t], [p], S, go, rows_per_lane=R, gap_extend=ge)[0]
    assert triple(got) == (40, 8, n)


# ---- 6. thousands of mixed pairs, a scorer run twice ---------------------------------------------------------
def test_pairs_outnumber_waves_and_scorer_reruns(eng):
    """3000 pairs of 1..200 letters through one affine Scorer, twice, the second time over other
    letters; every seventh pair against the reference both times."""
    import torch
    rng = np.random.default_rng(20241019)
    N = 3000
    nl, ml = rng.integers(1, 201, N), rng.integers(1, 201, N)
    S = matrix("blast", 4)
    go, ge = 9, 1
    to, po = np.concatenate([[0], np.cumsum(nl)]), np.concatenate([[0], np.cumsum(ml)])
    pairs = [(int(to[k]), int(nl[k]), int(po[k]), int(ml[k])) for k in range(N)]
    # R = 1: patterns of more than 64 letters run several strips through the wave's boundary row
    sc = eng.Scorer(LOCAL, S, go, pairs, rows_per_lane=1, gap_extend=ge)
    info = sc.info()
    assert info["rows_per_lane"] == 1 and 0 < info["num_waves"] <= N
    for run in range(2):
        ta = synthetic.random_sequence(177 + run, int(to[-1]), 4)
        pa = synthetic.mutate(np.resize(ta, int(po[-1])), 199 + run, 4, int(po[-1]))
        dt, dp = torch.from_numpy(ta).cuda(), torch.from_numpy(pa).cuda()
        sc.run(dt.data_ptr(), dp.data_ptr())
        got = sc.results()
        assert (got["status"] == 0).all()
        for k in range(0, N, 7):
            t, p = ta[to[k]:to[k + 1]], pa[po[k]:po[k + 1]]
            assert triple(got[k]) == gotoh_ref(LOCAL, t, p, S, go, ge), (run, k, len(t), len(p))
    sc.close()


def test_query_against_a_database_shares_one_pattern(eng):
    """Every pair at pattern_offset 0, as a search does; protein, automatic R."""
    import torch
    rng = np.random.default_rng(8)
    S = matrix("blosum50", 23)
    q = synthetic.random_sequence(51, 150, 20)
    lens = rng.integers(30, 260, 60)
    offs = np.concatenate([[0], np.cumsum(lens)])
    ta = synthetic.random_sequence(52, int(offs[-1]), 20)
    for k in range(0, 60, 4):  # some texts hold a mutated piece of the query
        L = min(int(lens[k]), 120)
        ta[offs[k]:offs[k] + L] = synthetic.mutate(q, 60 + k, 20, L)
    sc = eng.Scorer(LOCAL, S, 12, [(int(offs[k]), int(lens[k]), 0, 150) for k in range(60)], gap_extend=2)
    dt, dq = torch.from_numpy(ta).cuda(), torch.from_numpy(q).cuda()
    sc.run(dt.data_ptr(), dq.data_ptr())
    got = sc.results()
    sc.close()
    for k in range(60):
        assert triple(got[k]) == gotoh_ref(LOCAL, ta[offs[k]:offs[k + 1]], q, S, 12, 2), k


# ---- 7. bad input -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["text", "pattern"])
@pytest.mark.parametrize("A", [4, 23])
def test_out_of_alphabet_byte_is_rejected(eng, side, A):
    S = matrix("blast" if A == 4 else "blosum50", A)
    t, p = related_pair(11, 150, 90, A)
    (t if side == "text" else p)[70] = A
    with pytest.raises(eng.SaError) as e:
        eng.score_batch(GLOBAL, [t, t[:10]], [p, p[:10]], S, 11, gap_extend=2)
    assert e.value.code == 1  # SA_ERR_INVALID


# ---- 8. empty sides -------------------------------------------------------------------------------------------
def test_empty_sides(eng):
    S = matrix("blast", 4)
    x, none = synthetic.random_sequence(5, 37, 4), np.zeros(0, dtype=np.int8)
    go, ge = 11, 2
    texts, patterns = [none, x, none, x[:1], none], [x, none, none, none, x[:1]]
    got = eng.score_batch(GLOBAL, texts, patterns, S, go, gap_extend=ge)
    assert [triple(r) for r in got] == [(-(go + 36 * ge), 37, 0), (-(go + 36 * ge), 0, 37), (0, 0, 0), (-go, 0, 1),
                                        (-go, 1, 0)]
    assert [triple(r) for r in got] == [gotoh_ref(GLOBAL, t, p, S, go, ge) for t, p in zip(texts, patterns)]
    got = eng.score_batch(LOCAL, texts, patterns, S, go, gap_extend=ge)
    assert [triple(r) for r in got] == [(0, 0, 0)] * 5
    assert (got["status"] == 0).all()


# ---- 9. the C++ extension ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["global", "local"])
def test_cpp_score_affine_check(mode):
    out = subprocess.run([os.path.join(PKG, "bin", "sa_score_affine_check"), mode, "96", "700"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert json.loads(out.stdout.strip().splitlines()[-1])["mismatches"] == 0
