"""Banded extension (sa_hip.h: sa_score_batch_extend_band, sa_scorer_create_extend_band,
sa_align_pairs_extend_band): extension alignment inside |j - i| <= width of the anchor's diagonal. Cells out
of band are minus infinity, border cells included; the row maxima, B and the stop row i* are those of the
banded matrix, and a row without an in-band cell drops under every X >= 0.
The reference of this file is ext_band_ref: test_band_at_gpu.fill_by_diagonals in global mode on the band
{-w, w}, test_extend_gpu.stop_row on it (masked cells are NEG), the first maximum in row-major order over the
rows < i*, and test_align_affine_gpu's walk on the prefixes the result cell cuts. It is pinned on the CPU
against a plain double loop that never touches an out-of-band cell, by re-scoring its strings and by the
identities (W1), (W2) and (W3) of sa_hip.h; the GPU is then compared with it, every forced rows_per_lane of
the scorer and the aligner once."""
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
from test_align_affine_gpu import EDGE_SHAPES, KEYS, NEG, alphabet_of, many_pairs, pick, rescore, walk
from test_band_at_gpu import band_at_ref, fill_by_diagonals
from test_band_gpu import digest
from test_extend_gpu import NONE, SMALL_GAPS, SMALL_X, extend_ref, random_small_pairs, stop_row, xd
from test_fit_gpu import cell
from test_score_gpu import related_pair

gpu = pytest.mark.gpu

GLOBAL, LOCAL, FIT, ENDS = 0, 1, 2, 16
GAPS = [(11, 2), (5, 5)]
SMALL_W = (0, 1, 3, 40)
WIDTHS = (0, 1, 63, 64, 65)


# ---- the reference of this file ------------------------------------------------------------------------
_FILLS = {}  # (key, go, ge, w) -> (H, D): the newest few are kept; the fill does not depend on the X-drop


def banded_fill(t, p, S, go, ge, w, key=None):
    fk = (key, go, ge, w)
    if key is None or fk not in _FILLS:
        H, D = fill_by_diagonals(GLOBAL, t, p, S, go, ge, -w, w)
        if key is None:
            return H, D
        while len(_FILLS) >= 12:
            _FILLS.pop(next(iter(_FILLS)))
        _FILLS[fk] = (H, D)
    return _FILLS[fk]


def ext_band_ref(t, p, S, go, ge, xdrop, w, alphabet=None, key=None):
    """The keys of align_pairs_affine plus end_pattern and end_text of the scorers and stop_row."""
    t, p = np.asarray(t, dtype=np.int64), np.asarray(p, dtype=np.int64)
    n, m = len(t), len(p)
    alphabet = alphabet or alphabet_of(S)
    bi = bj = 0
    istar = m + 1
    if n and m:
        H, D = banded_fill(t, p, S, go, ge, w, key)
        istar = stop_row(H, xdrop)  # a row of NEG lies more than any X below B >= 0
        sub = H[1:istar, 1:]
        if sub.size and sub.max() > 0:
            bi, bj = (int(v) + 1 for v in np.unravel_index(int(sub.argmax()), sub.shape))  # first maximum, row-major
    else:
        H, D = np.zeros((m + 1, n + 1), dtype=np.int64), np.zeros((m + 1, n + 1), dtype=np.uint8)
    assert abs(bj - bi) <= w
    res, ended = walk(GLOBAL, t[:bj], p[:bi], H[:bi + 1, :bj + 1], D[:bi + 1, :bj + 1], go, ge, alphabet)
    assert ended == "origin"
    res["start_text"] = res["start_pattern"] = 0
    res["end_pattern"], res["end_text"], res["stop_row"] = bi, bj, istar
    assert res["score"] == (int(H[bi, bj]) if bi else 0)
    return res


def ext_band_by_loops(t, p, S, go, ge, xdrop, w):
    """(score, end_pattern, end_text, i*) by a plain double loop over the in-band cells alone: a dictionary of
    the cells that exist, r, B and i* row by row; the rows from i* on are not even computed."""
    n, m = len(t), len(p)
    if n == 0 or m == 0:
        return 0, 0, 0, m + 1
    H, E, F = {(0, 0): 0}, {}, {}
    for j in range(1, min(n, w) + 1):
        H[0, j] = -(go + (j - 1) * ge)
    B, best, bi, bj = 0, 0, 0, 0
    for i in range(1, m + 1):
        if i <= w:
            H[i, 0] = -(go + (i - 1) * ge)
        r = None
        for j in range(max(1, i - w), min(n, i + w) + 1):
            e = [v for v in ((E[i, j - 1] - ge) if (i, j - 1) in E else None, (H[i, j - 1] - go) if (i, j - 1) in H else None) if v is not None]
            f = [v for v in ((F[i - 1, j] - ge) if (i - 1, j) in F else None, (H[i - 1, j] - go) if (i - 1, j) in H else None) if v is not None]
            if e:
                E[i, j] = max(e)
            if f:
                F[i, j] = max(f)
            H[i, j] = max(e + f + [H[i - 1, j - 1] + int(S[p[i - 1]][t[j - 1]])])  # the diagonal neighbour of an in-band cell is in band
            if r is None or H[i, j] > r:
                r, rj = H[i, j], j
        if xdrop is not NONE and (r is None or B - r > xdrop):
            return best, bi, bj, i
        if r is not None:
            B = max(B, r)
            if r > best:
                best, bi, bj = r, i, rj
    return best, bi, bj, m + 1


def check(eng, texts, patterns, S, go, ge, xdrop, w, wants, what, Rs=(1, 2, 4, 8)):
    """Every forced rows_per_lane of the banded extension scorer (W4: also through gap_extend=None when
    go == ge), and the banded extension aligner once."""
    for R in Rs:
        got = eng.score_batch(GLOBAL, texts, patterns, S, go, rows_per_lane=R, gap_extend=ge, xdrop=xd(eng, xdrop), width=w)
        assert [cell(g) for g in got] == [cell(x) for x in wants], (what, "score", go, ge, xdrop, w, R)
        if go == ge:
            got = eng.score_batch(GLOBAL, texts, patterns, S, go, rows_per_lane=R, xdrop=xd(eng, xdrop), width=w)
            assert [cell(g) for g in got] == [cell(x) for x in wants], (what, "score, gap_extend=None", go, xdrop, w, R)
    got = eng.align_pairs_affine(GLOBAL, texts, patterns, S, go, ge, xdrop=xd(eng, xdrop), width=w)
    for k, (g, x) in enumerate(zip(got, wants)):
        assert pick(g) == pick(x), (what, "align", go, ge, xdrop, w, k, len(patterns[k]), len(texts[k]))
    return got


# ---- the reference of this file is sound (CPU) ---------------------------------------------------------
def test_the_banded_fill_equals_the_plain_loops():
    for k, (A, t, p) in enumerate(random_small_pairs()):
        S = matrix("blast" if A == 4 else "blosum50", A)
        for go, ge in SMALL_GAPS:
            for w in SMALL_W:
                for x in SMALL_X:
                    want = ext_band_by_loops(t, p, S, go, ge, x, w)
                    got = ext_band_ref(t, p, S, go, ge, x, w, key=("small", k))
                    assert cell(got) + (got["stop_row"],) == want, (k, go, ge, x, w)


def test_the_strings_rescore_and_w1_w2_w3_hold_on_the_reference():
    bound = 0
    for k, (A, t, p) in enumerate(random_small_pairs(20, 53300)):
        S = matrix("blast" if A == 4 else "blosum50", A)
        alpha = alphabet_of(S)
        n, m = len(t), len(p)
        for go, ge in SMALL_GAPS:
            for x in SMALL_X:
                full = extend_ref(t, p, S, go, ge, x, key=("w small", k))
                # W1: a width that admits every cell
                for w in (max(n, m), 1 << 30):
                    assert ext_band_ref(t, p, S, go, ge, x, w) == full, (k, go, ge, x, w)
                last = None
                for w in SMALL_W:
                    res = ext_band_ref(t, p, S, go, ge, x, w, key=("w small", k))
                    if 0 <= ge <= go:
                        assert rescore(res, S, go, ge, alpha) == res["score"], (k, go, ge, x, w)
                    assert res["aligned_text"].replace("-", "") == "".join(alpha[c] for c in t[:res["end_text"]])
                    assert res["aligned_pattern"].replace("-", "") == "".join(alpha[c] for c in p[:res["end_pattern"]])
                    # the walk stays in band
                    i, j = res["end_pattern"], res["end_text"]
                    for a, b in zip(reversed(res["aligned_text"]), reversed(res["aligned_pattern"])):
                        j, i = j - (a != "-"), i - (b != "-")
                        assert abs(j - i) <= w
                    # W2: the global band-at alignment of the prefixes inside {-w, w}
                    g = band_at_ref(GLOBAL, t[:res["end_text"]], p[:res["end_pattern"]], S, go, ge, -w, w)
                    assert (g["score"], g["aligned_text"], g["aligned_pattern"]) == (res["score"], res["aligned_text"], res["aligned_pattern"])
                    # W3: without a drop, non-decreasing in w and never above the unbanded score
                    if x is NONE:
                        assert (last is None or res["score"] >= last) and res["score"] <= full["score"], (k, go, ge, w)
                        last = res["score"]
                        bound += res["score"] < full["score"]
    assert bound >= 8  # the band binds in the small cases too


# ---- 1. edge shapes ----------------------------------------------------------------------------------------
SHAPES = EDGE_SHAPES + [(63, 70), (65, 60), (511, 520), (513, 500)]  # (m, n)


def shape_pairs(A, seed=81000):
    pairs = [related_pair(seed + 3 * m + 5 * n + A, n, m, A) for m, n in SHAPES]
    return [t for t, _ in pairs], [p for _, p in pairs]


@gpu
@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("go,ge", GAPS)
@pytest.mark.parametrize("A,mat", [(4, "blast"), (23, "blosum50")])
def test_edge_shapes(eng, A, mat, go, ge, w):
    S = matrix(mat, A)
    texts, patterns = shape_pairs(A)
    for x in (NONE, 20):
        wants = [ext_band_ref(t, p, S, go, ge, x, w, key=("shape", A, k)) for k, (t, p) in enumerate(zip(texts, patterns))]
        check(eng, texts, patterns, S, go, ge, x, w, wants, "edges")


# ---- 2. W1 on the device -------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("go,ge", GAPS)
def test_w1_on_the_device(eng, go, ge):
    S = matrix("blast", 4)
    texts, patterns = shape_pairs(4)
    for x in (eng.NO_XDROP, 20):
        for R in (1, 2, 4, 8):
            full = eng.score_batch(GLOBAL, texts, patterns, S, go, rows_per_lane=R, gap_extend=ge, xdrop=x)
            # one width per call: every pair's own max(n, m), pair by pair, and 2^30 for all at once
            own = [eng.score_batch(GLOBAL, [t], [p], S, go, rows_per_lane=R, gap_extend=ge, xdrop=x, width=max(len(t), len(p)))[0]
                   for t, p in zip(texts, patterns)] if R == 8 else None
            big = eng.score_batch(GLOBAL, texts, patterns, S, go, rows_per_lane=R, gap_extend=ge, xdrop=x, width=1 << 30)
            assert big.tobytes() == full.tobytes(), (go, ge, x, R)
            if own is not None:
                assert [cell(o) for o in own] == [cell(f) for f in full], (go, ge, x)
        full = eng.align_pairs_affine(GLOBAL, texts, patterns, S, go, ge, xdrop=x)
        assert eng.align_pairs_affine(GLOBAL, texts, patterns, S, go, ge, xdrop=x, width=1 << 30) == full
        assert eng.align_pairs_affine(GLOBAL, texts, patterns, S, go, ge, xdrop=x, width=max(max(len(t), len(p)) for t, p in zip(texts, patterns))) == full


# ---- 3. tall and wide pairs: rows past n + w, strips with empty windows, columns never reached ---------------
@gpu
@pytest.mark.parametrize("w", (0, 5, 64))
def test_tall_and_wide_pairs(eng, w):
    S = matrix("blast", 4)
    pairs = [related_pair(8300 + 3 * m + 5 * n, n, m, 4) for m, n in ((700, 100), (100, 700))]
    texts, patterns = [t for t, _ in pairs], [p for _, p in pairs]
    for go, ge in GAPS:
        for x in (NONE, 20):
            wants = [ext_band_ref(t, p, S, go, ge, x, w, key=("tall", k)) for k, (t, p) in enumerate(pairs)]
            if x is not NONE:
                assert wants[0]["stop_row"] <= 100 + w + 1  # the first row without an in-band cell drops at the latest
            check(eng, texts, patterns, S, go, ge, x, w, wants, "tall and wide")


# ---- 4. the band binds ------------------------------------------------------------------------------------------
def inserted_pairs(count=20, seed=8400):
    """A pattern of 120 letters and its text: the pattern lightly mutated, with 12 foreign letters inserted at
    its middle. Beyond the block the alignment lies 12 diagonals off the anchor's."""
    out = []
    for k in range(count):
        p = synthetic.random_sequence(seed + 2 * k, 120, 4).astype(np.int8)
        src = synthetic.mutate(p, seed + 2 * k + 1, 4, 120).astype(np.int8)
        block = synthetic.random_sequence(seed + 500 + k, 12, 4).astype(np.int8)
        out.append((np.concatenate([src[:60], block, src[60:]]).astype(np.int8), p))
    return out


def inserted_wants(S, go, ge, w):
    return [ext_band_ref(t, p, S, go, ge, NONE, w, key=("inserted", k)) for k, (t, p) in enumerate(inserted_pairs())]


def test_the_band_binds_on_the_reference():
    S = matrix("blast", 4)
    narrow, wide = inserted_wants(S, 11, 2, 5), inserted_wants(S, 11, 2, 64)
    differ = sum(cell(a) != cell(b) for a, b in zip(narrow, wide))
    assert 2 * differ >= len(narrow), differ
    assert all(a["score"] <= b["score"] for a, b in zip(narrow, wide))


@gpu
def test_the_band_binds(eng):
    S = matrix("blast", 4)
    pairs = inserted_pairs()
    texts, patterns = [t for t, _ in pairs], [p for _, p in pairs]
    narrow, wide = inserted_wants(S, 11, 2, 5), inserted_wants(S, 11, 2, 64)
    assert 2 * sum(cell(a) != cell(b) for a, b in zip(narrow, wide)) >= len(pairs)
    check(eng, texts, patterns, S, 11, 2, NONE, 5, narrow, "binds, narrow")
    check(eng, texts, patterns, S, 11, 2, NONE, 64, wide, "binds, wide")


# ---- 5. the drop fires inside the band --------------------------------------------------------------------------
DROP_GAP, DROP_X, DROP_W = (16, 4), 50, (5, 16, 64)
LINEAR_GAP = (12, 12)  # a linear gap dear enough that unrelated letters lose score row after row


def chimeric_pairs(count=10, seed=8500, length=600, related=150):
    out = []
    for k in range(count):
        t = synthetic.random_sequence(seed + 2 * k, length, 4).astype(np.int8)
        p = synthetic.random_sequence(seed + 2 * k + 1, length, 4).astype(np.int8)
        p[:related] = synthetic.mutate(t[:related], seed + 900 + k, 4, related)
        out.append((t, p))
    return out


def chimeric_wants(S, go, ge, w):
    return [ext_band_ref(t, p, S, go, ge, DROP_X, w, key=("chimeric", k)) for k, (t, p) in enumerate(chimeric_pairs())]


@pytest.mark.parametrize("go,ge", [DROP_GAP, LINEAR_GAP])
def test_the_drop_fires_inside_the_band_on_the_reference(go, ge):
    S = matrix("blast", 4)
    for w in DROP_W:
        wants = chimeric_wants(S, go, ge, w)
        rows = [x["stop_row"] for x in wants]
        assert all(r <= 600 for r in rows), (w, rows)             # every case stops before row m
        assert len({(r - 1) // 64 for r in rows}) >= 2, (w, rows)  # in at least two different 64-row strips
        assert all(x["score"] > 200 for x in wants)  # and each got well into its related part first


@gpu
@pytest.mark.parametrize("go,ge", [DROP_GAP, LINEAR_GAP])
@pytest.mark.parametrize("w", DROP_W)
def test_the_drop_fires_inside_the_band(eng, go, ge, w):
    S = matrix("blast", 4)
    pairs = chimeric_pairs()
    wants = chimeric_wants(S, go, ge, w)
    assert all(x["stop_row"] <= 600 for x in wants)
    check(eng, [t for t, _ in pairs], [p for _, p in pairs], S, go, ge, DROP_X, w, wants, "drop")


# ---- 6. ties: the row-major-first of two equal maxima lies out of band ------------------------------------------
TIE_W = 25


def tie_pair():
    """X over letters 0 and 1. The text is 30 letters 2 and X; the pattern is X, 30 letters 3 and X. Under free
    gaps the unbanded maximum 5 |X| is first met at (|X|, 30 + |X|), 30 diagonals off; inside a width of 25 only
    the pattern's second X reaches it, at (|X| + 30 + |X|, 30 + |X|), 20 diagonals off."""
    X = synthetic.random_sequence(86, 20, 2).astype(np.int8)
    t = np.concatenate([np.full(30, 2, dtype=np.int8), X]).astype(np.int8)
    p = np.concatenate([X, np.full(30, 3, dtype=np.int8), X]).astype(np.int8)
    return t, p


def test_the_tie_pair_holds_its_tie():
    S = matrix("blast", 4)
    t, p = tie_pair()
    assert cell(extend_ref(t, p, S, 0, 0, NONE)) == (100, 20, 50)
    assert cell(ext_band_ref(t, p, S, 0, 0, NONE, TIE_W)) == (100, 70, 50)
    H, _ = banded_fill(t, p, S, 0, 0, 1 << 20)
    assert int(H[20, 50]) == int(H[70, 50]) == int(H[1:, 1:].max()) == 100  # two equal maxima of the unbanded matrix


@gpu
def test_ties(eng):
    S = matrix("blast", 4)
    t, p = tie_pair()
    for go, ge in ((0, 0), (4, 0)):
        for x in (NONE, 20):
            for w in (TIE_W, 19, 30):
                check(eng, [t], [p], S, go, ge, x, w, [ext_band_ref(t, p, S, go, ge, x, w, key="tie")], "ties")


# ---- 7. pairs outnumber waves; a scorer run again on new arena contents ------------------------------------------
def mixed_pairs():
    """many_pairs three times over with a tall, a wide, an inserted and a chimeric pair in every 25th place."""
    texts, patterns = many_pairs()
    texts, patterns = list(texts) * 3, list(patterns) * 3
    special = [related_pair(8300 + 3 * 700 + 5 * 100, 100, 700, 4), related_pair(8300 + 3 * 100 + 5 * 700, 700, 100, 4),
               inserted_pairs(1)[0], chimeric_pairs(1)[0]]
    for k in range(0, len(texts), 25):
        texts[k], patterns[k] = (np.asarray(a, dtype=np.int8) for a in special[(k // 25) % len(special)])
    return texts, patterns


@gpu
@pytest.mark.parametrize("w,x", [(5, 20), (64, NONE)])
def test_pairs_outnumber_waves_and_reruns(eng, w, x):
    import torch
    S = matrix("blast", 4)
    go, ge = 11, 2
    texts, patterns = mixed_pairs()
    to = np.concatenate([[0], np.cumsum([len(t) for t in texts])])
    po = np.concatenate([[0], np.cumsum([len(p) for p in patterns])])
    dt, dp = torch.from_numpy(np.concatenate(texts)).cuda(), torch.from_numpy(np.concatenate(patterns)).cuda()
    sc = eng.Scorer(GLOBAL, S, go, [(int(to[k]), len(texts[k]), int(po[k]), len(patterns[k])) for k in range(len(texts))],
                    gap_extend=ge, xdrop=xd(eng, x), width=w)
    assert sc.info()["num_waves"] < len(texts)
    sc.run(dt.data_ptr(), dp.data_ptr())
    first = sc.results().copy()
    # new arena contents of the same shapes: every sequence reversed in place
    rt, rp = [t[::-1].copy() for t in texts], [p[::-1].copy() for p in patterns]
    dt2, dp2 = torch.from_numpy(np.concatenate(rt)).cuda(), torch.from_numpy(np.concatenate(rp)).cuda()
    sc.run(dt2.data_ptr(), dp2.data_ptr())
    second = sc.results().copy()
    sc.run(dt.data_ptr(), dp.data_ptr())
    third = sc.results().copy()
    sc.close()
    assert digest(first.tolist()) == digest(third.tolist())
    assert first.tolist() == eng.score_batch(GLOBAL, texts, patterns, S, go, gap_extend=ge, xdrop=xd(eng, x), width=w).tolist()
    assert second.tolist() == eng.score_batch(GLOBAL, rt, rp, S, go, gap_extend=ge, xdrop=xd(eng, x), width=w).tolist()
    got = eng.align_pairs_affine(GLOBAL, texts, patterns, S, go, ge, xdrop=xd(eng, x), width=w)
    assert [g["score"] for g in got] == first["score"].tolist()
    rng = np.random.default_rng(5)
    for k in list(range(0, 100, 25)) + rng.choice(len(texts), 100, replace=False).tolist():
        want = ext_band_ref(texts[k], patterns[k], S, go, ge, x, w)
        assert cell(first[k]) == cell(want) and pick(got[k]) == pick(want), int(k)
        assert cell(second[k]) == cell(ext_band_ref(rt[k], rp[k], S, go, ge, x, w)), int(k)


# ---- 8. negative and zero penalties ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("go,ge", [(-2, -1), (4, 0)])
def test_negative_and_zero_penalties(eng, go, ge):
    S = matrix("blast", 4)
    pairs = [related_pair(8800 + 3 * m + 5 * n, n, m, 4) for m, n in ((9, 65), (64, 70), (129, 120), (70, 200))]
    texts, patterns = [t for t, _ in pairs], [p for _, p in pairs]
    for w in (0, 3, 64):
        for x in (5, NONE):
            wants = [ext_band_ref(t, p, S, go, ge, x, w, key=("penalties", k)) for k, (t, p) in enumerate(pairs)]
            check(eng, texts, patterns, S, go, ge, x, w, wants, "penalties")


# ---- 11. beyond the arena budget -------------------------------------------------------------------------------------
BIG, BIG_W, BIG_BUDGET = 6000, 64, 8 << 20


def big_pair():
    t = synthetic.random_sequence(181, BIG, 4).astype(np.int8)
    return t, synthetic.mutate(t, 182, 4, BIG).astype(np.int8)


@gpu
def test_a_pair_beyond_the_arena_budget_aligns_inside_its_width():
    """In a process of its own (the budget is read once per process): 6000 x 6000 needs about 18.7 MB of
    directions, the budget is 8 MiB; inside a width of 64 it needs about 2.2 MB and aligns."""
    env = dict(os.environ, SA_TRACE_ARENA_BYTES=str(BIG_BUDGET))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "big"], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    child = json.loads(out.stdout.strip().splitlines()[-1])
    assert child["unbanded_error"] == 4  # SA_ERR_UNSUPPORTED
    plan = subprocess.run([os.path.join(PKG, "bin", "sa_trace_plan_check"), "--mode", "global", "--gap", "11", "--gap-extend", "2",
                           "--budget", str(BIG_BUDGET), "--extend", "none", "--width", str(BIG_W), f"{BIG}x{BIG}"],
                          capture_output=True, text=True, check=True)
    plan = json.loads(plan.stdout)
    assert child["arena_bytes"] == plan["arena_bytes"] and 2.0e6 < plan["arena_bytes"] < 2.4e6
    assert child["num_chunks"] == 1
    # W2: the band-at global aligner on the prefixes, and the strings re-score
    assert child["w2"] is True
    t, p = big_pair()
    S = matrix("blast", 4)
    res = child["result"]
    assert rescore(res, S, 11, 2, alphabet_of(S)) == res["score"] == child["score"][0]
    assert res["aligned_text"].replace("-", "") == "".join("ATCG"[c] for c in t[:child["score"][2]])
    assert res["aligned_pattern"].replace("-", "") == "".join("ATCG"[c] for c in p[:child["score"][1]])
    assert res["num_bytes"] > 5000


def _big_child():
    from sa_amd import engine as eng
    S = matrix("blast", 4)
    t, p = big_pair()
    out = {}
    try:
        eng.align_pairs_affine(GLOBAL, [t], [p], S, 11, 2, xdrop=eng.NO_XDROP)
        out["unbanded_error"] = 0
    except eng.SaError as e:
        out["unbanded_error"] = e.code
    got = eng.align_pairs_affine(GLOBAL, [t], [p], S, 11, 2, xdrop=eng.NO_XDROP, width=BIG_W)[0]
    stats = eng.affine_last_stats()
    sc = eng.score_batch(GLOBAL, [t], [p], S, 11, gap_extend=2, xdrop=eng.NO_XDROP, width=BIG_W)[0]
    et, ep = int(sc["end_text"]), int(sc["end_pattern"])
    pre = eng.align_pairs_affine(GLOBAL, [t[:et]], [p[:ep]], S, 11, 2, bands=[(-BIG_W, BIG_W)])[0]
    out["w2"] = (pre["score"], pre["aligned_text"], pre["aligned_pattern"]) == (got["score"], got["aligned_text"], got["aligned_pattern"])
    out.update(result=got, score=list(cell(sc)), arena_bytes=stats["arena_bytes"], num_chunks=stats["num_chunks"])
    print(json.dumps(out))


# ---- 12. refusals -----------------------------------------------------------------------------------------------------
@gpu
def test_refusals(eng):
    S = matrix("blast", 4)
    x = synthetic.random_sequence(1, 50, 4).astype(np.int8)
    y = x[:20]
    scorer = lambda mode, **kw: eng.Scorer(mode, S, 11, [(0, 50, 0, 20)], gap_extend=2, **kw)  # noqa: E731
    stats = eng.align_pairs_affine(GLOBAL, [x], [y], S, 11, 2, xdrop=20, width=3) and eng.affine_last_stats()
    assert stats["num_chunks"] == 1 and stats["arena_bytes"] > 0
    # a negative width, a bad xdrop, a mode other than global
    for mode, xdrop, w in ((GLOBAL, 20, -1), (GLOBAL, -2, 3), (GLOBAL, 1 << 30, 3), (LOCAL, 20, 3), (FIT, 20, 3), (ENDS | 15, eng.NO_XDROP, 3)):
        for call in (lambda: eng.score_batch(mode, [x], [y], S, 11, gap_extend=2, xdrop=xdrop, width=w),
                     lambda: eng.score_batch(mode, [x], [y], S, 5, xdrop=xdrop, width=w),
                     lambda: scorer(mode, xdrop=xdrop, width=w),
                     lambda: eng.align_pairs_affine(mode, [x], [y], S, 11, 2, xdrop=xdrop, width=w)):
            with pytest.raises(eng.SaError) as e:
                call()
            assert e.value.code == 1, (mode, xdrop, w)
    # the band's sentinel: (max|S| + G)(n + m) + G (n + m) >= 2^29 at G = 2^22, n + m = 70, which the unbanded
    # extension still takes
    assert len(eng.score_batch(GLOBAL, [x], [y], S, 1 << 22, gap_extend=2, xdrop=20)) == 1
    for call in (lambda: eng.score_batch(GLOBAL, [x], [y], S, 1 << 22, gap_extend=2, xdrop=20, width=3),
                 lambda: eng.align_pairs_affine(GLOBAL, [x], [y], S, 1 << 22, 2, xdrop=20, width=3)):
        with pytest.raises(eng.SaError) as e:
            call()
        assert e.value.code == 4 and "scores may reach the band's sentinel" in str(e.value)
    # band= and bands= with xdrop= are still refused at the C ABI, by the planner's message
    p, S_keep, alpha_keep = eng._params(GLOBAL, S, 0, None, 0)
    out = (eng.SaScoreResult * 1)()
    res = (eng.SaResult * 1)()
    hp = (eng.SaHostPair * 1)(eng.SaHostPair(x.ctypes.data, 50, y.ctypes.data, 20))
    dpair = (eng.SaPair * 1)(eng.SaPair(0, 50, 0, 20))
    h = ctypes.c_void_p()
    L = eng.lib
    from sa_amd.engine import _variant
    for kw in ({"band": 3}, {"bands": [(0, 30)]}):
        with pytest.raises(ValueError, match="xdrop= takes no band"):
            _variant(11, 2, kw.get("band"), kw.get("bands"), 20, None, 1)
    # null arguments and zero pairs
    assert L.sa_score_batch_extend_band(ctypes.byref(p), 11, 2, 20, 3, hp, 1, 0, out) == 0
    assert L.sa_score_batch_extend_band(None, 11, 2, 20, 3, hp, 1, 0, out) == 1
    assert L.sa_score_batch_extend_band(ctypes.byref(p), 11, 2, 20, 3, None, 1, 0, out) == 1
    assert L.sa_score_batch_extend_band(ctypes.byref(p), 11, 2, 20, 3, hp, 1, 0, None) == 1
    assert L.sa_score_batch_extend_band(ctypes.byref(p), 11, 2, 20, 3, None, 0, 0, None) == 0
    assert L.sa_score_batch_extend_band(ctypes.byref(p), 11, 2, 20, -1, hp, 1, 0, out) == 1
    assert b"width must be >= 0" in L.sa_last_error()
    assert L.sa_align_pairs_extend_band(ctypes.byref(p), 11, 2, 20, 3, hp, 1, 0, res, None, None) == 0
    assert L.sa_align_pairs_extend_band(ctypes.byref(p), 11, 2, 20, 3, hp, 1, 0, None, None, None) == 1
    assert L.sa_align_pairs_extend_band(ctypes.byref(p), 11, 2, 20, -1, hp, 1, 0, res, None, None) == 1
    assert L.sa_align_pairs_extend_band(ctypes.byref(p), 11, 2, 20, 3, None, 0, 0, None, None, None) == 0
    assert L.sa_scorer_create_extend_band(ctypes.byref(p), 11, 2, 20, 3, None, 1, 0, ctypes.byref(h)) == 1
    assert L.sa_scorer_create_extend_band(ctypes.byref(p), 11, 2, 20, 3, dpair, 1, 0, None) == 1
    assert L.sa_scorer_create_extend_band(ctypes.byref(p), 11, 2, 20, -1, dpair, 1, 0, ctypes.byref(h)) == 1
    # the existing combinations at the C ABI: an extension has no _banded or _band_at function, so the planner's
    # refusal is reached through the plan-check tool, which builds the spec the keywords would
    for flag in (["--band", "3"], ["--band-at", "-3:3"]):
        for width in ([], ["--width", "3"]):
            o = subprocess.run([os.path.join(PKG, "bin", "sa_score_plan_check"), "--mode", "global", "--gap", "11", "--gap-extend", "2",
                                "--extend", "20"] + flag + width + ["50x20"], capture_output=True, text=True, check=True)
            o = json.loads(o.stdout)
            assert o == {"error": 4, "message": "extension alignment inside a band (band or bands with xdrop) is not built"}
    # empty sides, zero pairs
    none = np.zeros(0, dtype=np.int8)
    assert eng.align_pairs_affine(GLOBAL, [], [], S, 11, 2, xdrop=20, width=3) == []
    texts, patterns = [none, x[:5], none, x], [none, none, x[:5], x[:20]]
    for w in (0, 3):
        wants = [ext_band_ref(t, q, S, 11, 2, 20, w) for t, q in zip(texts, patterns)]
        assert [cell(v) for v in wants[:3]] == [(0, 0, 0)] * 3
        got = check(eng, texts, patterns, S, 11, 2, 20, w, wants, "empty")
        assert all(g["aligned_text"] == "" and g["num_bytes"] == 0 for g in got[:3])
    got = eng.align_pairs_affine(GLOBAL, [x], [x[:40]], S, 11, 2, strings=False, xdrop=20, width=3)[0]
    want = ext_band_ref(x, x[:40], S, 11, 2, 20, 3)
    assert got == {k: want[k] for k in KEYS[:4]}


# ---- 13. the C++ functions --------------------------------------------------------------------------------------------
@gpu
def test_cpp_extend_band_check():
    out = subprocess.run([os.path.join(PKG, "bin", "sa_extend_band_check"), "700", "64"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1] == "OK 64"


if __name__ == "__main__" and sys.argv[1:] == ["big"]:
    _big_child()
