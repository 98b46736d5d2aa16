"""Alignments under affine gap penalties (sa_align_pairs_affine, sa_search_affine,
alignSequencesGPUAffine): the traced Gotoh fill and the three-state walk of DESIGN.md §3.5. The
reference has no affine code, so parity is pinned as in test_score_affine_gpu.py: with
gap_open == gap_extend every output is the reference's for that linear gap and its 894 recorded
results apply, strings included; the general case is checked against affine_ref below, an
independent numpy fill with a plain Python walk; and affine_ref is itself checked on the CPU against a
plain double loop, against the oracle, and by re-scoring its strings."""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import DNA, PKG, PROT, encode, load, matrix, same_result  # first: it puts oracle/ and the package on the path

import oracle
from sa_amd import synthetic
from test_score_affine_gpu import gotoh_matrix
from test_score_gpu import related_pair

gpu = pytest.mark.gpu

GLOBAL, LOCAL = 0, 1
NEG = -(1 << 40)  # minus infinity: no score comes near it
LEFT, DIAG, TOP, STOP, EEXT, FEXT = 0, 1, 2, 3, 4, 8
KEYS = ("score", "num_bytes", "start_text", "start_pattern", "aligned_text", "aligned_pattern")
U64 = (1 << 64) - 1


# ---- the reference of this file ------------------------------------------------------------------------
def nibbles_by_diagonals(mode, t, p, S, go, ge):
    """(H, D) of Gotoh's recurrence swept by anti-diagonals: D[i][j] is the direction nibble of the
    interior cell (i, j): bits 0-1 the source of H with the reference's tie rule (left := E, up := F),
    STOP for a local cell whose unclamped H is <= 0; bit 2: E extends (strictly better than opening);
    bit 3: F extends."""
    t, p, S = np.asarray(t, dtype=np.int64), np.asarray(p, dtype=np.int64), np.asarray(S, dtype=np.int64)
    n, m = len(t), len(p)
    local = mode == LOCAL
    H = np.zeros((m + 1, n + 1), dtype=np.int64)
    if not local:
        H[0, 1:] = -(go + np.arange(n) * ge)
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
        h = np.maximum(dg, np.maximum(e, f))
        src = np.where(dg > np.maximum(e, f), DIAG, np.where(e >= f, LEFT, TOP))
        if local:
            src = np.where(h <= 0, STOP, src)
            h = np.maximum(h, 0)
        D[i, j] = src + EEXT * (ee > eo) + FEXT * (fe > fo)
        H[i, j], E[i, j], F[i, j] = h, e, f
    return H, D


def nibbles_by_loops(mode, t, p, S, go, ge):
    """The same as a plain double loop over the cells."""
    n, m = len(t), len(p)
    local = mode == LOCAL
    H = [[0] * (n + 1) for _ in range(m + 1)]
    D = [[0] * (n + 1) for _ in range(m + 1)]
    if not local:
        for j in range(1, n + 1):
            H[0][j] = -(go + (j - 1) * ge)
        for i in range(1, m + 1):
            H[i][0] = -(go + (i - 1) * ge)
    F, Hup = [NEG] * (n + 1), H[0]
    for i in range(1, m + 1):
        E = NEG
        for j in range(1, n + 1):
            ee, eo, fe, fo = E - ge, H[i][j - 1] - go, F[j] - ge, Hup[j] - go
            E, F[j] = max(ee, eo), max(fe, fo)
            dg = Hup[j - 1] + int(S[p[i - 1]][t[j - 1]])
            h = max(dg, E, F[j])
            src = DIAG if dg > max(E, F[j]) else LEFT if E >= F[j] else TOP
            if local and h <= 0:
                src = STOP
            D[i][j] = src + (EEXT if ee > eo else 0) + (FEXT if fe > fo else 0)
            H[i][j] = max(h, 0) if local else h
        Hup = H[i]
    return np.array(H, dtype=np.int64), np.array(D, dtype=np.uint8)


def walk(mode, t, p, H, D, go, ge, alphabet):
    """oracle_align's loop (oracle/sa_oracle.c) with a state in {H, E, F}. Returns the result and how
    the walk ended ("stop", "border" or "origin")."""
    n, m = len(t), len(p)
    local = mode == LOCAL
    gapc = alphabet[-1]
    if local:
        if H.max() <= 0:
            i = j = 0
        else:
            i, j = (int(v) for v in np.unravel_index(int(H.argmax()), H.shape))  # first maximum, row-major
        score = int(H[i, j])
    else:
        i, j = m, n
        k = max(n, m)
        score = int(H[m, n]) if n and m else (-(go + (k - 1) * ge) if k else 0)
    ti, pi, state, at, ap, ended = j - 1, i - 1, DIAG, [], [], "origin"
    while (i > 0 and j > 0) if local else (i > 0 or j > 0):
        nxt = DIAG
        if j == 0:
            d = TOP
        elif i == 0:
            d = LEFT
        else:
            nib = int(D[i, j])
            d = (nib & 3) if state == DIAG else state
            if d == STOP:
                ended = "stop"
                break
            if d == LEFT:
                nxt = LEFT if nib & EEXT else DIAG
            if d == TOP:
                nxt = TOP if nib & FEXT else DIAG
        tt, tp = d in (DIAG, LEFT), d in (DIAG, TOP)
        at.append(alphabet[t[j - 1]] if tt else gapc)
        ap.append(alphabet[p[i - 1]] if tp else gapc)
        j, i, state = j - tt, i - tp, nxt
        if local and (i == 0 or j == 0):
            ended = "border"
            break
        ti, pi = max(ti - tt, 0), max(pi - tp, 0)
    return {"score": score, "num_bytes": len(at), "start_text": ti & U64, "start_pattern": pi & U64,
            "aligned_text": "".join(reversed(at)), "aligned_pattern": "".join(reversed(ap))}, ended


def alphabet_of(S):
    return (DNA if len(S) == 4 else PROT) + "-"


def affine_ref(mode, t, p, S, go, ge, alphabet=None, how=False):
    t, p = np.asarray(t, dtype=np.int64), np.asarray(p, dtype=np.int64)
    H, D = nibbles_by_diagonals(mode, t, p, S, go, ge)
    res, ended = walk(mode, t, p, H, D, go, ge, alphabet or alphabet_of(S))
    return (res, ended) if how else res


def rescore(res, S, go, ge, alphabet):
    """The score of an alignment read from its two strings: substitution scores, and go + (k - 1) ge
    for each run of k gap letters on one side."""
    lut = {c: k for k, c in enumerate(alphabet[:-1])}
    total, run = 0, None
    for a, b in zip(res["aligned_text"], res["aligned_pattern"]):
        side = "t" if a == alphabet[-1] else "p" if b == alphabet[-1] else None
        if side is None:
            total += int(S[lut[b]][lut[a]])
        else:
            total -= ge if side == run else go
        run = side
    return total


def gap_runs(res):
    """Lengths of the gap runs of both aligned strings."""
    runs = []
    for s in (res["aligned_text"], res["aligned_pattern"]):
        k = 0
        for c in s + "x":
            if c == "-":
                k += 1
            elif k:
                runs.append(k)
                k = 0
    return runs


def gap_run_spans(res):
    """Of a global alignment: the (first, last) text columns of every run of gaps in the aligned pattern
    (a run along a row), and the (first, last) pattern rows of every run of gaps in the aligned text."""
    spans = {"columns": [], "rows": []}
    for kind, gapped, letters in (("columns", res["aligned_pattern"], res["aligned_text"]),
                                  ("rows", res["aligned_text"], res["aligned_pattern"])):
        pos, first = 0, None  # letters of the other side consumed so far: its column or row
        for g, c in zip(gapped + "x", letters + "x"):
            pos += c != "-"
            if g == "-" and first is None:
                first = pos
            elif g != "-" and first is not None:
                spans[kind].append((first, pos - 1))
                first = None
    return spans


_REF = {}


def ref_cached(key, *args):
    """affine_ref once per case, shared by the tests that meet the case again."""
    if key not in _REF:
        _REF[key] = affine_ref(*args)
    return _REF[key]


def pick(r):
    return {k: r[k] for k in KEYS}


# ---- 1. the reference of this file is sound (CPU) ------------------------------------------------------
def random_small_pairs(count, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        A = 4 if k % 2 else 23
        n, m = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        out.append((A,) + (related_pair(seed + 10 * k, n, m, A) if k % 3 else
                           (synthetic.random_sequence(seed + 10 * k, n, 4), synthetic.random_sequence(seed + 10 * k + 1, m, 4))))
    return out


def test_affine_ref_equals_the_plain_loops():
    for k, (A, t, p) in enumerate(random_small_pairs(40, 4100)):
        S = matrix("blast" if A == 4 else "blosum50", A)
        go, ge = ((11, 1), (5, 5), (4, 0), (3, 7), (-2, -1))[k % 5]
        for mode in (GLOBAL, LOCAL):
            H1, D1 = nibbles_by_diagonals(mode, t, p, S, go, ge)
            H2, D2 = nibbles_by_loops(mode, t, p, S, go, ge)
            assert (H1 == H2).all() and (D1 == D2).all(), (k, mode)
            assert (H1 == gotoh_matrix(mode, t, p, S, go, ge)).all(), (k, mode)


def test_affine_ref_equals_the_oracle_when_open_equals_extend():
    for k, (A, t, p) in enumerate(random_small_pairs(30, 5200)):
        S = matrix("blast" if A == 4 else "blosum50", A)
        for mode in (GLOBAL, LOCAL):
            for g in (-3, 0, 2, 5):
                assert affine_ref(mode, t, p, S, g, g) == oracle.align(mode, t, p, S, g), (k, mode, g)
    none, x = np.zeros(0, dtype=np.int8), synthetic.random_sequence(5, 5, 4)
    for mode in (GLOBAL, LOCAL):
        for t, p in ((none, none), (none, x), (x, none), (x[:1], x[:1])):
            assert affine_ref(mode, t, p, matrix("blast", 4), 3, 3) == oracle.align(mode, t, p, matrix("blast", 4), 3)


def test_affine_ref_strings_rescore_to_its_score():
    for k, (A, t, p) in enumerate(random_small_pairs(30, 6300)):
        S = matrix("blast" if A == 4 else "blosum50", A)
        for mode in (GLOBAL, LOCAL):
            for go, ge in ((11, 1), (5, 5), (4, 0)):
                res = affine_ref(mode, t, p, S, go, ge)
                assert rescore(res, S, go, ge, alphabet_of(S)) == res["score"], (k, mode, go, ge)


# ---- 2. gap_open == gap_extend is the linear gap: the reference's recorded results ---------------------------
@gpu
def test_degenerate_affine_equals_the_reference_goldens(eng):
    cases = load("random_pairs.json") + load("edge_pairs.json") + load("gap_pairs.json")
    key = lambda c: (c["mode"], c["A"], json.dumps(c["matrix"]), c["gap"])  # noqa: E731
    groups = {}
    for c in cases:
        groups.setdefault(key(c), []).append(c)
    checked = 0
    for (mode, A, mat, gap), grp in groups.items():
        got = eng.align_pairs_affine(mode, [encode(c["text"], A) for c in grp], [encode(c["pattern"], A) for c in grp],
                                     matrix(json.loads(mat), A), gap, gap)
        for c, g in zip(grp, got):
            assert same_result(g, c["result"]), (mode, A, gap, c["text"][:40], c["pattern"][:40])
            checked += 1
    assert checked == 894


# ---- 3. strip, lane and body edges ---------------------------------------------------------------------------
EDGE_SHAPES = [(1, 1), (1, 300), (7, 63), (8, 64), (9, 65), (8, 1), (9, 127), (7, 129), (511, 1), (511, 64), (512, 63),
               (512, 65), (512, 300), (513, 1), (513, 64), (513, 127), (513, 129), (1027, 63), (1027, 65), (1027, 300),
               (9, 300), (511, 129), (1, 64), (8, 127)]  # (m, n)


@gpu
@pytest.mark.parametrize("go,ge", [(11, 2), (3, 1)])
@pytest.mark.parametrize("A,mat", [(4, "blast"), (23, "blosum50")])
def test_strip_lane_and_body_edges(eng, A, mat, go, ge):
    S = matrix(mat, A)
    pairs = [related_pair(9000 + 3 * m + 5 * n + A, n, m, A) for m, n in EDGE_SHAPES]
    texts, patterns = [t for t, _ in pairs], [p for _, p in pairs]
    for mode in (GLOBAL, LOCAL):
        got = eng.align_pairs_affine(mode, texts, patterns, S, go, ge)
        for k, (t, p) in enumerate(pairs):
            want = ref_cached(("edges", A, mode, go, ge) + EDGE_SHAPES[k], mode, t, p, S, go, ge)
            assert pick(got[k]) == want, (A, mode, EDGE_SHAPES[k])


# ---- 4. long gaps across every hand-off -------------------------------------------------------------------
def with_blocks(seed, length, row_cut=None, col_cut=None):
    """A text and a pattern that are one random protein sequence of `length` letters, the pattern with
    40 letters of its own after its first row_cut letters (a run down rows row_cut + 1 .. row_cut + 40),
    the text with 40 of its own after the base letter col_cut (a run along the row)."""
    base = synthetic.random_sequence(seed, length, 20)
    t, p = base, base
    if col_cut is not None:
        t = np.concatenate([base[:col_cut], synthetic.random_sequence(seed + 1, 40, 20), base[col_cut:]])
    if row_cut is not None:
        p = np.concatenate([base[:row_cut], synthetic.random_sequence(seed + 2, 40, 20), base[row_cut:]])
    return t.astype(np.int8), p.astype(np.int8)


LONG_GAPS = {
    "row 8": with_blocks(100, 150, row_cut=4),             # rows 5 .. 44 over the lane edges from row 8 on
    "row 512": with_blocks(110, 600, row_cut=490),         # rows 491 .. 530: lane 0 of strip 1 to lane 63 of strip 0
    "column 64": with_blocks(120, 150, col_cut=44),        # columns 45 .. 84 over the body edge
    # n = 190: columns 143 .. 182 hold column n - 10 = 180; at rows 143 .. 150 (lanes 17, 18) columns
    # 175 and up are steps 192 and up, the tail body, so the run crosses into it
    "column n - 10": with_blocks(130, 150, col_cut=142),
    "row 8 and column 64": with_blocks(140, 150, row_cut=4, col_cut=48),  # columns 49 .. 88 after the 40 rows
}
# the row and the column that each pair's run must cross (n - 10 of the 190-letter text is 180)
LONG_GAP_CROSSES = {"row 8": {"rows": 8}, "row 512": {"rows": 512}, "column 64": {"columns": 64},
                    "column n - 10": {"columns": 190 - 10}, "row 8 and column 64": {"rows": 8, "columns": 64}}


def test_long_gap_pairs_have_one_run_of_forty():
    """The premise of the next test, on the CPU: the optimum holds the block as one run of 40, and
    the run crosses the row or column the case is named after."""
    S = matrix("blosum50", 23)
    for name, (t, p) in LONG_GAPS.items():
        res = ref_cached(("long", name, GLOBAL), GLOBAL, t, p, S, 11, 1)
        runs = 2 if "and" in name else 1
        assert gap_runs(res) == [40] * runs, (name, gap_runs(res))
        assert res["score"] == rescore(res, S, 11, 1, alphabet_of(S))
        spans = gap_run_spans(res)
        assert sorted(k for k in spans if spans[k]) == sorted(LONG_GAP_CROSSES[name]), (name, spans)
        for kind, line in LONG_GAP_CROSSES[name].items():
            (first, last), = spans[kind]
            assert last - first == 39 and first <= line <= last, (name, kind, first, last)
        if name == "column n - 10":
            assert len(t) == 190 and len(p) == 150
        same = sum(int(S[c][c]) for c in (t if len(t) < len(p) else p)) if runs == 1 else None
        if same is not None:  # every shared letter matched, one gap of 40: nothing scores higher
            assert res["score"] == same - (11 + 39)


@gpu
def test_long_gaps_cross_every_hand_off(eng):
    S = matrix("blosum50", 23)
    names = list(LONG_GAPS)
    texts, patterns = [LONG_GAPS[k][0] for k in names], [LONG_GAPS[k][1] for k in names]
    for mode in (GLOBAL, LOCAL):
        got = eng.align_pairs_affine(mode, texts, patterns, S, 11, 1)
        for k, name in enumerate(names):
            want = ref_cached(("long", name, mode), mode, texts[k], patterns[k], S, 11, 1)
            assert pick(got[k]) == want, (mode, name)
            if mode == GLOBAL:
                assert gap_runs(got[k]) == [40] * (2 if "and" in name else 1), name


# ---- 5. local cases ----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("m,n", [(60, 200), (300, 150)])
def test_local_ties_for_the_maximum(eng, m, n):
    S = matrix("blast", 4)
    x1, x2 = "ATCGACTG", "GGAACCTT"
    t = encode(x2 + "A" * (n - 16) + x1, 4)
    p = encode(x1 + "T" * (m - 16) + x2, 4)
    want = affine_ref(LOCAL, t, p, S, 10, 1)
    assert (want["score"], want["aligned_text"]) == (40, x1)  # of the two cells that hold 40, the earlier row
    assert pick(eng.align_pairs_affine(LOCAL, [t], [p], S, 10, 1)[0]) == want


@gpu
def test_local_without_a_positive_cell(eng):
    S = matrix("blast", 4)
    t, p = encode("A" * 70, 4), encode("T" * 30, 4)
    got = eng.align_pairs_affine(LOCAL, [t], [p], S, 11, 2)[0]
    lin = eng.align_pair(LOCAL, t, p, S, 11)
    assert pick(got) == affine_ref(LOCAL, t, p, S, 11, 2)
    assert (got["score"], got["num_bytes"], got["aligned_text"], got["aligned_pattern"]) == (0, 0, "", "")
    assert (got["start_text"], got["start_pattern"]) == (lin["start_text"], lin["start_pattern"])


@gpu
def test_local_walks_end_on_a_stop_cell_and_on_the_border(eng):
    S = matrix("blosum50", 23)
    q = synthetic.random_sequence(77, 60, 20)
    junk = [synthetic.random_sequence(78 + k, 50, 20) for k in range(3)]
    inside = (np.concatenate([junk[0], q, junk[1]]), np.concatenate([junk[2][:20], q, junk[2][20:]]))
    at_border = (np.concatenate([q, junk[0]]), np.concatenate([q[:45], junk[1]]))
    want_in, how_in = affine_ref(LOCAL, *inside, S, 11, 2, how=True)
    want_b, how_b = affine_ref(LOCAL, *at_border, S, 11, 2, how=True)
    assert (how_in, how_b) == ("stop", "border")
    got = eng.align_pairs_affine(LOCAL, [inside[0], at_border[0]], [inside[1], at_border[1]], S, 11, 2)
    assert [pick(g) for g in got] == [want_in, want_b]


# ---- 6. empty sides and tiny pairs ------------------------------------------------------------------------
@gpu
def test_empty_sides_and_tiny_pairs(eng):
    S = matrix("blast", 4)
    x, none = synthetic.random_sequence(5, 5, 4), np.zeros(0, dtype=np.int8)
    texts, patterns = [none, x, none, x[:1]], [none, none, x, x[1:2]]  # (m, n) = (0,0), (0,5), (5,0), (1,1)
    for mode in (GLOBAL, LOCAL):
        got = eng.align_pairs_affine(mode, texts, patterns, S, 11, 2)
        assert [pick(g) for g in got] == [affine_ref(mode, t, p, S, 11, 2) for t, p in zip(texts, patterns)], mode
    got = eng.align_pairs_affine(GLOBAL, texts, patterns, S, 11, 2)
    assert [g["score"] for g in got[:3]] == [0, -(11 + 4 * 2), -(11 + 4 * 2)]
    assert (got[1]["aligned_pattern"], got[2]["aligned_text"]) == ("-----", "-----")


# ---- 7. more pairs than waves, chunking, reruns --------------------------------------------------------------
MANY, MANY_GAP = 3000, (9, 1)


def many_pairs():
    rng = np.random.default_rng(20250412)
    nl, ml = rng.integers(1, 97, MANY), rng.integers(1, 97, MANY)
    ta = synthetic.random_sequence(311, int(nl.sum()), 4)
    pa = synthetic.mutate(np.resize(ta, int(ml.sum())), 312, 4, int(ml.sum()))
    to, po = np.concatenate([[0], np.cumsum(nl)]), np.concatenate([[0], np.cumsum(ml)])
    return [ta[to[k]:to[k + 1]] for k in range(MANY)], [pa[po[k]:po[k + 1]] for k in range(MANY)]


def digest(results):
    return hashlib.sha256(json.dumps([[r[k] for k in KEYS] for r in results]).encode()).hexdigest()


def run_many(eng):
    texts, patterns = many_pairs()
    got = eng.align_pairs_affine(LOCAL, texts, patterns, matrix("blast", 4), *MANY_GAP)
    return texts, patterns, got, eng.affine_last_stats()["num_chunks"]


@gpu
def test_pairs_outnumber_waves_chunks_and_reruns(eng):
    S = matrix("blast", 4)
    texts, patterns, got, chunks = run_many(eng)
    assert chunks == 1
    rng = np.random.default_rng(3)
    for k in rng.choice(MANY, 150, replace=False):
        assert pick(got[k]) == affine_ref(LOCAL, texts[k], patterns[k], S, *MANY_GAP), int(k)
    scores = eng.score_batch(LOCAL, texts, patterns, S, MANY_GAP[0], gap_extend=MANY_GAP[1])
    assert [g["score"] for g in got] == scores["score"].tolist()
    # the same call over at least three chunks of the direction arena, in a process of its own (the
    # budget is read once per process)
    env = dict(os.environ, SA_TRACE_ARENA_BYTES=str(32 << 20))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "many"], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    child = json.loads(out.stdout.strip().splitlines()[-1])
    assert child["num_chunks"] >= 3
    assert child["digest"] == digest(got)
    # and once more in this process
    assert digest(run_many(eng)[2]) == digest(got)


# ---- 8. search ---------------------------------------------------------------------------------------------
@gpu
def test_search_affine(eng):
    import torch
    rng = np.random.default_rng(17)
    S = matrix("blosum50", 23)
    go, ge, K = 11, 2, 10
    q = synthetic.random_sequence(900, 200, 20)
    texts = []
    for k in range(300):
        n = int(rng.integers(20, 401))
        if k % 4 == 0:  # some texts hold a mutated piece of the query with a block left out
            piece = synthetic.mutate(q, 1000 + k, 20, 200)
            cut = int(rng.integers(20, 120))
            body = np.concatenate([piece[:cut], piece[cut + 15:]])[:n]
            t = np.concatenate([synthetic.random_sequence(2000 + k, n - len(body), 20), body])
        else:
            t = synthetic.random_sequence(3000 + k, n, 20)
        texts.append(t.astype(np.int8))
    # text 8 holds the query itself and text 40 is a copy of it: the top two ranks tie, the lower index first
    texts[8] = np.concatenate([synthetic.random_sequence(41, 60, 20), q, synthetic.random_sequence(42, 70, 20)]).astype(np.int8)
    texts[40] = texts[8].copy()
    scores, hits = eng.search(LOCAL, q, texts, S, go, K, gap_extend=ge)
    offs = np.concatenate([[0], np.cumsum([len(t) for t in texts])])
    sc = eng.Scorer(LOCAL, S, go, [(int(offs[k]), len(texts[k]), 0, len(q)) for k in range(300)], gap_extend=ge)
    dt, dq = torch.from_numpy(np.concatenate(texts)).cuda(), torch.from_numpy(q).cuda()
    sc.run(dt.data_ptr(), dq.data_ptr())
    want_scores = sc.results()
    sc.close()
    assert scores.tolist() == want_scores.tolist()
    rank = sorted(range(300), key=lambda i: (-int(scores["score"][i]), i))
    assert [h["index"] for h in hits] == rank[:K]
    assert rank[:2] == [8, 40] and scores[8] == scores[40]
    pairs = eng.align_pairs_affine(LOCAL, [texts[h["index"]] for h in hits], [q] * K, S, go, ge)
    for h, pr in zip(hits, pairs):
        assert pick(h) == pick(pr) == affine_ref(LOCAL, texts[h["index"]], q, S, go, ge), h["index"]
        assert h["score"] == int(scores["score"][h["index"]])
    # gap_extend == gap: the linear search, every value
    s_lin, h_lin = eng.search(LOCAL, q, texts, S, 5, K)
    s_aff, h_aff = eng.search(LOCAL, q, texts, S, 5, K, gap_extend=5)
    assert s_aff.tolist() == s_lin.tolist() and h_aff == h_lin
    # k = 0: scores only; k beyond the texts: every text
    s0, h0 = eng.search(LOCAL, q, texts[:6], S, go, 0, gap_extend=ge)
    assert h0 == [] and s0.tolist() == scores[:6].tolist()
    s9, h9 = eng.search(LOCAL, q, texts[:6], S, go, 9, gap_extend=ge)
    assert [h["index"] for h in h9] == sorted(range(6), key=lambda i: (-int(scores["score"][i]), i))


# ---- 9. bad input -------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("side", ["text", "pattern"])
@pytest.mark.parametrize("A", [4, 23])
def test_out_of_alphabet_byte_is_rejected(eng, side, A):
    S = matrix("blast" if A == 4 else "blosum50", A)
    t, p = related_pair(11, 150, 90, A)
    (t if side == "text" else p)[70] = A
    with pytest.raises(eng.SaError) as e:
        eng.align_pairs_affine(GLOBAL, [t, t[:10]], [p, p[:10]], S, 11, 2)
    assert e.value.code == 1  # SA_ERR_INVALID
    with pytest.raises(eng.SaError) as e:
        eng.search(LOCAL, p, [t, t[:10]], S, 11, 2, gap_extend=2)
    assert e.value.code == 1


@gpu
def test_pairs_over_the_limits_and_null_arguments(eng):
    import ctypes
    S = matrix("blast", 4)
    x = synthetic.random_sequence(1, 50, 4)
    with pytest.raises(eng.SaError) as e:  # (|S| + 2 |g|) (n + m) reaches 2^30
        eng.align_pairs_affine(GLOBAL, [x], [x], S, 1 << 24, 2)
    assert e.value.code == 4  # SA_ERR_UNSUPPORTED
    p, S_keep, alpha_keep = eng._params(GLOBAL, S, 0, None, 0)
    res = (eng.SaResult * 1)()
    hp = (eng.SaHostPair * 1)(eng.SaHostPair(x.ctypes.data, 50, x.ctypes.data, 50))
    buf = ctypes.create_string_buffer(100)
    one = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    assert eng.lib.sa_align_pairs_affine(None, 11, 2, hp, 1, 0, res, None, None) == 1
    assert eng.lib.sa_align_pairs_affine(ctypes.byref(p), 11, 2, None, 1, 0, res, None, None) == 1
    assert eng.lib.sa_align_pairs_affine(ctypes.byref(p), 11, 2, hp, 1, 0, None, None, None) == 1
    assert eng.lib.sa_align_pairs_affine(ctypes.byref(p), 11, 2, hp, 1, 0, res, one, None) == 1  # one string side only
    assert eng.lib.sa_align_pairs_affine(ctypes.byref(p), 11, 2, hp, -1, 0, res, None, None) == 1
    hp[0].text = None
    assert eng.lib.sa_align_pairs_affine(ctypes.byref(p), 11, 2, hp, 1, 0, res, None, None) == 1
    nh = ctypes.c_int64(0)
    assert eng.lib.sa_search_affine(ctypes.byref(p), 11, 2, x.ctypes.data, 50, None, None, 1, 1, 0, None, None, None, None, None,
                                    ctypes.byref(nh)) == 1
    assert eng.lib.sa_search_affine(ctypes.byref(p), 11, 2, x.ctypes.data, 50, None, None, 0, 0, 0, None, None, None, None, None,
                                    None) == 1
    # zero pairs, and results without strings
    assert eng.align_pairs_affine(GLOBAL, [], [], S, 11, 2) == []
    got = eng.align_pairs_affine(GLOBAL, [x], [x[:40]], S, 11, 2, strings=False)[0]
    want = affine_ref(GLOBAL, x, x[:40], S, 11, 2)
    assert got == {k: want[k] for k in KEYS[:4]}


# ---- 10. the C++ extension -------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["global", "local"])
def test_cpp_align_affine_check(mode):
    out = subprocess.run([os.path.join(PKG, "bin", "sa_align_affine_check"), mode, "700", "96"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1] == "OK 96"


if __name__ == "__main__" and sys.argv[1:] == ["many"]:
    from sa_amd import engine
    _, _, results, num_chunks = run_many(engine)
    print(json.dumps({"digest": digest(results), "num_chunks": num_chunks}))
