"""Chained seeds (sa_hip.h: sa_score_batch_chains, sa_scorer_create_chains, sa_align_pairs_chains): every pair
carries a colinear chain of seeds; the rectangle between two consecutive seeds is a global alignment, the two
ends are the seeds functions' halves, and one call returns the sum with the seeds' scores, the covered intervals
and the joined strings. The reference of this file is chains_ref: identity (C1), the composition of
test_extend_gpu's extend_ref on the sliced and reversed ends and of test_align_affine_gpu's affine_ref in global
mode on the sliced gaps. It is pinned on the CPU by (C2) against test_seeds_gpu's seeds_ref, by (C3), by the
mirror identity (C4) and by re-scoring its strings; the GPU is then compared with it exactly, every field and
both strings, at every forced rows_per_lane of the scorer, through the linear kernels, and in the aligner."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, matrix  # first: it puts oracle/ and the package on the path

from sa_amd import synthetic
from test_align_affine_gpu import affine_ref, alphabet_of, pick, rescore
from test_extend_gpu import GAPS, NONE, SMALL_GAPS, SMALL_X, extend_ref, random_small_pairs, xd
from test_seeds_gpu import FIELDS, fields, seeds_ref

gpu = pytest.mark.gpu

GLOBAL = 0


# ---- the reference of this file ------------------------------------------------------------------------
def chains_ref(t, p, chain, S, go, ge, xdrop, alphabet=None):
    """(C1): the keys of align_pairs_affine, the fields of sa_seed_result, and the pieces."""
    t, p = np.asarray(t, dtype=np.int64), np.asarray(p, dtype=np.int64)
    chain = [tuple(int(v) for v in sd) for sd in chain]
    alphabet = alphabet or alphabet_of(S)
    gapc = alphabet[-1]
    letters = lambda seq: "".join(alphabet[c] for c in seq)  # noqa: E731
    assert len(chain) >= 1
    ts0, ps0, _ = chain[0]
    te, pe = chain[-1][0] + chain[-1][2], chain[-1][1] + chain[-1][2]
    assert te <= len(t) and pe <= len(p)
    left = extend_ref(t[:ts0][::-1], p[:ps0][::-1], S, go, ge, xdrop, alphabet)
    right = extend_ref(t[te:], p[pe:], S, go, ge, xdrop, alphabet)
    score = left["score"] + right["score"]
    at, ap = left["aligned_text"][::-1], left["aligned_pattern"][::-1]
    gaps = []
    for i, (ts, ps, L) in enumerate(chain):
        score += sum(int(S[p[ps + q]][t[ts + q]]) for q in range(L))
        at += letters(t[ts:ts + L])
        ap += letters(p[ps:ps + L])
        if i + 1 == len(chain):
            break
        a, b = ts + L, ps + L
        nts, nps, _ = chain[i + 1]
        assert a <= nts and b <= nps
        gt, gp = t[a:nts], p[b:nps]
        if len(gt) and len(gp):
            g = affine_ref(GLOBAL, gt, gp, S, go, ge, alphabet)
            gaps.append(g)
            score += g["score"]
            at += g["aligned_text"]
            ap += g["aligned_pattern"]
        elif len(gt) + len(gp):
            k = len(gt) + len(gp)
            score -= go + (k - 1) * ge
            at += letters(gt) if len(gt) else gapc * k
            ap += letters(gp) if len(gp) else gapc * k
    at += right["aligned_text"]
    ap += right["aligned_pattern"]
    res = {"score": score, "begin_text": ts0 - left["end_text"], "begin_pattern": ps0 - left["end_pattern"],
           "end_text": te + right["end_text"], "end_pattern": pe + right["end_pattern"], "aligned_text": at, "aligned_pattern": ap,
           "num_bytes": len(at), "left": left, "right": right, "gaps": gaps}
    res["start_text"], res["start_pattern"] = res["begin_text"], res["begin_pattern"]
    assert len(at) == len(ap)
    return res


_REFS = {}  # key -> chains_ref: computed once per process, shared by the tests that meet the case again


def cached_ref(key, t, p, chain, S, go, ge, xdrop):
    k = (key, go, ge, xdrop)
    if k not in _REFS:
        _REFS[k] = chains_ref(t, p, chain, S, go, ge, xdrop)
    return _REFS[k]


def mirror(t, p, chain):
    n, m = len(t), len(p)
    return t[::-1].copy(), p[::-1].copy(), [(n - ts - L, m - ps - L, L) for ts, ps, L in chain[::-1]]


def check(eng, texts, patterns, chains, S, go, ge, xdrop, wants, what, Rs=(1, 2, 4, 8)):
    """Every forced rows_per_lane of the chains scorer (the linear kernels too when go == ge, through
    gap_extend=None), and the chains aligner: every field and both strings."""
    x = xd(eng, xdrop)
    for R in Rs:
        got = eng.score_batch(GLOBAL, texts, patterns, S, go, rows_per_lane=R, gap_extend=ge, xdrop=x, chains=chains)
        assert got.dtype == eng.SEED_DTYPE and (got["status"] == 0).all()
        assert [fields(g) for g in got] == [fields(w) for w in wants], (what, "score", go, ge, xdrop, R)
        if go == ge:
            got = eng.score_batch(GLOBAL, texts, patterns, S, go, rows_per_lane=R, xdrop=x, chains=chains)
            assert [fields(g) for g in got] == [fields(w) for w in wants], (what, "score, gap_extend=None", go, xdrop, R)
    got = eng.align_pairs_affine(GLOBAL, texts, patterns, S, go, ge, xdrop=x, chains=chains)
    for k, (g, w) in enumerate(zip(got, wants)):
        assert pick(g) == pick(w), (what, "align", go, ge, xdrop, k, chains[k][:4], len(patterns[k]), len(texts[k]))
    return got


# ---- 1. the reference of this file is sound (CPU) ------------------------------------------------------
def random_chain(rng, n, m, count):
    """`count` colinear seeds without overlap inside n x m, some adjacent, some of length 0, some after a gap
    with an empty side."""
    chain, te, pe = [], 0, 0
    for k in range(count):
        kind = int(rng.integers(0, 5))
        ts = te + (0 if kind == 0 else int(rng.integers(0, (n - te) // (count - k) + 1)))
        ps = pe + (0 if kind in (0, 1) else int(rng.integers(0, (m - pe) // (count - k) + 1)))
        L = 0 if kind == 2 else int(rng.integers(0, min(n - ts, m - ps, 6) + 1))
        chain.append((ts, ps, L))
        te, pe = ts + L, ps + L
    return chain


def small_cases(count=40, seed=81100):
    rng = np.random.default_rng(seed)
    return [(A, t, p, random_chain(rng, len(t), len(p), 1 + k % 4)) for k, (A, t, p) in enumerate(random_small_pairs(count, seed))]


def test_c2_a_chain_of_one_is_the_seed():
    for k, (A, t, p, chain) in enumerate(small_cases()):
        S = matrix("blast" if A == 4 else "blosum50", A)
        for go, ge in SMALL_GAPS:
            for x in SMALL_X:
                want = seeds_ref(t, p, chain[0], S, go, ge, x)
                got = chains_ref(t, p, chain[:1], S, go, ge, x)
                assert pick(got) == pick(want) and fields(got) == fields(want), (k, go, ge, x)


def test_c3_cutting_a_seed_changes_nothing():
    for k, (A, t, p, chain) in enumerate(small_cases()):
        S = matrix("blast" if A == 4 else "blosum50", A)
        cut = []
        for ts, ps, L in chain:
            a = L // 2
            cut += [(ts, ps, a), (ts + a, ps + a, L - a)]
        for go, ge in SMALL_GAPS[:3]:
            a, b = chains_ref(t, p, chain, S, go, ge, 20), chains_ref(t, p, cut, S, go, ge, 20)
            assert pick(a) == pick(b) and fields(a) == fields(b), (k, go, ge)


def test_c4_the_mirrored_chain_mirrors_score_and_intervals_and_not_every_string():
    """The header states (C4) for scores and intervals: the ends mirror exactly, a gap's string is the global
    aligner's on the reversed rectangle, whose tie rules are not symmetric. Both halves of that are checked."""
    differ = 0
    for k, (A, t, p, chain) in enumerate(small_cases()):
        S = matrix("blast" if A == 4 else "blosum50", A)
        n, m = len(t), len(p)
        mt, mp, mchain = mirror(t, p, chain)
        for go, ge in SMALL_GAPS:
            if not 0 <= ge <= go:
                continue  # a border gap run costs its closed form, an interior one may open cell by cell: sa_hip.h (C4)
            for x in (3, 20, NONE):
                a, b = chains_ref(t, p, chain, S, go, ge, x), chains_ref(mt, mp, mchain, S, go, ge, x)
                assert fields(b) == (a["score"], n - a["end_text"], m - a["end_pattern"], n - a["begin_text"], m - a["begin_pattern"]), (k, go, ge, x)
                assert pick(b["left"]) == pick(a["right"]) and pick(b["right"]) == pick(a["left"])
                assert [g["score"] for g in b["gaps"]] == [g["score"] for g in a["gaps"]][::-1]
                # every gap's string is the global aligner's on the reversed rectangle, by construction; it is
                # the reverse of this pair's gap string only where the walk met no tie
                differ += b["aligned_text"] != a["aligned_text"][::-1] or b["aligned_pattern"] != a["aligned_pattern"][::-1]
    assert differ > 0  # the global walk's tie rules are not symmetric: sa_hip.h says so


def test_the_strings_of_the_reference_rescore_and_cover_their_intervals():
    for k, (A, t, p, chain) in enumerate(small_cases()):
        S = matrix("blast" if A == 4 else "blosum50", A)
        alpha = alphabet_of(S)
        for go, ge in ((11, 1), (5, 5), (4, 0)):
            res = chains_ref(t, p, chain, S, go, ge, NONE)
            assert res["aligned_text"].replace("-", "") == "".join(alpha[c] for c in t[res["begin_text"]:res["end_text"]])
            assert res["aligned_pattern"].replace("-", "") == "".join(alpha[c] for c in p[res["begin_pattern"]:res["end_pattern"]])
            assert res["begin_text"] <= chain[0][0] and chain[-1][0] + chain[-1][2] <= res["end_text"]
            # rescore reads a run of gap letters as one gap; two pieces that meet in gaps on the same side are two
            # gaps to the definition: the difference is go - ge per such junction, never anything else
            diff = rescore(res, S, go, ge, alpha) - res["score"]
            assert diff >= 0 and (go == ge and diff == 0 or go != ge and diff % (go - ge) == 0), (k, go, ge, diff)


# ---- 2. the shapes that can go wrong -------------------------------------------------------------------
def build_case(seed, A, left, seeds, gaps, right, indel=False):
    """A pair from its pieces: left = (rows, columns) of the left end, seeds = [L, ...], gaps = [(rows, columns),
    ...] between them, right = (rows, columns). The pattern's pieces are the text's mutated to their length, so
    that every piece runs along related letters; a seed's letters are the text's, with one changed now and then."""
    letters = 20 if A == 23 else A
    assert len(gaps) == len(seeds) - 1
    tparts, pparts, chain = [], [], []
    k = [seed]

    def fresh(length):
        k[0] += 1
        return synthetic.random_sequence(k[0], length, letters).astype(np.int8)

    def related(tp, rows):
        k[0] += 1
        if len(tp) == 0 or rows == 0:
            return fresh(rows)
        return synthetic.mutate(np.resize(tp, max(rows, 1)), k[0], letters, rows).astype(np.int8)

    def piece(rows, cols, reverse=False):
        tp = fresh(cols)
        pp = related(tp[::-1], rows)[::-1] if reverse else related(tp, rows)
        if indel and rows == cols == 130:
            # 40 letters of the text against nothing, then 40 of the pattern: the walk runs along row 0 and column n
            pp = np.concatenate([tp[40:], fresh(40)]).astype(np.int8)
        tparts.append(tp)
        pparts.append(pp)

    piece(*left, reverse=True)
    for i, L in enumerate(seeds):
        ts, ps = sum(map(len, tparts)), sum(map(len, pparts))
        sd = fresh(L)
        sp = sd.copy()
        if L and (i + seed) % 3 == 0:
            sp[L // 2] = (sp[L // 2] + 1) % 4  # a seed's letters need not match
        tparts.append(sd)
        pparts.append(sp)
        chain.append((ts, ps, L))
        if i < len(gaps):
            piece(*gaps[i])
    piece(*right)
    t, p = np.concatenate(tparts).astype(np.int8), np.concatenate(pparts).astype(np.int8)
    return t, p, chain


SHAPES = [
    # (left, seeds, gaps, right): rows x columns
    ((20, 25), [5, 5, 5, 5], [(1, 1), (1, 9), (9, 1)], (30, 20)),            # gap rectangles of 1 x 1, 1 x k, k x 1
    ((7, 7), [15, 1, 0], [(65, 3), (3, 130)], (12, 9)),                        # a second strip at R = 1; a third body
    ((10, 10), [15, 15], [(513, 70)], (10, 10)),                               # a second strip of the traced R = 8 instance
    ((5, 5), [15, 15], [(130, 130)], (5, 5)),                                  # with indel=True: an indel of 40, the walk hugs a border
    ((33, 40), [15], [], (70, 64)),                                            # a chain of 1
    ((33, 40), [0, 100], [(20, 24)], (70, 64)),                                # of 2; seeds of length 0 and 100
    ((64, 65), [1, 1, 1], [(0, 0), (0, 0)], (129, 63)),                        # adjacent seeds of length 1
    ((0, 0), [15, 15, 15], [(30, 34), (28, 25)], (0, 0)),                      # both ends empty: from (0, 0) to (n, m)
    ((0, 0), [15, 15], [(30, 34)], (40, 44)),                                  # only the left end empty
    ((40, 44), [15, 15], [(30, 34)], (0, 0)),                                  # only the right end empty
    ((0, 9), [15, 15], [(0, 7)], (9, 0)),                                      # crossed empties: ts > 0 with ps = 0; an empty-side gap
    ((12, 12), [15, 0, 0, 15], [(0, 5), (6, 0), (3, 3)], (12, 12)),            # both kinds of empty-side gap, length-0 seeds between
]


def shape_cases(A, seed=82200):
    out = [build_case(seed + 100 * k + A, A, *sh, indel=(sh[2] == [(130, 130)])) for k, sh in enumerate(SHAPES)]
    rng = np.random.default_rng(seed + A)
    for count in (70, 200):  # the combine's strided loops and the join beyond 64 pieces
        gaps = [(int(rng.integers(0, 9)), int(rng.integers(0, 9))) for _ in range(count - 1)]
        seeds = [int(rng.integers(0, 12)) for _ in range(count)]
        seeds[count // 2] = 100
        out.append(build_case(seed + 7 * count + A, A, (30, 30), seeds, gaps, (30, 30)))
    return out


def test_the_shape_cases_have_their_shapes():
    cases = shape_cases(4)
    assert sorted({len(c[2]) for c in cases}) == [1, 2, 3, 4, 70, 200]
    rects = set()
    for t, p, chain in cases:
        n, m = len(t), len(p)
        assert all(ts + L <= nts and ps + L <= nps for (ts, ps, L), (nts, nps, _) in zip(chain, chain[1:]))
        assert chain[-1][0] + chain[-1][2] <= n and chain[-1][1] + chain[-1][2] <= m
        rects |= {(nps - ps - L, nts - ts - L) for (ts, ps, L), (nts, nps, _) in zip(chain, chain[1:])}
    assert {(1, 1), (1, 9), (9, 1), (65, 3), (3, 130), (513, 70), (130, 130), (0, 0), (0, 5), (6, 0)} <= rects
    assert any(c[2][0][:2] == (0, 0) and c[2][-1][0] + c[2][-1][2] == len(c[0]) and c[2][-1][1] + c[2][-1][2] == len(c[1]) for c in cases)
    assert {L for c in cases for _, _, L in c[2]} >= {0, 1, 100}
    # the indel pair: its gap's walk runs along the borders
    t, p, chain = cases[3]
    g = chains_ref(t, p, chain, matrix("blast", 4), 11, 2, NONE)["gaps"][0]
    assert g["aligned_pattern"].startswith("-" * 40) and g["aligned_text"].endswith("-" * 40)


@gpu
@pytest.mark.parametrize("go,ge", GAPS)
@pytest.mark.parametrize("A,mat", [(4, "blast"), (23, "blosum50")])
def test_shapes(eng, A, mat, go, ge):
    S = matrix(mat, A)
    cases = shape_cases(A)
    texts, patterns, chains = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    for x in (NONE, 20):
        wants = [cached_ref(("shape", A, k), t, p, ch, S, go, ge, x) for k, (t, p, ch) in enumerate(cases)]
        check(eng, texts, patterns, chains, S, go, ge, x, wants, "shapes")


@gpu
def test_negative_penalties(eng):
    S = matrix("blast", 4)
    cases = shape_cases(4)[:2] + shape_cases(4)[4:12]
    texts, patterns, chains = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    wants = [chains_ref(t, p, ch, S, -2, -1, 20) for t, p, ch in cases]
    check(eng, texts, patterns, chains, S, -2, -1, 20, wants, "negative penalties")


# ---- 3. packed arenas, a scorer reused ------------------------------------------------------------------
SENTINEL = 77  # outside every alphabet: a read of it fails the call


def flipped(p):
    """Other contents for the same shapes: every seventh pattern letter changed."""
    q = p.copy()
    q[::7] = (q[::7] + 1) % 4
    return q


def packed(cases, flip=False):
    """The pairs one after another with one sentinel byte before each, between them and after the last: a read
    one letter past any piece of a pair, to either side, is a read of a sentinel."""
    ta, pa, pairs = [np.int8(SENTINEL)], [np.int8(SENTINEL)], []
    for t, p, _ in cases:
        if flip:
            p = flipped(p)
        pairs.append((len(ta), len(t), len(pa), len(p)))
        ta += list(t) + [np.int8(SENTINEL)]
        pa += list(p) + [np.int8(SENTINEL)]
    return np.array(ta, dtype=np.int8), np.array(pa, dtype=np.int8), pairs


@gpu
@pytest.mark.parametrize("go,ge", GAPS)
def test_packed_arenas_and_a_scorer_reused(eng, go, ge):
    import torch
    S = matrix("blast", 4)
    cases = shape_cases(4)[:2] + shape_cases(4)[4:]
    chains = [c[2] for c in cases]
    ta, pa, pairs = packed(cases)
    tb, pb, _ = packed(cases, flip=True)
    dt, dp = torch.from_numpy(ta).cuda(), torch.from_numpy(pa).cuda()
    for x in (NONE, 20):
        wants = [cached_ref(("shape", 4, k if k < 2 else k + 2), t, p, ch, S, go, ge, x) for k, (t, p, ch) in enumerate(cases)]
        changed = [chains_ref(t, flipped(p), ch, S, go, ge, x) for t, p, ch in cases[:4]]
        for R in (1, 2, 4, 8):
            for lin in ((False, True) if go == ge else (False,)):
                sc = eng.Scorer(GLOBAL, S, go, pairs, rows_per_lane=R, gap_extend=None if lin else ge, xdrop=xd(eng, x), chains=chains)
                assert sc.info()["rows_per_lane"] == R and sc.info()["device_bytes"] > 0
                for rerun in range(2):
                    sc.run(dt.data_ptr(), dp.data_ptr())
                    got = sc.results()
                    assert [fields(g) for g in got] == [fields(w) for w in wants], (x, R, lin, rerun)
                # sa_scorer_fetch on a chains scorer: the score with the absolute end cell
                ends = sc.score_results()
                assert [(int(e["score"]), int(e["end_text"]), int(e["end_pattern"])) for e in ends] == \
                       [(w["score"], w["end_text"], w["end_pattern"]) for w in wants]
                # new arena contents under the same scorer
                dt2, dp2 = torch.from_numpy(tb).cuda(), torch.from_numpy(pb).cuda()
                sc.run(dt2.data_ptr(), dp2.data_ptr())
                got = sc.results()
                sc.close()
                assert [fields(g) for g in got[:4]] == [fields(w) for w in changed], (x, R, lin, "new contents")


# ---- 4. letters outside the alphabet ---------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("where", ["gap", "seed", "left end", "right end"])
def test_a_bad_letter_in_any_piece_is_rejected(eng, where):
    S = matrix("blast", 4)
    t, p, chain = build_case(83300, 4, (20, 20), [15, 15], [(30, 34)], (20, 20))
    # (seed, offset from its first letter): inside the 30 x 34 gap, inside seed 1, the letter before seed 0, the one after seed 1
    sd, off = {"gap": (0, 15 + 10), "seed": (1, 3), "left end": (0, -1), "right end": (1, 15)}[where]
    for side in ("text", "pattern"):
        tt, pp = t.copy(), p.copy()
        if side == "text":
            tt[chain[sd][0] + off] = 9
        else:
            pp[chain[sd][1] + off] = 9
        for call in (lambda: eng.score_batch(GLOBAL, [tt], [pp], S, 11, gap_extend=2, xdrop=eng.NO_XDROP, chains=[chain]),
                     lambda: eng.align_pairs_affine(GLOBAL, [tt], [pp], S, 11, 2, xdrop=eng.NO_XDROP, chains=[chain])):
            with pytest.raises(eng.SaError) as e:
                call()
            assert e.value.code == 1 and "alphabet" in str(e.value), (where, side)
    # the same chain with clean letters passes
    assert eng.score_batch(GLOBAL, [t], [p], S, 11, gap_extend=2, xdrop=eng.NO_XDROP, chains=[chain])[0]["status"] == 0


# ---- 5. the X-drop on the ends -------------------------------------------------------------------------------
def chimeric_case():
    """test_extend_gpu's chimeric construction on both ends: the text has letters 0 and 1 only; the pattern is the
    text along the chain (two letters 3 inserted in the second gap), 40 letters 2 that match nothing from 30 letters
    before the chain and from 45 after it, and the text again beyond them. Both ends drop under X = 20, and
    without a drop both run on through the junk to the pair's corners."""
    t = synthetic.random_sequence(84400, 400, 2).astype(np.int8)
    junk, ins = np.full(40, 2, dtype=np.int8), np.full(2, 3, dtype=np.int8)
    p = np.concatenate([t[:80], junk, t[120:205], ins, t[205:290], junk, t[330:]]).astype(np.int8)
    return t, p, [(150, 150, 15), (180, 180, 15), (230, 232, 15)]


def test_the_chimeric_case_drops_on_both_ends():
    S = matrix("blast", 4)
    t, p, chain = chimeric_case()
    w = chains_ref(t, p, chain, S, 16, 4, 20)
    # junk row k lies min(4 k, 16 + 4 (k - 1)) below the best: 24 at k = 6, the first above 20
    assert w["left"]["stop_row"] == 30 + 6 and w["right"]["stop_row"] == 45 + 6
    assert (w["begin_text"], w["begin_pattern"], w["end_text"], w["end_pattern"]) == (120, 120, 290, 292)
    full = chains_ref(t, p, chain, S, 16, 4, NONE)
    assert (full["begin_text"], full["begin_pattern"], full["end_text"], full["end_pattern"]) == (0, 0, 400, 402) and full["score"] > w["score"]


@gpu
def test_the_xdrop_on_the_ends(eng):
    S = matrix("blast", 4)
    t, p, chain = chimeric_case()
    for x in (20, NONE):
        check(eng, [t], [p], [chain], S, 16, 4, x, [cached_ref("chimeric", t, p, chain, S, 16, 4, x)], "xdrop")


# ---- 6. (C2) on the device -----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("go,ge", GAPS)
def test_c2_on_the_device(eng, go, ge):
    S = matrix("blast", 4)
    cases = [build_case(85500 + k, 4, (rows, cols), [L], [], (cols, rows)) for k, (rows, cols, L) in
             enumerate(((0, 0, 0), (65, 70, 15), (0, 40, 64), (130, 3, 1), (200, 190, 0), (513, 100, 100)))]
    texts, patterns = [c[0] for c in cases], [c[1] for c in cases]
    seeds = [c[2][0] for c in cases]
    for x in (eng.NO_XDROP, 20):
        a = eng.score_batch(GLOBAL, texts, patterns, S, go, gap_extend=ge, xdrop=x, seeds=seeds)
        b = eng.score_batch(GLOBAL, texts, patterns, S, go, gap_extend=ge, xdrop=x, chains=[[s] for s in seeds])
        assert a.tolist() == b.tolist(), (x, "score")
        a = eng.align_pairs_affine(GLOBAL, texts, patterns, S, go, ge, xdrop=x, seeds=seeds)
        b = eng.align_pairs_affine(GLOBAL, texts, patterns, S, go, ge, xdrop=x, chains=[[s] for s in seeds])
        assert a == b, (x, "align")


# ---- 7. the Python keywords ------------------------------------------------------------------------------------
def test_chains_excludes_the_other_keywords():
    from sa_amd import engine
    t = np.zeros(10, np.int8)
    S = matrix("blast", 4)
    for extra in ({"seeds": [(0, 0, 0)]}, {"band": 3}, {"bands": [(-1, 1)]}, {"width": 3}):
        with pytest.raises(ValueError) as e:
            engine.score_batch(GLOBAL, [t], [t], S, 11, gap_extend=2, xdrop=20, chains=[[(0, 0, 1)]], **extra)
        assert "chains=" in str(e.value) and next(iter(extra)) in str(e.value)
    with pytest.raises(ValueError) as e:
        engine.score_batch(GLOBAL, [t], [t], S, 11, gap_extend=2, chains=[[(0, 0, 1)]])
    assert "xdrop" in str(e.value)
    with pytest.raises(ValueError):
        engine.score_batch(GLOBAL, [t, t], [t, t], S, 11, gap_extend=2, xdrop=20, chains=[[(0, 0, 1)]])


@gpu
def test_refusals_name_the_pair_and_the_seed(eng):
    S = matrix("blast", 4)
    t = synthetic.random_sequence(86600, 50, 4).astype(np.int8)
    for chains, code, words in (([[(0, 0, 5)], []], 1, ("pair 1", "no seed")),
                                ([[(0, 0, 5)], [(0, 0, 5), (3, 9, 2)]], 1, ("pair 1, seed 1", "begins before")),
                                ([[(0, 0, 5), (10, 10, 41)], [(0, 0, 5)]], 1, ("pair 0, seed 1", "does not lie inside"))):
        for call in (lambda: eng.score_batch(GLOBAL, [t, t], [t, t], S, 11, gap_extend=2, xdrop=20, chains=chains),
                     lambda: eng.align_pairs_affine(GLOBAL, [t, t], [t, t], S, 11, 2, xdrop=20, chains=chains)):
            with pytest.raises(eng.SaError) as e:
                call()
            assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)
    with pytest.raises(eng.SaError) as e:
        eng.score_batch(1, [t], [t], S, 11, gap_extend=2, xdrop=20, chains=[[(0, 0, 5)]])  # SA_LOCAL
    assert e.value.code == 1 and "SA_GLOBAL" in str(e.value)


# ---- 8. beyond the arena budget -----------------------------------------------------------------------------------
BIG_BUDGET = 8 << 20


def big_case():
    """About 6000 x 6000 with 60 seeds of 15 letters, the gaps between them 70 to 95 letters a side."""
    rng = np.random.default_rng(87700)
    gaps = [(int(rng.integers(70, 96)), int(rng.integers(70, 96))) for _ in range(59)]
    return build_case(87700, 4, (100, 100), [15] * 60, gaps, (110, 104))


@gpu
def test_a_long_pair_beyond_the_arena_budget_aligns_along_its_chain():
    """In a process of its own (the budget is read once per process): the pair's full directions are 18 MiB, the
    budget is 8 MiB and the chain's pieces take 3 MiB, where the seeds aligner on the first seed alone is refused."""
    t, p, chain = big_case()
    assert 5800 <= len(t) <= 6200 and 5800 <= len(p) <= 6200 and len(chain) == 60
    env = dict(os.environ, SA_TRACE_ARENA_BYTES=str(BIG_BUDGET))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "big"], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    child = json.loads(out.stdout.strip().splitlines()[-1])
    assert child["one_seed_error"] == 4  # SA_ERR_UNSUPPORTED
    want = chains_ref(t, p, chain, matrix("blast", 4), 11, 2, 20)
    assert child["result"] == pick(want)
    assert child["score"] == [want[f] for f in FIELDS]
    assert child["num_chunks"] == 1 and 0 < child["arena_bytes"] < BIG_BUDGET // 2


# ---- 9. the C++ functions --------------------------------------------------------------------------------------------
@gpu
def test_cpp_chains_check():
    out = subprocess.run([os.path.join(PKG, "bin", "sa_chains_check"), "700", "96", "8"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1] == "OK 96"


if __name__ == "__main__" and sys.argv[1:] == ["big"]:
    # the child of test_a_long_pair_beyond_the_arena_budget_aligns_along_its_chain
    from sa_amd import engine
    S_ = matrix("blast", 4)
    t_, p_, chain_ = big_case()
    try:
        engine.align_pairs_affine(GLOBAL, [t_], [p_], S_, 11, 2, xdrop=20, seeds=[chain_[0]])
        code = 0
    except engine.SaError as err:
        code = err.code
    res_ = engine.align_pairs_affine(GLOBAL, [t_], [p_], S_, 11, 2, xdrop=20, chains=[chain_])[0]
    stats_ = engine.affine_last_stats()
    sc_ = engine.score_batch(GLOBAL, [t_], [p_], S_, 11, gap_extend=2, xdrop=20, chains=[chain_])[0]
    print(json.dumps({"one_seed_error": code, "result": pick(res_), "arena_bytes": stats_["arena_bytes"],
                      "num_chunks": stats_["num_chunks"], "score": [int(sc_[f]) for f in FIELDS]}))
