"""Banded seed extension (sa_hip.h: sa_score_batch_seeds_band, sa_scorer_create_seeds_band,
sa_align_pairs_seeds_band; sa_scorer_fetch_seeds serves the scorer unchanged): both halves of a seeded pair are
banded extensions, each inside |j - i| <= width of its own matrix, the left half's being that of the reversed
prefixes. The reference of this file is seeds_band_ref: identity (S1), test_seeds_gpu.seeds_ref's composition
with test_extend_band_gpu.ext_band_ref for the halves. It is pinned on the CPU by (S2), by the mirror
identity (S3), which is exact because the band is symmetric, and by (W1); the GPU is then compared with it,
every field and both strings, at every forced rows_per_lane of the scorer and in the aligner once, and with the
library's own banded extension functions on host-reversed halves."""
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
from test_align_affine_gpu import alphabet_of, pick, rescore
from test_extend_band_gpu import ext_band_ref
from test_extend_gpu import GAPS, NONE, xd
from test_seeds_gpu import (BIG, BIG_BARE, BIG_BUDGET, HALF, SEED_L, XDROP, XGAP, big_pair, edge_cases, fields, mirror, mirrored,
                            seeds_ref, small_cases, xdrop_cases)

gpu = pytest.mark.gpu

GLOBAL, LOCAL, FIT, ENDS = 0, 1, 2, 16
WIDTHS = (0, 5, 64)


# ---- the reference of this file ------------------------------------------------------------------------
def seeds_band_ref(t, p, seed, S, go, ge, xdrop, w, alphabet=None, key=None):
    """(S1) with the banded extension: the keys of align_pairs_affine, the fields of sa_seed_result, the halves."""
    t, p = np.asarray(t, dtype=np.int64), np.asarray(p, dtype=np.int64)
    ts, ps, L = (int(v) for v in seed)
    assert ts + L <= len(t) and ps + L <= len(p)
    alphabet = alphabet or alphabet_of(S)
    left = ext_band_ref(t[:ts][::-1], p[:ps][::-1], S, go, ge, xdrop, w, alphabet, key=(key, ts, ps, L, "left") if key else None)
    right = ext_band_ref(t[ts + L:], p[ps + L:], S, go, ge, xdrop, w, alphabet, key=(key, ts, ps, L, "right") if key else None)
    mid = sum(int(S[p[ps + q]][t[ts + q]]) for q in range(L))
    res = {"score": left["score"] + mid + right["score"],
           "begin_text": ts - left["end_text"], "begin_pattern": ps - left["end_pattern"],
           "end_text": ts + L + right["end_text"], "end_pattern": ps + L + right["end_pattern"],
           "aligned_text": left["aligned_text"][::-1] + "".join(alphabet[c] for c in t[ts:ts + L]) + right["aligned_text"],
           "aligned_pattern": left["aligned_pattern"][::-1] + "".join(alphabet[c] for c in p[ps:ps + L]) + right["aligned_pattern"],
           "left_stop": left["stop_row"], "right_stop": right["stop_row"], "left": left, "right": right}
    res["num_bytes"] = len(res["aligned_text"])
    res["start_text"], res["start_pattern"] = res["begin_text"], res["begin_pattern"]
    return res


_REFS = {}


def cached_ref(key, t, p, seed, S, go, ge, xdrop, w):
    k = (key, tuple(seed), go, ge, xdrop, w)
    if k not in _REFS:
        _REFS[k] = seeds_band_ref(t, p, seed, S, go, ge, xdrop, w, key=key)
    return _REFS[k]


def check(eng, texts, patterns, seeds, S, go, ge, xdrop, w, wants, what, Rs=(1, 2, 4, 8)):
    x = xd(eng, xdrop)
    for R in Rs:
        got = eng.score_batch(GLOBAL, texts, patterns, S, go, rows_per_lane=R, gap_extend=ge, xdrop=x, seeds=seeds, width=w)
        assert got.dtype == eng.SEED_DTYPE and (got["status"] == 0).all()
        assert [fields(g) for g in got] == [fields(v) for v in wants], (what, "score", go, ge, xdrop, w, R)
        if go == ge:
            got = eng.score_batch(GLOBAL, texts, patterns, S, go, rows_per_lane=R, xdrop=x, seeds=seeds, width=w)
            assert [fields(g) for g in got] == [fields(v) for v in wants], (what, "score, gap_extend=None", go, xdrop, w, R)
    got = eng.align_pairs_affine(GLOBAL, texts, patterns, S, go, ge, xdrop=x, seeds=seeds, width=w)
    for k, (g, v) in enumerate(zip(got, wants)):
        assert pick(g) == pick(v), (what, "align", go, ge, xdrop, w, k, seeds[k], len(patterns[k]), len(texts[k]))
    return got


# ---- the reference of this file is sound (CPU) ---------------------------------------------------------
def test_s2_s3_and_w1_on_the_reference():
    differs = 0
    for k, (A, t, p, sd) in enumerate(small_cases(24, 91100)):
        S = matrix("blast" if A == 4 else "blosum50", A)
        mt, mp, msd = mirror(t, p, sd)
        for go, ge in ((11, 1), (5, 5), (-2, -1)):
            for x in (3, 20, NONE):
                full = seeds_ref(t, p, sd, S, go, ge, x)
                for w in (0, 1, 3, 40):
                    a = seeds_band_ref(t, p, sd, S, go, ge, x, w)
                    # S3: exact, ties included
                    b = seeds_band_ref(mt, mp, msd, S, go, ge, x, w)
                    want = mirrored(a, len(t), len(p))
                    assert {f: b[f] for f in want} == want, (k, sd, go, ge, x, w)
                    # S2: the seed at the origin is the banded extension
                    o, e = seeds_band_ref(t, p, (0, 0, 0), S, go, ge, x, w), ext_band_ref(t, p, S, go, ge, x, w)
                    assert pick(o) == pick(e) and fields(o) == (e["score"], 0, 0, e["end_text"], e["end_pattern"])
                    # W1
                    if w == 40:
                        assert pick(a) == pick(full) and fields(a) == fields(full), (k, sd, go, ge, x)
                    differs += fields(a) != fields(full)
    assert differs >= 20  # the band binds


# ---- 9. (S1): edge halves, against the reference and against the library's banded extension -------------------
def test_the_edge_cases_draw_from_the_edge_sizes():
    cases = edge_cases(4)
    assert {sd[1] for _, _, sd in cases} >= set(HALF) and {sd[2] for _, _, sd in cases} >= set(SEED_L)


@gpu
@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("go,ge", GAPS)
@pytest.mark.parametrize("A,mat", [(4, "blast"), (23, "blosum50")])
def test_edge_halves(eng, A, mat, go, ge, w):
    S = matrix(mat, A)
    cases = edge_cases(A)
    texts, patterns, seeds = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    for x in (NONE, 20):
        wants = [cached_ref(("edge", A, k), t, p, sd, S, go, ge, x, w) for k, (t, p, sd) in enumerate(cases)]
        check(eng, texts, patterns, seeds, S, go, ge, x, w, wants, "edge halves")


@gpu
@pytest.mark.parametrize("w", WIDTHS)
def test_s1_against_the_banded_extension_functions(eng, w):
    S = matrix("blast", 4)
    cases = edge_cases(4)
    texts, patterns, seeds = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    lt = [np.ascontiguousarray(t[:sd[0]][::-1]) for t, _, sd in cases]
    lp = [np.ascontiguousarray(p[:sd[1]][::-1]) for _, p, sd in cases]
    rt = [np.ascontiguousarray(t[sd[0] + sd[2]:]) for t, _, sd in cases]
    rp = [np.ascontiguousarray(p[sd[1] + sd[2]:]) for _, p, sd in cases]
    for go, ge in GAPS:
        for x in (20, eng.NO_XDROP):
            got = eng.score_batch(GLOBAL, texts, patterns, S, go, gap_extend=ge, xdrop=x, seeds=seeds, width=w)
            al = eng.align_pairs_affine(GLOBAL, texts, patterns, S, go, ge, xdrop=x, seeds=seeds, width=w)
            left = eng.score_batch(GLOBAL, lt, lp, S, go, gap_extend=ge, xdrop=x, width=w)
            right = eng.score_batch(GLOBAL, rt, rp, S, go, gap_extend=ge, xdrop=x, width=w)
            la = eng.align_pairs_affine(GLOBAL, lt, lp, S, go, ge, xdrop=x, width=w)
            ra = eng.align_pairs_affine(GLOBAL, rt, rp, S, go, ge, xdrop=x, width=w)
            for k, (t, p, (ts, ps, L)) in enumerate(cases):
                mid = sum(int(S[p[ps + q]][t[ts + q]]) for q in range(L))
                assert fields(got[k]) == (int(left[k]["score"]) + mid + int(right[k]["score"]), ts - int(left[k]["end_text"]),
                                          ps - int(left[k]["end_pattern"]), ts + L + int(right[k]["end_text"]),
                                          ps + L + int(right[k]["end_pattern"])), (go, ge, x, k)
                seed_t, seed_p = "".join("ATCG"[c] for c in t[ts:ts + L]), "".join("ATCG"[c] for c in p[ps:ps + L])
                assert al[k]["aligned_text"] == la[k]["aligned_text"][::-1] + seed_t + ra[k]["aligned_text"], (go, ge, x, k)
                assert al[k]["aligned_pattern"] == la[k]["aligned_pattern"][::-1] + seed_p + ra[k]["aligned_pattern"], (go, ge, x, k)
                assert al[k]["score"] == int(got[k]["score"])


# ---- 10. (S3) on the device, and the drop on each side -------------------------------------------------------------
def test_the_xdrop_cases_stop_inside_their_halves_inside_the_band():
    S = matrix("blast", 4)
    for w in WIDTHS:
        left = right = 0
        for k, (t, p, sd) in enumerate(xdrop_cases()):
            v = cached_ref(("xdrop", k), t, p, sd, S, *XGAP, XDROP, w)
            left += v["left_stop"] <= sd[1]
            right += v["right_stop"] <= len(p) - sd[1] - sd[2]
            assert v["score"] >= 5 * (sd[2] + 60)
        assert left >= 1 and right >= 1, (w, left, right)


@gpu
@pytest.mark.parametrize("w", WIDTHS)
def test_the_xdrop_on_each_side_and_the_mirror(eng, w):
    S = matrix("blast", 4)
    cases = xdrop_cases()
    texts, patterns, seeds = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    wants = [cached_ref(("xdrop", k), t, p, sd, S, *XGAP, XDROP, w) for k, (t, p, sd) in enumerate(cases)]
    check(eng, texts, patterns, seeds, S, *XGAP, XDROP, w, wants, "xdrop")
    nodrop = [cached_ref(("xdrop", k), t, p, sd, S, *XGAP, NONE, w) for k, (t, p, sd) in enumerate(cases)]
    check(eng, texts, patterns, seeds, S, *XGAP, NONE, w, nodrop, "xdrop, none", Rs=(8,))
    # S3 on the device: the mirrored pairs, from this call's own results; the edge cases with them
    cases = cases + edge_cases(4)
    texts, patterns, seeds = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    mir = [mirror(*c) for c in cases]
    for go, ge in GAPS + [XGAP]:
        for x in (XDROP, eng.NO_XDROP):
            a = eng.score_batch(GLOBAL, texts, patterns, S, go, gap_extend=ge, xdrop=x, seeds=seeds, width=w)
            b = eng.score_batch(GLOBAL, [c[0] for c in mir], [c[1] for c in mir], S, go, gap_extend=ge, xdrop=x, seeds=[c[2] for c in mir], width=w)
            aa = eng.align_pairs_affine(GLOBAL, texts, patterns, S, go, ge, xdrop=x, seeds=seeds, width=w)
            bb = eng.align_pairs_affine(GLOBAL, [c[0] for c in mir], [c[1] for c in mir], S, go, ge, xdrop=x, seeds=[c[2] for c in mir], width=w)
            for k, (t, p, _) in enumerate(cases):
                n, m = len(t), len(p)
                assert fields(b[k]) == (int(a[k]["score"]), n - int(a[k]["end_text"]), m - int(a[k]["end_pattern"]),
                                        n - int(a[k]["begin_text"]), m - int(a[k]["begin_pattern"])), (go, ge, x, k)
                assert (bb[k]["aligned_text"], bb[k]["aligned_pattern"]) == (aa[k]["aligned_text"][::-1], aa[k]["aligned_pattern"][::-1]), (go, ge, x, k)
                assert (bb[k]["start_text"], bb[k]["start_pattern"]) == (n - int(a[k]["end_text"]), m - int(a[k]["end_pattern"]))


# ---- W1 and a scorer run again ---------------------------------------------------------------------------------------
@gpu
def test_w1_and_a_scorer_run_again_on_new_arena_contents(eng):
    import torch
    S = matrix("blast", 4)
    cases = edge_cases(4) + xdrop_cases()
    texts, patterns, seeds = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    for go, ge in GAPS:
        for x in (20, eng.NO_XDROP):
            full = eng.score_batch(GLOBAL, texts, patterns, S, go, gap_extend=ge, xdrop=x, seeds=seeds)
            for w in (max(max(len(t), len(p)) for t, p in zip(texts, patterns)), 1 << 30):
                assert eng.score_batch(GLOBAL, texts, patterns, S, go, gap_extend=ge, xdrop=x, seeds=seeds, width=w).tobytes() == full.tobytes()
            assert (eng.align_pairs_affine(GLOBAL, texts, patterns, S, go, ge, xdrop=x, seeds=seeds, width=1 << 30) ==
                    eng.align_pairs_affine(GLOBAL, texts, patterns, S, go, ge, xdrop=x, seeds=seeds))
    to = np.concatenate([[0], np.cumsum([len(t) for t in texts])])
    po = np.concatenate([[0], np.cumsum([len(p) for p in patterns])])
    pairs = [(int(to[k]), len(texts[k]), int(po[k]), len(patterns[k])) for k in range(len(texts))]
    # new arena contents of the same shapes: every letter replaced by its complement; the seeds stay where they are
    ct, cp = [(3 - t).astype(np.int8) for t in texts], [(3 - p).astype(np.int8)[::1] for p in patterns]
    cp[0] = patterns[0].copy()  # and one pair that differs in more than its letters' names
    sc = eng.Scorer(GLOBAL, S, 11, pairs, gap_extend=2, xdrop=20, seeds=seeds, width=5, rows_per_lane=1)
    d1 = (torch.from_numpy(np.concatenate(texts)).cuda(), torch.from_numpy(np.concatenate(patterns)).cuda())
    d2 = (torch.from_numpy(np.concatenate(ct)).cuda(), torch.from_numpy(np.concatenate(cp)).cuda())
    sc.run(d1[0].data_ptr(), d1[1].data_ptr())
    first, ends = sc.results().copy(), sc.score_results().copy()
    sc.run(d2[0].data_ptr(), d2[1].data_ptr())
    second = sc.results().copy()
    sc.close()
    assert first.tolist() == eng.score_batch(GLOBAL, texts, patterns, S, 11, gap_extend=2, xdrop=20, seeds=seeds, width=5).tolist()
    assert second.tolist() == eng.score_batch(GLOBAL, ct, cp, S, 11, gap_extend=2, xdrop=20, seeds=seeds, width=5).tolist()
    # sa_scorer_fetch on a banded seeds scorer: the score with the absolute end cell
    assert [(int(e["score"]), int(e["end_text"]), int(e["end_pattern"])) for e in ends] == \
           [(int(f["score"]), int(f["end_text"]), int(f["end_pattern"])) for f in first]


# ---- 11. beyond the arena budget -------------------------------------------------------------------------------------
BIG_W = 64


@gpu
def test_the_bare_centre_beyond_the_arena_budget_aligns_inside_its_width():
    """In a process of its own (the budget is read once per process): the bare centre of 6000 x 6000 has two
    halves of 3000 x 3000, 9 MiB of directions together under a budget of 8 MiB. Inside a width of 64 each half
    takes about 1.1 MB and the pair aligns."""
    env = dict(os.environ, SA_TRACE_ARENA_BYTES=str(BIG_BUDGET))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "big"], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    child = json.loads(out.stdout.strip().splitlines()[-1])
    assert child["unbanded_error"] == 4 and "halves" in child["unbanded_message"]  # SA_ERR_UNSUPPORTED
    plan = subprocess.run([os.path.join(PKG, "bin", "sa_trace_plan_check"), "--mode", "global", "--gap", "11", "--gap-extend", "2",
                           "--budget", str(BIG_BUDGET), "--width", str(BIG_W), "--seeds", "%d:%d:%d" % BIG_BARE, f"{BIG}x{BIG}"],
                          capture_output=True, text=True, check=True)
    plan = json.loads(plan.stdout)
    assert child["arena_bytes"] == plan["arena_bytes"] == sum(it["dir_bytes"] for it in plan["items"]) and 2.0e6 < plan["arena_bytes"] < 2.4e6
    assert child["num_chunks"] == 1
    assert child["s1"] is True  # the halves through the banded extension aligner, host-reversed
    S = matrix("blast", 4)
    t, p = big_pair()
    res, sc = child["result"], child["score"]
    assert res["score"] == sc[0] and (res["start_text"], res["start_pattern"]) == (sc[1], sc[2])
    assert res["aligned_text"].replace("-", "") == "".join("ATCG"[c] for c in t[sc[1]:sc[3]])
    assert res["aligned_pattern"].replace("-", "") == "".join("ATCG"[c] for c in p[sc[2]:sc[4]])
    # the strings re-score, but for a gap that runs across the bare anchor: two gaps to the definition
    assert rescore(res, S, 11, 2, alphabet_of(S)) in (res["score"], res["score"] + 11 - 2)
    assert res["num_bytes"] > 5000


def _big_child():
    from sa_amd import engine as eng
    S = matrix("blast", 4)
    t, p = big_pair()
    ts, ps, L = BIG_BARE
    out = {}
    try:
        eng.align_pairs_affine(GLOBAL, [t], [p], S, 11, 2, xdrop=eng.NO_XDROP, seeds=[BIG_BARE])
        out["unbanded_error"], out["unbanded_message"] = 0, ""
    except eng.SaError as e:
        out["unbanded_error"], out["unbanded_message"] = e.code, str(e)
    got = eng.align_pairs_affine(GLOBAL, [t], [p], S, 11, 2, xdrop=eng.NO_XDROP, seeds=[BIG_BARE], width=BIG_W)[0]
    stats = eng.affine_last_stats()
    sc = eng.score_batch(GLOBAL, [t], [p], S, 11, gap_extend=2, xdrop=eng.NO_XDROP, seeds=[BIG_BARE], width=BIG_W)[0]
    halves = eng.align_pairs_affine(GLOBAL, [np.ascontiguousarray(t[:ts][::-1]), t[ts + L:]], [np.ascontiguousarray(p[:ps][::-1]), p[ps + L:]],
                                    S, 11, 2, xdrop=eng.NO_XDROP, width=BIG_W)
    out["s1"] = (got["score"] == halves[0]["score"] + halves[1]["score"] and
                 got["aligned_text"] == halves[0]["aligned_text"][::-1] + halves[1]["aligned_text"] and
                 got["aligned_pattern"] == halves[0]["aligned_pattern"][::-1] + halves[1]["aligned_pattern"])
    out.update(result=got, score=list(fields(sc)), arena_bytes=stats["arena_bytes"], num_chunks=stats["num_chunks"])
    print(json.dumps(out))


# ---- 12. refusals -----------------------------------------------------------------------------------------------------
@gpu
def test_refusals(eng):
    S = matrix("blast", 4)
    x = synthetic.random_sequence(1, 50, 4).astype(np.int8)
    y = x[:20]
    sd = [(10, 5, 3)]
    scorer = lambda mode, **kw: eng.Scorer(mode, S, 11, [(0, 50, 0, 20)], gap_extend=2, **kw)  # noqa: E731
    assert len(eng.score_batch(GLOBAL, [x], [y], S, 11, gap_extend=2, xdrop=20, seeds=sd, width=0)) == 1
    for mode, xdrop, w, seeds in ((GLOBAL, 20, -1, sd), (GLOBAL, -2, 3, sd), (GLOBAL, 1 << 30, 3, sd), (LOCAL, 20, 3, sd), (FIT, 20, 3, sd),
                                  (ENDS | 15, eng.NO_XDROP, 3, sd), (GLOBAL, 20, 3, [(48, 5, 3)]), (GLOBAL, 20, 3, [(10, 18, 3)])):
        for call in (lambda: eng.score_batch(mode, [x], [y], S, 11, gap_extend=2, xdrop=xdrop, seeds=seeds, width=w),
                     lambda: scorer(mode, xdrop=xdrop, seeds=seeds, width=w),
                     lambda: eng.align_pairs_affine(mode, [x], [y], S, 11, 2, xdrop=xdrop, seeds=seeds, width=w)):
            with pytest.raises(eng.SaError) as e:
                call()
            assert e.value.code == 1, (mode, xdrop, w, seeds)
    # the band's sentinel, which the unbanded seeds call stays clear of
    assert len(eng.score_batch(GLOBAL, [x], [y], S, 1 << 22, gap_extend=2, xdrop=20, seeds=sd)) == 1
    with pytest.raises(eng.SaError) as e:
        eng.score_batch(GLOBAL, [x], [y], S, 1 << 22, gap_extend=2, xdrop=20, seeds=sd, width=3)
    assert e.value.code == 4 and "scores may reach the band's sentinel" in str(e.value)
    # null seeds, and a seeds fetch on a scorer that is none
    p, S_keep, alpha_keep = eng._params(GLOBAL, S, 0, None, 0)
    out = np.zeros(1, eng.SEED_DTYPE)
    res = (eng.SaResult * 1)()
    hp = (eng.SaHostPair * 1)(eng.SaHostPair(x.ctypes.data, 50, y.ctypes.data, 20))
    dpair = (eng.SaPair * 1)(eng.SaPair(0, 50, 0, 20))
    one = np.array([[10, 5, 3]], dtype=np.uint64)
    h = ctypes.c_void_p()
    L = eng.lib
    assert L.sa_score_batch_seeds_band(ctypes.byref(p), 11, 2, 20, 3, one.ctypes.data, hp, 1, 0, out.ctypes.data) == 0
    assert L.sa_score_batch_seeds_band(ctypes.byref(p), 11, 2, 20, 3, None, hp, 1, 0, out.ctypes.data) == 1
    assert b"seeds is null" in L.sa_last_error()
    assert L.sa_score_batch_seeds_band(ctypes.byref(p), 11, 2, 20, -1, one.ctypes.data, hp, 1, 0, out.ctypes.data) == 1
    assert b"width must be >= 0" in L.sa_last_error()
    assert L.sa_score_batch_seeds_band(ctypes.byref(p), 11, 2, 20, 3, None, None, 0, 0, None) == 0
    assert L.sa_align_pairs_seeds_band(ctypes.byref(p), 11, 2, 20, 3, one.ctypes.data, hp, 1, 0, res, None, None) == 0
    assert L.sa_align_pairs_seeds_band(ctypes.byref(p), 11, 2, 20, 3, None, hp, 1, 0, res, None, None) == 1
    assert L.sa_align_pairs_seeds_band(ctypes.byref(p), 11, 2, 20, -1, one.ctypes.data, hp, 1, 0, res, None, None) == 1
    assert L.sa_scorer_create_seeds_band(ctypes.byref(p), 11, 2, 20, 3, None, dpair, 1, 0, ctypes.byref(h)) == 1
    assert L.sa_scorer_create_seeds_band(ctypes.byref(p), 11, 2, 20, 3, one.ctypes.data, dpair, 1, 0, None) == 1
    sc = eng.Scorer(GLOBAL, S, 11, [(0, 50, 0, 20)], gap_extend=2, xdrop=20, width=3)
    assert L.sa_scorer_fetch_seeds(sc.handle, out.ctypes.data, None) == 1
    sc.close()
    # band= and bands= with seeds= stay refused as they were, with or without width=
    for kw in ({"band": 3}, {"bands": [(0, 30)]}):
        for wkw in ({}, {"width": 3}):
            with pytest.raises(ValueError, match="xdrop= takes no band"):
                eng.score_batch(GLOBAL, [x], [y], S, 11, gap_extend=2, xdrop=20, seeds=sd, **kw, **wkw)
    # empty halves and zero pairs
    assert len(eng.score_batch(GLOBAL, [], [], S, 11, gap_extend=2, xdrop=20, seeds=np.zeros((0, 3)), width=3)) == 0
    assert eng.align_pairs_affine(GLOBAL, [], [], S, 11, 2, xdrop=20, seeds=np.zeros((0, 3)), width=3) == []
    none = np.zeros(0, dtype=np.int8)
    texts, patterns, seeds = [none, x, x, x], [none, none, y, y], [(0, 0, 0), (50, 0, 0), (0, 0, 20), (50, 20, 0)]
    for w in (0, 3):
        wants = [seeds_band_ref(t, q, s, S, 11, 2, 20, w) for t, q, s in zip(texts, patterns, seeds)]
        check(eng, texts, patterns, seeds, S, 11, 2, 20, w, wants, "empty")


if __name__ == "__main__" and sys.argv[1:] == ["big"]:
    _big_child()
