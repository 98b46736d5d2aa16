"""Banded alignment on a diagonal of the caller's (sa_hip.h: sa_score_batch_band_at,
sa_scorer_create_band_at, sa_align_pairs_band_at, sa_band_reachable): one band lo <= j - i <= hi per
pair, in global, local, fit and all 16 ends-free modes. Out-of-band cells are minus infinity in H, E and
F, border cells included; a border cell that costs is real only with the origin in band.
The reference of this file is band_at_ref: a numpy fill by anti-diagonals with those rules, the result
pick of test_ends_gpu.ends_end (minus infinity never wins it) and the walks of test_ends_gpu and
test_align_affine_gpu. It is pinned on the CPU against a plain double loop, against ends_ref where the
band admits every cell, against band_ref at the band the half-width derives, and by re-scoring its
strings; the GPU is then compared with it. Every GPU case asserts that its inputs are reachable, so none
is dropped silently; only the refusal test holds an unreachable pair."""
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
from test_align_affine_gpu import (DIAG, EDGE_SHAPES, EEXT, FEXT, KEYS, LEFT, NEG, STOP, TOP, affine_ref, alphabet_of,
                                   many_pairs, pick, rescore, walk)
from test_band_gpu import band_limits, band_ref, digest
from test_ends_gpu import ends_end, ends_ref, ends_walk
from test_fit_gpu import cell
from test_score_gpu import related_pair

gpu = pytest.mark.gpu

GLOBAL, LOCAL, FIT = 0, 1, 2
ENDS, TB, TE, PB, PE = 16, 1, 2, 4, 8
OVERLAP = ENDS | 15
ALL_MODES = [GLOBAL, LOCAL, FIT] + [ENDS | f for f in range(16)]


def flags_of(mode):
    """The free ends of a mode that is not local: global has none, fit the text's two."""
    return {GLOBAL: 0, FIT: TB | TE}.get(mode, mode & 15)


# ---- the reference of this file ------------------------------------------------------------------------
def borders(mode, n, m, go, ge, lo, hi):
    """(row 0, column 0) of H: H[0][0] = 0 iff the origin is in band; a free border cell is 0 iff in band;
    a border cell that costs is minus one gap run iff it and the origin are in band; else NEG."""
    tfree = mode == LOCAL or bool(flags_of(mode) & TB)
    pfree = mode == LOCAL or bool(flags_of(mode) & PB)
    origin = lo <= 0 <= hi
    row0, col0 = [NEG] * (n + 1), [NEG] * (m + 1)
    for j in range(n + 1):
        if lo <= j <= hi:
            row0[j] = 0 if j == 0 or tfree else -(go + (j - 1) * ge) if origin else NEG
    for i in range(m + 1):
        if lo <= -i <= hi:
            col0[i] = 0 if i == 0 or pfree else -(go + (i - 1) * ge) if origin else NEG
    return row0, col0


def fill_by_diagonals(mode, t, p, S, go, ge, lo, hi):
    """(H, D) swept by anti-diagonals over the in-band cells of each; D as
    test_align_affine_gpu.nibbles_by_diagonals has it."""
    t, p, S = np.asarray(t, dtype=np.int64), np.asarray(p, dtype=np.int64), np.asarray(S, dtype=np.int64)
    n, m = len(t), len(p)
    local = mode == LOCAL
    H = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    E = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    F = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    D = np.zeros((m + 1, n + 1), dtype=np.uint8)
    row0, col0 = borders(mode, n, m, go, ge, lo, hi)
    H[0, :], H[:, 0] = row0, col0
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
        # a run extends a run that exists: minus infinity minus ge is not above minus infinity minus go
        D[i, j] = src + EEXT * ((ee > eo) & (E[i, j - 1] > NEG // 2)) + FEXT * ((fe > fo) & (F[i - 1, j] > NEG // 2))
        # a cell that nothing real reaches stays minus infinity (NEG plus a few scores otherwise)
        dead = h < NEG // 2
        H[i, j], E[i, j], F[i, j] = np.where(dead, NEG, h), np.where(e < NEG // 2, NEG, e), np.where(f < NEG // 2, NEG, f)
    return H, D


def fill_by_loops(mode, t, p, S, go, ge, lo, hi):
    """The same as a plain double loop over all cells, the band a test per cell and minus infinity None."""
    n, m = len(t), len(p)
    local = mode == LOCAL
    row0, col0 = borders(mode, n, m, go, ge, lo, hi)
    none = lambda v: None if v == NEG else v  # noqa: E731
    sub = lambda v, k: None if v is None else v - k  # noqa: E731
    best = lambda *v: max([x for x in v if x is not None], default=None)  # noqa: E731
    H = [[None] * (n + 1) for _ in range(m + 1)]
    E = [[None] * (n + 1) for _ in range(m + 1)]
    F = [[None] * (n + 1) for _ in range(m + 1)]
    D = [[0] * (n + 1) for _ in range(m + 1)]
    H[0] = [none(v) for v in row0]
    for i in range(m + 1):
        H[i][0] = none(col0[i])
    gt = lambda a, b: a is not None and (b is None or a > b)  # noqa: E731
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            if not lo <= j - i <= hi:
                continue
            ee, eo, fe, fo = sub(E[i][j - 1], ge), sub(H[i][j - 1], go), sub(F[i - 1][j], ge), sub(H[i - 1][j], go)
            e, f = best(ee, eo), best(fe, fo)
            dg = None if H[i - 1][j - 1] is None else H[i - 1][j - 1] + int(S[p[i - 1]][t[j - 1]])
            h = best(dg, e, f)
            E[i][j], F[i][j] = e, f
            if h is None:
                continue
            src = DIAG if gt(dg, best(e, f)) else LEFT if not gt(f, e) else TOP
            if local and h <= 0:
                src = STOP
            D[i][j] = src + (EEXT if gt(ee, eo) else 0) + (FEXT if gt(fe, fo) else 0)
            H[i][j] = max(h, 0) if local else h
    return H, D


def reachable_by_fill(mode, t, p, S, go, ge, lo, hi):
    """Some candidate of the mode holds a real value."""
    if mode == LOCAL:
        return True
    H, _ = fill_by_loops(mode, t, p, S, go, ge, lo, hi)
    n, m, f = len(t), len(p), flags_of(mode)
    cand = [(m, n)] + ([(m, j) for j in range(n + 1)] if f & TE else []) + ([(i, n) for i in range(m + 1)] if f & PE else [])
    return any(H[i][j] is not None for i, j in cand)


_FILLS = {}  # (key, local, free row 0, free column 0, go, ge, lo, hi) -> (H, D): the newest few are kept


def band_at_ref(mode, t, p, S, go, ge, lo, hi, alphabet=None, key=None):
    """The alignment of mode inside lo <= j - i <= hi: the keys of align_pairs_affine plus end_text and
    end_pattern of the scorers and `inside`, whether every cell of the walk lies in the band. The pair
    must be reachable. With `key` (naming the pair and the scheme) the fill is shared by the modes with
    the same free begins."""
    t, p = np.asarray(t, dtype=np.int64), np.asarray(p, dtype=np.int64)
    n, m = len(t), len(p)
    alphabet = alphabet or alphabet_of(S)
    fl = 0 if mode == LOCAL else flags_of(mode)
    fk = (key, mode == LOCAL, bool(fl & TB), bool(fl & PB), go, ge, lo, hi)
    if key is None or fk not in _FILLS:
        H, D = fill_by_diagonals(mode, t, p, S, go, ge, lo, hi)
        if key is not None:
            while len(_FILLS) >= 8:
                _FILLS.pop(next(iter(_FILLS)))
            _FILLS[fk] = (H, D)
    else:
        H, D = _FILLS[fk]
    if mode in (GLOBAL, LOCAL):
        if mode == GLOBAL:
            assert H[m, n] > NEG // 2, "unreachable"
        res, _ = walk(mode, t, p, H, D, go, ge, alphabet)
        if mode == LOCAL:
            i, j = (0, 0) if H.max() <= 0 else (int(v) for v in np.unravel_index(int(H.argmax()), H.shape))
            res["score"] = max(res["score"], 0)  # 0 at (0, 0) without a positive cell, the origin in band or not
        else:
            i, j = m, n
            res["score"] = int(H[m, n])
        res["end_pattern"], res["end_text"] = i, j
    else:
        res = ends_walk(t, p, H, D, flags_of(mode), alphabet)
        assert res["score"] > NEG // 2, "unreachable"
        i, j = res["end_pattern"], res["end_text"]
    inside = lo <= j - i <= hi or (mode == LOCAL and res["score"] == 0)  # the empty local alignment is reported at (0, 0)
    for a, b in zip(reversed(res["aligned_text"]), reversed(res["aligned_pattern"])):
        j, i = j - (a != "-"), i - (b != "-")
        inside = inside and lo <= j - i <= hi
    res["inside"] = inside
    return res


_REF = {}


def ref_cached(key, *args, fill=None):
    """band_at_ref once per case, shared by the tests that meet the case again, and never changed."""
    if key not in _REF:
        _REF[key] = band_at_ref(*args, key=fill)
    return _REF[key]


def check(eng, mode, texts, patterns, S, go, ge, bands, wants, what, Rs=(1, 2, 4, 8)):
    """Every forced rows_per_lane of the band-at scorer, and the band-at aligner. The inputs are reachable."""
    for t, p, (lo, hi) in zip(texts, patterns, bands):
        assert eng.band_reachable(mode, len(t), len(p), lo, hi), (what, mode, len(t), len(p), lo, hi)
    for R in Rs:
        got = eng.score_batch(mode, texts, patterns, S, go, rows_per_lane=R, gap_extend=ge, bands=bands)
        assert [cell(g) for g in got] == [cell(x) for x in wants], (what, "score", mode, R)
    got = eng.align_pairs_affine(mode, texts, patterns, S, go, ge, bands=bands)
    for k, (g, x) in enumerate(zip(got, wants)):
        assert pick(g) == pick(x), (what, "align", mode, k, len(patterns[k]), len(texts[k]), bands[k])


# ---- 1. the reference of this file is sound (CPU) ------------------------------------------------------
def random_small_pairs(count, seed, nmax=40):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        A = 4 if k % 2 else 23
        n, m = int(rng.integers(1, nmax + 1)), int(rng.integers(1, nmax + 1))
        out.append((A,) + related_pair(seed + 10 * k, n, m, A))
    return out


def random_band(rng, n, m):
    lo = int(rng.integers(-m - 2, n + 3))
    return lo, lo + int(rng.integers(0, 12))


def test_band_at_ref_equals_the_plain_loops():
    rng = np.random.default_rng(1)
    for k, (A, t, p) in enumerate(random_small_pairs(60, 31100)):
        S = matrix("blast" if A == 4 else "blosum50", A)
        go, ge = ((11, 1), (5, 5), (4, 0), (3, 7), (-2, -1))[k % 5]
        for mode in (GLOBAL, LOCAL, FIT, ENDS | (k % 16), ENDS | ((5 * k + 3) % 16)):
            lo, hi = random_band(rng, len(t), len(p))
            H1, D1 = fill_by_diagonals(mode, t, p, S, go, ge, lo, hi)
            H2, D2 = fill_by_loops(mode, t, p, S, go, ge, lo, hi)
            real = np.array([[v is not None for v in row] for row in H2])
            assert ((H1 > NEG // 2) == real).all(), (k, mode, lo, hi)
            assert (H1[real] == np.array([[0 if v is None else v for v in row] for row in H2])[real]).all(), (k, mode, lo, hi)
            assert (D1[real] == np.array(D2, dtype=np.uint8)[real]).all(), (k, mode, lo, hi)
            jj, ii = np.meshgrid(np.arange(len(t) + 1), np.arange(len(p) + 1))
            assert not real[(jj - ii < lo) | (jj - ii > hi)].any()


def test_band_at_ref_equals_ends_ref_when_the_band_admits_every_cell():
    for k, (A, t, p) in enumerate(random_small_pairs(30, 32200)):
        S = matrix("blast" if A == 4 else "blosum50", A)
        go, ge = ((11, 1), (5, 5), (4, 0), (0, 0), (-2, -1))[k % 5]
        n, m = len(t), len(p)
        for f in range(16):
            got = band_at_ref(ENDS | f, t, p, S, go, ge, -m, n)
            assert got["inside"] and {x: got[x] for x in got if x != "inside"} == ends_ref(t, p, S, go, ge, f, key=("full", k)), (k, f)
        for mode in (GLOBAL, LOCAL):
            assert pick(band_at_ref(mode, t, p, S, go, ge, -m, n)) == affine_ref(mode, t, p, S, go, ge), (k, mode)
        assert pick(band_at_ref(FIT, t, p, S, go, ge, -m - 7, n + 9)) == pick(ends_ref(t, p, S, go, ge, TB | TE))


def test_band_at_ref_equals_band_ref_at_the_derived_band():
    for k, (A, t, p) in enumerate(random_small_pairs(30, 33300)):
        S = matrix("blast" if A == 4 else "blosum50", A)
        go, ge = ((11, 1), (5, 5), (4, 0), (3, 7), (-2, -1))[k % 5]
        for w in (0, 1, 3, 9):
            lo, hi = band_limits(len(t), len(p), w)
            for mode in (GLOBAL, LOCAL):
                assert band_at_ref(mode, t, p, S, go, ge, lo, hi) == band_ref(mode, t, p, S, go, ge, w), (k, w, mode)


def test_band_at_ref_strings_rescore_and_stay_inside_the_band():
    rng = np.random.default_rng(2)
    seen = 0
    for k, (A, t, p) in enumerate(random_small_pairs(40, 34400)):
        S = matrix("blast" if A == 4 else "blosum50", A)
        alpha = alphabet_of(S)
        for go, ge in ((11, 1), (5, 5), (4, 0)):
            for mode in ALL_MODES:
                lo, hi = random_band(rng, len(t), len(p))
                if not reachable_by_fill(mode, t, p, S, go, ge, lo, hi):
                    continue
                seen += 1
                res = band_at_ref(mode, t, p, S, go, ge, lo, hi)
                assert rescore(res, S, go, ge, alpha) == res["score"], (k, go, ge, mode, lo, hi)
                assert res["inside"], (k, go, ge, mode, lo, hi)
                if mode not in (GLOBAL, LOCAL):
                    assert res["score"] <= ends_ref(t, p, S, go, ge, flags_of(mode))["score"]
    assert seen > 500


def crop(t, p, lo, hi):
    """A fit pair whose band lies inside the text, lo >= 0 and m + hi <= n, as the pair of the text's
    columns lo + 1 .. m + hi under the band 0 .. hi - lo: the same cells, text indices lower by lo."""
    return t[lo:len(p) + hi], (0, hi - lo)


def test_a_fit_band_inside_the_text_is_the_band_of_the_cropped_text():
    for k, (A, t, p) in enumerate(random_small_pairs(30, 35500, nmax=30)):
        S = matrix("blast" if A == 4 else "blosum50", A)
        t = np.resize(t, len(p) + 25)
        for lo, hi in ((0, 3), (5, 5), (7, 20), (2, 25)):
            a = band_at_ref(FIT, t, p, S, 11, 2, lo, hi)
            tc, (l2, h2) = crop(t, p, lo, hi)
            b = band_at_ref(FIT, tc, p, S, 11, 2, l2, h2)
            b["start_text"] += lo
            b["end_text"] += lo
            assert a == b, (k, lo, hi)


def fit_band(n, m, w):
    """A band of half-width w that a fit can use: around the middle of the diagonals 0 .. n - m of the
    windows, or for a pattern longer than its text from diagonal n - m (the end cell's) to diagonal 0."""
    return ((n - m) // 2 - w, (n - m) // 2 + w) if n >= m else (n - m - w, w)


# ---- 2. the three identities of sa_hip.h ---------------------------------------------------------------------
SHAPES = EDGE_SHAPES + [(63, 70), (65, 60), (511, 520), (513, 500)]  # (m, n)
WIDTHS = [0, 1, 63, 64, 65]


def shape_pairs(A, seed=41000):
    pairs = [related_pair(seed + 3 * m + 5 * n + A, n, m, A) for m, n in SHAPES]
    return [t for t, _ in pairs], [p for _, p in pairs]


@gpu
@pytest.mark.parametrize("w", WIDTHS)
def test_the_derived_band_is_the_banded_function(eng, w):
    S = matrix("blast", 4)
    texts, patterns = shape_pairs(4)
    bands = [band_limits(len(t), len(p), w) for t, p in zip(texts, patterns)]
    for go, ge in ((11, 2), (5, 5)):
        for mode in (GLOBAL, LOCAL):
            for R in (1, 2, 4, 8):
                a = eng.score_batch(mode, texts, patterns, S, go, rows_per_lane=R, gap_extend=ge, bands=bands)
                b = eng.score_batch(mode, texts, patterns, S, go, rows_per_lane=R, gap_extend=ge, band=w)
                assert a.tobytes() == b.tobytes(), (mode, go, ge, R)
            assert (eng.align_pairs_affine(mode, texts, patterns, S, go, ge, bands=bands) ==
                    eng.align_pairs_affine(mode, texts, patterns, S, go, ge, band=w)), (mode, go, ge)


@gpu
@pytest.mark.parametrize("A,mat", [(4, "blast"), (23, "blosum50")])
def test_the_whole_rectangle_is_the_unbanded_function_and_fit_is_its_flag_set(eng, A, mat):
    S = matrix(mat, A)
    texts, patterns = shape_pairs(A)
    bands = [(-len(p), len(t)) for t, p in zip(texts, patterns)]
    wide = [(-(1 << 31), (1 << 31) - 1)] * len(texts)  # any int32 limits: as if clipped
    go, ge = 11, 2
    for mode in ALL_MODES:
        for R in (1, 2, 4, 8):
            a = eng.score_batch(mode, texts, patterns, S, go, rows_per_lane=R, gap_extend=ge, bands=bands)
            b = eng.score_batch(mode, texts, patterns, S, go, rows_per_lane=R, gap_extend=ge)
            assert a.tobytes() == b.tobytes(), (mode, R)
        full = eng.align_pairs_affine(mode, texts, patterns, S, go, ge)
        assert eng.align_pairs_affine(mode, texts, patterns, S, go, ge, bands=bands) == full, mode
        assert eng.align_pairs_affine(mode, texts, patterns, S, go, ge, bands=wide) == full, mode
    # SA_ENDS_FREE | TB | TE equals SA_FIT under a band that binds, too
    bands = [fit_band(len(t), len(p), 3) for t, p in zip(texts, patterns)]
    for t, p, (lo, hi) in zip(texts, patterns, bands):
        assert eng.band_reachable(FIT, len(t), len(p), lo, hi)
    for R in (1, 2, 4, 8):
        a = eng.score_batch(ENDS | TB | TE, texts, patterns, S, go, rows_per_lane=R, gap_extend=ge, bands=bands)
        assert a.tobytes() == eng.score_batch(FIT, texts, patterns, S, go, rows_per_lane=R, gap_extend=ge, bands=bands).tobytes()
    assert (eng.align_pairs_affine(ENDS | TB | TE, texts, patterns, S, go, ge, bands=bands) ==
            eng.align_pairs_affine(FIT, texts, patterns, S, go, ge, bands=bands))
    # a linear caller passes its penalty twice: bands without gap_extend
    lin = eng.score_batch(FIT, texts, patterns, S, 5, bands=bands)
    assert lin.tobytes() == eng.score_batch(FIT, texts, patterns, S, 5, gap_extend=5, bands=bands).tobytes()


# ---- 3. a read inside a window: fit and all 16 flag sets ------------------------------------------------------
READ_MS = [63, 64, 65, 150, 513]
READ_WS = [0, 5, 64]


def read_band(mode, n, m, c, w):
    """[c - w, c + w], stretched to the origin where the text's begin is not free and to diagonal n - m
    where its end is not: fit and every flag set with TB and TE keep the band as it is, and every other
    flag set has a reachable case of its own."""
    f = flags_of(mode)
    lo, hi = c - w, c + w
    if not f & TB:
        lo = min(lo, 0)
    if not f & TE:
        hi = max(hi, n - m)
    return lo, hi


def read_in_window(m, c):
    """A text of m + 300 letters that holds a mutated copy of the pattern from letter c on."""
    n = m + 300
    t = synthetic.random_sequence(500 + m, n, 4).astype(np.int8)
    p = synthetic.mutate(t[c:c + m], 501 + m + c, 4, m).astype(np.int8)
    return t, p


@gpu
@pytest.mark.parametrize("w", READ_WS)
@pytest.mark.parametrize("m", READ_MS)
def test_a_read_inside_a_window(eng, m, w):
    S = matrix("blast", 4)
    n = m + 300
    centres = [0, 1, 63, 64, 130, n - m]
    pairs = [read_in_window(m, c) for c in centres]
    texts, patterns = [t for t, _ in pairs], [p for _, p in pairs]
    # in the order of the free begins and of the stretch: a pair's fill serves the flag sets that share them
    for mode in [FIT] + sorted([ENDS | f for f in range(16)], key=lambda x: (x & TB, x & PB, x & TE)):
        bands = [read_band(mode, n, m, c, w) for c in centres]
        wants = [ref_cached(("read", m, c, mode if mode != FIT else ENDS | TB | TE) + bands[k], mode, texts[k], patterns[k], S, 11, 2,
                            *bands[k], fill=("read", m, c)) for k, c in enumerate(centres)]
        assert all(x["inside"] for x in wants)
        check(eng, mode, texts, patterns, S, 11, 2, bands, wants, "read")
    # the windows start past body 0 and end before n: at c = 130, w = 5 no strip meets columns 1..64 or n
    assert read_band(FIT, n, m, 130, 5) == (125, 135)


# ---- 4. a band that enters through column 0 past whole strips, and one that leaves through column n --------
@gpu
@pytest.mark.parametrize("f", [PB, PB | PE | TE])
@pytest.mark.parametrize("lo,hi", [(-700, -560), (-70, -1)])
def test_the_band_enters_through_column_0(eng, f, lo, hi):
    """m = 1100, n = 600, hi < 0: no cell of rows 1 .. -hi is in band. With hi = -560 strip 0 is empty at
    R = 8 and strips 0 to 7 at R = 1; the rows before -hi + 1 store no direction word."""
    S = matrix("blast", 4)
    m, n = 1100, 600
    p = synthetic.random_sequence(610, m, 4).astype(np.int8)
    start = (-lo - hi) // 2
    t = synthetic.mutate(np.resize(p[start:], n), 611, 4, n).astype(np.int8)
    if f == PB:
        # without a free end the alignment ends in (m, n) on diagonal -500, which neither band holds: the
        # pair is refused as it stands, and runs with its band stretched to that diagonal
        assert not eng.band_reachable(ENDS | f, n, m, lo, hi)
        with pytest.raises(eng.SaError) as e:
            eng.score_batch(ENDS | f, [t], [p], S, 11, gap_extend=2, bands=[(lo, hi)])
        assert e.value.code == 1 and "pair 0" in str(e.value)
        lo, hi = min(lo, n - m), max(hi, n - m)
    want = ref_cached(("column 0", f, lo, hi), ENDS | f, t, p, S, 11, 2, lo, hi)
    assert want["inside"] and want["start_text"] == 0 and -hi <= want["start_pattern"] <= -lo
    check(eng, ENDS | f, [t], [p], S, 11, 2, [(lo, hi)], [want], "column 0")
    # beside an unbanded-like pair in one call: the row buffer and the direction arena are shared
    x, y = related_pair(612, 300, 280, 4)
    w2 = ref_cached(("column 0 mate", f), ENDS | f, x, y, S, 11, 2, -280, 300)
    check(eng, ENDS | f, [x, t, x], [y, p, y], S, 11, 2, [(-280, 300), (lo, hi), (-280, 300)], [w2, want, w2], "column 0, mixed")


@gpu
@pytest.mark.parametrize("f", [TB | PE, 15])
@pytest.mark.parametrize("lo,hi", [(100, 140), (1, 64)])
def test_the_band_leaves_through_column_n(eng, f, lo, hi):
    """m = 1100, n = 300, lo > 0: the band starts on row 0 and leaves through column n at rows n - hi ..
    n - lo; the strips below hold no in-band cell, and only the in-band rows of column n are candidates."""
    S = matrix("blast", 4)
    m, n = 1100, 300
    t = synthetic.random_sequence(620, n, 4).astype(np.int8)
    at = (lo + hi) // 2
    p = np.resize(synthetic.mutate(t[at:], 621, 4, n - at), m).astype(np.int8)
    want = ref_cached(("column n", f, lo, hi), ENDS | f, t, p, S, 11, 2, lo, hi)
    assert want["inside"] and want["end_text"] == n and n - hi <= want["end_pattern"] <= n - lo and want["start_pattern"] == 0
    check(eng, ENDS | f, [t], [p], S, 11, 2, [(lo, hi)], [want], "column n")
    # the unbanded best of column n lies elsewhere or scores more: the fold is masked, not merely unused
    full = ends_ref(t, p, S, 11, 2, f)
    assert full["score"] >= want["score"]


# ---- 5. ties ---------------------------------------------------------------------------------------------------
@gpu
def test_ties_with_one_candidate_out_of_band(eng):
    """test_ends_gpu's tie pairs under bands that admit one of the tied cells only. The text is X, junk, Y
    and the pattern Y, junk, X: (L, n) and (m, L) tie at 5 L, and (L, n) wins without a band."""
    S = matrix("blast", 4)
    m, n, L = 600, 300, 65
    X, Y = synthetic.random_sequence(72, L, 2), synthetic.random_sequence(73, L, 2)
    p = np.full(m, 2, dtype=np.int8)
    p[:L], p[m - L:] = Y, X
    t = np.full(n, 3, dtype=np.int8)
    t[:L], t[n - L:] = X, Y
    for go, ge in ((11, 2), (5, 5)):
        assert cell(ends_ref(t, p, S, go, ge, 15)) == (5 * L, L, n)
        # diagonal of Y against Y is n - L, of X against X -(m - L)
        for (lo, hi), end in (((-m, n), (L, n)), ((-m, n - L - 1), (m, L)), ((-(m - L) + 1, n), (L, n)),
                              ((-(m - L), n - L), (L, n))):
            want = band_at_ref(OVERLAP, t, p, S, go, ge, lo, hi)
            assert cell(want) == (5 * L,) + end, (lo, hi)
            check(eng, OVERLAP, [t], [p], S, go, ge, [(lo, hi)], [want], "ties")
    # a border candidate equal to an interior one: m = 1, every substitution -4, gap 1: H[1][j] = -1 = H[1][0]
    S4 = np.full((4, 4), -4, dtype=np.int32)
    t, p = synthetic.random_sequence(3, 70, 4), synthetic.random_sequence(4, 1, 4)
    for go, ge in ((1, 1), (1, 3)):
        # all of row 1 ties with (1, 0): (1, 1) wins; (1, 0) out of band; (1, 1) reached over (1, 0) only and
        # lower; a band inside the text: its first column
        for (lo, hi), end in (((-1, 69), (1, 1)), ((0, 69), (1, 1)), ((-1, 0), (1, 0)), ((3, 9), (1, 4))):
            want = band_at_ref(FIT, t, p, S4, go, ge, lo, hi)
            assert cell(want) == (-1,) + end, (lo, hi)
            check(eng, FIT, [t], [p], S4, go, ge, [(lo, hi)], [want], "flat")
            check(eng, ENDS | TB | TE, [t], [p], S4, go, ge, [(lo, hi)], [want], "flat")


# ---- 6. stale boundary rows: more pairs than waves, long pairs between short ones, per-pair centres --------
def mapped_pairs():
    """many_pairs three times over with, every 25th, a read of 700 to 1500 letters in a text 400 longer;
    each pair's band is 8 diagonals around a random centre in 0 .. n - m."""
    texts, patterns = many_pairs()
    texts, patterns = list(texts) * 3, list(patterns) * 3
    rng = np.random.default_rng(199)
    bands = []
    for k in range(len(texts)):
        if k % 25 == 0:
            m = int(rng.integers(700, 1501))
            t = synthetic.random_sequence(17000 + k, m + 400, 4).astype(np.int8)
            c = int(rng.integers(0, 401))
            texts[k], patterns[k] = t, synthetic.mutate(t[c:], 17001 + k, 4, m).astype(np.int8)
        else:
            n, m = len(texts[k]), len(patterns[k])
            if m > n:
                texts[k], patterns[k], n, m = patterns[k], texts[k], m, n
            c = int(rng.integers(0, n - m + 1))
        bands.append((c - 8, c + 8))
    return texts, patterns, bands


@gpu
def test_pairs_outnumber_waves_and_reruns(eng):
    import torch
    S = matrix("blast", 4)
    go, ge = 9, 1
    texts, patterns, bands = mapped_pairs()
    for t, p, (lo, hi) in zip(texts, patterns, bands):
        assert eng.band_reachable(FIT, len(t), len(p), lo, hi)
    to = np.concatenate([[0], np.cumsum([len(t) for t in texts])])
    po = np.concatenate([[0], np.cumsum([len(p) for p in patterns])])
    dt, dp = torch.from_numpy(np.concatenate(texts)).cuda(), torch.from_numpy(np.concatenate(patterns)).cuda()
    sc = eng.Scorer(FIT, S, go, [(int(to[k]), len(texts[k]), int(po[k]), len(patterns[k])) for k in range(len(texts))],
                    gap_extend=ge, bands=bands)
    assert sc.info()["num_waves"] < len(texts)
    sc.run(dt.data_ptr(), dp.data_ptr())
    first = sc.results().copy()
    sc.run(dt.data_ptr(), dp.data_ptr())
    second = sc.results().copy()
    sc.close()
    assert digest(first.tolist()) == digest(second.tolist())
    assert first.tolist() == eng.score_batch(FIT, texts, patterns, S, go, gap_extend=ge, bands=bands).tolist()
    got = eng.align_pairs_affine(FIT, texts, patterns, S, go, ge, bands=bands)
    assert [g["score"] for g in got] == first["score"].tolist()
    rng = np.random.default_rng(4)
    for k in list(range(0, len(texts), 375)) + rng.choice(len(texts), 120, replace=False).tolist():
        want = band_at_ref(FIT, texts[k], patterns[k], S, go, ge, *bands[k])
        assert cell(first[k]) == cell(want) and pick(got[k]) == pick(want), int(k)
    again = eng.align_pairs_affine(FIT, texts, patterns, S, go, ge, bands=bands)
    assert digest([[r[k] for k in KEYS] for r in again]) == digest([[r[k] for k in KEYS] for r in got])


# ---- 7. negative and zero penalties -------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("go,ge", [(3, 7), (0, 0), (-2, -1), (4, 0)])
def test_negative_and_zero_penalties(eng, go, ge):
    S = matrix("blast", 4)
    shapes = [(9, 65), (64, 70), (129, 120), (513, 500), (300, 700)]  # (m, n)
    pairs = [related_pair(1200 + 3 * m + 5 * n, n, m, 4) for m, n in shapes]
    texts, patterns = [t for t, _ in pairs], [p for _, p in pairs]
    for f in (0, 3, 15, 9):
        for w in (0, 5, 64):
            # around the main diagonal and the corner's: reachable for every flag set
            bands = [(min(0, len(t) - len(p)) - w, max(0, len(t) - len(p)) + w) for t, p in pairs]
            if f & TB and f & TE:
                bands = [fit_band(len(t), len(p), w) for t, p in pairs]
            wants = [band_at_ref(ENDS | f, t, p, S, go, ge, lo, hi) for (t, p), (lo, hi) in zip(pairs, bands)]
            check(eng, ENDS | f, texts, patterns, S, go, ge, bands, wants, "penalties")


# ---- 8. empty sides, zero pairs, refusals ----------------------------------------------------------------------------
@gpu
def test_empty_sides_and_zero_pairs(eng):
    S = matrix("blast", 4)
    x, none = synthetic.random_sequence(1, 50, 4), np.zeros(0, dtype=np.int8)
    for mode in ALL_MODES:
        assert eng.align_pairs_affine(mode, [], [], S, 11, 2, bands=[]) == []
        assert len(eng.score_batch(mode, [], [], S, 11, gap_extend=2, bands=np.zeros((0, 2), np.int32))) == 0
    for go, ge in ((11, 2), (-3, 1), (2, -1), (4, 0)):
        for mode in ALL_MODES:
            texts, patterns, bands = [], [], []
            for t, p in ((none, none), (x[:5], none), (none, x[:5]), (x[:1], x[1:2])):
                for lo, hi in ((-5, 5), (0, 0), (-3, 0), (0, 2), (-4, -2), (2, 3), (-1, 1)):
                    if eng.band_reachable(mode, len(t), len(p), lo, hi):
                        texts.append(t), patterns.append(p), bands.append((lo, hi))
            assert len(texts) >= 8, mode
            wants = [band_at_ref(mode, t, p, S, go, ge, lo, hi) for t, p, (lo, hi) in zip(texts, patterns, bands)]
            check(eng, mode, texts, patterns, S, go, ge, bands, wants, "empty")
    got = eng.align_pairs_affine(FIT, [x], [x[:40]], S, 11, 2, strings=False, bands=[(2, 6)])[0]
    want = band_at_ref(FIT, x, x[:40], S, 11, 2, 2, 6)
    assert got == {k: want[k] for k in KEYS[:4]}


@gpu
def test_refusals(eng):
    S = matrix("blast", 4)
    x = synthetic.random_sequence(1, 50, 4)
    y = x[:20]
    # lo > hi, and band= with bands=
    for call in (lambda: eng.score_batch(FIT, [x], [y], S, 11, gap_extend=2, bands=[(5, 4)]),
                 lambda: eng.Scorer(FIT, S, 11, [(0, 50, 0, 20)], gap_extend=2, bands=[(5, 4)]),
                 lambda: eng.align_pairs_affine(LOCAL, [x], [y], S, 11, 2, bands=[(5, 4)])):
        with pytest.raises(eng.SaError) as e:
            call()
        assert e.value.code == 1 and "pair 0" in str(e.value)
    with pytest.raises(ValueError):
        eng.score_batch(GLOBAL, [x], [y], S, 11, gap_extend=2, band=3, bands=[(0, 30)])
    # an unreachable pair in the middle of a batch: the whole call is refused, its index named, nothing run
    assert not eng.band_reachable(FIT, 50, 20, 31, 40) and eng.band_reachable(FIT, 50, 20, 0, 30)
    stats = eng.align_pairs_affine(FIT, [x], [y], S, 11, 2, bands=[(0, 30)]) and eng.affine_last_stats()
    for call in (lambda: eng.score_batch(FIT, [x, x, x], [y, y, y], S, 11, gap_extend=2, bands=[(0, 30), (31, 40), (0, 30)]),
                 lambda: eng.align_pairs_affine(FIT, [x, x, x], [y, y, y], S, 11, 2, bands=[(0, 30), (31, 40), (0, 30)])):
        with pytest.raises(eng.SaError) as e:
            call()
        assert e.value.code == 1 and "pair 1" in str(e.value) and "[31, 40]" in str(e.value)
    assert stats["num_chunks"] == 1
    # the score limit is the banded one
    with pytest.raises(eng.SaError) as e:
        eng.align_pairs_affine(FIT, [x], [y], S, 1 << 22, 2, bands=[(0, 30)])
    assert e.value.code == 4
    # an out-of-alphabet byte
    bad = x.copy()
    bad[10] = 4
    for call in (lambda: eng.score_batch(FIT, [bad, x], [y, y], S, 11, gap_extend=2, bands=[(0, 30), (0, 30)]),
                 lambda: eng.align_pairs_affine(OVERLAP, [bad, x], [y, y], S, 11, 2, bands=[(0, 30), (0, 30)])):
        with pytest.raises(eng.SaError) as e:
            call()
        assert e.value.code == 1
    # null arguments
    p, S_keep, alpha_keep = eng._params(FIT, S, 0, None, 0)
    res = (eng.SaResult * 1)()
    out = (eng.SaScoreResult * 1)()
    hp = (eng.SaHostPair * 1)(eng.SaHostPair(x.ctypes.data, 50, y.ctypes.data, 20))
    b = np.array([[0, 30]], dtype=np.int32)
    buf = ctypes.create_string_buffer(100)
    one = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    h = ctypes.c_void_p()
    L = eng.lib
    assert L.sa_align_pairs_band_at(ctypes.byref(p), 11, 2, None, hp, 1, 0, res, None, None) == 1  # bands == NULL
    assert L.sa_score_batch_band_at(ctypes.byref(p), 11, 2, None, hp, 1, 0, out) == 1
    assert L.sa_scorer_create_band_at(ctypes.byref(p), 11, 2, None, (eng.SaPair * 1)(eng.SaPair(0, 50, 0, 20)), 1, 0, ctypes.byref(h)) == 1
    assert L.sa_align_pairs_band_at(ctypes.byref(p), 11, 2, None, hp, 0, 0, res, None, None) == 0   # no pair reads it
    assert L.sa_score_batch_band_at(ctypes.byref(p), 11, 2, None, hp, 0, 0, out) == 0
    assert L.sa_align_pairs_band_at(None, 11, 2, b.ctypes.data, hp, 1, 0, res, None, None) == 1
    assert L.sa_align_pairs_band_at(ctypes.byref(p), 11, 2, b.ctypes.data, None, 1, 0, res, None, None) == 1
    assert L.sa_align_pairs_band_at(ctypes.byref(p), 11, 2, b.ctypes.data, hp, 1, 0, None, None, None) == 1
    assert L.sa_align_pairs_band_at(ctypes.byref(p), 11, 2, b.ctypes.data, hp, 1, 0, res, one, None) == 1
    assert L.sa_align_pairs_band_at(ctypes.byref(p), 11, 2, b.ctypes.data, hp, -1, 0, res, None, None) == 1
    assert L.sa_score_batch_band_at(None, 11, 2, b.ctypes.data, hp, 1, 0, out) == 1
    assert L.sa_score_batch_band_at(ctypes.byref(p), 11, 2, b.ctypes.data, None, 1, 0, out) == 1
    assert L.sa_score_batch_band_at(ctypes.byref(p), 11, 2, b.ctypes.data, hp, 1, 0, None) == 1
    assert L.sa_scorer_create_band_at(ctypes.byref(p), 11, 2, b.ctypes.data, None, 1, 0, ctypes.byref(h)) == 1
    assert L.sa_scorer_create_band_at(ctypes.byref(p), 11, 2, b.ctypes.data, None, 0, 0, None) == 1
    p.mode = 3
    assert L.sa_score_batch_band_at(ctypes.byref(p), 11, 2, b.ctypes.data, hp, 1, 0, out) == 1
    assert eng.lib.sa_band_reachable(3, 50, 20, eng.SaBand(0, 30)) == -1
    # the banded functions on the half-width still refuse the modes without a diagonal of their own
    for call in (lambda: eng.score_batch(FIT, [x], [x], S, 11, gap_extend=2, band=5),
                 lambda: eng.align_pairs_affine(OVERLAP, [x], [x], S, 11, 2, band=5)):
        with pytest.raises(eng.SaError) as e:
            call()
        assert e.value.code == 4  # SA_ERR_UNSUPPORTED


# ---- 9. beyond the arena budget -----------------------------------------------------------------------------------
BIG_M, BIG_N, BIG_C, BIG_W, BIG_BUDGET = 6000, 40000, 21000, 100, 8 << 20


def big_pair():
    t = synthetic.random_sequence(161, BIG_N, 4).astype(np.int8)
    return t, synthetic.mutate(t[BIG_C:], 162, 4, BIG_M).astype(np.int8)


@gpu
def test_a_fit_pair_beyond_the_arena_budget_aligns_inside_its_band():
    """In a process of its own (the budget is read once per process): a 6000-letter read in a 40000-letter
    text needs 118 MiB of directions, the budget is 8 MiB, the band of 100 diagonals around the read's
    place takes 2.6 MiB. The reference is band_at_ref on the text's columns under the band (crop, pinned
    above)."""
    env = dict(os.environ, SA_TRACE_ARENA_BYTES=str(BIG_BUDGET))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "big"], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    child = json.loads(out.stdout.strip().splitlines()[-1])
    assert child["unbanded_error"] == 4  # SA_ERR_UNSUPPORTED
    lo, hi = BIG_C - BIG_W, BIG_C + BIG_W
    plan = subprocess.run([os.path.join(PKG, "bin", "sa_trace_plan_check"), "--mode", "fit", "--gap", "11", "--gap-extend", "2",
                           "--budget", str(BIG_BUDGET), "--band-at", f"{lo}:{hi}", f"{BIG_N}x{BIG_M}"], capture_output=True, text=True, check=True)
    plan = json.loads(plan.stdout)
    assert child["arena_bytes"] == plan["arena_bytes"] == plan["pairs"][0]["dir_bytes"] < BIG_BUDGET
    assert child["num_chunks"] == 1
    t, p = big_pair()
    tc, (l2, h2) = crop(t, p, lo, hi)
    want = band_at_ref(FIT, tc, p, matrix("blast", 4), 11, 2, l2, h2)
    want["start_text"] += lo
    want["end_text"] += lo
    assert want["inside"] and child["result"] == pick(want)
    assert child["score"] == [want["score"], want["end_pattern"], want["end_text"]]


# ---- 10. the C++ functions --------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["global", "local", "fit", "overlap"])
def test_cpp_band_at_check(mode):
    out = subprocess.run([os.path.join(PKG, "bin", "sa_band_at_check"), mode, "700", "96"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1] == "OK 96"


if __name__ == "__main__" and sys.argv[1:] == ["big"]:
    # the child of test_a_fit_pair_beyond_the_arena_budget_aligns_inside_its_band
    from sa_amd import engine
    S_ = matrix("blast", 4)
    t_, p_ = big_pair()
    try:
        engine.align_pairs_affine(FIT, [t_], [p_], S_, 11, 2)
        code = 0
    except engine.SaError as err:
        code = err.code
    b_ = [(BIG_C - BIG_W, BIG_C + BIG_W)]
    res_ = engine.align_pairs_affine(FIT, [t_], [p_], S_, 11, 2, bands=b_)[0]
    stats_ = engine.affine_last_stats()
    sc_ = engine.score_batch(FIT, [t_], [p_], S_, 11, gap_extend=2, bands=b_)[0]
    print(json.dumps({"unbanded_error": code, "result": pick(res_), "arena_bytes": stats_["arena_bytes"],
                      "num_chunks": stats_["num_chunks"], "score": [int(sc_["score"]), int(sc_["end_pattern"]), int(sc_["end_text"])]}))
