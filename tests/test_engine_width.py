"""CPU: which C function, with which scalar arguments, score_batch, Scorer and align_pairs_affine call when
width= is given beside every combination of gap_extend=, band=, bands=, xdrop= and seeds=, and which
combinations they refuse with which ValueError. The C entry points are replaced by recorders, as in
test_engine_variant.py, so nothing runs on a device. The table is written out by hand from the rule of the
interface: width= is the band of an extension, so it goes with xdrop= (and seeds=) only; a call that was
refused without width= is refused by the same words with it; width= with band= or bands= and width= without
xdrop= have messages of their own. Without width= every call is what test_engine_variant.py records."""
from __future__ import annotations

import ctypes
import itertools

import numpy as np
import pytest

from sa_amd import engine

GAP, GAP_EXTEND, BAND, XDROP, WIDTH = 5, 2, 3, 7, 9
BANDS = [(-1, 1), (-2, 2)]
SEEDS = [(1, 1, 2), (0, 2, 1)]
TEXTS = [np.array([0, 1, 2, 3], np.int8), np.array([3, 2, 1, 0], np.int8)]
PATTERNS = [np.array([0, 1, 1, 3], np.int8), np.array([3, 2, 2, 0], np.int8)]
PAIRS = [(0, 4, 0, 4), (4, 4, 4, 4)]
S = np.where(np.eye(4, dtype=bool), 2, -1).astype(np.int32)

E_BOTH = "band= and bands= exclude each other"
E_XBAND = "xdrop= takes no band: extension alignment inside a band is not built"
E_SBAND = "seeds= takes no band: seed extension inside a band is not built"
E_SNOX = "seeds= requires xdrop= (NO_XDROP for none)"
E_WBAND = "width= takes neither band= nor bands=: it is the band of an extension (xdrop=), about its anchor's diagonal"
E_WNOX = "width= requires xdrop= (NO_XDROP for none)"

# (gap_extend, band, bands, xdrop, seeds) present, width= always -> the ValueError, or (suffix, scalars after
# params). The three functions agree: align_pairs_affine resolves the variant before it looks for a gap model.
WITH_WIDTH = {
    (0, 0, 0, 0, 0): E_WNOX,
    (0, 0, 0, 0, 1): E_SNOX,
    (0, 0, 0, 1, 0): ("_extend_band", (5, 5, 7, 9)),
    (0, 0, 0, 1, 1): ("_seeds_band", (5, 5, 7, 9)),
    (0, 0, 1, 0, 0): E_WBAND,
    (0, 0, 1, 0, 1): E_SBAND,
    (0, 0, 1, 1, 0): E_XBAND,
    (0, 0, 1, 1, 1): E_XBAND,
    (0, 1, 0, 0, 0): E_WBAND,
    (0, 1, 0, 0, 1): E_SBAND,
    (0, 1, 0, 1, 0): E_XBAND,
    (0, 1, 0, 1, 1): E_XBAND,
    (0, 1, 1, 0, 0): E_BOTH,
    (0, 1, 1, 0, 1): E_BOTH,
    (0, 1, 1, 1, 0): E_BOTH,
    (0, 1, 1, 1, 1): E_BOTH,
    (1, 0, 0, 0, 0): E_WNOX,
    (1, 0, 0, 0, 1): E_SNOX,
    (1, 0, 0, 1, 0): ("_extend_band", (5, 2, 7, 9)),
    (1, 0, 0, 1, 1): ("_seeds_band", (5, 2, 7, 9)),
    (1, 0, 1, 0, 0): E_WBAND,
    (1, 0, 1, 0, 1): E_SBAND,
    (1, 0, 1, 1, 0): E_XBAND,
    (1, 0, 1, 1, 1): E_XBAND,
    (1, 1, 0, 0, 0): E_WBAND,
    (1, 1, 0, 0, 1): E_SBAND,
    (1, 1, 0, 1, 0): E_XBAND,
    (1, 1, 0, 1, 1): E_XBAND,
    (1, 1, 1, 0, 0): E_BOTH,
    (1, 1, 1, 0, 1): E_BOTH,
    (1, 1, 1, 1, 0): E_BOTH,
    (1, 1, 1, 1, 1): E_BOTH,
}
SUFFIXES = ("", "_affine", "_banded", "_band_at", "_extend", "_seeds", "_extend_band", "_seeds_band")


@pytest.fixture
def calls(monkeypatch):
    """Every entry point a variant can reach records (name, arguments) and reports success. The caller's seeds
    are read behind their pointer while the call lasts, and take the pointer's place."""
    made = []

    def recorder(name):
        def record(*a):
            a = list(a)
            if name.endswith("_seeds"):
                a[4] = list((ctypes.c_uint64 * 6).from_address(a[4]))
            if name.endswith("_seeds_band"):
                a[5] = list((ctypes.c_uint64 * 6).from_address(a[5]))
            made.append((name, a))
            return 0
        return record

    names = ["sa_score_batch" + s for s in SUFFIXES] + ["sa_scorer_create" + s for s in SUFFIXES]
    names += ["sa_align_pairs" + s for s in SUFFIXES[1:]] + ["sa_align_batch"]
    for name in names:
        monkeypatch.setattr(engine.lib, name, recorder(name))
    return made


def _keywords(key, width, with_gap_extend=True):
    ge, band, bands, xdrop, seeds = key
    kw = {"band": BAND if band else None, "bands": BANDS if bands else None, "xdrop": XDROP if xdrop else None,
          "seeds": SEEDS if seeds else None, "width": width}
    if with_gap_extend:
        kw["gap_extend"] = GAP_EXTEND if ge else None
    return kw


def _check_call(made, prefix, expected, pairs_at):
    suffix, scalars = expected
    assert len(made) == 1, made
    name, a = made[0]
    assert name == prefix + suffix
    k = 1 + len(scalars)
    assert tuple(a[1:k]) == scalars
    if suffix == "_seeds_band":
        assert a[k] == [1, 1, 2, 0, 2, 1]
        k += 1
    assert k == pairs_at(a)
    assert tuple(a[k + 1:k + 3]) == (2, 0)  # two pairs, device 0


def test_the_new_entry_points_are_exported():
    for name in ("sa_score_batch_extend_band", "sa_scorer_create_extend_band", "sa_align_pairs_extend_band",
                 "sa_score_batch_seeds_band", "sa_scorer_create_seeds_band", "sa_align_pairs_seeds_band"):
        assert name in engine.EXPORTS and hasattr(engine.lib, name)


@pytest.mark.parametrize("key", list(itertools.product((0, 1), repeat=5)))
def test_variant_of_every_keyword_combination_with_width(calls, key):
    want = WITH_WIDTH[key]
    kw = _keywords(key, WIDTH)
    align = lambda: engine.align_pairs_affine(engine.SA_GLOBAL, TEXTS, PATTERNS, S, GAP, GAP_EXTEND if key[0] else None,  # noqa: E731
                                              **_keywords(key, WIDTH, with_gap_extend=False))
    for prefix, call, tail in (("sa_score_batch", lambda: engine.score_batch(engine.SA_GLOBAL, TEXTS, PATTERNS, S, GAP, **kw), 4),
                               ("sa_scorer_create", lambda: engine.Scorer(engine.SA_GLOBAL, S, GAP, PAIRS, **kw), 4),
                               ("sa_align_pairs", align, 6)):
        del calls[:]
        if isinstance(want, str):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == want
            assert not calls
        else:
            out = call()
            _check_call(calls, prefix, want, lambda a: len(a) - tail)  # params, ..., pairs, np, device, then 1 or 3 outputs
            if prefix == "sa_score_batch":
                assert out.dtype == (engine.SEED_DTYPE if key[4] else engine.SCORE_DTYPE)
            if prefix == "sa_scorer_create":
                assert out.seeded is bool(key[4])


@pytest.mark.parametrize("key", list(itertools.product((0, 1), repeat=5)))
def test_width_none_is_the_call_without_the_keyword(calls, key):
    """width=None reaches what the call without the keyword reaches: the same function, the same arguments, or
    the same ValueError."""
    def run(call):
        del calls[:]
        try:
            call()
        except ValueError as e:
            return str(e)
        return [(n, [x for x in a if isinstance(x, (int, list))]) for n, a in calls]

    with_none, without = _keywords(key, None), _keywords(key, None)
    del without["width"]
    for make in (lambda kw: (lambda: engine.score_batch(engine.SA_GLOBAL, TEXTS, PATTERNS, S, GAP, **kw)),
                 lambda kw: (lambda: engine.Scorer(engine.SA_GLOBAL, S, GAP, PAIRS, **kw))):
        a, b = run(make(with_none)), run(make(without))
        assert type(a) is type(b)
        if isinstance(a, str):
            assert a == b
        else:
            assert [n for n, _ in a] == [n for n, _ in b] and len(a) == 1
            assert [x for x in a[0][1] if not isinstance(x, int) or abs(x) < 1 << 20] == [x for x in b[0][1] if not isinstance(x, int) or abs(x) < 1 << 20]


def test_a_width_of_zero_is_a_width(calls):
    engine.score_batch(engine.SA_GLOBAL, TEXTS, PATTERNS, S, GAP, xdrop=engine.NO_XDROP, width=0)
    assert calls[0][0] == "sa_score_batch_extend_band" and tuple(calls[0][1][1:5]) == (5, 5, -1, 0)
