"""CPU: which C function, with which scalar arguments, score_batch, Scorer and align_pairs_affine call for
every combination of gap_extend=, band=, bands=, xdrop= and seeds=, and which combinations they refuse with
which ValueError. The C entry points are replaced by recorders, so nothing runs on a device; loading the
library is enough. The table below is written out from the six-way ladders these three functions had before
they shared one resolver: it is the record of what they chose, not a product of the code under test."""
from __future__ import annotations

import ctypes
import itertools

import numpy as np
import pytest

from sa_amd import engine

GAP, GAP_EXTEND, BAND, XDROP = 5, 2, 3, 7
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

# (gap_extend, band, bands, xdrop, seeds) present -> the ValueError, or (suffix, scalars after params).
# score_batch and Scorer: without gap_extend the gap is linear, gap_open = gap_extend = GAP.
SCORE = {
    (0, 0, 0, 0, 0): ("", ()),
    (0, 0, 0, 0, 1): E_SNOX,
    (0, 0, 0, 1, 0): ("_extend", (5, 5, 7)),
    (0, 0, 0, 1, 1): ("_seeds", (5, 5, 7)),
    (0, 0, 1, 0, 0): ("_band_at", (5, 5)),
    (0, 0, 1, 0, 1): E_SBAND,
    (0, 0, 1, 1, 0): E_XBAND,
    (0, 0, 1, 1, 1): E_XBAND,
    (0, 1, 0, 0, 0): ("_banded", (5, 5, 3)),
    (0, 1, 0, 0, 1): E_SBAND,
    (0, 1, 0, 1, 0): E_XBAND,
    (0, 1, 0, 1, 1): E_XBAND,
    (0, 1, 1, 0, 0): E_BOTH,
    (0, 1, 1, 0, 1): E_BOTH,
    (0, 1, 1, 1, 0): E_BOTH,
    (0, 1, 1, 1, 1): E_BOTH,
    (1, 0, 0, 0, 0): ("_affine", (5, 2)),
    (1, 0, 0, 0, 1): E_SNOX,
    (1, 0, 0, 1, 0): ("_extend", (5, 2, 7)),
    (1, 0, 0, 1, 1): ("_seeds", (5, 2, 7)),
    (1, 0, 1, 0, 0): ("_band_at", (5, 2)),
    (1, 0, 1, 0, 1): E_SBAND,
    (1, 0, 1, 1, 0): E_XBAND,
    (1, 0, 1, 1, 1): E_XBAND,
    (1, 1, 0, 0, 0): ("_banded", (5, 2, 3)),
    (1, 1, 0, 0, 1): E_SBAND,
    (1, 1, 0, 1, 0): E_XBAND,
    (1, 1, 0, 1, 1): E_XBAND,
    (1, 1, 1, 0, 0): E_BOTH,
    (1, 1, 1, 0, 1): E_BOTH,
    (1, 1, 1, 1, 0): E_BOTH,
    (1, 1, 1, 1, 1): E_BOTH,
}
# align_pairs_affine: the same refusals. With gap_extend the same functions, sa_align_pairs_affine for the plain
# one. With gap_extend=None the ladder asked for seeds and xdrop first and went to sa_align_batch (one device)
# for everything else, a band included; None here is "sa_align_batch, no scalar".
ALIGN = {k: v for k, v in SCORE.items() if k[0] == 1}
ALIGN.update({
    (0, 0, 0, 0, 0): None,
    (0, 0, 0, 0, 1): E_SNOX,
    (0, 0, 0, 1, 0): ("_extend", (5, 5, 7)),
    (0, 0, 0, 1, 1): ("_seeds", (5, 5, 7)),
    (0, 0, 1, 0, 0): None,
    (0, 0, 1, 0, 1): E_SBAND,
    (0, 0, 1, 1, 0): E_XBAND,
    (0, 0, 1, 1, 1): E_XBAND,
    (0, 1, 0, 0, 0): None,
    (0, 1, 0, 0, 1): E_SBAND,
    (0, 1, 0, 1, 0): E_XBAND,
    (0, 1, 0, 1, 1): E_XBAND,
    (0, 1, 1, 0, 0): E_BOTH,
    (0, 1, 1, 0, 1): E_BOTH,
    (0, 1, 1, 1, 0): E_BOTH,
    (0, 1, 1, 1, 1): E_BOTH,
})
SUFFIXES = ("", "_affine", "_banded", "_band_at", "_extend", "_seeds")


@pytest.fixture
def calls(monkeypatch):
    """Every entry point a variant can reach records (name, arguments) and reports success. The caller's bands
    or seeds are read behind their pointer while the call lasts, and take the pointer's place."""
    made = []

    def recorder(name):
        def record(*a):
            a = list(a)
            if name.endswith("_band_at"):
                a[3] = list((ctypes.c_int32 * 4).from_address(a[3]))
            if name.endswith("_seeds"):
                a[4] = list((ctypes.c_uint64 * 6).from_address(a[4]))
            made.append((name, a))
            return 0
        return record

    names = ["sa_score_batch" + s for s in SUFFIXES] + ["sa_scorer_create" + s for s in SUFFIXES]
    names += ["sa_align_pairs" + s for s in SUFFIXES[1:]] + ["sa_align_batch"]
    for name in names:
        monkeypatch.setattr(engine.lib, name, recorder(name))
    return made


def _keywords(key, with_gap_extend=True):
    ge, band, bands, xdrop, seeds = key
    kw = {"band": BAND if band else None, "bands": BANDS if bands else None, "xdrop": XDROP if xdrop else None,
          "seeds": SEEDS if seeds else None}
    if with_gap_extend:
        kw["gap_extend"] = GAP_EXTEND if ge else None
    return kw


def _check_call(made, prefix, expected, pairs_at):
    """One call, of prefix + suffix, the scalars after params and, for bands and seeds, the caller's values
    after them; then the pairs, their number and the device."""
    suffix, scalars = expected
    assert len(made) == 1, made
    name, a = made[0]
    assert name == prefix + suffix
    k = 1 + len(scalars)
    assert tuple(a[1:k]) == scalars
    if suffix == "_band_at":
        assert a[k] == [-1, 1, -2, 2]
        k += 1
    if suffix == "_seeds":
        assert a[k] == [1, 1, 2, 0, 2, 1]
        k += 1
    assert k == pairs_at(a)
    assert tuple(a[k + 1:k + 3]) == (2, 0)  # two pairs, device 0


@pytest.mark.parametrize("key", list(itertools.product((0, 1), repeat=5)))
def test_variant_of_every_keyword_combination(calls, key):
    want = SCORE[key]
    kw = _keywords(key)
    for prefix, call, nargs in (("sa_score_batch", lambda: engine.score_batch(engine.SA_GLOBAL, TEXTS, PATTERNS, S, GAP, **kw), 5),
                                ("sa_scorer_create", lambda: engine.Scorer(engine.SA_GLOBAL, S, GAP, PAIRS, **kw), 5)):
        del calls[:]
        if isinstance(want, str):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == want
            assert not calls
        else:
            call()
            _check_call(calls, prefix, want, lambda a: len(a) - (nargs - 1))  # params, ..., pairs, np, device, out

    want = ALIGN[key]
    del calls[:]
    align = lambda: engine.align_pairs_affine(engine.SA_GLOBAL, TEXTS, PATTERNS, S, GAP, GAP_EXTEND if key[0] else None,  # noqa: E731
                                              **_keywords(key, with_gap_extend=False))
    if isinstance(want, str):
        with pytest.raises(ValueError) as e:
            align()
        assert str(e.value) == want
        assert not calls
    elif want is None:
        align()
        assert [n for n, _ in calls] == ["sa_align_batch"]
        assert tuple(calls[0][1][2:4]) == (2, 1) and len(calls[0][1]) == 7  # two pairs, one device
    else:
        align()
        _check_call(calls, "sa_align_pairs", want, lambda a: len(a) - 6)  # params, ..., pairs, np, device, res, at, ap


def test_align_batch_has_no_gap_model(calls):
    engine.align_batch(engine.SA_GLOBAL, TEXTS, PATTERNS, S, GAP, num_gpus=3)
    assert [n for n, _ in calls] == ["sa_align_batch"]
    assert tuple(calls[0][1][2:4]) == (2, 3)
