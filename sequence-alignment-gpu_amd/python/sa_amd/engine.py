"""ctypes binding of the C ABI in include/sa_hip.h (libsa_hip.so).

The product path: every call goes to the HIP engine. If the shared library is missing this
module raises at import time — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

PKG_ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
LIB_PATH = os.environ.get("SA_HIP_LIB", os.path.join(PKG_ROOT, "lib", "libsa_hip.so"))

SA_GLOBAL, SA_LOCAL = 0, 1
# sa_mode SA_FIT (semi-global): the whole pattern inside the text, the text free at both ends. Taken by
# score_batch, Scorer, align_pairs_affine and search; Plan, align_pair and align_batch answer
# SA_ERR_UNSUPPORTED.
FIT = SA_FIT = 2
# sa_mode SA_ENDS_FREE: global alignment with free sequence ends, mode = ENDS_FREE | flags (16..31).
# Taken and refused by the same functions as FIT; the banded functions (band=) refuse it too.
ENDS_FREE = 16
FREE_TEXT_BEGIN, FREE_TEXT_END, FREE_PATTERN_BEGIN, FREE_PATTERN_END = 1, 2, 4, 8
OVERLAP = ENDS_FREE | 15
# xdrop= of score_batch, Scorer and align_pairs_affine (sa_hip.h SA_NO_XDROP): extension alignment that
# never stops early
NO_XDROP = -1
STATUS = {0: "SA_OK", 1: "SA_ERR_INVALID", 2: "SA_ERR_NOMEM", 3: "SA_ERR_HIP", 4: "SA_ERR_UNSUPPORTED",
          5: "SA_ERR_TIMEOUT"}

# sa_plan_fill_kind (include/sa_hip.h SA_FILL_*)
FILL_KINDS = {0: "strips", 1: "band", 2: "pair", 3: "pair_chain", 4: "band3"}

# Symbols declared in include/sa_hip.h (checked by tests/test_capi.py).
EXPORTS = ("sa_align_pair", "sa_plan_create", "sa_plan_destroy", "sa_plan_fill", "sa_plan_traceback",
           "sa_plan_fetch_results", "sa_plan_fetch_alignment", "sa_plan_info", "sa_plan_device_results", "sa_plan_copy_results",
           "sa_device_count", "sa_last_error", "sa_abi_version", "sa_selftest", "sa_plan_fetch_directions", "sa_release_workspace",
           "sa_plan_output_bytes", "sa_plan_fetch_all", "sa_align_batch", "sa_batch_deal", "sa_build_id",
           "sa_batch_last_stats", "sa_plan_fill_kind", "sa_score_batch", "sa_scorer_create", "sa_scorer_run",
           "sa_scorer_fetch", "sa_scorer_info", "sa_scorer_destroy", "sa_search", "sa_score_batch_affine",
           "sa_scorer_create_affine", "sa_align_pairs_affine", "sa_search_affine", "sa_affine_last_stats",
           "sa_score_batch_banded", "sa_scorer_create_banded", "sa_align_pairs_banded",
           "sa_score_batch_band_at", "sa_scorer_create_band_at", "sa_align_pairs_band_at", "sa_band_reachable",
           "sa_score_batch_extend", "sa_scorer_create_extend", "sa_align_pairs_extend",
           "sa_score_batch_seeds", "sa_scorer_create_seeds", "sa_scorer_fetch_seeds", "sa_align_pairs_seeds",
           "sa_score_batch_extend_band", "sa_scorer_create_extend_band", "sa_align_pairs_extend_band",
           "sa_score_batch_seeds_band", "sa_scorer_create_seeds_band", "sa_align_pairs_seeds_band",
           "sa_score_batch_chains", "sa_scorer_create_chains", "sa_align_pairs_chains",
           "sa_align_pairs_cigar", "sa_cigars_ops", "sa_cigars_num_ops", "sa_cigars_destroy", "sa_cigar_from_strings",
           "sa_cigar_format", "sa_cigar_last_stats",
           "sa_chain_anchors", "sa_chain_anchors_host", "sa_chain_set_seeds", "sa_chain_set_off", "sa_chain_set_destroy",
           "sa_chain_last_stats")
# flags of align_pairs_cigar and cigar_from_strings (sa_hip.h sa_cigar_flags) and the BAM op codes
CIGAR_M, CIGAR_EQX = 0, 1
CIGAR_OPS = {0: "M", 1: "I", 2: "D", 7: "=", 8: "X"}


class SaParams(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int32), ("alphabet_size", ctypes.c_int32), ("gap_penalty", ctypes.c_int32),
                ("rows_per_lane", ctypes.c_int32), ("score_matrix", ctypes.c_void_p), ("alphabet", ctypes.c_char_p)]


class SaPair(ctypes.Structure):
    _fields_ = [("text_offset", ctypes.c_uint64), ("text_len", ctypes.c_uint64),
                ("pattern_offset", ctypes.c_uint64), ("pattern_len", ctypes.c_uint64)]


class SaResult(ctypes.Structure):
    _fields_ = [("score", ctypes.c_int32), ("status", ctypes.c_int32), ("num_alignment_bytes", ctypes.c_uint64),
                ("start_text", ctypes.c_uint64), ("start_pattern", ctypes.c_uint64)]


class SaScoreResult(ctypes.Structure):
    _fields_ = [("score", ctypes.c_int32), ("status", ctypes.c_int32), ("end_text", ctypes.c_uint64),
                ("end_pattern", ctypes.c_uint64)]


class SaBand(ctypes.Structure):
    _fields_ = [("lo", ctypes.c_int32), ("hi", ctypes.c_int32)]


class SaAlignSpec(ctypes.Structure):
    _fields_ = [("gap_open", ctypes.c_int32), ("gap_extend", ctypes.c_int32), ("band", ctypes.c_int32),
                ("xdrop", ctypes.c_int32), ("width", ctypes.c_int32), ("extend", ctypes.c_int32),
                ("bands", ctypes.c_void_p), ("seeds", ctypes.c_void_p), ("chain_off", ctypes.c_void_p)]


class SaCigarResult(ctypes.Structure):
    _fields_ = [("score", ctypes.c_int32), ("status", ctypes.c_int32), ("num_alignment_bytes", ctypes.c_uint64),
                ("start_text", ctypes.c_uint64), ("start_pattern", ctypes.c_uint64), ("ops_off", ctypes.c_uint64),
                ("num_ops", ctypes.c_uint32), ("matches", ctypes.c_uint32), ("mismatches", ctypes.c_uint32),
                ("text_gap_letters", ctypes.c_uint32), ("pattern_gap_letters", ctypes.c_uint32),
                ("gap_opens", ctypes.c_uint32)]


# max_gap= and max_diag= of chain_anchors (sa_hip.h SA_CHAIN_NO_LIMIT)
NO_LIMIT = 2 ** 31 - 1


class SaChainParams(ctypes.Structure):
    _fields_ = [("match", ctypes.c_int32), ("gap_open", ctypes.c_int32), ("gap_extend", ctypes.c_int32), ("skip", ctypes.c_int32),
                ("max_gap", ctypes.c_int32), ("max_diag", ctypes.c_int32), ("lookback", ctypes.c_int32)]


class SaChainResult(ctypes.Structure):
    _fields_ = [("score", ctypes.c_int32), ("status", ctypes.c_int32), ("seeds_off", ctypes.c_uint64),
                ("num_seeds", ctypes.c_uint32), ("last_anchor", ctypes.c_uint32)]


class SaError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{STATUS.get(code, code)}: {msg}")
        self.code = code


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"HIP engine not built: {LIB_PATH} is missing (run __graft_entry__.build())")
    # One HIP runtime per process: torch ships its own libamdhip64 (soname libamdhip64.so.7, but its
    # libraries NEED "libamdhip64.so"). Loaded first, torch's runtime also satisfies our NEEDED
    # libamdhip64.so.7; loaded after us it would start a second runtime that sees no GPU.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    P, I, U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    L.sa_align_pair.argtypes = [ctypes.POINTER(SaParams), P, U64, P, U64, I, ctypes.POINTER(SaResult), P, P, U64,
                                ctypes.POINTER(ctypes.c_double)]
    L.sa_plan_create.argtypes = [ctypes.POINTER(SaParams), ctypes.POINTER(SaPair), ctypes.c_int64, I,
                                 ctypes.POINTER(P)]
    L.sa_plan_destroy.argtypes = [P]
    L.sa_plan_fill.argtypes = [P, P, P, P]
    L.sa_plan_traceback.argtypes = [P, P]
    L.sa_plan_fetch_results.argtypes = [P, P, P]
    L.sa_plan_fetch_alignment.argtypes = [P, ctypes.c_int64, P, P, U64, P]
    L.sa_plan_info.argtypes = [P, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32),
                               ctypes.POINTER(U64), ctypes.POINTER(U64)]
    L.sa_plan_fetch_directions.argtypes = [P, ctypes.c_int64, P, P]
    L.sa_plan_fill_kind.argtypes = [P]
    L.sa_plan_fill_kind.restype = I
    L.sa_plan_device_results.argtypes = [P]
    L.sa_plan_device_results.restype = P
    L.sa_plan_copy_results.argtypes = [P, P, P]
    L.sa_plan_copy_results.restype = I
    L.sa_device_count.argtypes = [ctypes.POINTER(I)]
    L.sa_last_error.restype = ctypes.c_char_p
    L.sa_selftest.argtypes = [I]
    L.sa_release_workspace.argtypes = [I]
    L.sa_plan_output_bytes.argtypes = [P]
    L.sa_plan_output_bytes.restype = U64
    L.sa_plan_fetch_all.argtypes = [P, ctypes.POINTER(SaResult), P, P, U64, P, P]
    L.sa_align_batch.argtypes = [ctypes.POINTER(SaParams), P, ctypes.c_int64, I, ctypes.POINTER(SaResult), P, P]
    L.sa_batch_deal.argtypes = [P, ctypes.c_int64, I, P]
    L.sa_build_id.restype = ctypes.c_char_p
    L.sa_batch_last_stats.argtypes = [ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), P,
                                      ctypes.c_int32, ctypes.POINTER(ctypes.c_double)]
    L.sa_score_batch.argtypes = [ctypes.POINTER(SaParams), P, ctypes.c_int64, I, P]
    L.sa_scorer_create.argtypes = [ctypes.POINTER(SaParams), ctypes.POINTER(SaPair), ctypes.c_int64, I,
                                   ctypes.POINTER(P)]
    L.sa_score_batch_affine.argtypes = [ctypes.POINTER(SaParams), ctypes.c_int32, ctypes.c_int32, P, ctypes.c_int64, I, P]
    L.sa_scorer_create_affine.argtypes = [ctypes.POINTER(SaParams), ctypes.c_int32, ctypes.c_int32,
                                          ctypes.POINTER(SaPair), ctypes.c_int64, I, ctypes.POINTER(P)]
    L.sa_scorer_run.argtypes = [P, P, P, P]
    L.sa_scorer_fetch.argtypes = [P, P, P]
    L.sa_scorer_info.argtypes = [P, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(U64)]
    L.sa_scorer_destroy.argtypes = [P]
    L.sa_search.argtypes = [ctypes.POINTER(SaParams), P, U64, P, P, ctypes.c_int64, I, I, P, P, P, P, P,
                            ctypes.POINTER(ctypes.c_int64)]
    L.sa_align_pairs_affine.argtypes = [ctypes.POINTER(SaParams), ctypes.c_int32, ctypes.c_int32, P, ctypes.c_int64, I,
                                        ctypes.POINTER(SaResult), P, P]
    L.sa_search_affine.argtypes = [ctypes.POINTER(SaParams), ctypes.c_int32, ctypes.c_int32, P, U64, P, P, ctypes.c_int64,
                                   I, I, P, P, P, P, P, ctypes.POINTER(ctypes.c_int64)]
    I32 = ctypes.c_int32
    L.sa_score_batch_banded.argtypes = [ctypes.POINTER(SaParams), I32, I32, I32, P, ctypes.c_int64, I, P]
    L.sa_scorer_create_banded.argtypes = [ctypes.POINTER(SaParams), I32, I32, I32, ctypes.POINTER(SaPair), ctypes.c_int64, I,
                                          ctypes.POINTER(P)]
    L.sa_align_pairs_banded.argtypes = [ctypes.POINTER(SaParams), I32, I32, I32, P, ctypes.c_int64, I,
                                        ctypes.POINTER(SaResult), P, P]
    L.sa_score_batch_band_at.argtypes = [ctypes.POINTER(SaParams), I32, I32, P, P, ctypes.c_int64, I, P]
    L.sa_scorer_create_band_at.argtypes = [ctypes.POINTER(SaParams), I32, I32, P, ctypes.POINTER(SaPair), ctypes.c_int64, I,
                                           ctypes.POINTER(P)]
    L.sa_align_pairs_band_at.argtypes = [ctypes.POINTER(SaParams), I32, I32, P, P, ctypes.c_int64, I,
                                         ctypes.POINTER(SaResult), P, P]
    L.sa_score_batch_extend.argtypes = [ctypes.POINTER(SaParams), I32, I32, I32, P, ctypes.c_int64, I, P]
    L.sa_scorer_create_extend.argtypes = [ctypes.POINTER(SaParams), I32, I32, I32, ctypes.POINTER(SaPair), ctypes.c_int64, I,
                                          ctypes.POINTER(P)]
    L.sa_align_pairs_extend.argtypes = [ctypes.POINTER(SaParams), I32, I32, I32, P, ctypes.c_int64, I,
                                        ctypes.POINTER(SaResult), P, P]
    L.sa_score_batch_seeds.argtypes = [ctypes.POINTER(SaParams), I32, I32, I32, P, P, ctypes.c_int64, I, P]
    L.sa_scorer_create_seeds.argtypes = [ctypes.POINTER(SaParams), I32, I32, I32, P, ctypes.POINTER(SaPair), ctypes.c_int64, I,
                                         ctypes.POINTER(P)]
    L.sa_scorer_fetch_seeds.argtypes = [P, P, P]
    L.sa_align_pairs_seeds.argtypes = [ctypes.POINTER(SaParams), I32, I32, I32, P, P, ctypes.c_int64, I,
                                       ctypes.POINTER(SaResult), P, P]
    L.sa_score_batch_extend_band.argtypes = [ctypes.POINTER(SaParams), I32, I32, I32, I32, P, ctypes.c_int64, I, P]
    L.sa_scorer_create_extend_band.argtypes = [ctypes.POINTER(SaParams), I32, I32, I32, I32, ctypes.POINTER(SaPair), ctypes.c_int64, I,
                                               ctypes.POINTER(P)]
    L.sa_align_pairs_extend_band.argtypes = [ctypes.POINTER(SaParams), I32, I32, I32, I32, P, ctypes.c_int64, I,
                                             ctypes.POINTER(SaResult), P, P]
    L.sa_score_batch_seeds_band.argtypes = [ctypes.POINTER(SaParams), I32, I32, I32, I32, P, P, ctypes.c_int64, I, P]
    L.sa_scorer_create_seeds_band.argtypes = [ctypes.POINTER(SaParams), I32, I32, I32, I32, P, ctypes.POINTER(SaPair), ctypes.c_int64, I,
                                              ctypes.POINTER(P)]
    L.sa_align_pairs_seeds_band.argtypes = [ctypes.POINTER(SaParams), I32, I32, I32, I32, P, P, ctypes.c_int64, I,
                                            ctypes.POINTER(SaResult), P, P]
    L.sa_score_batch_chains.argtypes = [ctypes.POINTER(SaParams), I32, I32, I32, P, P, P, ctypes.c_int64, I, P]
    L.sa_scorer_create_chains.argtypes = [ctypes.POINTER(SaParams), I32, I32, I32, P, P, ctypes.POINTER(SaPair), ctypes.c_int64, I,
                                          ctypes.POINTER(P)]
    L.sa_align_pairs_chains.argtypes = [ctypes.POINTER(SaParams), I32, I32, I32, P, P, P, ctypes.c_int64, I,
                                        ctypes.POINTER(SaResult), P, P]
    L.sa_align_pairs_cigar.argtypes = [ctypes.POINTER(SaParams), ctypes.POINTER(SaAlignSpec), I32, P, ctypes.c_int64, I,
                                       ctypes.POINTER(SaCigarResult), ctypes.POINTER(P)]
    L.sa_cigars_ops.argtypes = [P]
    L.sa_cigars_ops.restype = P
    L.sa_cigars_num_ops.argtypes = [P]
    L.sa_cigars_num_ops.restype = U64
    L.sa_cigars_destroy.argtypes = [P]
    L.sa_cigar_from_strings.argtypes = [ctypes.c_char_p, ctypes.c_char_p, U64, ctypes.c_char, I32, P, U64,
                                        ctypes.POINTER(SaCigarResult)]
    L.sa_cigar_format.argtypes = [P, U64, P, U64]
    L.sa_cigar_last_stats.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(U64), ctypes.POINTER(U64)]
    L.sa_chain_anchors.argtypes = [ctypes.POINTER(SaChainParams), P, P, ctypes.c_int64, I, P, ctypes.POINTER(P)]
    L.sa_chain_anchors_host.argtypes = [ctypes.POINTER(SaChainParams), P, P, ctypes.c_int64, P, ctypes.POINTER(P)]
    L.sa_chain_set_seeds.argtypes = [P]
    L.sa_chain_set_seeds.restype = P
    L.sa_chain_set_off.argtypes = [P]
    L.sa_chain_set_off.restype = P
    L.sa_chain_set_destroy.argtypes = [P]
    L.sa_chain_last_stats.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(U64)]
    L.sa_band_reachable.argtypes = [I32, U64, U64, SaBand]
    L.sa_band_reachable.restype = I
    L.sa_affine_last_stats.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                       ctypes.POINTER(U64), ctypes.POINTER(ctypes.c_int32)]
    for name in EXPORTS:
        getattr(L, name)
    check_build_id(L)
    return L


def check_build_id(L) -> None:
    """Refuse a library built from other sources than the ones next to it (buildid.py). SA_HIP_LIB
    (an explicitly chosen experiment build) and SA_ALLOW_STALE=1 skip the check."""
    from . import buildid
    if "SA_HIP_LIB" in os.environ or os.environ.get("SA_ALLOW_STALE") == "1":
        return
    built = L.sa_build_id().decode()
    want = buildid.source_hash()
    if built != want:
        raise ImportError(f"stale HIP engine: {LIB_PATH} was built from sources {built}, the tree holds {want} "
                          f"(rebuild: make -C {PKG_ROOT})")


lib = _load()


def _check(rc: int) -> None:
    if rc != 0:
        raise SaError(rc, lib.sa_last_error().decode(errors="replace"))


def _params(mode: int, S: np.ndarray, gap: int, alphabet: bytes | None, rows_per_lane: int):
    S = np.ascontiguousarray(S, dtype=np.int32).ravel()
    A = int(round(np.sqrt(S.size)))
    if A * A != S.size:
        raise ValueError("score matrix must be square")
    if alphabet is None:
        alphabet = b"ATCG-" if A == 4 else b"ARNDCQEGHILKMFPSTWYVBZX-"[: A] + b"-"
    p = SaParams(mode, A, gap, rows_per_lane, S.ctypes.data, alphabet)
    return p, S, alphabet


def ends_free(text_begin: bool = False, text_end: bool = False, pattern_begin: bool = False,
              pattern_end: bool = False) -> int:
    """The ends-free mode (sa_hip.h SA_ENDS_FREE) in which the named sequence ends cost nothing: all
    four is OVERLAP, the text's two is FIT, none is global alignment."""
    return (ENDS_FREE | (FREE_TEXT_BEGIN if text_begin else 0) | (FREE_TEXT_END if text_end else 0) |
            (FREE_PATTERN_BEGIN if pattern_begin else 0) | (FREE_PATTERN_END if pattern_end else 0))


def _bands(bands, num_pairs: int) -> np.ndarray:
    """`bands` as the (num_pairs, 2) int32 array of sa_band the band-at functions take."""
    b = np.ascontiguousarray(bands, dtype=np.int32).reshape(-1, 2)
    if len(b) != num_pairs:
        raise ValueError(f"bands holds {len(b)} (lo, hi) pairs for {num_pairs} pairs")
    return b


# numpy view of sa_seed_result (include/sa_hip.h): int32 score, int32 status, uint64 x 4
SEED_DTYPE = np.dtype([("score", "<i4"), ("status", "<i4"), ("begin_text", "<u8"), ("begin_pattern", "<u8"),
                       ("end_text", "<u8"), ("end_pattern", "<u8")])


def _seeds(seeds, num_pairs: int, xdrop, band, bands) -> np.ndarray:
    """`seeds` as the (num_pairs, 3) uint64 array of sa_seed the seeds functions take, after the checks the
    three callers share: seeds= requires xdrop= (NO_XDROP for none) and takes no band."""
    if band is not None or bands is not None:
        raise ValueError("seeds= takes no band: seed extension inside a band is not built")
    if xdrop is None:
        raise ValueError("seeds= requires xdrop= (NO_XDROP for none)")
    a = np.asarray(seeds, dtype=np.int64).reshape(-1, 3)
    if (a < 0).any():
        raise ValueError("seeds= holds a negative value")
    if len(a) != num_pairs:
        raise ValueError(f"seeds holds {len(a)} (text_pos, pattern_pos, length) triples for {num_pairs} pairs")
    return np.ascontiguousarray(a, dtype=np.uint64)


def _chains(chains, num_pairs: int, xdrop, seeds, band, bands, width):
    """`chains` (per pair, a list of (text_pos, pattern_pos, length) triples) as the flat (total, 3) uint64 array of
    sa_seed and the num_pairs + 1 uint64 chain_off the chains functions take, after the checks the three callers
    share: chains= excludes seeds=, band=, bands= and width=, and requires xdrop= (NO_XDROP for none)."""
    for name, other in (("seeds", seeds), ("band", band), ("bands", bands), ("width", width)):
        if other is not None:
            raise ValueError(f"chains= and {name}= exclude each other" + ("" if name == "seeds" else ": chained seeds inside a band are not built"))
    if xdrop is None:
        raise ValueError("chains= requires xdrop= (NO_XDROP for none)")
    if len(chains) != num_pairs:
        raise ValueError(f"chains holds {len(chains)} chains for {num_pairs} pairs")
    per = [np.asarray(c, dtype=np.int64).reshape(-1, 3) for c in chains]
    if any((c < 0).any() for c in per):
        raise ValueError("chains= holds a negative value")
    flat = np.ascontiguousarray(np.concatenate(per) if per else np.zeros((0, 3)), dtype=np.uint64)
    off = np.zeros(num_pairs + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in per], dtype=np.uint64)
    # one word more than the seeds: a call without any seed still passes an address, and the library names the pair
    return np.ascontiguousarray(np.concatenate([flat.ravel(), [0]]).astype(np.uint64)), off


def _variant(gap: int, gap_extend, band, bands, xdrop, seeds, num_pairs: int, width=None, chains=None):
    """The variant that the keywords of score_batch, Scorer and align_pairs_affine name, resolved once: the
    suffix of the C function (sa_score_batch<suffix>, sa_scorer_create<suffix>, sa_align_pairs<suffix>), the
    arguments that go between params and the pairs, and the array those point into, to keep alive over the
    call. Without `gap_extend` the gap is linear, gap_open = gap_extend = gap; with nothing else either, there
    is no gap model: the suffix is empty. `width` (an extension's or a seeds call's half-width about the anchor's
    diagonal) is checked after everything else, so a call that was refused before is refused by the same words.
    `chains` (chained seeds, a list of triples per pair) is checked first: it excludes every keyword but xdrop."""
    if chains is not None:
        flat, off = _chains(chains, num_pairs, xdrop, seeds, band, bands, width)
        ge = gap if gap_extend is None else gap_extend
        return "_chains", (gap, ge, xdrop, flat.ctypes.data, off.ctypes.data), (flat, off)
    if band is not None and bands is not None:
        raise ValueError("band= and bands= exclude each other")
    if xdrop is not None and (band is not None or bands is not None):
        raise ValueError("xdrop= takes no band: extension alignment inside a band is not built")
    ge = gap if gap_extend is None else gap_extend
    if seeds is not None:
        sd = _seeds(seeds, num_pairs, xdrop, band, bands)
        if width is not None:
            return "_seeds_band", (gap, ge, xdrop, width, sd.ctypes.data), sd
        return "_seeds", (gap, ge, xdrop, sd.ctypes.data), sd
    if width is not None:
        if band is not None or bands is not None:
            raise ValueError("width= takes neither band= nor bands=: it is the band of an extension (xdrop=), about its anchor's diagonal")
        if xdrop is None:
            raise ValueError("width= requires xdrop= (NO_XDROP for none)")
        return "_extend_band", (gap, ge, xdrop, width), None
    if xdrop is not None:
        return "_extend", (gap, ge, xdrop), None
    if bands is not None:
        b = _bands(bands, num_pairs)
        return "_band_at", (gap, ge, b.ctypes.data), b
    if band is not None:
        return "_banded", (gap, ge, band), None
    if gap_extend is not None:
        return "_affine", (gap, ge), None
    return _NO_GAP_MODEL


_NO_GAP_MODEL = ("", (), None)


def band_reachable(mode: int, n: int, m: int, lo: int, hi: int) -> bool:
    """sa_band_reachable (host only, no device call): whether a pair of n text and m pattern letters has
    an alignment of `mode` inside the band lo <= j - i <= hi. The band-at functions (bands=) refuse a
    call that holds a pair without one: filter with this first."""
    r = lib.sa_band_reachable(mode, n, m, SaBand(lo, hi))
    if r < 0:
        raise SaError(1, "sa_band_reachable: bad mode")
    return bool(r)


def selftest(device: int = 0) -> None:
    _check(lib.sa_selftest(device))


def align_pair(mode: int, text: np.ndarray, pattern: np.ndarray, S: np.ndarray, gap: int,
               alphabet: bytes | None = None, device: int = 0, rows_per_lane: int = 0) -> dict:
    """One pair from host memory through the HIP engine (synchronous)."""
    text = np.ascontiguousarray(text, dtype=np.int8)
    pattern = np.ascontiguousarray(pattern, dtype=np.int8)
    p, S_keep, alpha_keep = _params(mode, S, gap, alphabet, rows_per_lane)
    n, m = len(text), len(pattern)
    cap = max(1, n + m)
    at = ctypes.create_string_buffer(cap)
    ap = ctypes.create_string_buffer(cap)
    res = SaResult()
    fill_us = ctypes.c_double()
    _check(lib.sa_align_pair(ctypes.byref(p), text.ctypes.data, n, pattern.ctypes.data, m, device,
                             ctypes.byref(res), at, ap, cap, ctypes.byref(fill_us)))
    L = res.num_alignment_bytes
    return {"score": res.score, "num_bytes": L, "start_text": res.start_text, "start_pattern": res.start_pattern,
            "aligned_text": at.raw[:L].decode(), "aligned_pattern": ap.raw[:L].decode(), "fill_us": fill_us.value}


# numpy view of sa_result (include/sa_hip.h): int32 score, int32 status, uint64 x 3
RESULT_DTYPE = np.dtype([("score", "<i4"), ("status", "<i4"), ("num_bytes", "<u8"), ("start_text", "<u8"),
                         ("start_pattern", "<u8")])
assert RESULT_DTYPE.itemsize == ctypes.sizeof(SaResult)


class SaHostPair(ctypes.Structure):
    _fields_ = [("text", ctypes.c_void_p), ("text_len", ctypes.c_uint64), ("pattern", ctypes.c_void_p),
                ("pattern_len", ctypes.c_uint64)]


def _host_pairs(texts, patterns):
    """The pairs of a call from host memory: the sa_host_pair array, and the contiguous int8 arrays it points
    into, to keep alive over the call."""
    ts = [np.ascontiguousarray(t, dtype=np.int8) for t in texts]
    ps = [np.ascontiguousarray(x, dtype=np.int8) for x in patterns]
    hp = (SaHostPair * max(1, len(ts)))(*[SaHostPair(t.ctypes.data, len(t), x.ctypes.data, len(x)) for t, x in zip(ts, ps)])
    return hp, ts, ps


def _result_dict(r, text=None, pattern=None) -> dict:
    """An sa_result as the dict the aligners return; with the bytes that begin with the pair's aligned strings,
    those too."""
    L = r.num_alignment_bytes
    d = {"score": r.score, "num_bytes": L, "start_text": r.start_text, "start_pattern": r.start_pattern}
    if text is not None:
        d["aligned_text"] = bytes(text[:L]).decode()
        d["aligned_pattern"] = bytes(pattern[:L]).decode()
    return d


def batch_deal(cells: list[int], num_shards: int) -> list[int]:
    """sa_batch_deal: the pair -> shard assignment sa_align_batch uses (host only)."""
    c = np.ascontiguousarray(cells, dtype=np.uint64)
    out = np.zeros(max(1, len(c)), np.int32)
    _check(lib.sa_batch_deal(c.ctypes.data, len(c), num_shards, out.ctypes.data))
    return out[: len(c)].tolist()


def batch_last_stats() -> dict:
    """sa_batch_last_stats: the calling thread's last sa_align_batch (shards, RCCL or not, per-shard
    wall ms from upload to traceback end, gather wall ms)."""
    ns, rc = ctypes.c_int32(0), ctypes.c_int32(0)
    ms = np.zeros(64, np.float64)
    g = ctypes.c_double(0)
    _check(lib.sa_batch_last_stats(ctypes.byref(ns), ctypes.byref(rc), ms.ctypes.data, 64, ctypes.byref(g)))
    return {"num_shards": ns.value, "used_rccl": bool(rc.value), "shard_ms": ms[: ns.value].round(3).tolist(),
            "gather_ms": round(g.value, 3)}


def align_batch(mode: int, texts: list[np.ndarray], patterns: list[np.ndarray], S: np.ndarray, gap: int,
                num_gpus: int = 1, alphabet: bytes | None = None, strings: bool = True) -> list[dict]:
    """sa_align_batch: independent pairs from host memory over devices 0..num_gpus-1 (synchronous)."""
    return _align_host_pairs(mode, texts, patterns, S, gap, num_gpus, alphabet, strings, _NO_GAP_MODEL)


def align_pairs_affine(mode: int, texts: list[np.ndarray], patterns: list[np.ndarray], S: np.ndarray, gap_open: int,
                       gap_extend: int, device: int = 0, strings: bool = True, band: int | None = None,
                       bands=None, xdrop: int | None = None, seeds=None, width: int | None = None, chains=None) -> list[dict]:
    """sa_align_pairs_affine: independent pairs from host memory aligned on `device` under gap open /
    gap extend (synchronous). The keys are those of Plan.all_alignments; without strings, the scalar
    ones. With gap_open == gap_extend == g every value is align_pair's for gap g. `mode` may also be FIT
    or an ends-free mode (ends_free(), OVERLAP): start_text and start_pattern are then the 0-based
    indices of the first aligned letters. With `band` (SA_GLOBAL and SA_LOCAL only),
    sa_align_pairs_banded: the alignment inside the diagonal band of that half-width (sa_hip.h). With
    `bands` (an (np, 2) int32 array or a list of (lo, hi), one per pair; not with `band`),
    sa_align_pairs_band_at: pair k inside lo <= j - i <= hi of bands[k], in every mode. With `xdrop`
    (NO_XDROP or 0 .. 2**30 - 1; mode SA_GLOBAL, no band), sa_align_pairs_extend: extension alignment, from
    the origin to the best cell of the rows before the X-drop's stop row; both starts are 0. With `seeds`
    (one (text_pos, pattern_pos, length) per pair; requires `xdrop`, mode SA_GLOBAL, no band),
    sa_align_pairs_seeds: the extension to both sides of each pair's seed joined with the seed's letters;
    start_text and start_pattern are the 0-based indices of the first aligned letters. With `width` (>= 0;
    requires `xdrop`, takes neither `band` nor `bands`), sa_align_pairs_extend_band or, with `seeds`,
    sa_align_pairs_seeds_band: the same inside |j - i| <= width of each extension's own matrix, with direction
    bytes for the band only. With `chains` (per pair, a list of colinear (text_pos, pattern_pos, length) seeds;
    requires `xdrop`, excludes `seeds`, `band`, `bands` and `width`), sa_align_pairs_chains: the extension at the
    chain's two ends and the global alignment of every rectangle between two consecutive seeds, joined with the
    seeds' letters, with direction bytes for those pieces only."""
    variant = _variant(gap_open, gap_extend, band, bands, xdrop, seeds, len(texts), width, chains)
    if gap_extend is None and xdrop is None:  # as ever: without a gap model, align_batch on one device, band or no band
        return align_batch(mode, texts, patterns, S, gap_open, 1, None, strings)
    return _align_host_pairs(mode, texts, patterns, S, gap_open, device, None, strings, variant)


CIGAR_COUNTS = ("matches", "mismatches", "text_gap_letters", "pattern_gap_letters", "gap_opens")


def _align_spec(variant, gap_open: int) -> SaAlignSpec:
    """The sa_align_spec of a variant that _variant resolved: the arguments between params and the pairs of the
    sa_align_pairs<suffix> function, by name. Without a gap model (suffix "") the gap is linear."""
    suffix, args, _ = variant
    spec = SaAlignSpec(gap_open, gap_open, -1, NO_XDROP, -1, 0, None, None, None)
    names = {"": (), "_affine": ("gap_open", "gap_extend"), "_banded": ("gap_open", "gap_extend", "band"),
             "_band_at": ("gap_open", "gap_extend", "bands"), "_extend": ("gap_open", "gap_extend", "xdrop"),
             "_extend_band": ("gap_open", "gap_extend", "xdrop", "width"),
             "_seeds": ("gap_open", "gap_extend", "xdrop", "seeds"),
             "_seeds_band": ("gap_open", "gap_extend", "xdrop", "width", "seeds"),
             "_chains": ("gap_open", "gap_extend", "xdrop", "seeds", "chain_off")}[suffix]
    for name, value in zip(names, args):
        setattr(spec, name, value)
    spec.extend = int("xdrop" in names)
    return spec


def cigar_format(ops) -> str:
    """sa_cigar_format: BAM-packed ops (len << 4 | code) as text, "12=1X3I"."""
    ops = np.ascontiguousarray(ops, dtype=np.uint32)
    buf = ctypes.create_string_buffer(12 * len(ops) + 1)
    _check(lib.sa_cigar_format(ops.ctypes.data, len(ops), buf, len(buf)))
    return buf.value.decode()


def cigar_from_strings(aligned_text, aligned_pattern, gap_letter="-", eqx: bool = True, cap: int | None = None) -> dict:
    """sa_cigar_from_strings (host only, no device call): the CIGAR of two aligned strings as sa_hip.h defines it,
    for the callers of Plan, align_pair and align_batch. `cap` (default: as many ops as there are columns) is
    the size of the op buffer; one that is too small raises SaError. Returns cigar (uint32 ops), cigar_string,
    num_ops and the five counts."""
    at = aligned_text.encode() if isinstance(aligned_text, str) else bytes(aligned_text)
    ap = aligned_pattern.encode() if isinstance(aligned_pattern, str) else bytes(aligned_pattern)
    if len(at) != len(ap):
        raise ValueError(f"the aligned strings have {len(at)} and {len(ap)} columns")
    gap = gap_letter.encode() if isinstance(gap_letter, str) else bytes(gap_letter)
    cap = len(at) if cap is None else cap
    ops = np.zeros(max(1, cap), np.uint32)
    res = SaCigarResult()
    _check(lib.sa_cigar_from_strings(at, ap, len(at), gap, CIGAR_EQX if eqx else CIGAR_M, ops.ctypes.data, cap, ctypes.byref(res)))
    ops = ops[: res.num_ops].copy()
    d = {"cigar": ops, "cigar_string": cigar_format(ops), "num_ops": res.num_ops}
    d.update({k: getattr(res, k) for k in CIGAR_COUNTS})
    return d


def align_pairs_cigar(mode: int, texts: list[np.ndarray], patterns: list[np.ndarray], S: np.ndarray, gap_open: int,
                      gap_extend: int, device: int = 0, eqx: bool = True, band: int | None = None, bands=None,
                      xdrop: int | None = None, seeds=None, width: int | None = None, chains=None) -> list[dict]:
    """sa_align_pairs_cigar: the pairs aligned as align_pairs_affine aligns them under the same keywords (which are
    resolved and refused by the same rules and words), with each alignment returned as a CIGAR instead of two
    strings: the strings are made on the device, encoded there and never copied to the host. The dicts are those
    of align_pairs_affine(strings=False) plus cigar (uint32 BAM ops, len << 4 | code, = and X under `eqx`, else M),
    cigar_string, num_ops, ops_off (the pair's first op in the call's op array) and matches, mismatches,
    text_gap_letters (columns of I), pattern_gap_letters (columns of D) and gap_opens, which are counted from the
    letters whatever `eqx` is. Without `gap_extend` (None) the gap is linear: gap_extend = gap_open."""
    variant = _variant(gap_open, gap_extend, band, bands, xdrop, seeds, len(texts), width, chains)
    spec = _align_spec(variant, gap_open)
    p, S_keep, alpha_keep = _params(mode, S, gap_open, None, 0)
    hp, ts, ps = _host_pairs(texts, patterns)
    n = len(ts)
    res = (SaCigarResult * max(1, n))()
    handle = ctypes.c_void_p()
    _check(lib.sa_align_pairs_cigar(ctypes.byref(p), ctypes.byref(spec), CIGAR_EQX if eqx else CIGAR_M, hp, n, device, res,
                                    ctypes.byref(handle)))
    try:
        total = lib.sa_cigars_num_ops(handle)
        addr = lib.sa_cigars_ops(handle)
        ops = np.ctypeslib.as_array(ctypes.cast(addr, ctypes.POINTER(ctypes.c_uint32)), (total,)).copy() if addr else np.zeros(0, np.uint32)
    finally:
        lib.sa_cigars_destroy(handle)
    # the records as tuples of Python ints in one pass (a ctypes field read per value costs more than the rest)
    rows = np.frombuffer(res, dtype=CIGAR_DTYPE, count=n).tolist()
    keys = tuple(k for k in CIGAR_DTYPE.names if k != "status")
    cap = 12 * max([r[6] for r in rows], default=0) + 1
    buf = ctypes.create_string_buffer(cap)  # one text buffer for every pair: an op is at most 9 digits and a letter
    base, out = ops.ctypes.data, []
    for r in rows:
        off, num = r[5], r[6]
        _check(lib.sa_cigar_format(base + 4 * off, num, buf, cap))
        d = dict(zip(keys, r[:1] + r[2:]))
        d["cigar"] = ops[off: off + num]
        d["cigar_string"] = buf.value.decode()
        out.append(d)
    return out


# numpy view of sa_cigar_result (include/sa_hip.h), the names those of the dicts align_pairs_cigar returns
CIGAR_DTYPE = np.dtype([("score", "<i4"), ("status", "<i4"), ("num_bytes", "<u8"), ("start_text", "<u8"), ("start_pattern", "<u8"),
                        ("ops_off", "<u8"), ("num_ops", "<u4"), ("matches", "<u4"), ("mismatches", "<u4"),
                        ("text_gap_letters", "<u4"), ("pattern_gap_letters", "<u4"), ("gap_opens", "<u4")])
assert CIGAR_DTYPE.itemsize == ctypes.sizeof(SaCigarResult)


def cigar_last_stats() -> dict:
    """sa_cigar_last_stats: the calling thread's last align_pairs_cigar (device ms of the two encoder passes, bytes
    of ops copied to the host, bytes of the two string arenas that were not)."""
    e, o, s = ctypes.c_double(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    _check(lib.sa_cigar_last_stats(ctypes.byref(e), ctypes.byref(o), ctypes.byref(s)))
    return {"encode_ms": e.value, "ops_bytes": o.value, "string_bytes_not_copied": s.value}


# numpy view of sa_chain_result (include/sa_hip.h)
CHAIN_DTYPE = np.dtype([("score", "<i4"), ("status", "<i4"), ("seeds_off", "<u8"), ("num_seeds", "<u4"), ("last_anchor", "<u4")])
assert CHAIN_DTYPE.itemsize == ctypes.sizeof(SaChainResult)


def canonical_order(anchors) -> np.ndarray:
    """One pair's anchors, an (A, 3) array of (text_pos, pattern_pos, length), in the canonical order the chaining
    functions want: non-decreasing (text end, pattern end, length)."""
    a = np.asarray(anchors, dtype=np.int64).reshape(-1, 3)
    return a[np.lexsort((a[:, 2], a[:, 1] + a[:, 2], a[:, 0] + a[:, 2]))]


def chain_anchors(anchors, match: int, gap_open: int, gap_extend: int, skip: int = 0, max_gap: int = NO_LIMIT,
                  max_diag: int = NO_LIMIT, lookback: int = 64, device: int = 0, host: bool = False, sort: bool = True):
    """sa_chain_anchors: one colinear, overlap-free chain per pair out of a seeder's unfiltered anchors (the
    definition is in sa_hip.h). `anchors` holds one (A_k, 3) array or list of (text_pos, pattern_pos, length)
    triples per pair; a pair may have none. Returns (results, chains): results[k] is a dict of score, seeds_off,
    num_seeds and last_anchor (an index into the pair's anchors in canonical order), chains[k] the pair's chain as
    an (num_seeds, 3) int64 array, the form chains= of score_batch, Scorer, align_pairs_affine and
    align_pairs_cigar accepts. Those refuse a pair without a seed: drop the pairs whose num_seeds is 0 first.
    sort=True puts each pair's anchors in canonical order first (np.lexsort, on the host); with sort=False a pair
    out of order is refused. host=True calls sa_chain_anchors_host, the same definition without a device."""
    per = [np.asarray(a, dtype=np.int64).reshape(-1, 3) for a in anchors]
    if any((a < 0).any() for a in per):
        raise ValueError("anchors holds a negative value")
    if sort:
        per = [canonical_order(a) for a in per]
    n = len(per)
    flat = np.concatenate(per + [np.zeros((1, 3), np.int64)]).astype(np.uint64)  # one triple more: never a null address
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(a) for a in per], dtype=np.uint64)
    cp = SaChainParams(match, gap_open, gap_extend, skip, max_gap, max_diag, lookback)
    res = (SaChainResult * max(1, n))()
    handle = ctypes.c_void_p()
    if host:
        _check(lib.sa_chain_anchors_host(ctypes.byref(cp), flat.ctypes.data, off.ctypes.data, n, res, ctypes.byref(handle)))
    else:
        _check(lib.sa_chain_anchors(ctypes.byref(cp), flat.ctypes.data, off.ctypes.data, n, device, res, ctypes.byref(handle)))
    try:
        rows = np.frombuffer(res, dtype=CHAIN_DTYPE, count=n)
        coff = np.ctypeslib.as_array(ctypes.cast(lib.sa_chain_set_off(handle), ctypes.POINTER(ctypes.c_uint64)), (n + 1,)).copy()
        addr = lib.sa_chain_set_seeds(handle)
        total = int(coff[n])
        seeds = (np.ctypeslib.as_array(ctypes.cast(addr, ctypes.POINTER(ctypes.c_uint64)), (total, 3)).astype(np.int64) if addr
                 else np.zeros((0, 3), np.int64))
    finally:
        lib.sa_chain_set_destroy(handle)
    if len(seeds) != total or (n and not (coff[:-1] == rows["seeds_off"]).all()):
        raise SaError(1, "sa_chain_anchors: the seed offsets do not add up")
    keys = ("score", "seeds_off", "num_seeds", "last_anchor")
    results = [dict(zip(keys, (r[0], r[2], r[3], r[4]))) for r in rows.tolist()]
    chains = [seeds[int(coff[k]): int(coff[k + 1])] for k in range(n)]
    return results, chains


def chain_last_stats() -> dict:
    """sa_chain_last_stats: the calling thread's last chain_anchors on a device (device ms of the recurrence and of
    the walk, bytes of device memory held)."""
    d, w, b = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_uint64(0)
    _check(lib.sa_chain_last_stats(ctypes.byref(d), ctypes.byref(w), ctypes.byref(b)))
    return {"dp_ms": d.value, "walk_ms": w.value, "device_bytes": b.value}


def affine_last_stats() -> dict:
    """sa_affine_last_stats: the calling thread's last affine alignment call (device ms of the traced
    fills and of the walks, direction-arena bytes, chunks)."""
    f, w, b, c = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_uint64(0), ctypes.c_int32(0)
    _check(lib.sa_affine_last_stats(ctypes.byref(f), ctypes.byref(w), ctypes.byref(b), ctypes.byref(c)))
    return {"fill_ms": f.value, "walk_ms": w.value, "arena_bytes": b.value, "num_chunks": c.value}


def _align_host_pairs(mode, texts, patterns, S, gap, where, alphabet, strings, variant) -> list[dict]:
    """align_batch (no gap model: `where` is num_gpus) and align_pairs_affine (`variant` of _variant, `where` the
    device): one packing of the host pairs and buffers."""
    p, S_keep, alpha_keep = _params(mode, S, gap, alphabet, 0)
    hp, ts, ps = _host_pairs(texts, patterns)
    n = len(ts)
    bufs_t = [ctypes.create_string_buffer(max(1, len(t) + len(x))) for t, x in zip(ts, ps)] if strings else []
    bufs_p = [ctypes.create_string_buffer(max(1, len(t) + len(x))) for t, x in zip(ts, ps)] if strings else []
    at = (ctypes.c_void_p * max(1, n))(*[ctypes.addressof(b) for b in bufs_t]) if strings else None
    ap = (ctypes.c_void_p * max(1, n))(*[ctypes.addressof(b) for b in bufs_p]) if strings else None
    res = (SaResult * max(1, n))()
    suffix, args, keep = variant
    fn = getattr(lib, "sa_align_pairs" + suffix) if suffix else lib.sa_align_batch
    _check(fn(ctypes.byref(p), *args, hp, n, where, res, at, ap))
    if not strings:
        return [_result_dict(r) for r in res[:n]]
    return [_result_dict(r, bufs_t[i].raw, bufs_p[i].raw) for i, r in enumerate(res[:n])]


class Plan:
    """Many pairs, device-resident arenas, explicit stream (for benches and the batch path)."""

    def __init__(self, mode: int, S: np.ndarray, gap: int, pairs: list[tuple[int, int, int, int]],
                 device: int = 0, alphabet: bytes | None = None, rows_per_lane: int = 0):
        self._p, self._S, self._alpha = _params(mode, S, gap, alphabet, rows_per_lane)
        arr = (SaPair * max(1, len(pairs)))(*[SaPair(*pr) for pr in pairs])
        self.num_pairs = len(pairs)
        self.pairs = pairs
        self.device = device
        h = ctypes.c_void_p()
        _check(lib.sa_plan_create(ctypes.byref(self._p), arr, len(pairs), device, ctypes.byref(h)))
        self.handle = h

    def close(self) -> None:
        if getattr(self, "handle", None):
            lib.sa_plan_destroy(self.handle)
            self.handle = None

    __del__ = close

    def info(self) -> dict:
        ns, r, db, mb = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib.sa_plan_info(self.handle, ctypes.byref(ns), ctypes.byref(r), ctypes.byref(db), ctypes.byref(mb)))
        kind = lib.sa_plan_fill_kind(self.handle)
        return {"num_strips": ns.value, "rows_per_lane": r.value, "device_bytes": db.value, "mask_bytes": mb.value,
                "fill_kernel": FILL_KINDS.get(kind, kind)}

    def fill(self, d_text: int, d_pattern: int, stream: int | None = None) -> None:
        _check(lib.sa_plan_fill(self.handle, d_text, d_pattern, stream))

    def traceback(self, stream: int | None = None) -> None:
        _check(lib.sa_plan_traceback(self.handle, stream))

    def results(self, stream: int | None = None) -> list[dict]:
        out = (SaResult * max(1, self.num_pairs))()
        _check(lib.sa_plan_fetch_results(self.handle, out, stream))
        return [_result_dict(r) for r in out[: self.num_pairs]]

    def results_array(self, stream: int | None = None) -> np.ndarray:
        """Every pair's sa_result as one numpy structured array (RESULT_DTYPE): no per-pair objects."""
        out = np.empty(max(1, self.num_pairs), RESULT_DTYPE)
        _check(lib.sa_plan_fetch_results(self.handle, out.ctypes.data, stream))
        return out[: self.num_pairs]

    def copy_results(self, d_dst: int, stream: int | None = None) -> None:
        """Asynchronous device-to-device copy of every pair's sa_result (32 bytes each) to d_dst."""
        _check(lib.sa_plan_copy_results(self.handle, d_dst, stream))

    def directions(self, index: int, stream: int | None = None) -> np.ndarray:
        """Decoded (m+1)x(n+1) DIRECTION matrix of pair `index` (reference layout, for verification)."""
        n, m = self.pairs[index][1], self.pairs[index][3]
        M = np.empty((m + 1) * (n + 1), dtype=np.uint8)
        _check(lib.sa_plan_fetch_directions(self.handle, index, M.ctypes.data, stream))
        return M

    def alignment(self, index: int, stream: int | None = None) -> tuple[str, str]:
        cap = max(1, self.pairs[index][1] + self.pairs[index][3])
        at = ctypes.create_string_buffer(cap)
        ap = ctypes.create_string_buffer(cap)
        _check(lib.sa_plan_fetch_alignment(self.handle, index, at, ap, cap, stream))
        r = self.results(stream)[index]
        return at.raw[: r["num_bytes"]].decode(), ap.raw[: r["num_bytes"]].decode()

    def all_alignments(self, stream: int | None = None) -> list[dict]:
        """Every pair's result with its aligned strings, fetched in one pass (sa_plan_fetch_all)."""
        nb = int(lib.sa_plan_output_bytes(self.handle))
        tb = np.empty(max(1, nb), np.uint8)
        pb = np.empty(max(1, nb), np.uint8)
        out = (SaResult * max(1, self.num_pairs))()
        offs = np.zeros(max(1, self.num_pairs), np.uint64)
        _check(lib.sa_plan_fetch_all(self.handle, out, tb.ctypes.data, pb.ctypes.data, max(1, nb),
                                     offs.ctypes.data, stream))
        return [_result_dict(r, tb[o:], pb[o:]) for r, o in zip(out[: self.num_pairs], offs.tolist())]


# numpy view of sa_score_result (include/sa_hip.h): int32 score, int32 status, uint64 x 2
SCORE_DTYPE = np.dtype([("score", "<i4"), ("status", "<i4"), ("end_text", "<u8"), ("end_pattern", "<u8")])
assert SCORE_DTYPE.itemsize == ctypes.sizeof(SaScoreResult)


def score_batch(mode: int, texts: list[np.ndarray], patterns: list[np.ndarray], S: np.ndarray, gap: int,
                device: int = 0, rows_per_lane: int = 0, gap_extend: int | None = None, band: int | None = None,
                bands=None, xdrop: int | None = None, seeds=None, width: int | None = None, chains=None) -> np.ndarray:
    """sa_score_batch: the score and scored cell of every pair from host memory (SCORE_DTYPE), without
    direction planes or traceback (synchronous). With `gap_extend`, sa_score_batch_affine: `gap` is
    the gap-open penalty and a gap of k letters costs gap + (k - 1) * gap_extend. With `band`,
    sa_score_batch_banded: the scores inside the diagonal band of that half-width (sa_hip.h); without
    `gap_extend` the gap is linear, gap_open = gap_extend = gap. `mode` is SA_GLOBAL, SA_LOCAL, FIT or
    an ends-free mode (ends_free(), OVERLAP; not with `band`): end_pattern and end_text are the cell the
    score is read from. With `bands` (an (np, 2) int32 array or a list of (lo, hi), one per pair; not with
    `band`), sa_score_batch_band_at: pair k inside lo <= j - i <= hi of bands[k], in every mode; a pair
    without an alignment in its band fails the call (band_reachable). With `xdrop` (NO_XDROP or
    0 .. 2**30 - 1; mode SA_GLOBAL, no band), sa_score_batch_extend: extension alignment, the best cell of
    the rows before the X-drop's stop row, anchored at the origin; without `gap_extend` the gap is linear.
    With `seeds` (one (text_pos, pattern_pos, length) per pair; requires `xdrop`, mode SA_GLOBAL, no band),
    sa_score_batch_seeds: the extension to both sides of each pair's seed plus the seed's score, as a
    SEED_DTYPE array (score, status, begin_text, begin_pattern, end_text, end_pattern). With `width` (>= 0;
    requires `xdrop`, takes neither `band` nor `bands`), sa_score_batch_extend_band or, with `seeds`,
    sa_score_batch_seeds_band: the extension inside |j - i| <= width of its own matrix, the same width on both
    sides of a seed; a width of max(n, m) or more is the unbanded call. With `chains` (per pair, a list of colinear,
    non-overlapping (text_pos, pattern_pos, length) seeds; requires `xdrop`, mode SA_GLOBAL; excludes `seeds`,
    `band`, `bands` and `width`), sa_score_batch_chains: the seeds' scores, the global score of every rectangle
    between two consecutive seeds and the extensions of the chain's two ends, as a SEED_DTYPE array."""
    suffix, args, keep = _variant(gap, gap_extend, band, bands, xdrop, seeds, len(texts), width, chains)
    p, S_keep, alpha_keep = _params(mode, S, gap, None, rows_per_lane)
    hp, ts, ps = _host_pairs(texts, patterns)
    n = len(ts)
    out = np.zeros(max(1, n), SEED_DTYPE if seeds is not None or chains is not None else SCORE_DTYPE)
    _check(getattr(lib, "sa_score_batch" + suffix)(ctypes.byref(p), *args, hp, n, device, out.ctypes.data))
    return out[:n]


class Scorer:
    """Scores of many pairs, device-resident arenas, explicit stream (beside Plan: no planes, no traceback).
    With `gap_extend`, an affine scorer (sa_scorer_create_affine): `gap` is the gap-open penalty. With
    `band`, a banded scorer (sa_scorer_create_banded; without `gap_extend` the gap is linear). With
    `bands`, one (lo, hi) per pair, a band-at scorer (sa_scorer_create_band_at; not with `band`). With
    `xdrop`, an extension scorer (sa_scorer_create_extend; mode SA_GLOBAL, no band). With `seeds` (one
    (text_pos, pattern_pos, length) per pair; requires `xdrop`), a seeds scorer (sa_scorer_create_seeds):
    results() is then a SEED_DTYPE array. With `width` (requires `xdrop`), the banded extension scorer or seeds
    scorer (sa_scorer_create_extend_band, sa_scorer_create_seeds_band). With `chains` (per pair, a list of seeds;
    requires `xdrop`, excludes `seeds`, `band`, `bands` and `width`), a chains scorer (sa_scorer_create_chains):
    results() is a SEED_DTYPE array, as a seeds scorer's. `mode` as score_batch takes it."""

    def __init__(self, mode: int, S: np.ndarray, gap: int, pairs: list[tuple[int, int, int, int]],
                 device: int = 0, rows_per_lane: int = 0, gap_extend: int | None = None, band: int | None = None,
                 bands=None, xdrop: int | None = None, seeds=None, width: int | None = None, chains=None):
        suffix, args, keep = _variant(gap, gap_extend, band, bands, xdrop, seeds, len(pairs), width, chains)
        self._p, self._S, self._alpha = _params(mode, S, gap, None, rows_per_lane)
        arr = (SaPair * max(1, len(pairs)))(*[SaPair(*pr) for pr in pairs])
        self.num_pairs = len(pairs)
        self.pairs = pairs
        self.device = device
        h = ctypes.c_void_p()
        self.seeded = seeds is not None or chains is not None
        _check(getattr(lib, "sa_scorer_create" + suffix)(ctypes.byref(self._p), *args, arr, len(pairs), device, ctypes.byref(h)))
        self.handle = h

    def close(self) -> None:
        if getattr(self, "handle", None):
            lib.sa_scorer_destroy(self.handle)
            self.handle = None

    __del__ = close

    def info(self) -> dict:
        nw, r, db = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_uint64()
        _check(lib.sa_scorer_info(self.handle, ctypes.byref(nw), ctypes.byref(r), ctypes.byref(db)))
        return {"num_waves": nw.value, "rows_per_lane": r.value, "device_bytes": db.value}

    def run(self, d_text: int, d_pattern: int, stream: int | None = None) -> None:
        _check(lib.sa_scorer_run(self.handle, d_text, d_pattern, stream))

    def results(self, stream: int | None = None) -> np.ndarray:
        """Every pair's sa_score_result as one numpy structured array (SCORE_DTYPE); synchronises. A seeds
        scorer returns its sa_seed_result array (SEED_DTYPE); score_results() has its sa_score_result view."""
        if self.seeded:
            out = np.zeros(max(1, self.num_pairs), SEED_DTYPE)
            _check(lib.sa_scorer_fetch_seeds(self.handle, out.ctypes.data, stream))
            return out[: self.num_pairs]
        return self.score_results(stream)

    def score_results(self, stream: int | None = None) -> np.ndarray:
        """sa_scorer_fetch: SCORE_DTYPE of every pair; on a seeds scorer the score with the absolute end cell."""
        out = np.zeros(max(1, self.num_pairs), SCORE_DTYPE)
        _check(lib.sa_scorer_fetch(self.handle, out.ctypes.data, stream))
        return out[: self.num_pairs]


def search(mode: int, query: np.ndarray, texts: list[np.ndarray], S: np.ndarray, gap: int, k: int,
           device: int = 0, strings: bool = True, gap_extend: int | None = None) -> tuple[np.ndarray, list[dict]]:
    """sa_search: `query` (the pattern) against every text. Returns (scores, hits): scores is a
    SCORE_DTYPE array over the texts; hits holds the min(k, len(texts)) best (score descending, ties
    to the lower index), each {"index", "score", "num_bytes", "start_text", "start_pattern"} and, with
    strings, "aligned_text" / "aligned_pattern", as align_pair gives them for that pair. With
    `gap_extend`, sa_search_affine: `gap` is the gap-open penalty, and the hits are aligned under the
    gap model they were ranked by, as align_pairs_affine gives them. In mode FIT or an ends-free mode
    (ends_free(), OVERLAP) the hits of a linear search are aligned as align_pairs_affine aligns them with
    gap_open = gap_extend = gap."""
    p, S_keep, alpha_keep = _params(mode, S, gap, None, 0)
    q = np.ascontiguousarray(query, dtype=np.int8)
    ts = [np.ascontiguousarray(t, dtype=np.int8) for t in texts]
    n = len(ts)
    tp = (ctypes.c_void_p * max(1, n))(*[t.ctypes.data for t in ts])
    tl = np.array([len(t) for t in ts] or [0], dtype=np.uint64)
    scores = np.zeros(max(1, n), SCORE_DTYPE)
    kk = max(1, k)
    idx = np.zeros(kk, np.int64)
    res = (SaResult * kk)()
    cap = max(1, int(tl.max()) + len(q))
    bufs_t = [ctypes.create_string_buffer(cap) for _ in range(k)] if strings else []
    bufs_p = [ctypes.create_string_buffer(cap) for _ in range(k)] if strings else []
    at = (ctypes.c_void_p * kk)(*[ctypes.addressof(b) for b in bufs_t]) if strings else None
    ap = (ctypes.c_void_p * kk)(*[ctypes.addressof(b) for b in bufs_p]) if strings else None
    nh = ctypes.c_int64(0)
    if gap_extend is None:
        _check(lib.sa_search(ctypes.byref(p), q.ctypes.data, len(q), tp, tl.ctypes.data, n, k, device, scores.ctypes.data,
                             idx.ctypes.data, res, at, ap, ctypes.byref(nh)))
    else:
        _check(lib.sa_search_affine(ctypes.byref(p), gap, gap_extend, q.ctypes.data, len(q), tp, tl.ctypes.data, n, k,
                                    device, scores.ctypes.data, idx.ctypes.data, res, at, ap, ctypes.byref(nh)))
    hits = [{"index": int(idx[h]), **(_result_dict(res[h], bufs_t[h].raw, bufs_p[h].raw) if strings else _result_dict(res[h]))}
            for h in range(nh.value)]
    return scores[:n], hits
