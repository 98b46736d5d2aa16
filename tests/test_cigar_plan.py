"""CIGAR output (sa_hip.h: sa_align_pairs_cigar, sa_cigar_from_strings, sa_cigar_format) on the CPU: the reference of
the CIGAR tests, cigar_ref, written from the definition in sa_hip.h and pinned by a round trip (its ops expanded
over the input letters rebuild both strings of the existing CPU references, in every mode and for extensions, seeds
and chains); the two host functions against it; the exports and the layout of the two new structures; and every
refusal of a spec, which sa_align_pairs_cigar answers before its first device call, so without a GPU."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, matrix  # first: it puts oracle/ and the package on the path

from test_align_affine_gpu import affine_ref, alphabet_of
from test_chains_gpu import chains_ref, random_chain
from test_ends_gpu import ends_ref
from test_extend_gpu import extend_ref, random_small_pairs
from test_fit_gpu import fit_ref
from test_seeds_gpu import seeds_ref

GLOBAL, LOCAL = 0, 1
M, I, D, EQ, X = 0, 1, 2, 7, 8
LETTER = {M: "M", I: "I", D: "D", EQ: "=", X: "X"}
COUNTS = ("matches", "mismatches", "text_gap_letters", "pattern_gap_letters", "gap_opens")
INVALID, UNSUPPORTED = 1, 4


# ---- the reference of the CIGAR tests ------------------------------------------------------------------------------
def cigar_ref(at, ap, gap_letter="-", eqx=True):
    """sa_hip.h's definition, column by column: (ops, counts). An op is len << 4 | code."""
    assert len(at) == len(ap)
    codes = []
    counts = dict.fromkeys(COUNTS, 0)
    for a, b in zip(at, ap):
        if a == gap_letter:
            code = I
            counts["text_gap_letters"] += 1
        elif b == gap_letter:
            code = D
            counts["pattern_gap_letters"] += 1
        else:
            counts["matches" if a == b else "mismatches"] += 1
            code = (EQ if a == b else X) if eqx else M
        codes.append(code)
    ops = []
    for c in codes:
        if ops and ops[-1][1] == c:
            ops[-1][0] += 1
        else:
            ops.append([1, c])
            counts["gap_opens"] += c in (I, D)
    return [n << 4 | c for n, c in ops], counts


def cigar_text(ops):
    return "".join(f"{op >> 4}{LETTER[op & 15]}" for op in ops)


def expand(ops, text_letters, pattern_letters, start_text, start_pattern, gap_letter="-"):
    """The two aligned strings that `ops` describe over the ungapped letters from the two starts, and where they end."""
    at, ap, j, i = [], [], start_text, start_pattern
    for op in ops:
        n, c = op >> 4, op & 15
        at.append(gap_letter * n if c == I else text_letters[j:j + n])
        ap.append(gap_letter * n if c == D else pattern_letters[i:i + n])
        j += 0 if c == I else n
        i += 0 if c == D else n
    return "".join(at), "".join(ap), j, i


def round_trip(res, t, p, S, starts=None):
    """cigar_ref of a reference's strings, under both flags, rebuilds them from the letters. `starts`: the candidates
    for (start_text, start_pattern) where the mode keeps the reference's quirks."""
    alphabet = alphabet_of(S)
    tl, pl = "".join(alphabet[c] for c in t), "".join(alphabet[c] for c in p)
    at, ap = res["aligned_text"], res["aligned_pattern"]
    starts = starts or [(res["start_text"], res["start_pattern"])]
    for eqx in (True, False):
        ops, counts = cigar_ref(at, ap, alphabet[-1], eqx)
        assert sum(op >> 4 for op in ops) == len(at) == res["num_bytes"]
        assert all(op >> 4 >= 1 for op in ops) and all(a & 15 != b & 15 for a, b in zip(ops, ops[1:]))
        assert {op & 15 for op in ops} <= ({I, D, EQ, X} if eqx else {I, D, M})
        assert counts["matches"] + counts["mismatches"] + counts["text_gap_letters"] + counts["pattern_gap_letters"] == len(at)
        assert counts["gap_opens"] == sum(op & 15 in (I, D) for op in ops)
        assert any(expand(ops, tl, pl, a, b, alphabet[-1])[:2] == (at, ap) for a, b in starts), (at, ap, cigar_text(ops), starts)
        if eqx:
            assert counts["matches"] == sum(op >> 4 for op in ops if op & 15 == EQ)
            assert counts["mismatches"] == sum(op >> 4 for op in ops if op & 15 == X)


def scheme(A):
    return matrix("blast" if A == 4 else "blosum50", A)


def small_pairs(count=24, seed=91100, nmax=40):
    return random_small_pairs(count, seed, nmax)


_STRINGS = None


def reference_strings():
    """Aligned strings of every kind of reference, computed once: (aligned_text, aligned_pattern) pairs."""
    global _STRINGS
    if _STRINGS is None:
        out = []
        rng = np.random.default_rng(91200)
        for k, (A, t, p) in enumerate(small_pairs()):
            S = scheme(A)
            go, ge = ((11, 2), (5, 5))[k % 2]
            res = [affine_ref(GLOBAL, t, p, S, go, ge), affine_ref(LOCAL, t, p, S, go, ge), fit_ref(t, p, S, go, ge),
                   ends_ref(t, p, S, go, ge, 15), extend_ref(t, p, S, go, ge, 20),
                   chains_ref(t, p, random_chain(rng, len(t), len(p), 1 + k % 4), S, go, ge, None)]
            out += [(r["aligned_text"], r["aligned_pattern"]) for r in res]
        _STRINGS = out
    return _STRINGS


# ---- 1. cigar_ref is pinned by the round trip ----------------------------------------------------------------------
def test_round_trip_global_local_fit_and_overlap():
    for k, (A, t, p) in enumerate(small_pairs()):
        S = scheme(A)
        go, ge = ((11, 2), (5, 5))[k % 2]
        g = affine_ref(GLOBAL, t, p, S, go, ge)
        round_trip(g, t, p, S, [(0, 0)])  # both sides whole; the starts keep the reference's clamp
        loc = affine_ref(LOCAL, t, p, S, go, ge)
        # local keeps the reference's start-index quirk: a walk that ends on a STOP cell reports one before the first
        # aligned letter, clamped at 0
        a, b = loc["start_text"], loc["start_pattern"]
        round_trip(loc, t, p, S, [(a, b), (a + 1, b), (a, b + 1), (a + 1, b + 1)])
        round_trip(fit_ref(t, p, S, go, ge), t, p, S)
        round_trip(ends_ref(t, p, S, go, ge, 15), t, p, S)


def test_round_trip_extension_seeds_and_chains():
    rng = np.random.default_rng(91300)
    for k, (A, t, p) in enumerate(small_pairs(seed=91400)):
        S = scheme(A)
        go, ge = ((11, 2), (5, 5))[k % 2]
        xdrop = (None, 20, 3)[k % 3]
        round_trip(extend_ref(t, p, S, go, ge, xdrop), t, p, S)
        n, m = len(t), len(p)
        ts, ps = int(rng.integers(0, n + 1)), int(rng.integers(0, m + 1))
        seed = (ts, ps, int(rng.integers(0, min(n - ts, m - ps) + 1)))
        round_trip(seeds_ref(t, p, seed, S, go, ge, xdrop), t, p, S)
        round_trip(chains_ref(t, p, random_chain(rng, n, m, 1 + k % 5), S, go, ge, xdrop), t, p, S)


def test_cigar_ref_on_known_strings():
    assert cigar_text(cigar_ref("ACGT-A", "AC-TTA")[0]) == "2=1D1=1I1="
    assert cigar_text(cigar_ref("ACGT-A", "AC-TTA", eqx=False)[0]) == "2M1D1M1I1M"
    assert cigar_text(cigar_ref("AAAA", "AATA")[0]) == "2=1X1="
    ops, counts = cigar_ref("A--CC-", "ATT-CG")
    assert cigar_text(ops) == "1=2I1D1=1I"
    assert counts == {"matches": 2, "mismatches": 0, "text_gap_letters": 3, "pattern_gap_letters": 1, "gap_opens": 3}
    assert cigar_ref("", "") == ([], dict.fromkeys(COUNTS, 0))


# ---- 2. the host functions equal cigar_ref -------------------------------------------------------------------------
def boundary_strings():
    """Strings of 63, 64, 65, 128 and 129 columns with runs of every op, some of them across columns 64 and 128."""
    rng = np.random.default_rng(91500)
    out = []
    for n in (63, 64, 65, 128, 129):
        out.append(("A" * n, "A" * n))
        out.append(("AC" * n, "AG" * n))
        for _ in range(6):
            at, ap = [], []
            while len(at) < n:
                kind, run = int(rng.integers(0, 4)), int(rng.integers(1, 70))
                for _ in range(min(run, n - len(at))):
                    a = "ATCG"[int(rng.integers(0, 4))]
                    b = a if kind == 0 else "ATCG"[int(rng.integers(0, 4))]
                    at.append("-" if kind == 2 else a)
                    ap.append("-" if kind == 3 else b)
            out.append(("".join(at), "".join(ap)))
    return out


def test_from_strings_and_format_equal_cigar_ref():
    from sa_amd import engine
    cases = reference_strings() + boundary_strings() + [("", ""), ("-" * 70, "ACGT" * 17 + "AC"), ("ACGT" * 17 + "AC", "-" * 70),
                                                        ("----", "----"), ("-", "A"), ("A", "-"), ("A", "C")]
    for at, ap in cases:
        for eqx in (True, False):
            ops, counts = cigar_ref(at, ap, "-", eqx)
            got = engine.cigar_from_strings(at, ap, "-", eqx)
            assert got["cigar"].dtype == np.uint32 and got["cigar"].tolist() == ops, (at, ap, eqx)
            assert got["num_ops"] == len(ops) and {k: got[k] for k in COUNTS} == counts, (at, ap, eqx)
            assert got["cigar_string"] == cigar_text(ops) == engine.cigar_format(ops)
    assert engine.cigar_format([]) == ""
    # another gap letter, and bytes as well as str
    assert engine.cigar_from_strings(b"AC*T", b"A*GT", "*")["cigar_string"] == "1=1D1I1="


def test_cap_too_small_is_refused_and_still_counts():
    from sa_amd import engine
    at, ap = b"AAC-TT--G", b"AAGGT-AAG"
    ops, counts = cigar_ref(at.decode(), ap.decode())
    assert len(ops) == 7
    res = engine.SaCigarResult()
    buf = (ctypes.c_uint32 * 8)(*([0xFFFFFFFF] * 8))
    for cap in (0, 1, 6):
        rc = engine.lib.sa_cigar_from_strings(at, ap, len(at), b"-", engine.CIGAR_EQX, buf if cap else None, cap, ctypes.byref(res))
        assert rc == INVALID and b"cap" in engine.lib.sa_last_error()
        assert res.num_ops == 7 and res.matches == counts["matches"] and res.num_alignment_bytes == len(at)
        assert list(buf[:cap]) == ops[:cap] and all(v == 0xFFFFFFFF for v in buf[cap:])  # nothing past cap is written
    assert engine.lib.sa_cigar_from_strings(at, ap, len(at), b"-", engine.CIGAR_EQX, buf, 7, None) == 0  # counts may be NULL
    assert list(buf[:7]) == ops
    with pytest.raises(engine.SaError) as e:
        engine.cigar_from_strings(at, ap, cap=3)
    assert e.value.code == INVALID
    assert engine.lib.sa_cigar_from_strings(at, ap, len(at), b"-", 2, buf, 8, None) == INVALID  # unknown flags bits
    # the text buffer of sa_cigar_format: too small is refused, and so is a code that is no op
    arr = np.array(ops, dtype=np.uint32)
    text = ctypes.create_string_buffer(len(cigar_text(ops)))
    assert engine.lib.sa_cigar_format(arr.ctypes.data, len(arr), text, len(text)) == INVALID
    bad = np.array([5 << 4 | 3], dtype=np.uint32)
    text = ctypes.create_string_buffer(16)
    assert engine.lib.sa_cigar_format(bad.ctypes.data, 1, text, 16) == INVALID


# ---- 3. the C ABI ---------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("sa_align_pairs_cigar", "sa_cigars_ops", "sa_cigars_num_ops", "sa_cigars_destroy", "sa_cigar_from_strings",
               "sa_cigar_format", "sa_cigar_last_stats")


def test_the_library_exports_the_new_symbols():
    from sa_amd import engine
    for name in NEW_SYMBOLS:
        assert name in engine.EXPORTS and hasattr(engine.lib, name), name
    for name in ("align_pairs_cigar", "cigar_from_strings", "cigar_format", "cigar_last_stats"):
        assert callable(getattr(engine, name))
    assert engine.cigar_last_stats().keys() == {"encode_ms", "ops_bytes", "string_bytes_not_copied"}


def test_the_ctypes_structures_have_the_layout_of_the_header(tmp_path):
    from sa_amd import engine
    fields = {"sa_cigar_result": engine.SaCigarResult, "sa_align_spec": engine.SaAlignSpec}
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "sa_hip.h"', "int main(void) {"]
    for name, cls in fields.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in cls._fields_]
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    want = {}
    for name, cls in fields.items():
        want[name] = str(ctypes.sizeof(cls))
        want.update({f"{name}.{f}": str(getattr(cls, f).offset) for f, _ in cls._fields_})
    assert got == want
    assert ctypes.sizeof(engine.SaCigarResult) == 64


# ---- 4. every refusal of a spec comes before the device ------------------------------------------------------------
def call(engine, spec, flags=1, num_pairs=1, with_out=True, device=0):
    S = np.ascontiguousarray(matrix("blast", 4), dtype=np.int32)
    params = engine.SaParams(GLOBAL, 4, 0, 0, S.ctypes.data, b"ATCG-")
    t = np.zeros(8, np.int8)
    hp = (engine.SaHostPair * 1)(engine.SaHostPair(t.ctypes.data, 8, t.ctypes.data, 8))
    res = (engine.SaCigarResult * 1)()
    handle = ctypes.c_void_p(0xDEAD)
    rc = engine.lib.sa_align_pairs_cigar(ctypes.byref(params), ctypes.byref(spec) if spec is not None else None, flags, hp, num_pairs,
                                         device, res, ctypes.byref(handle) if with_out else None)
    if with_out and rc != 0:
        assert handle.value is None  # on failure *out stays NULL
    return rc, engine.lib.sa_last_error().decode()


def spec_of(engine, **kw):
    fields = dict(gap_open=11, gap_extend=2, band=-1, xdrop=engine.NO_XDROP, width=-1, extend=0, bands=None, seeds=None, chain_off=None)
    fields.update(kw)
    return engine.SaAlignSpec(**fields)


def test_spec_refusals_name_their_fields_and_precede_the_device():
    from sa_amd import engine
    bands = (engine.SaBand * 1)(engine.SaBand(-3, 3))
    seeds = (ctypes.c_uint64 * 3)(0, 0, 4)
    off = (ctypes.c_uint64 * 2)(0, 1)
    pb, ps, po = (ctypes.cast(x, ctypes.c_void_p).value for x in (bands, seeds, off))
    refused = [
        (dict(band=4, bands=pb), ("spec->band", "spec->bands")),
        (dict(band=4, extend=1), ("spec->extend", "spec->band")),
        (dict(bands=pb, extend=1), ("spec->extend", "spec->bands")),
        (dict(width=8), ("spec->width", "spec->extend")),
        (dict(seeds=ps), ("spec->seeds", "spec->extend")),
        (dict(chain_off=po, extend=1), ("spec->chain_off", "spec->seeds")),
        (dict(chain_off=po, seeds=ps, extend=1, width=8), ("spec->chain_off", "spec->width")),
    ]
    # a device that no machine has: a call that got past the checks would fail with SA_ERR_HIP, not SA_ERR_INVALID
    for device in (0, 1 << 20):
        for kw, words in refused:
            rc, msg = call(engine, spec_of(engine, **kw), device=device)
            assert rc == INVALID and msg.startswith("sa_align_pairs_cigar: ") and all(w in msg for w in words), (kw, rc, msg)
        for flags in (2, 3, -1, 1 << 8):
            rc, msg = call(engine, spec_of(engine), flags=flags, device=device)
            assert rc == INVALID and "flags" in msg, (flags, rc, msg)
        rc, msg = call(engine, None, device=device)
        assert rc == INVALID and "spec is null" in msg
        rc, msg = call(engine, spec_of(engine), with_out=False, device=device)
        assert rc == INVALID and "out is null" in msg
    rc, msg = call(engine, spec_of(engine), device=1 << 20)
    assert rc == 3  # SA_ERR_HIP: a spec that passes the checks reaches the device
    assert engine.cigar_last_stats() == {"encode_ms": 0.0, "ops_bytes": 0, "string_bytes_not_copied": 0}


def test_a_run_must_fit_28_bits():
    from sa_amd import engine
    S = np.ascontiguousarray(matrix("blast", 4), dtype=np.int32)
    params = engine.SaParams(GLOBAL, 4, 0, 0, S.ctypes.data, b"ATCG-")
    t = np.zeros(8, np.int8)
    spec = spec_of(engine)
    res = (engine.SaCigarResult * 1)()
    handle = ctypes.c_void_p()
    for n, m, want in (((1 << 28) - 8, 8, UNSUPPORTED), (1 << 27, 1 << 27, UNSUPPORTED)):
        hp = (engine.SaHostPair * 1)(engine.SaHostPair(t.ctypes.data, n, t.ctypes.data, m))  # refused before a letter is read
        rc = engine.lib.sa_align_pairs_cigar(ctypes.byref(params), ctypes.byref(spec), 1, hp, 1, 1 << 20, res, ctypes.byref(handle))
        assert rc == want and "2^28" in engine.lib.sa_last_error().decode()


def test_the_python_keywords_are_refused_in_the_words_of_align_pairs_affine():
    from sa_amd import engine
    S = matrix("blast", 4)
    t = [np.zeros(8, np.int8)]
    for kw in (dict(band=3, bands=[(-3, 3)]), dict(band=3, xdrop=5), dict(width=4), dict(seeds=[(0, 0, 2)]),
               dict(seeds=[(0, 0, 2)], xdrop=5, band=3), dict(chains=[[(0, 0, 2)]], xdrop=5, width=4), dict(chains=[[(0, 0, 2)]]),
               dict(chains=[[(0, 0, 2)]], xdrop=5, seeds=[(0, 0, 2)])):
        with pytest.raises(ValueError) as a:
            engine.align_pairs_affine(GLOBAL, t, t, S, 11, 2, **kw)
        with pytest.raises(ValueError) as b:
            engine.align_pairs_cigar(GLOBAL, t, t, S, 11, 2, **kw)
        assert str(a.value) == str(b.value), kw
