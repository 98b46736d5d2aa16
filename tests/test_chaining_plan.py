"""Chaining (sa_hip.h: sa_chain_anchors, sa_chain_anchors_host) on the CPU: the reference of the chaining tests,
chain_ref, written from the definition in sa_hip.h and pinned against a brute force over all subsequences; the host
function against it, on the random sets and on every case of tests/test_chaining_gpu.py; the identities K1, K4 and
K5; the layout of the two new structures; every refusal, through the host function and through sa_chain_anchors,
which refuses before its first device call and so without a GPU; and bin/sa_chain_plan_check."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG  # first: it puts the package on the path

INVALID, HIP, UNSUPPORTED = 1, 3, 4
NO_LIMIT = 2 ** 31 - 1
PARAMS = ("match", "gap_open", "gap_extend", "skip", "max_gap", "max_diag", "lookback")


def params(match=5, gap_open=11, gap_extend=2, skip=0, max_gap=NO_LIMIT, max_diag=NO_LIMIT, lookback=64):
    return dict(match=match, gap_open=gap_open, gap_extend=gap_extend, skip=skip, max_gap=max_gap, max_diag=max_diag, lookback=lookback)


def canonical(anchors):
    a = np.asarray(anchors, dtype=np.int64).reshape(-1, 3)
    return a[np.lexsort((a[:, 2], a[:, 1] + a[:, 2], a[:, 0] + a[:, 2]))]


# ---- the reference of the chaining tests ---------------------------------------------------------------------------
def transition(j, i, match, gap_open, gap_extend, skip, max_gap, max_diag, **_):
    """value(j -> i) and o of sa_hip.h for two anchors (x, y, L), or None when the transition is not admissible (the
    lookback apart). Python integers: exact."""
    exj, eyj = j[0] + j[2], j[1] + j[2]
    x, y, L = i
    o = max(0, exj - x, eyj - y)
    if o >= L:
        return None
    dx, dy = x + o - exj, y + o - eyj
    dd = abs(dx - dy)
    if dx > max_gap or dy > max_gap or dd > max_diag:
        return None
    return match * (L - o) - (gap_open + (dd - 1) * gap_extend if dd else 0) - skip * min(dx, dy), o


def chain_ref(anchors, match, gap_open, gap_extend, skip=0, max_gap=NO_LIMIT, max_diag=NO_LIMIT, lookback=64):
    """sa_hip.h's definition for one pair's anchors in canonical order: score, num_seeds, last_anchor, the seeds and
    the anchors' indices. The window of an anchor is evaluated at once, in int64 (a cost stays below 2^52)."""
    a = np.asarray(anchors, dtype=np.int64).reshape(-1, 3)
    n = len(a)
    if n == 0:
        return {"score": 0, "num_seeds": 0, "last_anchor": 0, "seeds": [], "indices": []}
    x, y, L = a[:, 0], a[:, 1], a[:, 2]
    ex, ey = x + L, y + L
    f = np.zeros(n, np.int64)
    pred = np.full(n, -1, np.int64)
    cut = np.zeros(n, np.int64)
    for i in range(n):
        lo = max(0, i - lookback)
        f[i] = match * L[i]
        if i == lo:
            continue
        o = np.maximum(0, np.maximum(ex[lo:i] - x[i], ey[lo:i] - y[i]))
        dx, dy = x[i] + o - ex[lo:i], y[i] + o - ey[lo:i]
        dd = np.abs(dx - dy)
        ok = (o < L[i]) & (dx <= max_gap) & (dy <= max_gap) & (dd <= max_diag)
        if not ok.any():
            continue
        cost = np.where(dd > 0, gap_open + (dd - 1) * gap_extend, 0) + skip * np.minimum(dx, dy)
        v = np.where(ok, f[lo:i] + match * (L[i] - o) - cost, np.iinfo(np.int64).min)
        k = len(v) - 1 - int(np.argmax(v[::-1]))  # among equal values the largest j
        if v[k] > f[i]:  # only when strictly better than starting anew
            f[i], pred[i], cut[i] = v[k], lo + k, o[k]
    end = int(np.argmax(f))  # ties to the lowest index
    indices = [end]
    while pred[indices[-1]] >= 0:
        indices.append(int(pred[indices[-1]]))
    indices.reverse()
    seeds = [(int(x[i] + cut[i]), int(y[i] + cut[i]), int(L[i] - cut[i])) for i in indices]
    return {"score": int(f[end]), "num_seeds": len(seeds), "last_anchor": end, "seeds": seeds, "indices": indices}


def brute_force(anchors, p):
    """The best score over every index-increasing subsequence with admissible consecutive transitions."""
    a = [tuple(int(v) for v in r) for r in anchors]
    best = 0
    for mask in range(1, 1 << len(a)):
        picked = [a[i] for i in range(len(a)) if mask >> i & 1]
        score = p["match"] * picked[0][2]
        for j, i in zip(picked, picked[1:]):
            tr = transition(j, i, **p)
            if tr is None:
                break
            score += tr[0]
        else:
            best = max(best, score)
    return best


def is_chain_of(anchors, res):
    """(K1): colinear, no overlap, every L >= 1, each seed the tail of an input anchor that shares its end."""
    seeds = res["seeds"]
    ends = {(int(x + L), int(y + L)): int(L) for x, y, L in sorted(map(tuple, anchors), key=lambda r: r[2])}
    for k, (x, y, L) in enumerate(seeds):
        if L < 1 or ends.get((x + L, y + L), 0) < L:
            return False
        if k and (seeds[k - 1][0] + seeds[k - 1][2] > x or seeds[k - 1][1] + seeds[k - 1][2] > y):
            return False
    if not seeds:
        return len(anchors) == 0
    x, y, L = (int(v) for v in anchors[res["last_anchor"]])
    return (x + L, y + L) == (seeds[-1][0] + seeds[-1][2], seeds[-1][1] + seeds[-1][2])


def random_sets(count=300, seed=97100):
    """Sets of up to 9 anchors in a 30 x 30 range with drawn parameters, max_diag = 0 and max_gap = 3 among them."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.integers(0, 10))
        L = rng.integers(1, 9, n)
        x = rng.integers(0, 31 - L)
        near = np.minimum(30 - L, x + rng.integers(0, 4, n))
        y = np.where(rng.integers(0, 3, n) > 0, near, rng.integers(0, 31 - L))
        p = params(int(rng.integers(1, 7)), int(rng.integers(0, 12)), int(rng.integers(0, 4)), int(rng.integers(0, 3)),
                   (NO_LIMIT, 3, 10, 0)[int(rng.integers(0, 4))], (NO_LIMIT, 0, 2, 7)[int(rng.integers(0, 4))], (9, 64, 1024)[int(rng.integers(0, 3))])
        out.append((canonical(np.stack([x, y, L], axis=1)), p))
    return out


def same(got_result, got_chain, want):
    return ({k: got_result[k] for k in ("score", "num_seeds", "last_anchor")} == {k: want[k] for k in ("score", "num_seeds", "last_anchor")}
            and [tuple(r) for r in np.asarray(got_chain).tolist()] == want["seeds"])


def check_call(engine, pairs, p, wants, what, **where):
    """One call of engine.chain_anchors against the references of its pairs: every field, seeds_off and every seed."""
    results, chains = engine.chain_anchors(pairs, sort=False, **p, **where)
    assert len(results) == len(chains) == len(pairs)
    off = 0
    for k, (r, c, w) in enumerate(zip(results, chains, wants)):
        assert r["seeds_off"] == off, (what, k, "seeds_off")
        assert same(r, c, w), (what, k, len(pairs[k]), r, w["score"], w["num_seeds"], w["last_anchor"])
        off += w["num_seeds"]


# ---- 1. chain_ref is pinned by the brute force ---------------------------------------------------------------------
def test_chain_ref_equals_the_brute_force_and_returns_chains():
    seen = set()
    for a, p in random_sets():
        res = chain_ref(a, **p)
        assert res["score"] == brute_force(a, p), (a.tolist(), p)  # (K3): lookback >= 9 >= the count
        assert is_chain_of(a, res), (a.tolist(), p, res)
        # the chain's own score, from the transitions the definition names
        total = p["match"] * int(a[res["indices"][0]][2]) if len(a) else 0
        for j, i in zip(res["indices"], res["indices"][1:]):
            value, o = transition(tuple(int(v) for v in a[j]), tuple(int(v) for v in a[i]), **p)
            total += value
        assert total == res["score"]
        seen.add((p["max_gap"], p["max_diag"]))
    assert {(3, 0), (NO_LIMIT, NO_LIMIT)} <= seen


def test_chain_ref_on_known_sets():
    # two anchors on one diagonal, the second overlapping the first by 3 letters: its tail of 7 joins
    res = chain_ref([(0, 0, 10), (7, 7, 10)], **params())
    assert res["score"] == 85 and res["seeds"] == [(0, 0, 10), (10, 10, 7)]
    # a diagonal change of 2 costs 11 + 2; of 0, nothing; and a predecessor that only equals starting anew is not taken
    assert chain_ref([(0, 0, 10), (12, 10, 10)], **params())["score"] == 100 - 13
    assert chain_ref([(0, 0, 10), (15, 15, 10)], **params())["score"] == 100
    res = chain_ref([(0, 0, 1), (2, 1, 4)], **params(gap_open=5))
    assert res["score"] == 20 and res["seeds"] == [(2, 1, 4)] and res["last_anchor"] == 1
    assert chain_ref([], **params()) == {"score": 0, "num_seeds": 0, "last_anchor": 0, "seeds": [], "indices": []}


# ---- 2. the host function equals chain_ref -------------------------------------------------------------------------
def test_the_host_function_equals_chain_ref_on_the_random_sets():
    from sa_amd import engine
    sets = random_sets()
    for a, p in sets:
        check_call(engine, [a], p, [chain_ref(a, **p)], "random set", host=True)
    # and many pairs in one call, empty ones among them, under one parameter set
    p = params(3, 4, 1, 1, 10, 7, 64)
    pairs = [a for a, _ in sets]
    check_call(engine, pairs, p, [chain_ref(a, **p) for a in pairs], "random sets in one call", host=True)


def test_the_host_function_equals_chain_ref_on_the_cases_of_the_gpu_file():
    from sa_amd import engine
    import test_chaining_gpu as g
    for name, pairs, p in g.all_cases():
        check_call(engine, pairs, p, g.refs(name, pairs, p), name, host=True)


def test_sort_puts_the_anchors_in_canonical_order():
    from sa_amd import engine
    rng = np.random.default_rng(97200)
    for a, p in random_sets(40, 97300):
        shuffled = a[rng.permutation(len(a))]
        r, c = engine.chain_anchors([shuffled], host=True, **p)
        assert same(r[0], c[0], chain_ref(a, **p))
        assert (engine.canonical_order(shuffled) == a).all()


# ---- 3. the identities ---------------------------------------------------------------------------------------------
def test_k1_every_output_is_a_chain_of_tails():
    from sa_amd import engine
    for a, p in random_sets(120, 97400):
        r, c = engine.chain_anchors([a], sort=False, host=True, **p)
        res = dict(r[0], seeds=[tuple(s) for s in c[0].tolist()])
        assert is_chain_of(a, res), (a.tolist(), p, res)


def test_k4_a_valid_chain_comes_back_unchanged():
    from sa_amd import engine
    rng = np.random.default_rng(97500)
    for k in range(40):
        n = int(rng.integers(1, 30))
        L = rng.integers(1, 20, n)
        gx, gy = rng.integers(0, 9, n) * rng.integers(0, 2, n), rng.integers(0, 9, n) * rng.integers(0, 2, n)
        x = np.cumsum(gx + L) - L
        y = np.cumsum(gy + L) - L
        chain = np.stack([x, y, L], axis=1)
        match = int(rng.integers(1, 9))
        p = params(match, 0, 0, 0, NO_LIMIT, NO_LIMIT, int(rng.integers(1, 5)))
        r, c = engine.chain_anchors([chain], sort=False, host=True, **p)
        assert r[0]["score"] == match * int(L.sum()) and r[0]["last_anchor"] == n - 1 and (c[0] == chain).all(), (k, chain.tolist())


def test_k5_neighbours_and_shifts_change_nothing():
    from sa_amd import engine
    sets = random_sets(60, 97600)
    p = params(4, 6, 1, 1, 10, NO_LIMIT, 64)
    pairs = [a for a, _ in sets]
    together, chains = engine.chain_anchors(pairs, sort=False, host=True, **p)
    for k, a in enumerate(pairs):
        alone, chain = engine.chain_anchors([a], sort=False, host=True, **p)
        assert {f: together[k][f] for f in ("score", "num_seeds", "last_anchor")} == {f: alone[0][f] for f in ("score", "num_seeds", "last_anchor")}
        assert (chains[k] == chain[0]).all()
        moved, mchain = engine.chain_anchors([a + np.array([1000, 77, 0])], sort=False, host=True, **p)
        assert {f: moved[0][f] for f in ("score", "num_seeds", "last_anchor")} == {f: alone[0][f] for f in ("score", "num_seeds", "last_anchor")}
        assert (mchain[0] == chain[0] + np.array([1000, 77, 0])).all()


# ---- 4. the C ABI --------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("sa_chain_anchors", "sa_chain_anchors_host", "sa_chain_set_seeds", "sa_chain_set_off", "sa_chain_set_destroy",
               "sa_chain_last_stats")


def plan_check_output():
    out = subprocess.run([os.path.join(PKG, "bin", "sa_chain_plan_check")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.strip().splitlines()


def test_the_plan_check_program_passes():
    assert plan_check_output()[-1] == "OK 300"


def test_the_library_exports_the_new_symbols_with_the_layout_of_the_header():
    from sa_amd import engine
    for name in NEW_SYMBOLS:
        assert name in engine.EXPORTS and hasattr(engine.lib, name), name
    assert engine.NO_LIMIT == NO_LIMIT and callable(engine.chain_anchors)
    assert engine.chain_last_stats().keys() == {"dp_ms", "walk_ms", "device_bytes"}
    sizes = dict(line.split()[1:] for line in plan_check_output() if line.startswith("sizeof "))
    assert int(sizes["sa_chain_params"]) == ctypes.sizeof(engine.SaChainParams) == 28
    assert int(sizes["sa_chain_result"]) == ctypes.sizeof(engine.SaChainResult) == 24
    assert [f for f, _ in engine.SaChainParams._fields_] == list(PARAMS)
    assert [(f, getattr(engine.SaChainResult, f).offset) for f, _ in engine.SaChainResult._fields_] == [
        ("score", 0), ("status", 4), ("seeds_off", 8), ("num_seeds", 16), ("last_anchor", 20)]
    from sa_amd import buildid
    names = {os.path.basename(f) for f in buildid.source_files()}
    assert {"sa_chain.hip", "sa_chain_plan.cpp", "sa_chain_plan.h", "chain_plan_check.cpp", "chaining_check.cpp"} <= names


# ---- 5. every refusal, by both functions, before the device --------------------------------------------------------
def call(engine, which, p, anchors, off, num_pairs=None, null=()):
    """The raw C call. `which`: "host", or a device number for sa_chain_anchors. Returns (status, message)."""
    cp = engine.SaChainParams(*[p[k] for k in PARAMS])
    a = np.ascontiguousarray(np.asarray(anchors, dtype=np.uint64).reshape(-1, 3))
    o = np.ascontiguousarray(off, dtype=np.uint64)
    n = len(o) - 1 if num_pairs is None else num_pairs
    res = (engine.SaChainResult * max(1, n))()
    handle = ctypes.c_void_p(0xDEAD)
    args = [None if "params" in null else ctypes.byref(cp), None if "anchors" in null else a.ctypes.data,
            None if "anchor_off" in null else o.ctypes.data, n]
    tail = [None if "results" in null else res, None if "out" in null else ctypes.byref(handle)]
    rc = engine.lib.sa_chain_anchors_host(*args, *tail) if which == "host" else engine.lib.sa_chain_anchors(*args, which, *tail)
    if "out" not in null and rc != 0:
        assert handle.value is None  # on failure *out stays NULL
    if rc == 0 and "out" not in null:
        engine.lib.sa_chain_set_destroy(handle)
    return rc, engine.lib.sa_last_error().decode()


TWO = [(0, 0, 4), (6, 6, 4)]
LIM = 2 ** 31 - 1
REFUSED = [
    # what, status, words of the message, params, anchors, anchor_off, nulls
    ("params null", INVALID, ("params",), {}, TWO, [0, 2], ("params",)),
    ("results null", INVALID, ("results",), {}, TWO, [0, 2], ("results",)),
    ("out null", INVALID, ("out",), {}, TWO, [0, 2], ("out",)),
    ("anchors null", INVALID, ("anchors",), {}, TWO, [0, 2], ("anchors",)),
    ("anchor_off null", INVALID, ("anchor_off",), {}, TWO, [0, 2], ("anchor_off",)),
    ("match 0", INVALID, ("match",), dict(match=0), TWO, [0, 2], ()),
    ("match 1025", INVALID, ("match",), dict(match=1025), TWO, [0, 2], ()),
    ("gap_open -1", INVALID, ("gap_open",), dict(gap_open=-1), TWO, [0, 2], ()),
    ("gap_open 2^20 + 1", INVALID, ("gap_open",), dict(gap_open=2 ** 20 + 1), TWO, [0, 2], ()),
    ("gap_extend -1", INVALID, ("gap_extend",), dict(gap_extend=-1), TWO, [0, 2], ()),
    ("gap_extend 2^20 + 1", INVALID, ("gap_extend",), dict(gap_extend=2 ** 20 + 1), TWO, [0, 2], ()),
    ("skip -1", INVALID, ("skip",), dict(skip=-1), TWO, [0, 2], ()),
    ("skip 2^20 + 1", INVALID, ("skip",), dict(skip=2 ** 20 + 1), TWO, [0, 2], ()),
    ("max_gap -1", INVALID, ("max_gap",), dict(max_gap=-1), TWO, [0, 2], ()),
    ("max_diag -1", INVALID, ("max_diag",), dict(max_diag=-1), TWO, [0, 2], ()),
    ("lookback 0", INVALID, ("lookback",), dict(lookback=0), TWO, [0, 2], ()),
    ("lookback 1025", INVALID, ("lookback",), dict(lookback=1025), TWO, [0, 2], ()),
    ("anchor_off[0] != 0", INVALID, ("anchor_off[0]",), {}, TWO, [1, 2], ()),
    ("anchor_off decreases", INVALID, ("anchor_off", "pair 1"), {}, TWO, [0, 2, 1], ()),
    ("L == 0", INVALID, ("pair 1", "anchor 1", "length 0"), {}, [(1, 1, 1), (0, 0, 4), (6, 6, 0)], [0, 1, 3], ()),
    ("text end out of order", INVALID, ("pair 1", "anchor 2", "order"), {}, [(1, 1, 1), (0, 0, 4), (6, 6, 4), (5, 9, 4)], [0, 1, 4], ()),
    ("pattern end out of order", INVALID, ("pair 0", "anchor 1", "order"), {}, [(2, 6, 4), (2, 5, 4)], [0, 2], ()),
    ("length out of order", INVALID, ("pair 0", "anchor 1", "order"), {}, [(2, 2, 4), (3, 3, 3)], [0, 2], ()),
    ("x + L at 2^31 - 1", UNSUPPORTED, ("pair 0", "anchor 1", "text", "2^31 - 1"), {}, [(0, 0, 4), (LIM - 4, 6, 4)], [0, 2], ()),
    ("y + L at 2^31 - 1", UNSUPPORTED, ("pair 0", "anchor 1", "pattern", "2^31 - 1"), {}, [(0, 0, 4), (6, LIM - 4, 4)], [0, 2], ()),
    ("x beyond 64 bits less L", UNSUPPORTED, ("pair 0", "anchor 0", "2^31 - 1"), {}, [(2 ** 64 - 2, 0, 4)], [0, 1], ()),
    ("match sum(L) at 2^30", UNSUPPORTED, ("pair 1", "2^30"), dict(match=1024), [(0, 0, 1), (0, 0, 2 ** 19), (2 ** 19, 2 ** 19, 2 ** 19)], [0, 1, 3], ()),
]


@pytest.mark.parametrize("which", ["host", 0, 1 << 20])
def test_refusals_name_the_pair_and_the_anchor_and_precede_the_device(which):
    from sa_amd import engine
    fn = "sa_chain_anchors_host: " if which == "host" else "sa_chain_anchors: "
    for what, status, words, kw, anchors, off, null in REFUSED:
        rc, msg = call(engine, which, params(**kw), anchors, off, null=null)
        assert rc == status and msg.startswith(fn) and all(w in msg for w in words), (what, rc, msg)
    rc, msg = call(engine, which, params(), TWO, [0, 2], num_pairs=-1)
    assert rc == INVALID and "num_pairs" in msg
    # the limits themselves pass: one below 2^31 - 1, and match sum(L) = 2^30 - 1024
    if which == "host":
        assert call(engine, which, params(), [(0, 0, 4), (LIM - 5, 6, 4)], [0, 2])[0] == 0
        assert call(engine, which, params(match=1024), [(0, 0, 2 ** 19), (2 ** 19, 2 ** 19, 2 ** 19 - 1)], [0, 2])[0] == 0
        assert call(engine, which, params(), [(0, 0, 0)], [0], num_pairs=0)[0] == 0  # no pairs: nothing to do
    if which == 1 << 20:
        # a device that no machine has: a call that passes the checks reaches the device and fails there
        assert call(engine, which, params(), TWO, [0, 2])[0] == HIP


def test_the_binding_refuses_what_it_can_see():
    from sa_amd import engine
    with pytest.raises(ValueError):
        engine.chain_anchors([[(0, -1, 3)]], 5, 11, 2, host=True)
    with pytest.raises(engine.SaError) as e:
        engine.chain_anchors([[(6, 6, 4), (0, 0, 4)]], 5, 11, 2, host=True, sort=False)
    assert e.value.code == INVALID and "pair 0, anchor 1" in str(e.value)
    r, c = engine.chain_anchors([], 5, 11, 2, host=True)
    assert r == [] and c == []
    r, c = engine.chain_anchors([[], []], 5, 11, 2, host=True)
    assert [x["num_seeds"] for x in r] == [0, 0] and all(x.shape == (0, 3) for x in c)
