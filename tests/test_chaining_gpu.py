"""Chaining on the device (sa_hip.h: sa_chain_anchors): chain_dp_kernel and chain_walk_kernel against chain_ref of
tests/test_chaining_plan.py, exactly, on score, num_seeds, last_anchor, seeds_off and every seed. The cases are
built here once per process and shared with the CPU file, which runs the host function over them; each aims at one
place where the kernels can go wrong: the 64-lane rounds and 64-anchor blocks, the ring's wrap, the trimming, the
limits, the tie rules, saturating costs, the walk's length and the work draw. Then the chain goes into chains= end
to end, and the C++ function is checked by bin/sa_chaining_check."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, matrix  # first: it puts oracle/ and the package on the path

from sa_amd import synthetic
from test_chaining_plan import NO_LIMIT, canonical, chain_ref, check_call, params

gpu = pytest.mark.gpu
GLOBAL = 0


# ---- the cases -----------------------------------------------------------------------------------------------------
def noisy_path(rng, count):
    """`count` anchors in canonical order: a path of exact matches with steps along its diagonal, diagonal changes and
    overlaps with the anchor before, duplicates, and hits off the path."""
    out, x, y = [], int(rng.integers(0, 50)), int(rng.integers(0, 50))
    while len(out) < count:
        L, roll = int(rng.integers(1, 25)), int(rng.integers(0, 16))
        if roll == 0 and out:
            out.append(out[-1])
        elif roll < 3:
            out.append((int(rng.integers(0, x + 200)), int(rng.integers(0, y + 200)), L))
        else:
            out.append((x, y, L))
            step = int(rng.integers(0, 8))
            x, y = x + L + step, y + L + step
            if roll == 3:
                x += int(rng.integers(1, 31))
            elif roll == 4:
                y += int(rng.integers(1, 31))
            elif roll == 5:
                x, y = x - min(L + step, int(rng.integers(1, 7))), y - min(L + step, int(rng.integers(1, 7)))
    return canonical(out)


def diagonal(count, L=3, step=0, x=5, y=9):
    """`count` anchors of length L on one diagonal, `step` letters between them."""
    k = np.arange(count) * (L + step)
    return np.stack([x + k, y + k, np.full(count, L)], axis=1).astype(np.int64)


def lookback_boundary(between):
    """A first anchor, `between` anchors that neither it nor the last can join, and a last one that only the first can
    precede: the last finds it iff lookback > between."""
    far = [(10, 5000 + q, 1) for q in range(between)]
    return np.array([(0, 0, 10)] + far + [(12, 12, 10)], dtype=np.int64)


def counts_case():
    rng = np.random.default_rng(98100)
    pairs = []
    for n in (0, 1, 2, 63, 64, 65, 128, 129, 1500):
        pairs += [noisy_path(rng, n), np.zeros((0, 3), np.int64)]
    return [("counts", pairs, params())]


def lookback_cases():
    rng = np.random.default_rng(98200)
    out = []
    for lb in (1, 63, 64, 65, 128, 1024):
        few, many = max(1, lb - 1 - lb // 3), 2 * lb + 37
        pairs = [noisy_path(rng, few), noisy_path(rng, many), diagonal(many, 2, 1)]
        pairs += [lookback_boundary(b) for b in (lb - 2, lb - 1, lb) if b >= 0]
        out.append((f"lookback {lb}", pairs, params(lookback=lb)))
        # a window that gaps cannot leave: the rounds the order lets the kernel skip
        out.append((f"lookback {lb}, max_gap 40", pairs, params(3, 4, 1, 1, 40, 12, lb)))
    return out


def trimming_case():
    first = (0, 0, 10)
    pairs = [[first, (7, 12, 10)],   # the text axis alone cuts 3
             [first, (12, 7, 10)],   # the pattern axis alone
             [first, (7, 8, 10)],    # both, 3 and 2
             [first, (1, 1, 10)],    # o = L - 1: one letter is left
             [first, (0, 1, 10)],    # o = L: not admissible, the second starts anew
             [first, (7, 7, 10), (14, 14, 10), (21, 22, 10)]]
    pairs = [np.array(p, dtype=np.int64) for p in pairs]
    return [("trimming, zero costs", pairs, params(5, 0, 0, 0)), ("trimming, 5 / 11 / 2", pairs, params()),
            ("trimming, match 1 and a skip cost", pairs, params(1, 1, 1, 1))]


def limits_case():
    first = (0, 0, 5)
    pairs = [[first, (5 + g, 5 + g, 5)] for g in (6, 7, 8)]                        # dx = dy = g about max_gap = 7
    pairs += [[first, (5 + 7, 5 + 4, 5)], [first, (5 + 8, 5 + 5, 5)]]              # dx alone at and beyond it
    pairs += [[first, (5 + 4, 5 + 7, 5)], [first, (5 + 5, 5 + 8, 5)]]              # dy alone
    pairs += [[first, (5 + d, 5, 5)] for d in (2, 3, 4)]                           # dd about max_diag = 3, on the text axis
    pairs += [[first, (5 + 1, 5 + 1 + d, 5)] for d in (2, 3, 4)]                   # and on the pattern axis
    pairs += [[first, (5, 5, 5)]]                                                  # max_gap = 0 would still take this one
    pairs = [canonical(p) for p in pairs]
    return [("limits 7 / 3", pairs, params(5, 1, 1, 0, 7, 3)), ("limits 0 / 0", pairs, params(5, 1, 1, 0, 0, 0)),
            ("no limits", pairs, params(5, 1, 1, 0))]


def ties_case():
    pairs = [[(0, 0, 3), (1, 0, 3), (6, 6, 3)],                   # two predecessors of equal value: the nearest wins
             [(0, 0, 3), (1, 0, 3), (2, 0, 3), (6, 6, 3)],        # three
             [(0, 0, 3), (20, 20, 3), (40, 40, 3)],               # under max_gap 5: three ends of equal f, the lowest wins
             [(2, 2, 3)] * 3,                                     # duplicates: none can follow its twin
             [(0, 0, 3), (0, 0, 3), (3, 3, 4), (3, 3, 4), (3, 3, 4)]]  # the later twin precedes, the earliest end wins
    pairs = [canonical(p) for p in pairs]
    anew = [canonical([(0, 0, 1), (2, 1, 4)])]                    # f(0) + value = 5 + 20 - 5 = 20 = match L: start anew
    return [("ties, zero costs", pairs, params(1, 0, 0, 0, 5)), ("a predecessor that equals starting anew", anew, params(5, 5, 2))]


def large_values_case():
    rng = np.random.default_rng(98300)
    # diagonal changes in the thousands under gap_extend = 2^20: every such cost saturates
    far = canonical([(0, 0, 20), (20, 4000, 30), (3000, 50, 25), (3030, 4030, 9), (9000, 4100, 12), (9012, 9000, 40)])
    mixed = np.concatenate([noisy_path(rng, 150), far + np.array([400, 400, 0])])
    heavy = diagonal(4, 262143)  # match sum(L) = 1024 * 1048572: 4096 below 2^30
    return [("gap_extend 2^20", [far, canonical(mixed)], params(5, 2 ** 20, 2 ** 20, 2 ** 20, NO_LIMIT, NO_LIMIT, 256)),
            ("match 1024 just under the limit", [heavy, heavy[:1]], params(1024, 2 ** 20, 2 ** 20))]


def walk_case():
    zero = [diagonal(n) for n in (1, 64, 65, 1000)]
    real = [diagonal(1000, 4, 2), canonical(np.concatenate([diagonal(1000, 4, 2), diagonal(300, 5, 7, 900, 100)]))]
    return [("a diagonal under zero costs", zero, params(2, 0, 0, 0, NO_LIMIT, NO_LIMIT, 1)), ("a chain of 1000", real, params())]


def draw_case():
    rng = np.random.default_rng(98400)
    return [("3000 small pairs", [noisy_path(rng, int(rng.integers(0, 6))) for _ in range(3000)], params(lookback=3))]


GROUPS = {"counts": counts_case, "lookback": lookback_cases, "trimming": trimming_case, "limits": limits_case, "ties": ties_case,
          "large values": large_values_case, "walk": walk_case, "draw": draw_case}
_CASES, _REFS = {}, {}


def cases(group):
    if group not in _CASES:
        _CASES[group] = GROUPS[group]()
    return _CASES[group]


def all_cases():
    return [c for group in GROUPS for c in cases(group)]


def refs(name, pairs, p):
    """chain_ref of every pair of a case, computed once per process and left unchanged."""
    if name not in _REFS:
        _REFS[name] = [chain_ref(a, **p) for a in pairs]
    return _REFS[name]


# ---- 1. the cases are what they say (CPU) --------------------------------------------------------------------------
def test_the_cases_have_their_shapes():
    (_, pairs, _), = cases("counts")
    assert [len(a) for a in pairs] == [0, 0, 1, 0, 2, 0, 63, 0, 64, 0, 65, 0, 128, 0, 129, 0, 1500, 0]
    for name, pairs, p in cases("lookback"):
        lb = p["lookback"]
        assert len(pairs[0]) < lb or lb == 1
        assert len(pairs[1]) > 2 * lb and len(pairs[2]) > 2 * lb
        if p["max_gap"] == NO_LIMIT:
            # the boundary pairs: the last anchor joins the first iff lookback reaches it
            for a, want in zip(pairs[3:], refs(name, pairs, p)[3:]):
                assert want["num_seeds"] == (2 if len(a) - 1 <= lb else 1), (name, len(a))
    name, pairs, p = cases("trimming")[0]
    want = refs(name, pairs, p)
    # pair 4: neither anchor can follow the other, two ends of equal f, and the lower index wins
    assert [w["seeds"][-1] for w in want[:5]] == [(10, 15, 7), (15, 10, 7), (10, 11, 7), (10, 10, 1), (0, 0, 10)]
    assert [w["num_seeds"] for w in want] == [2, 2, 2, 2, 1, 4]
    name, pairs, p = cases("limits")[0]
    assert [w["num_seeds"] for w in refs(name, pairs, p)] == [2, 2, 1, 2, 1, 2, 1, 2, 2, 1, 2, 2, 1, 2]
    name, pairs, p = cases("limits")[1]
    assert [w["num_seeds"] for w in refs(name, pairs, p)] == [1] * 13 + [2]
    name, pairs, p = cases("ties")[0]
    want = refs(name, pairs, p)
    assert want[0]["indices"] == [1, 2] and want[1]["indices"] == [2, 3] and want[2]["indices"] == [0]
    assert want[3]["indices"] == [0] and want[4]["indices"] == [1, 2]
    name, pairs, p = cases("ties")[1]
    assert refs(name, pairs, p)[0]["indices"] == [1]
    name, pairs, p = cases("large values")[0]
    assert refs(name, pairs, p)[0]["num_seeds"] == 1 and refs(name, pairs, p)[0]["score"] == 200  # every join saturates: the longest anchor alone
    name, pairs, p = cases("large values")[1]
    assert refs(name, pairs, p)[0]["score"] == 1024 * 1048572 == 2 ** 30 - 4096
    name, pairs, p = cases("walk")[0]
    assert [w["num_seeds"] for w in refs(name, pairs, p)] == [1, 64, 65, 1000]
    assert all(w["seeds"] == [tuple(r) for r in a.tolist()] for w, a in zip(refs(name, pairs, p), pairs))  # (K4)
    name, pairs, p = cases("walk")[1]
    assert [w["num_seeds"] >= 1000 for w in refs(name, pairs, p)] == [True, True]


# ---- 2. the device equals chain_ref --------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_the_device_equals_chain_ref(eng, group):
    for name, pairs, p in cases(group):
        check_call(eng, pairs, p, refs(name, pairs, p), name, device=0)
    stats = eng.chain_last_stats()
    assert stats["dp_ms"] > 0 and stats["device_bytes"] > 0


@gpu
def test_k5_on_the_device_a_pair_alone_and_among_others(eng):
    (name, pairs, p), = cases("counts")
    want = refs(name, pairs, p)
    for k in (6, 10, 16):  # 63, 65 and 1500 anchors
        check_call(eng, [pairs[k]], p, [want[k]], f"{name}, pair {k} alone", device=0)
        moved = pairs[k] + np.array([1000, 77, 0])
        r, c = eng.chain_anchors([moved], sort=False, device=0, **p)
        assert r[0]["score"] == want[k]["score"] and [tuple(s) for s in c[0].tolist()] == [(x + 1000, y + 77, L) for x, y, L in want[k]["seeds"]]


# ---- 3. end to end: anchors, the chain, and the chain in chains= ---------------------------------------------------
def read_cases():
    """Four pairs: a 300-letter text with a planted 40-letter repeat and a read made by synthetic.mutate; the last read
    without insertions or deletions."""
    out = []
    for k in range(4):
        t = synthetic.random_sequence(98500 + k, 300, 4)
        t[180:220] = t[60:100]
        p = synthetic.mutate(t, 98600 + k, 4, None, p_del=0.0 if k == 3 else 0.05)
        out.append((t, p))
    return out


def test_the_read_cases_have_anchors_off_the_path():
    for k, (t, p) in enumerate(read_cases()):
        a = synthetic.kmer_anchors(t, p, 6)
        assert len(a) >= 10 and (np.diff(a[:, 0] + a[:, 2]) >= 0).all()
        assert all((t[x:x + L] == p[y:y + L]).all() for x, y, L in a.tolist())
        assert (np.abs(a[:, 0] - a[:, 1]) >= 100).any(), k  # the repeat's hits
    assert len(read_cases()[3][1]) == 300


@gpu
def test_the_chain_goes_into_chains_end_to_end(eng):
    from test_align_affine_gpu import pick
    from test_chains_gpu import chains_ref
    S = matrix("blast", 4)
    reads = read_cases()
    anchors = [synthetic.kmer_anchors(t, p, 6) for t, p in reads]
    p = params(5, 11, 2)
    results, chains = eng.chain_anchors(anchors, device=0, **p)
    for k, a in enumerate(anchors):
        want = chain_ref(a, **p)
        assert results[k]["score"] == want["score"] and [tuple(s) for s in chains[k].tolist()] == want["seeds"], k
        assert results[k]["num_seeds"] >= 5
    assert (chains[3][:, 0] == chains[3][:, 1]).all()  # no indels: every seed on diagonal 0
    texts, patterns = [t for t, _ in reads], [q for _, q in reads]
    got = eng.align_pairs_affine(GLOBAL, texts, patterns, S, 11, 2, xdrop=eng.NO_XDROP, chains=chains)
    for k, g in enumerate(got):
        assert pick(g) == pick(chains_ref(texts[k], patterns[k], chains[k].tolist(), S, 11, 2, None)), k


# ---- 4. the C++ function -------------------------------------------------------------------------------------------
@gpu
def test_cpp_chaining():
    out = subprocess.run([os.path.join(PKG, "bin", "sa_chaining_check"), "300", "96"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1] == "OK 96"
