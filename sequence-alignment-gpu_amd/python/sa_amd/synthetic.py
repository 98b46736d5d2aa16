"""Deterministic synthetic inputs for the benchmark configs.

* ``random_sequence(seed, n, A)``: i.i.d. letters ``(splitmix64_k >> 33) % A`` where splitmix64_k is
  the k-th output of a splitmix64 stream seeded with ``seed`` (k = 1, 2, ...). The same stream is
  implemented in C in ``oracle/ref_driver.cpp`` (``fillbench``) so both sides see identical inputs.
* ``mutate(seq, seed, A, length)``: a vectorised restatement of the reference's ``mutate.py:4-59``
  mutation model — per source letter 5 % deletion, else 2 % replacement by a random letter (the
  reference's "insertion" branch emits a random letter in place of the source letter,
  ``mutate.py:50-52``), else 5 % substitution by a different letter — then trimmed / padded with
  random letters to ``length``. Draws come from splitmix64 (4 per source letter), not Python's
  ``random``, so results are reproducible across hosts.
"""
from __future__ import annotations

import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def splitmix64(seed: int, count: int, offset: int = 0) -> np.ndarray:
    """Outputs k = offset+1 .. offset+count of a splitmix64 stream (uint64 array)."""
    with np.errstate(over="ignore"):
        k = np.arange(offset + 1, offset + count + 1, dtype=np.uint64)
        z = np.uint64(seed) + k * GOLDEN
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def random_sequence(seed: int, n: int, A: int = 4) -> np.ndarray:
    """Alphabet-index sequence (int8) of length n."""
    return ((splitmix64(seed, n) >> np.uint64(33)) % np.uint64(A)).astype(np.int8)


def _uniform(seed: int, count: int, offset: int = 0) -> np.ndarray:
    return (splitmix64(seed, count, offset) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def mutate(seq: np.ndarray, seed: int, A: int = 4, length: int | None = None,
           p_del: float = 0.05, p_ins: float = 0.02, p_sub: float = 0.05) -> np.ndarray:
    seq = np.asarray(seq, dtype=np.int64)
    n = len(seq)
    u = _uniform(seed, 4 * n).reshape(n, 4) if n else np.zeros((0, 4))
    dele = u[:, 0] < p_del
    ins = ~dele & (u[:, 1] < p_ins)
    sub = ~dele & ~ins & (u[:, 2] < p_sub)
    out = seq.copy()
    out[ins] = np.minimum((u[ins, 3] * A).astype(np.int64), A - 1)
    shift = 1 + np.minimum((u[sub, 3] * (A - 1)).astype(np.int64), A - 2)
    out[sub] = (seq[sub] + shift) % A
    out = out[~dele]
    if length is not None:
        if len(out) >= length:
            out = out[:length]
        else:
            pad = random_sequence(seed ^ 0x5EED, length - len(out), A).astype(np.int64)
            out = np.concatenate([out, pad])
    return out.astype(np.int8)


def blast_matrix() -> np.ndarray:
    """scoreMatrices/dna/blast.txt of the reference: +5 match / -4 mismatch (4x4, row-major)."""
    S = np.full((4, 4), -4, dtype=np.int32)
    np.fill_diagonal(S, 5)
    return S


def kmer_anchors(text: np.ndarray, pattern: np.ndarray, k: int) -> np.ndarray:
    """The maximal exact-match diagonal runs of length >= k between `text` and `pattern`, every diagonal and every
    repeat, as an (A, 3) int64 array of (text_pos, pattern_pos, length) in the canonical order
    engine.chain_anchors wants: non-decreasing (text end, pattern end, length). A helper for the tests and the
    chaining bench, in numpy on the host (memory grows with the number of k-mer hits): it stands in for a seeder
    and is not one for users."""
    t, p = np.asarray(text, dtype=np.int64), np.asarray(pattern, dtype=np.int64)
    none = np.zeros((0, 3), np.int64)
    if k < 1 or len(t) < k or len(p) < k:
        return none
    win = np.lib.stride_tricks.sliding_window_view
    words = np.concatenate([win(t, k), win(p, k)])
    base = int(max(t.max(), p.max())) + 1
    if min(t.min(), p.min()) >= 0 and base ** k < 2 ** 62:
        ident = words @ (base ** np.arange(k - 1, -1, -1, dtype=np.int64))  # the k-mer as a number in that base: exact
    else:
        ident = np.unique(words, axis=0, return_inverse=True)[1].ravel()    # equal k-mers, equal numbers
    ti, pi = ident[: len(t) - k + 1], ident[len(t) - k + 1:]
    by = np.argsort(ti, kind="stable")
    lo, hi = np.searchsorted(ti[by], pi, "left"), np.searchsorted(ti[by], pi, "right")
    hits = hi - lo
    if hits.sum() == 0:
        return none
    i = np.repeat(np.arange(len(pi)), hits)                                   # pattern position of every k-mer hit
    j = by[np.repeat(lo, hits) + np.arange(hits.sum()) - np.repeat(np.cumsum(hits) - hits, hits)]  # its text position
    o = np.lexsort((j, j - i))                                                # along each diagonal
    i, j = i[o], j[o]
    start = np.ones(len(i), bool)
    start[1:] = (np.diff(j - i) != 0) | (np.diff(j) != 1)
    first = np.flatnonzero(start)
    length = np.diff(np.append(first, len(i))) + k - 1
    a = np.stack([j[first], i[first], length], axis=1).astype(np.int64)
    return a[np.lexsort((a[:, 2], a[:, 1] + a[:, 2], a[:, 0] + a[:, 2]))]
