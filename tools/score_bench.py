#!/usr/bin/env python3
"""Score-only path against the plan path, on one GPU (fails without one).

For each workload, in one process, after a warm-up and alternated round by round, timed with device
events around steps that end in a synchronise:
  (a) Scorer.run                      scores and scored cells, no planes
  (b) Plan.fill alone, and Plan.fill + Plan.traceback: the only way to the same scores without (a)
and the scores of (a) and (b) are asserted equal at the timed size. Then the forced rows-per-lane
sweep of the scorer (the numbers behind the automatic rule).

Workloads: `batch` 4096 pairs of 2048 x 2048 DNA, global (bench.py's batch config); `search` one
512-letter protein query, local, against 20000 seeded texts of 64..2048 letters.

With --gap-extend E the comparison is another one: the affine scorer (gap open --gap-open, gap extend
E; sa_scorer_create_affine) against the linear scorer of the same workload, Scorer.run of the two
alternated round by round in the same process, then the forced rows-per-lane sweep of the affine
scorer. The report holds the measured affine / linear ratio of the medians next to the ratio of the
planner's step-cost model. The plan path is not run.

With --gap-extend E --hits K the search workload alone: the affine Scorer.run beside search(k=K,
gap_extend=E) end to end, the device time of its traced fill and of its walk, and the
linear search(k=K) of the same data. With --hits K alone, the linear search(k=K) alone; --tree DIR
takes the package and library from another built checkout, which is how the parent commit's figure of
DESIGN.md 3.5 was taken.

With --mode fit the fit scorers (sa_hip.h: SA_FIT): a read-mapping workload, 40000 DNA reads of 140
to 160 letters, each a mutated piece of its own text window of 450 to 750 letters. The fit, global and
local scorers run on the same pairs, alternated round by round in one process after a warm-up, once
under the linear gap 5 and once under gap open 11 / gap extend 2. The report holds each median with its
min and max, the fit / global and fit / local ratios of the medians beside the ratios of the planner's
step-cost model, and whether the fit median is within the local median plus the local scorer's own
min-max spread. Then search(k = --hits, default 100) in fit and in local mode on the search workload
under 11 / 2, with the device times of the traced fill and of the walk.

With --mode ends the ends-free scorers (sa_hip.h: SA_ENDS_FREE): the read-mapping workload of --mode
fit, and an overlap workload, 40000 pairs of DNA reads of 140 to 160 letters in which the last 30 to 120
letters of each text are a mutated copy of the first letters of its pattern. On each workload, once under
the linear gap 5 and once under gap open 11 / gap extend 2, the scorers of SA_OVERLAP, SA_ENDS_FREE | TB |
PE, SA_ENDS_FREE | TB | TE, SA_ENDS_FREE alone, SA_FIT and SA_GLOBAL run alternated round by round in one
process after a warm-up (device events; median, min and max). The results of SA_ENDS_FREE | TB | TE and
SA_FIT, and of SA_ENDS_FREE alone and SA_GLOBAL, are asserted equal on every workload and gap. Each
ends-free mode is compared with the existing mode whose program it runs, SA_FIT when the text's end is
free and SA_GLOBAL otherwise: the report holds the ratio of the medians and whether the median lies
within the baseline's median plus the baseline's own min-max spread of the same run. With --tree DIR (a
built checkout without the modes, e.g. the parent commit) only SA_FIT and SA_GLOBAL run, on the same data:
the figures the existing modes are compared with across the two libraries.

With --mode extend the extension scorers and aligner (sa_hip.h: sa_scorer_create_extend,
sa_align_pairs_extend). Same work: on the read-mapping workload of --mode fit the extension scorer without
a drop beside the local scorer, whose program it runs, under the linear gap 5 and under 11 / 2, alternated
round by round (7 rounds unless --rounds says otherwise); the report says whether the extension's median
lies inside the local scorer's own min-max spread. The early exit: 2048 DNA pairs of 20000 letters, each
pattern a 5 %-mutated copy of its text for its first quarter and unrelated letters after, under gap open
16 / gap extend 4 (--exit-gap; under 11 / 2 and under the linear gap 5 unrelated DNA letters score upwards
against +5 / -4, about 0.2 a row, and no X-drop ever stops them): the extension scorer at X-drop 100, the extension scorer without a drop and the local scorer, alternated;
beside the measured ratio the model's, strips run over strips in all at the planned rows per lane, from
the stop rows of a row-by-row numpy reference on a 16-pair subsample, whose results the scorers' must
equal. Then sa_align_pairs_extend on 64 of these pairs at X-drop 100 and without a drop: the device time
of the traced fill and of the walk (sa_affine_last_stats).

With --mode seeds the seeds scorer and aligner (sa_hip.h: sa_scorer_create_seeds, sa_align_pairs_seeds) on the
reads of --mode mapped, each pair's seed the longest run of matching columns of its SA_FIT alignment under
11 / 2, computed once on the host. Under gap 5 / 5 and 11 / 2, without a drop and at --xdrop, alternated round
by round (7 rounds): (a) the seeds scorer, (b) two extension scorers over pre-reversed and sliced arenas of the
same halves, run one after the other (the same cells and the same programs: the yardstick), (c) the unbanded
SA_FIT scorer (under 5 / 5 the linear one, beside the linear kernels the others then run); the seeded scores are asserted equal to the composition of (b) at the timed size, and the
report holds (a) / (b) with (b)'s own min-max spread and (a) / (c) beside the ratio of the planner's step
costs. A second table has each window clipped to the read's span +- 32 letters. Then align_pairs_affine(seeds=)
end to end on 4000 of the pairs beside the two-call host composition, whose strings it must equal.

With --mode chain the chains scorer and aligner (sa_hip.h: sa_scorer_create_chains, sa_align_pairs_chains): 2048
DNA reads, each its own 10000-letter text mutated with substitutions and deletions so that its path drifts by
some hundred diagonals. A read's chain is the exact-match runs of at least 15 columns of its banded global
alignment under 11 / 2, computed once and cached under bench_out/. Alternated round by round after a warm-up (7
rounds, device events, median with min and max): (a) the chains scorer; (b) the composition of existing calls on
host-sliced pieces, one extension scorer per end and one affine global scorer over all gap rectangles as
separate pairs (the same cells and programs: the yardstick), whose sum with the seeds' scores the chained scores
are asserted equal to at the timed size; (c) the band-at global scorer on the narrowest band per pair that holds
the chain's diagonals +- 16, the alternative a caller has without chains. Beside each measured ratio the
planner's step-model ratio, and the mean shape of a gap piece with what the model charges for it. Then (d)
align_pairs_affine(chains=) on 64 of the pairs beside bands= with (c)'s bands: arena bytes, chunks, fill, walk
and end-to-end wall time.
    python3 tools/score_bench.py --mode chain [--small] --out profiles/r22/score_chain_bench.json
    python3 tools/score_bench.py [--out profiles/r09/score_bench.json] [--rounds 5] [--small]
With --mode cigar the CIGAR output (sa_hip.h: sa_align_pairs_cigar): align_pairs_affine with strings and
align_pairs_cigar with the same keywords, alternated in one process, on the long reads of --mode chain with their
chains (all 2048, and the first 64) and on the first 4000 reads of --mode mapped with their seeds: wall time end to
end, the device times of the fill, the walks and the encoder, and the bytes each call copies to the host.
    python3 tools/score_bench.py --mode cigar [--small] --out profiles/r23/score_cigar_bench.json

With --mode chaining the chaining (sa_hip.h: sa_chain_anchors) on the long reads of --mode chain, their anchors the
maximal exact matches of at least k = 11 and k = 15 letters (synthetic.kmer_anchors), under 5 / gap-open / gap-extend,
max_diag 500 and lookback 64: (a) the C call end to end, with the device time of its two kernels, against
sa_chain_anchors_host on the same anchors, alternated round by round, on all reads and on the first 64; (b) the chains
scorer on these chains and on the alignment-derived ones of --mode chain, pair by pair.
    python3 tools/score_bench.py --mode chaining [--small] [--out profiles/r24/score_chaining_bench.json]
With --mode extend --width W.. the banded extension (sa_hip.h: sa_scorer_create_extend_band,
sa_align_pairs_extend_band) on the chimeric pairs under --exit-gap, without a drop and at --xdrop: per X, the
unbanded extension scorer and, per width, the banded extension scorer and the band-at global scorer on {-w, w},
which covers the same cells; alternated round by round after a warm-up, medians with min and max, the planner's
step-model ratio beside each measured ratio, and the number of scores that equal the unbanded ones. Then the
aligners on 64 of the pairs: arena bytes, fill and walk ms of sa_affine_last_stats and end-to-end wall time.
With --mode seeds --width W.. the banded seeds scorer (sa_scorer_create_seeds_band) on the mapped reads with their
longest-match seeds beside the unbanded seeds scorer on the whole windows and on the windows clipped to the
read's span +- 32, the share of equal scores, and sa_align_pairs_seeds_band on 4000 of the reads.
    python3 tools/score_bench.py --mode extend --width 64 500 --out profiles/r21/score_extend_band_bench.json
    python3 tools/score_bench.py --mode seeds --width 16 64 --out profiles/r21/score_seeds_band_bench.json
    python3 tools/score_bench.py --mode seeds [--small] --out profiles/r18/score_seeds_bench.json
    python3 tools/score_bench.py --mode extend [--small] --out profiles/r17/score_extend_bench.json
    python3 tools/score_bench.py --mode ends [--small] --out profiles/r15/score_ends_bench.json
    python3 tools/score_bench.py --mode ends --tree ../parent --out profiles/r15/score_ends_bench_parent.json
With --band W [W ...] the banded scorer and aligner (sa_hip.h: sa_scorer_create_banded,
sa_align_pairs_banded): related pairs of about 20000 DNA letters, each pattern its text with 5 %
substitutions and 0.1 % deletions, under gap open / gap extend. Scorer.run of the unbanded affine scorer
and of the banded one at each W, alternated round by round after a warm-up (device events; median, min
and max), the measured banded / unbanded ratio of the medians beside the planner's (band steps over
full steps, each at its planned rows per lane); then align_pairs_affine with and without the band on the
first pairs (device time of the traced fill and of the walk, sa_affine_last_stats). On a subsample the
unbanded alignments' paths are read back from their strings: no banded score may exceed the unbanded
one, and where the path stays inside the band the two must be equal.

    python3 tools/score_bench.py --band 64 500 [--small] --out profiles/r14/score_band_bench.json
    python3 tools/score_bench.py --mode fit [--small] --out profiles/r13/score_fit_bench.json
    python3 tools/score_bench.py --gap-extend 2 [--gap-open 11] --out profiles/r10/score_affine_bench.json
    python3 tools/score_bench.py --gap-extend 2 --hits 100 --out profiles/r12/score_affine_hits.json
    python3 tools/score_bench.py --hits 100 --tree ../parent --out profiles/r12/parent_linear_search.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "sequence-alignment-gpu_amd", "python"))


def blosum50():
    with open(os.path.join(ROOT, "tests", "golden", "matrices.json")) as f:
        return np.array(json.load(f)["blosum50"], dtype=np.int32).reshape(23, 23)


def workloads(small: bool, search_only: bool = False):
    from sa_amd import synthetic
    if not search_only:
        npairs, side = (256, 2048) if small else (4096, 2048)
        ta = synthetic.random_sequence(1, npairs * side, 4)
        pa = synthetic.mutate(ta, 2, 4, npairs * side)
        yield {"name": "batch", "mode": 0, "S": synthetic.blast_matrix(), "gap": 5, "text": ta, "pattern": pa,
               "pairs": [(k * side, side, k * side, side) for k in range(npairs)]}
    ntexts = 2000 if small else 20000
    rng = np.random.default_rng(9)
    lens = rng.integers(64, 2049, ntexts)
    offs = np.concatenate([[0], np.cumsum(lens)])
    yield {"name": "search", "mode": 1, "S": blosum50(), "gap": 5, "text": synthetic.random_sequence(3, int(offs[-1]), 20),
           "pattern": synthetic.random_sequence(4, 512, 20),
           "pairs": [(int(offs[k]), int(lens[k]), 0, 512) for k in range(ntexts)]}


def timed(fn, sync) -> float:
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    sync()
    return e0.elapsed_time(e1)


def stats(ms: list[float]) -> dict:
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "runs": len(ms)}


def model_cost(pairs, R: int, local: bool, affine: bool, fit: bool = False) -> int:
    """The planner's instruction count of a workload (sa_score_plan.h: kScoreStep*, kScoreAffineStep*,
    kScoreFitStep*)."""
    base, row = (18, 14 if local else 10) if affine else (14, 10 if local else 6)
    step = base + R * row + (5 + (R - 1) if fit else 0)
    return sum((n + 63) * -(-m // (64 * R)) * step for _, n, _, m in pairs if n and m)


def mapping_workload(small: bool) -> dict:
    """DNA reads of 140..160 letters, each a mutated piece of its own text window of 450..750 letters."""
    from sa_amd import synthetic
    npairs = 4000 if small else 40000
    rng = np.random.default_rng(13)
    nl, ml = rng.integers(450, 751, npairs), rng.integers(140, 161, npairs)
    to, po = np.concatenate([[0], np.cumsum(nl)]), np.concatenate([[0], np.cumsum(ml)])
    text = synthetic.random_sequence(5, int(to[-1]), 4)
    at = rng.integers(0, nl - ml + 1)
    src = np.concatenate([text[to[k] + at[k]:to[k] + at[k] + ml[k]] for k in range(npairs)])
    pattern = synthetic.mutate(src, 6, 4, int(po[-1]))
    return {"name": "mapping", "S": synthetic.blast_matrix(), "text": text, "pattern": pattern,
            "pairs": [(int(to[k]), int(nl[k]), int(po[k]), int(ml[k])) for k in range(npairs)]}


def mapped_workload(small: bool) -> dict:
    """The shapes of mapping_workload with every read mutated on its own, so that read k does start at
    letter at[k] of its window: mapping_workload mutates the concatenated reads, whose deletions shift all
    later reads off their windows, which no band around at[k] would survive."""
    from sa_amd import synthetic
    npairs = 4000 if small else 40000
    rng = np.random.default_rng(13)
    nl, ml = rng.integers(450, 751, npairs), rng.integers(140, 161, npairs)
    to, po = np.concatenate([[0], np.cumsum(nl)]), np.concatenate([[0], np.cumsum(ml)])
    text = synthetic.random_sequence(5, int(to[-1]), 4)
    at = rng.integers(0, nl - ml + 1)
    # a piece 16 letters longer than the read where the window has them: about 5 % of it is deleted
    pattern = np.concatenate([synthetic.mutate(text[to[k] + at[k]:min(to[k] + at[k] + ml[k] + 16, to[k + 1])], 600 + k, 4, int(ml[k]))
                              for k in range(npairs)])
    return {"name": "mapped", "S": synthetic.blast_matrix(), "text": text, "pattern": pattern, "at": at,
            "pairs": [(int(to[k]), int(nl[k]), int(po[k]), int(ml[k])) for k in range(npairs)]}


MODES = {"global": 0, "local": 1, "fit": 2}


def overlap_workload(small: bool) -> dict:
    """Pairs of DNA reads of 140..160 letters: the last 30..120 letters of each text are a mutated copy of
    the first letters of its pattern (two reads that overlap end to start)."""
    from sa_amd import synthetic
    npairs = 4000 if small else 40000
    rng = np.random.default_rng(17)
    nl, ml, ov = rng.integers(140, 161, npairs), rng.integers(140, 161, npairs), rng.integers(30, 121, npairs)
    to, po, oo = (np.concatenate([[0], np.cumsum(x)]) for x in (nl, ml, ov))
    pattern = synthetic.random_sequence(7, int(po[-1]), 4)
    text = synthetic.random_sequence(8, int(to[-1]), 4).copy()
    heads = synthetic.mutate(np.concatenate([pattern[po[k]:po[k] + ov[k]] for k in range(npairs)]), 9, 4, int(oo[-1]))
    for k in range(npairs):
        text[to[k + 1] - ov[k]:to[k + 1]] = heads[oo[k]:oo[k + 1]]
    return {"name": "overlap", "S": synthetic.blast_matrix(), "text": text, "pattern": pattern,
            "pairs": [(int(to[k]), int(nl[k]), int(po[k]), int(ml[k])) for k in range(npairs)]}


# --mode ends: the scorers of a run, and for each ends-free one the existing mode whose program it runs
ENDS_MODES = {"overlap": 31, "ends_tb_pe": 16 | 1 | 8, "ends_tb_te": 16 | 1 | 2, "ends_none": 16, "fit": 2, "global": 0}
ENDS_BASE = {"overlap": "fit", "ends_tb_te": "fit", "ends_tb_pe": "global", "ends_none": "global"}


def ends_rows(args, engine, w, dt, dp, gap: int, gap_extend) -> dict:
    """The ends-free scorers of one gap model on one workload beside SA_FIT and SA_GLOBAL, alternated."""
    cells = sum(p[1] * p[3] for p in w["pairs"])
    affine = gap_extend is not None
    have = hasattr(engine, "ENDS_FREE")  # a --tree checkout from before the modes runs the existing two
    sc = {k: engine.Scorer(m, w["S"], gap, w["pairs"], gap_extend=gap_extend) for k, m in ENDS_MODES.items() if have or m < 16}
    row = {"name": w["name"] + ("_affine" if affine else "_linear"), "pairs": len(w["pairs"]), "cells": cells, "gap": gap,
           "gap_extend": gap_extend, "scorers": {k: s.info() for k, s in sc.items()}}
    res = {}
    for _ in range(2):  # warm-up
        for k, s in sc.items():
            s.run(dt.data_ptr(), dp.data_ptr())
            res[k] = s.results()
    if have:
        assert res["ends_tb_te"].tolist() == res["fit"].tolist(), "SA_ENDS_FREE | TB | TE and SA_FIT differ"
        assert res["ends_none"].tolist() == res["global"].tolist(), "SA_ENDS_FREE and SA_GLOBAL differ"
        assert (res["global"]["score"] <= res["ends_tb_pe"]["score"]).all() and (res["ends_tb_pe"]["score"] <= res["overlap"]["score"]).all()
        assert (res["fit"]["score"] <= res["overlap"]["score"]).all()
        row["identities_hold"] = True
        row["mean_score"] = {k: round(float(r["score"].mean()), 2) for k, r in res.items()}
    ms = {k: [] for k in sc}
    for _ in range(args.rounds):
        for k, s in sc.items():
            ms[k].append(timed(lambda: s.run(dt.data_ptr(), dp.data_ptr()), lambda: s.results()))
    for k, s in sc.items():
        row[k + "_run"] = stats(ms[k])
        row[k + "_gcups"] = round(cells / statistics.median(ms[k]) / 1e6, 1)
        s.close()
    med = {k: statistics.median(v) for k, v in ms.items()}
    row["compared"] = {}
    for k, base in ENDS_BASE.items():
        if k in sc:
            spread = max(ms[base]) - min(ms[base])
            row["compared"][k] = {"baseline": base, "over_baseline": round(med[k] / med[base], 4),
                                  "baseline_spread_ms": round(spread, 3),
                                  "within_baseline_plus_spread": bool(med[k] <= med[base] + spread)}
    return row


def related_workload(small: bool) -> dict:
    """Pairs of about 20000 DNA letters: each pattern is its text with 5 % substitutions and 0.1 %
    deletions, so the optimal path stays within a few tens of cells of the band's two diagonals."""
    from sa_amd import synthetic
    npairs, side = (128, 20000) if small else (2048, 20000)
    text = synthetic.random_sequence(21, npairs * side, 4)
    pats = [synthetic.mutate(text[k * side:(k + 1) * side], 1000 + k, 4, None, p_del=0.001, p_ins=0.0, p_sub=0.05) for k in range(npairs)]
    po = np.concatenate([[0], np.cumsum([len(x) for x in pats])])
    return {"name": "related", "S": synthetic.blast_matrix(), "text": text, "pattern": np.concatenate(pats),
            "pairs": [(k * side, side, int(po[k]), len(pats[k])) for k in range(npairs)]}


def band_model_cost(pairs, R: int, band: int) -> int:
    """The planner's instruction count of the banded global affine scorer (sa_score_plan.h: band_window):
    a strip is charged jmax - jmin + 64 steps."""
    step, rows, total = 18 + R * 10, 64 * R, 0
    for _, n, _, m in pairs:
        w = min(band, max(n, m))
        lo, hi = min(0, n - m) - w, max(0, n - m) + w
        for first in range(1, m + 1, rows):
            total += (min(n, min(m, first + rows - 1) + hi) - max(1, first + lo) + 64) * step
    return total


def path_diagonals(res) -> tuple[int, int]:
    """The lowest and highest j - i over the cells of a global alignment, read from its strings."""
    d = lo = hi = 0
    for a, b in zip(res["aligned_text"], res["aligned_pattern"]):
        d += (a != "-") - (b != "-")
        lo, hi = min(lo, d), max(hi, d)
    return lo, hi


def band_rows(args, engine, w, dt, dp) -> dict:
    import time
    go, ge, pairs = args.gap_open, args.gap_extend if args.gap_extend is not None else 2, w["pairs"]
    cells = sum(p[1] * p[3] for p in pairs)
    row = {"name": w["name"], "pairs": len(pairs), "cells": cells, "gap_open": go, "gap_extend": ge, "bands": {}}
    sc = {"unbanded": engine.Scorer(0, w["S"], go, pairs, gap_extend=ge)}
    for b in args.band:
        sc[str(b)] = engine.Scorer(0, w["S"], go, pairs, gap_extend=ge, band=b)
    res, t = {}, {k: [] for k in sc}
    for k, s in sc.items():  # warm-up, and the scores
        s.run(dt.data_ptr(), dp.data_ptr())
        res[k] = s.results()["score"].copy()
    for _ in range(args.rounds):
        for k, s in sc.items():
            t[k].append(timed(lambda: s.run(dt.data_ptr(), dp.data_ptr()), lambda: s.results()))
    row["unbanded"] = dict(stats(t["unbanded"]), **sc["unbanded"].info(), gcups=round(cells / statistics.median(t["unbanded"]) / 1e6, 1))
    full_model = model_cost(pairs, row["unbanded"]["rows_per_lane"], False, True)
    # the subsample: unbanded alignments, their paths, and the banded scores against them
    sub = list(range(0, len(pairs), max(1, len(pairs) // 16)))
    texts = [w["text"][pairs[k][0]:pairs[k][0] + pairs[k][1]] for k in sub]
    pats = [w["pattern"][pairs[k][2]:pairs[k][2] + pairs[k][3]] for k in sub]
    full = engine.align_pairs_affine(0, texts, pats, w["S"], go, ge)
    assert [f["score"] for f in full] == res["unbanded"][sub].tolist(), "the unbanded scorer and aligner differ"
    diags = [path_diagonals(f) for f in full]
    for b in args.band:
        k = str(b)
        info = sc[k].info()
        assert (res[k] <= res["unbanded"]).all(), f"band {b}: a banded score exceeds the unbanded one"
        free = [i for i, (pr, (dlo, dhi)) in enumerate(zip(sub, diags))
                if min(0, pairs[pr][1] - pairs[pr][3]) - b <= dlo and dhi <= max(0, pairs[pr][1] - pairs[pr][3]) + b]
        assert all(res[k][sub[i]] == full[i]["score"] for i in free), f"band {b}: scores differ where the band does not bind"
        model = band_model_cost(pairs, info["rows_per_lane"], b)
        row["bands"][k] = dict(stats(t[k]), **info, subsample=len(sub), subsample_band_does_not_bind=len(free),
                               pairs_with_the_unbanded_score=int((res[k] == res["unbanded"]).sum()),
                               banded_over_unbanded=round(statistics.median(t[k]) / statistics.median(t["unbanded"]), 4),
                               model_banded_over_unbanded=round(model / full_model, 4))
    for s in sc.values():
        s.close()
    # aligned runs on the first pairs: banded and unbanded alternated
    nal = min(len(pairs), 16 if args.small else 64)
    texts = [w["text"][p[0]:p[0] + p[1]] for p in pairs[:nal]]
    pats = [w["pattern"][p[2]:p[2] + p[3]] for p in pairs[:nal]]
    al = {k: {"fill_ms": [], "walk_ms": [], "wall_ms": []} for k in ["unbanded"] + [str(b) for b in args.band]}
    got = {}
    for rnd in range(1 + max(3, args.rounds // 2)):
        for k in al:
            t0 = time.perf_counter()
            got[k] = engine.align_pairs_affine(0, texts, pats, w["S"], go, ge, band=None if k == "unbanded" else int(k))
            wall = (time.perf_counter() - t0) * 1e3
            st = engine.affine_last_stats()
            if rnd:  # round 0 warms up
                al[k]["fill_ms"].append(st["fill_ms"]), al[k]["walk_ms"].append(st["walk_ms"]), al[k]["wall_ms"].append(wall)
            al[k]["arena_bytes"], al[k]["num_chunks"] = st["arena_bytes"], st["num_chunks"]
    row["aligned"] = {"pairs": nal}
    for k, v in al.items():
        same = sum(g == f for g, f in zip(got[k], got["unbanded"]))
        row["aligned"][k] = {"fill": stats(v["fill_ms"]), "walk": stats(v["walk_ms"]), "end_to_end_wall": stats(v["wall_ms"]),
                             "arena_bytes": v["arena_bytes"], "num_chunks": v["num_chunks"], "alignments_equal_to_unbanded": same}
    return row


def band_at_model_cost(pairs, bands, R: int) -> int:
    """The planner's instruction count of the band-at fit scorer (sa_score_plan.h: band_window_at): the
    affine fit step, charged jmax - jmin + 64 times per strip that holds an in-band cell."""
    step, rows, total = 18 + 4 + R * 11, 64 * R, 0
    for (_, n, _, m), (lo, hi) in zip(pairs, bands):
        lo, hi = max(lo, -m), min(hi, n)
        for first in range(1, m + 1, rows):
            ia, ib = max(first, 1 - hi), min(m, first + rows - 1, n - lo)
            if ia <= ib:
                total += (min(n, ib + hi) - max(1, ia + lo) + 64) * step
    return total


def fit_path_diagonals(res) -> tuple[int, int]:
    """The lowest and highest j - i over the cells of a fit alignment: it starts at (0, start_text)."""
    d = lo = hi = int(res["start_text"])
    for a, b in zip(res["aligned_text"], res["aligned_pattern"]):
        d += (a != "-") - (b != "-")
        lo, hi = min(lo, d), max(hi, d)
    return lo, hi


def mapped_rows(args, engine, w, dt, dp, gap: int, gap_extend) -> dict:
    """Fit scoring of the mapped workload inside the band [at - w, at + w] of each read's true offset,
    w = 16 and 64, beside the unbanded fit scorer of the same gap model, alternated."""
    pairs, cells, affine = w["pairs"], sum(p[1] * p[3] for p in w["pairs"]), gap_extend is not None
    bands = {b: [(int(a) - b, int(a) + b) for a in w["at"]] for b in (16, 64)}
    sc = {"fit": engine.Scorer(2, w["S"], gap, pairs, gap_extend=gap_extend)}
    for b in bands:
        sc[f"band_at_{b}"] = engine.Scorer(2, w["S"], gap, pairs, gap_extend=gap_extend, bands=bands[b])
    row = {"name": w["name"] + ("_affine" if affine else "_linear"), "pairs": len(pairs), "cells": cells, "gap": gap,
           "gap_extend": gap_extend, "scorers": {k: s.info() for k, s in sc.items()}}
    res = {}
    for _ in range(2):  # warm-up
        for k, s in sc.items():
            s.run(dt.data_ptr(), dp.data_ptr())
            res[k] = s.results()
    # a subsample aligned without a band: where its path lies inside the band the scores are equal
    sub = list(range(0, len(pairs), max(1, len(pairs) // 400)))
    texts = [w["text"][pairs[k][0]:pairs[k][0] + pairs[k][1]] for k in sub]
    pats = [w["pattern"][pairs[k][2]:pairs[k][2] + pairs[k][3]] for k in sub]
    full = engine.align_pairs_affine(2, texts, pats, w["S"], gap, gap if gap_extend is None else gap_extend)
    assert [f["score"] for f in full] == res["fit"]["score"][sub].tolist(), "the fit scorer and aligner differ"
    diags = [fit_path_diagonals(f) for f in full]
    ms = {k: [] for k in sc}
    for _ in range(args.rounds):
        for k, s in sc.items():
            ms[k].append(timed(lambda: s.run(dt.data_ptr(), dp.data_ptr()), lambda: s.results()))
    med = {k: statistics.median(v) for k, v in ms.items()}
    fit_model = model_cost(pairs, row["scorers"]["fit"]["rows_per_lane"], False, affine, True)
    row["fit_run"] = stats(ms["fit"])
    row["bands"] = {}
    for b in bands:
        k = f"band_at_{b}"
        assert (res[k]["score"] <= res["fit"]["score"]).all(), f"band {b}: a banded score exceeds the unbanded one"
        free = [i for i, (pr, (dlo, dhi)) in enumerate(zip(sub, diags)) if bands[b][pr][0] <= dlo and dhi <= bands[b][pr][1]]
        assert all(res[k]["score"][sub[i]] == full[i]["score"] for i in free), f"band {b}: scores differ where the band does not bind"
        model = band_at_model_cost(pairs, bands[b], row["scorers"][k]["rows_per_lane"])
        row["bands"][str(b)] = dict(stats(ms[k]), subsample=len(sub), subsample_band_does_not_bind=len(free),
                                    pairs_with_the_unbanded_score=int((res[k]["score"] == res["fit"]["score"]).sum()),
                                    banded_over_fit=round(med[k] / med["fit"], 4), model_banded_over_fit=round(model / fit_model, 4))
    for s in sc.values():
        s.close()
    return row


def chimeric_workload(small: bool) -> dict:
    """DNA pairs of 20000 letters: the pattern is its text with 5 % substitutions for its first quarter
    and unrelated letters after it."""
    from sa_amd import synthetic
    npairs, side = (128, 20000) if small else (2048, 20000)
    text = synthetic.random_sequence(31, npairs * side, 4)
    pattern = synthetic.random_sequence(32, npairs * side, 4).copy()
    q = side // 4
    for k in range(npairs):
        pattern[k * side:k * side + q] = synthetic.mutate(text[k * side:k * side + q], 2000 + k, 4, q, p_del=0.0, p_ins=0.0, p_sub=0.05)
    return {"name": "chimeric", "S": synthetic.blast_matrix(), "text": text, "pattern": pattern,
            "pairs": [(k * side, side, k * side, side) for k in range(npairs)]}


def extend_rowwise_ref(t, p, S, go: int, ge: int, xdrop):
    """(score, end_pattern, end_text, stop row) of extension alignment (sa_hip.h), row by row in numpy and
    no further than the stop row; xdrop None is no drop. For go >= ge >= 0, where a gap along the row never
    opens from a cell that a gap along the row reached: E[j] = max over k < j of
    max(diag, F)[k] - go - (j - 1 - k) ge, a running maximum."""
    assert go >= ge >= 0
    t, p, S = np.asarray(t, dtype=np.int64), np.asarray(p, dtype=np.int64), np.asarray(S, dtype=np.int64)
    n, m = len(t), len(p)
    if n == 0 or m == 0:
        return 0, 0, 0, m + 1
    NEG = -(1 << 40)
    cols = np.arange(n + 1, dtype=np.int64)
    Hup = np.concatenate([[0], -(go + (cols[1:] - 1) * ge)])
    F = np.full(n + 1, NEG, dtype=np.int64)
    B, best, bi, bj = 0, 0, 0, 0
    for i in range(1, m + 1):
        F = np.maximum(F - ge, Hup - go)
        hp = np.empty(n + 1, dtype=np.int64)
        hp[0] = -(go + (i - 1) * ge)
        hp[1:] = np.maximum(Hup[:-1] + S[p[i - 1], t], F[1:])
        acc = np.maximum.accumulate(hp + cols * ge)
        H = hp.copy()
        H[1:] = np.maximum(hp[1:], acc[:-1] - go - cols[:-1] * ge)
        r = int(H[1:].max())
        if xdrop is not None and B - r > xdrop:
            return best, bi, bj, i
        B = max(B, r)
        if r > best:
            best, bi, bj = r, i, 1 + int(H[1:].argmax())
        Hup = H
    return best, bi, bj, m + 1


def extend_same_work_rows(args, engine, w, dt, dp, gap: int, gap_extend) -> dict:
    """The extension scorer without a drop beside the local scorer of the same penalties, alternated."""
    cells, affine = sum(p[1] * p[3] for p in w["pairs"]), gap_extend is not None
    sc = {"local": engine.Scorer(1, w["S"], gap, w["pairs"], gap_extend=gap_extend),
          "extend_no_xdrop": engine.Scorer(0, w["S"], gap, w["pairs"], gap_extend=gap_extend, xdrop=engine.NO_XDROP)}
    row = {"name": w["name"] + ("_affine" if affine else "_linear"), "pairs": len(w["pairs"]), "cells": cells, "gap": gap,
           "gap_extend": gap_extend, "scorers": {k: s.info() for k, s in sc.items()}}
    res = {}
    for _ in range(2):  # warm-up
        for k, s in sc.items():
            s.run(dt.data_ptr(), dp.data_ptr())
            res[k] = s.results()
    assert (res["extend_no_xdrop"]["score"] <= res["local"]["score"]).all(), "an anchored score exceeds the local one"
    ms = {k: [] for k in sc}
    for _ in range(args.rounds):
        for k, s in sc.items():
            ms[k].append(timed(lambda: s.run(dt.data_ptr(), dp.data_ptr()), lambda: s.results()))
    for k, s in sc.items():
        row[k + "_run"] = stats(ms[k])
        row[k + "_gcups"] = round(cells / statistics.median(ms[k]) / 1e6, 1)
        s.close()
    med = statistics.median(ms["extend_no_xdrop"])
    row["extend_over_local"] = round(med / statistics.median(ms["local"]), 4)
    row["extend_inside_local_min_max"] = bool(min(ms["local"]) <= med <= max(ms["local"]))
    return row


def extend_early_exit_row(args, engine, w, dt, dp, go: int, ge: int, xdrop: int) -> dict:
    """The extension scorer at `xdrop`, without a drop, and the local scorer on the chimeric pairs."""
    pairs, cells = w["pairs"], sum(p[1] * p[3] for p in w["pairs"])
    sc = {"extend_xdrop": engine.Scorer(0, w["S"], go, pairs, gap_extend=ge, xdrop=xdrop),
          "extend_no_xdrop": engine.Scorer(0, w["S"], go, pairs, gap_extend=ge, xdrop=engine.NO_XDROP),
          "local": engine.Scorer(1, w["S"], go, pairs, gap_extend=ge)}
    row = {"name": w["name"], "pairs": len(pairs), "cells": cells, "gap_open": go, "gap_extend": ge, "xdrop": xdrop,
           "scorers": {k: s.info() for k, s in sc.items()}}
    res = {}
    for k, s in sc.items():  # warm-up, and the results
        s.run(dt.data_ptr(), dp.data_ptr())
        res[k] = s.results().copy()
    # the subsample against the reference: every pair at the X-drop (rows up to its stop row), four without one
    sub = list(range(0, len(pairs), max(1, len(pairs) // 16)))[:16]
    rows, run, total = 64 * row["scorers"]["extend_xdrop"]["rows_per_lane"], 0, 0
    stops = []
    for q, k in enumerate(sub):
        t, p = w["text"][pairs[k][0]:pairs[k][0] + pairs[k][1]], w["pattern"][pairs[k][2]:pairs[k][2] + pairs[k][3]]
        want = extend_rowwise_ref(t, p, w["S"], go, ge, xdrop)
        g = res["extend_xdrop"][k]
        assert (int(g["score"]), int(g["end_pattern"]), int(g["end_text"])) == want[:3], f"pair {k} differs from the reference at the X-drop"
        if q % 4 == 0:
            want0 = extend_rowwise_ref(t, p, w["S"], go, ge, None)
            g = res["extend_no_xdrop"][k]
            assert (int(g["score"]), int(g["end_pattern"]), int(g["end_text"])) == want0[:3], f"pair {k} differs from the reference without a drop"
        stops.append(want[3])
        run += -(-min(want[3], pairs[k][3]) // rows)
        total += -(-pairs[k][3] // rows)
    row["subsample"] = {"pairs": len(sub), "stop_rows": stops, "results_equal_the_reference": True,
                        "model_strips_run_over_total": round(run / total, 4)}
    ms = {k: [] for k in sc}
    for _ in range(args.rounds):
        for k, s in sc.items():
            ms[k].append(timed(lambda: s.run(dt.data_ptr(), dp.data_ptr()), lambda: s.results()))
    for k, s in sc.items():
        row[k + "_run"] = stats(ms[k])
        s.close()
    med = {k: statistics.median(v) for k, v in ms.items()}
    row["xdrop_over_no_xdrop"] = round(med["extend_xdrop"] / med["extend_no_xdrop"], 4)
    row["xdrop_over_local"] = round(med["extend_xdrop"] / med["local"], 4)
    row["no_xdrop_over_local"] = round(med["extend_no_xdrop"] / med["local"], 4)
    # aligned: the traced fill and the walk of the first pairs, with and without the drop, alternated
    nal = min(len(pairs), 16 if args.small else 64)
    texts = [w["text"][p[0]:p[0] + p[1]] for p in pairs[:nal]]
    pats = [w["pattern"][p[2]:p[2] + p[3]] for p in pairs[:nal]]
    al = {k: {"fill_ms": [], "walk_ms": []} for k in ("xdrop", "no_xdrop")}
    for rnd in range(1 + max(3, args.rounds // 2)):
        for k in al:
            got = engine.align_pairs_affine(0, texts, pats, w["S"], go, ge, strings=False, xdrop=xdrop if k == "xdrop" else engine.NO_XDROP)
            st = engine.affine_last_stats()
            want = res["extend_xdrop" if k == "xdrop" else "extend_no_xdrop"]["score"][:nal].tolist()
            assert [g["score"] for g in got] == want, "the aligner and the scorer differ"
            if rnd:  # round 0 warms up
                al[k]["fill_ms"].append(st["fill_ms"]), al[k]["walk_ms"].append(st["walk_ms"])
            al[k]["arena_bytes"], al[k]["num_chunks"] = st["arena_bytes"], st["num_chunks"]
    row["aligned"] = {"pairs": nal}
    for k, v in al.items():
        row["aligned"][k] = {"fill": stats(v["fill_ms"]), "walk": stats(v["walk_ms"]), "arena_bytes": v["arena_bytes"],
                             "num_chunks": v["num_chunks"]}
    return row


def longest_match_seeds(engine, w, go: int, ge: int):
    """Per pair the seed (text_pos, pattern_pos, length) of the longest run of matching columns of its SA_FIT
    alignment (the first of the longest), and the text span [start, end) the alignment covers."""
    pairs = w["pairs"]
    seeds, spans = [], []
    for lo in range(0, len(pairs), 4000):
        part = pairs[lo:lo + 4000]
        texts = [w["text"][p[0]:p[0] + p[1]] for p in part]
        pats = [w["pattern"][p[2]:p[2] + p[3]] for p in part]
        for r in engine.align_pairs_affine(2, texts, pats, w["S"], go, ge):
            a = np.frombuffer(r["aligned_text"].encode(), dtype=np.uint8)
            b = np.frombuffer(r["aligned_pattern"].encode(), dtype=np.uint8)
            eq = np.concatenate([[0], (a == b).astype(np.int8), [0]])
            edges = np.flatnonzero(np.diff(eq))  # run starts and ends, alternating
            starts, ends = edges[0::2], edges[1::2]
            k = int(np.argmax(ends - starts)) if len(starts) else -1
            c0, L = (int(starts[k]), int(ends[k] - starts[k])) if k >= 0 else (0, 0)
            tpos = int(r["start_text"]) + int((a[:c0] != ord("-")).sum())
            ppos = int(r["start_pattern"]) + int((b[:c0] != ord("-")).sum())
            seeds.append((tpos, ppos, L))
            spans.append((int(r["start_text"]), int(r["start_text"]) + int((a != ord("-")).sum())))
    return seeds, spans


def clip_workload(w, seeds, spans, margin: int = 32):
    """Every text window clipped to the read's span +- `margin` letters, as a mapper would clip it."""
    pairs, texts, out, sd = w["pairs"], [], [], []
    off = 0
    for (to, n, po, m), (ts, ps, L), (a, b) in zip(pairs, seeds, spans):
        lo, hi = max(0, a - margin), min(n, b + margin)
        texts.append(w["text"][to + lo:to + hi])
        out.append((off, hi - lo, po, m))
        sd.append((ts - lo, ps, L))
        off += hi - lo
    return dict(w, name=w["name"] + "_clipped", text=np.concatenate(texts), pairs=out), sd


def halves_workloads(w, seeds):
    """The halves of every pair as two extension workloads: the left halves reversed on the host, the right
    halves sliced; a half with an empty side stays as an empty pair."""
    lt, lp, rt, rp = [], [], [], []
    for (to, n, po, m), (ts, ps, L) in zip(w["pairs"], seeds):
        lt.append(w["text"][to:to + ts][::-1]), lp.append(w["pattern"][po:po + ps][::-1])
        rt.append(w["text"][to + ts + L:to + n]), rp.append(w["pattern"][po + ps + L:po + m])

    def pack(ts_, ps_):
        to = np.concatenate([[0], np.cumsum([len(x) for x in ts_])])
        po = np.concatenate([[0], np.cumsum([len(x) for x in ps_])])
        return {"text": np.ascontiguousarray(np.concatenate(ts_)), "pattern": np.ascontiguousarray(np.concatenate(ps_)),
                "pairs": [(int(to[k]), len(ts_[k]), int(po[k]), len(ps_[k])) for k in range(len(ts_))]}
    return pack(lt, lp), pack(rt, rp)


def seeds_rows(args, engine, w, seeds, gap: int, gap_extend, xdrop) -> dict:
    """(a) the seeds scorer, (b) two extension scorers over pre-reversed and sliced arenas of the same halves,
    run one after the other, (c) the unbanded fit scorer; alternated round by round. The seeded scores are
    asserted equal to the composition of (b) at the timed size."""
    import torch
    # gap open == gap extend is the linear recurrence: the extension and seeds scorers then run the linear
    # kernels (S4), and the fit scorer beside them is the linear one
    pairs, affine = w["pairs"], gap != gap_extend
    x = engine.NO_XDROP if xdrop is None else xdrop
    left, right = halves_workloads(w, seeds)
    dev = {k: (torch.from_numpy(v["text"]).cuda(), torch.from_numpy(v["pattern"]).cuda()) for k, v in (("w", w), ("l", left), ("r", right))}
    sc = {"seeds": engine.Scorer(0, w["S"], gap, pairs, gap_extend=gap_extend, xdrop=x, seeds=seeds),
          "left": engine.Scorer(0, w["S"], gap, left["pairs"], gap_extend=gap_extend, xdrop=x),
          "right": engine.Scorer(0, w["S"], gap, right["pairs"], gap_extend=gap_extend, xdrop=x),
          "fit": engine.Scorer(2, w["S"], gap, pairs, gap_extend=gap_extend if affine else None)}
    ptr = {"seeds": dev["w"], "fit": dev["w"], "left": dev["l"], "right": dev["r"]}
    run = {k: (lambda k=k: sc[k].run(ptr[k][0].data_ptr(), ptr[k][1].data_ptr())) for k in sc}
    row = {"name": w["name"] + ("_affine" if affine else "_linear") + ("_xdrop" if xdrop is not None else "_no_xdrop"),
           "pairs": len(pairs), "cells": sum(p[1] * p[3] for p in pairs), "half_cells": sum(p[1] * p[3] for p in left["pairs"] + right["pairs"]),
           "gap": gap, "gap_extend": gap_extend, "xdrop": xdrop, "scorers": {k: s.info() for k, s in sc.items()}}
    res = {}
    for _ in range(2):  # warm-up
        for k in sc:
            run[k]()
            res[k] = sc[k].results().copy()
    S = np.asarray(w["S"])
    mid = np.array([int(S[w["pattern"][po + ps:po + ps + L], w["text"][to + ts:to + ts + L]].sum()) for (to, _, po, _), (ts, ps, L) in zip(pairs, seeds)])
    sd = np.array(seeds, dtype=np.int64).reshape(-1, 3)
    g, l, r = res["seeds"], res["left"], res["right"]
    assert (g["score"] == l["score"] + mid + r["score"]).all(), "a seeded score differs from the composition"
    assert (g["begin_text"] == sd[:, 0] - l["end_text"]).all() and (g["begin_pattern"] == sd[:, 1] - l["end_pattern"]).all()
    assert (g["end_text"] == sd[:, 0] + sd[:, 2] + r["end_text"]).all() and (g["end_pattern"] == sd[:, 1] + sd[:, 2] + r["end_pattern"]).all()
    row["seeded_scores_equal_the_composition"] = True
    ms = {"seeds": [], "two_extend": [], "fit": []}

    def both():
        run["left"]()
        run["right"]()
    for _ in range(args.rounds):
        ms["seeds"].append(timed(run["seeds"], lambda: sc["seeds"].results()))
        ms["two_extend"].append(timed(both, lambda: (sc["left"].results(), sc["right"].results())))
        ms["fit"].append(timed(run["fit"], lambda: sc["fit"].results()))
    for k, v in ms.items():
        row[k + "_run"] = stats(v)
    med = {k: statistics.median(v) for k, v in ms.items()}
    items = [(0, n, 0, m) for _, n, _, m in left["pairs"] + right["pairs"]]
    model = model_cost(items, row["scorers"]["seeds"]["rows_per_lane"], True, affine) / model_cost(pairs, row["scorers"]["fit"]["rows_per_lane"], False, affine, True)
    spread = max(ms["two_extend"]) - min(ms["two_extend"])
    row["seeds_over_two_extend"] = round(med["seeds"] / med["two_extend"], 4)
    row["two_extend_spread_ms"] = round(spread, 3)
    row["seeds_below_two_extend_beyond_its_spread"] = bool(med["seeds"] < med["two_extend"] - spread)
    row["seeds_over_fit"] = round(med["seeds"] / med["fit"], 4)
    row["model_seeds_over_fit"] = round(model, 4)
    for s in sc.values():
        s.close()
    return row


def seeds_aligned_row(args, engine, w, seeds, go: int, ge: int, xdrop) -> dict:
    """sa_align_pairs_seeds end to end (wall clock, host arrays to host strings) on the first 4000 pairs beside
    the two-call host composition: reverse the prefixes, two sa_align_pairs_extend calls, reverse the left
    strings back and join the three pieces."""
    import time
    nal = min(len(w["pairs"]), 4000)
    pairs, sd = w["pairs"][:nal], seeds[:nal]
    texts = [w["text"][p[0]:p[0] + p[1]] for p in pairs]
    pats = [w["pattern"][p[2]:p[2] + p[3]] for p in pairs]
    x = engine.NO_XDROP if xdrop is None else xdrop

    def seeded():
        return engine.align_pairs_affine(0, texts, pats, w["S"], go, ge, xdrop=x, seeds=sd)

    def composed():
        lt = [np.ascontiguousarray(t[:s[0]][::-1]) for t, s in zip(texts, sd)]
        lp = [np.ascontiguousarray(p[:s[1]][::-1]) for p, s in zip(pats, sd)]
        rt = [t[s[0] + s[2]:] for t, s in zip(texts, sd)]
        rp = [p[s[1] + s[2]:] for p, s in zip(pats, sd)]
        la = engine.align_pairs_affine(0, lt, lp, w["S"], go, ge, xdrop=x)
        ra = engine.align_pairs_affine(0, rt, rp, w["S"], go, ge, xdrop=x)
        return [(a["aligned_text"][::-1] + "".join("ATCG"[c] for c in t[s[0]:s[0] + s[2]]) + b["aligned_text"],
                 a["aligned_pattern"][::-1] + "".join("ATCG"[c] for c in p[s[1]:s[1] + s[2]]) + b["aligned_pattern"])
                for a, b, t, p, s in zip(la, ra, texts, pats, sd)]
    got, want = seeded(), composed()
    assert [(g["aligned_text"], g["aligned_pattern"]) for g in got] == want, "a seeded alignment differs from the composition"
    ms = {"seeds": [], "composition": []}
    fill, walk = [], []
    for _ in range(max(3, args.rounds // 2)):
        t0 = time.perf_counter()
        seeded()
        ms["seeds"].append((time.perf_counter() - t0) * 1e3)
        s2 = engine.affine_last_stats()
        fill.append(s2["fill_ms"]), walk.append(s2["walk_ms"])
        t0 = time.perf_counter()
        composed()
        ms["composition"].append((time.perf_counter() - t0) * 1e3)
    return {"name": w["name"] + "_aligned", "pairs": nal, "gap_open": go, "gap_extend": ge, "xdrop": xdrop,
            "alignments_equal_the_composition": True, "seeds_end_to_end_wall": stats(ms["seeds"]),
            "composition_end_to_end_wall": stats(ms["composition"]), "seeds_traced_fill": stats(fill), "seeds_walk": stats(walk),
            "seeds_arena_bytes": s2["arena_bytes"], "seeds_chunks": s2["num_chunks"],
            "seeds_over_composition": round(statistics.median(ms["seeds"]) / statistics.median(ms["composition"]), 4)}


def chain_workload(small: bool) -> dict:
    """Reads of 10000 letters: every text mutated on its own (5 % substitutions, 5 % deletions, 2 % of the letters
    redrawn: synthetic.mutate), so that the read's path ends some 500 diagonals from where it starts."""
    from sa_amd import synthetic
    npairs, n = (128 if small else 2048), 10000
    text = synthetic.random_sequence(23, npairs * n, 4)
    pats = [synthetic.mutate(text[k * n:(k + 1) * n], 2300 + k, 4) for k in range(npairs)]
    po = np.concatenate([[0], np.cumsum([len(x) for x in pats])])
    return {"name": "long_reads", "S": synthetic.blast_matrix(), "text": text, "pattern": np.ascontiguousarray(np.concatenate(pats)).astype(np.int8),
            "pairs": [(k * n, n, int(po[k]), len(pats[k])) for k in range(npairs)]}


def exact_match_chains(engine, w, go: int, ge: int, min_len: int = 15, band: int = 256):
    """Per pair the chain of its exact-match runs of at least `min_len` columns in its banded global alignment
    (half-width `band` about the corner-to-corner diagonals), as (text_pos, pattern_pos, length) triples; cached."""
    cache = os.path.join(ROOT, "bench_out", f"chain_seeds_{len(w['pairs'])}_{go}_{ge}_{min_len}.npz")
    if os.path.exists(cache):
        z = np.load(cache)
        return [z["flat"][a:b].tolist() for a, b in zip(z["off"][:-1], z["off"][1:])]
    chains, pairs = [], w["pairs"]
    for lo in range(0, len(pairs), 256):
        part = pairs[lo:lo + 256]
        texts = [w["text"][p[0]:p[0] + p[1]] for p in part]
        pats = [w["pattern"][p[2]:p[2] + p[3]] for p in part]
        for r in engine.align_pairs_affine(0, texts, pats, w["S"], go, ge, band=band):
            a = np.frombuffer(r["aligned_text"].encode(), dtype=np.uint8)
            b = np.frombuffer(r["aligned_pattern"].encode(), dtype=np.uint8)
            eq = np.concatenate([[0], (a == b).astype(np.int8), [0]])
            edges = np.flatnonzero(np.diff(eq))
            starts, ends = edges[0::2], edges[1::2]
            keep = ends - starts >= min_len
            tpos = np.concatenate([[0], np.cumsum(a != ord("-"))])  # text letters before column c
            ppos = np.concatenate([[0], np.cumsum(b != ord("-"))])
            chains.append([(int(tpos[c]), int(ppos[c]), int(e - c)) for c, e in zip(starts[keep], ends[keep])])
    os.makedirs(os.path.dirname(cache), exist_ok=True)
    off = np.concatenate([[0], np.cumsum([len(c) for c in chains])])
    np.savez(cache, flat=np.array([s for c in chains for s in c], dtype=np.int64).reshape(-1, 3), off=off)
    return chains


def chain_pieces(w, chains):
    """The pieces of every chained pair as the workloads of the composition: the left ends reversed on the host, the
    right ends sliced, and every gap rectangle with two non-empty sides a pair of its own. Per pair also the sum
    of its seeds' scores and of its empty-side gaps' closed forms (under go, ge given later: the lengths)."""
    S = np.asarray(w["S"])
    lt, lp, rt, rp, gt, gp, gap_pair, seed_score, closed = [], [], [], [], [], [], [], [], []
    for k, ((to, n, po, m), ch) in enumerate(zip(w["pairs"], chains)):
        t, p = w["text"][to:to + n], w["pattern"][po:po + m]
        sd = np.array(ch, dtype=np.int64).reshape(-1, 3)
        ts0, ps0 = int(sd[0, 0]), int(sd[0, 1])
        te, pe = int(sd[-1, 0] + sd[-1, 2]), int(sd[-1, 1] + sd[-1, 2])
        lt.append(t[:ts0][::-1]), lp.append(p[:ps0][::-1]), rt.append(t[te:]), rp.append(p[pe:])
        total = int(sd[:, 2].sum())
        before = np.concatenate([[0], np.cumsum(sd[:, 2])[:-1]])
        col = np.arange(total)
        seed_score.append(int(S[p[np.repeat(sd[:, 1] - before, sd[:, 2]) + col], t[np.repeat(sd[:, 0] - before, sd[:, 2]) + col]].sum()))
        runs = []
        for (a, b, L), (c, d, _) in zip(ch, ch[1:]):
            gn, gm = c - a - L, d - b - L
            if gn and gm:
                gt.append(t[a + L:c]), gp.append(p[b + L:d]), gap_pair.append(k)
            elif gn + gm:
                runs.append(gn + gm)
        closed.append(runs)

    def pack(ts_, ps_):
        to = np.concatenate([[0], np.cumsum([len(x) for x in ts_])])
        po = np.concatenate([[0], np.cumsum([len(x) for x in ps_])])
        cat = lambda xs: np.ascontiguousarray(np.concatenate(xs) if xs else np.zeros(0)).astype(np.int8)  # noqa: E731
        return {"text": cat(ts_), "pattern": cat(ps_), "pairs": [(int(to[k]), len(ts_[k]), int(po[k]), len(ps_[k])) for k in range(len(ts_))]}
    return pack(lt, lp), pack(rt, rp), pack(gt, gp), np.array(gap_pair, dtype=np.int64), np.array(seed_score), closed


def chain_bands(w, chains, margin: int = 16):
    """The narrowest band per pair that holds the chain's diagonals, the origin's and the far corner's, +- margin."""
    out = []
    for (_, n, _, m), ch in zip(w["pairs"], chains):
        d = [ts - ps for ts, ps, _ in ch] + [0, n - m]
        out.append((min(d) - margin, max(d) + margin))
    return out


def chain_rows(args, engine, w, chains, go: int, ge: int, xdrop) -> dict:
    """(a), (b) and (c) of --mode chain, alternated round by round."""
    import torch
    pairs = w["pairs"]
    x = engine.NO_XDROP if xdrop is None else xdrop
    left, right, gaps, gap_pair, seed_score, closed = chain_pieces(w, chains)
    bands = chain_bands(w, chains)
    dev = {k: (torch.from_numpy(v["text"]).cuda(), torch.from_numpy(v["pattern"]).cuda()) for k, v in (("w", w), ("l", left), ("r", right), ("g", gaps))}
    sc = {"chains": engine.Scorer(0, w["S"], go, pairs, gap_extend=ge, xdrop=x, chains=chains),
          "left": engine.Scorer(0, w["S"], go, left["pairs"], gap_extend=ge, xdrop=x),
          "right": engine.Scorer(0, w["S"], go, right["pairs"], gap_extend=ge, xdrop=x),
          "gaps": engine.Scorer(0, w["S"], go, gaps["pairs"], gap_extend=ge),
          "band_at": engine.Scorer(0, w["S"], go, pairs, gap_extend=ge, bands=bands)}
    ptr = {"chains": dev["w"], "band_at": dev["w"], "left": dev["l"], "right": dev["r"], "gaps": dev["g"]}
    run = {k: (lambda k=k: sc[k].run(ptr[k][0].data_ptr(), ptr[k][1].data_ptr())) for k in sc}
    gshape = np.array([(p[3], p[1]) for p in gaps["pairs"]], dtype=np.int64).reshape(-1, 2)
    row = {"name": w["name"] + ("_xdrop" if xdrop is not None else "_no_xdrop"), "pairs": len(pairs), "cells": sum(p[1] * p[3] for p in pairs),
           "gap_open": go, "gap_extend": ge, "xdrop": xdrop, "scorers": {k: s.info() for k, s in sc.items()},
           "seeds_per_pair": round(float(np.mean([len(c) for c in chains])), 1), "seed_columns_per_pair": round(float(np.mean([sum(s[2] for s in c) for c in chains])), 1),
           "gap_items": len(gaps["pairs"]), "gap_rows_mean": round(float(gshape[:, 0].mean()), 1), "gap_columns_mean": round(float(gshape[:, 1].mean()), 1),
           "gap_columns_max": int(gshape[:, 1].max()), "gap_rows_max": int(gshape[:, 0].max()),
           "piece_cells": int(sum(p[1] * p[3] for p in gaps["pairs"] + left["pairs"] + right["pairs"])),
           "band_width_mean": round(float(np.mean([hi - lo + 1 for lo, hi in bands])), 1)}
    res = {}
    for _ in range(2):  # warm-up
        for k in sc:
            run[k]()
            res[k] = sc[k].results().copy()
    want = res["left"]["score"].astype(np.int64) + res["right"]["score"] + seed_score
    np.add.at(want, gap_pair, res["gaps"]["score"])
    want -= np.array([sum(go + (k - 1) * ge for k in runs) for runs in closed], dtype=np.int64)
    g = res["chains"]
    assert (g["score"] == want).all(), "a chained score differs from the composition"
    sd0 = np.array([c[0] for c in chains], dtype=np.int64)
    end = np.array([(c[-1][0] + c[-1][2], c[-1][1] + c[-1][2]) for c in chains], dtype=np.int64)
    assert (g["begin_text"] == sd0[:, 0] - res["left"]["end_text"]).all() and (g["begin_pattern"] == sd0[:, 1] - res["left"]["end_pattern"]).all()
    assert (g["end_text"] == end[:, 0] + res["right"]["end_text"]).all() and (g["end_pattern"] == end[:, 1] + res["right"]["end_pattern"]).all()
    row["chained_scores_equal_the_composition"] = True
    row["chains_reach_both_corners"] = int(((g["begin_text"] == 0) & (g["begin_pattern"] == 0)).sum()), int(sum(
        int(a["end_text"]) == p[1] and int(a["end_pattern"]) == p[3] for a, p in zip(g, pairs)))
    row["band_at_scores_equal_chains"] = int((res["band_at"]["score"] == g["score"]).sum())
    ms = {"chains": [], "composition": [], "band_at": []}

    def composed():
        run["left"]()
        run["right"]()
        run["gaps"]()
    for _ in range(args.rounds):
        ms["chains"].append(timed(run["chains"], lambda: sc["chains"].results()))
        ms["composition"].append(timed(composed, lambda: (sc["left"].results(), sc["right"].results(), sc["gaps"].results())))
        ms["band_at"].append(timed(run["band_at"], lambda: sc["band_at"].results()))
    for k, v in ms.items():
        row[k + "_run"] = stats(v)
    med = {k: statistics.median(v) for k, v in ms.items()}
    # the step model: the gaps as global pairs and the ends as extension pairs, each at its scorer's rows per lane, over
    # the band-at global program on the pairs' bands
    Rg, Re = row["scorers"]["gaps"]["rows_per_lane"], max(row["scorers"]["left"]["rows_per_lane"], 1)
    affine = go != ge
    m_gaps = model_cost(gaps["pairs"], Rg, False, affine)
    m_ends = model_cost(left["pairs"] + right["pairs"], Re, True, affine)
    m_band = band_at_model_cost(pairs, bands, row["scorers"]["band_at"]["rows_per_lane"])
    spread = max(ms["composition"]) - min(ms["composition"])
    row["chains_over_composition"] = round(med["chains"] / med["composition"], 4)
    row["composition_spread_ms"] = round(spread, 3)
    row["chains_within_composition_plus_its_spread"] = bool(med["chains"] <= med["composition"] + spread)
    row["chains_over_band_at"] = round(med["chains"] / med["band_at"], 4)
    row["model_chains_over_band_at"] = round((m_gaps + m_ends) / m_band, 4)
    row["model_gap_share_of_chains"] = round(m_gaps / (m_gaps + m_ends), 4)
    # what the model charges a mean gap item against the cells it holds: n + 63 steps of one strip for rows x n cells
    nbar, mbar = float(gshape[:, 1].mean()), float(gshape[:, 0].mean())
    row["gap_item_steps_mean"] = round(nbar + 63, 1)
    row["gap_item_lane_steps_used"] = round(nbar * mbar / ((nbar + 63) * 64 * Rg), 4)
    row["chains_us_per_gap_item"] = round(med["chains"] * 1e3 / max(len(gaps["pairs"]), 1), 4)
    for s in sc.values():
        s.close()
    return row


def chain_aligned_row(args, engine, w, chains, go: int, ge: int, xdrop) -> dict:
    """(d): align_pairs_affine(chains=) on 64 of the pairs beside bands= with the chain's bands, end to end."""
    nal = min(len(w["pairs"]), 64)
    pairs, ch = w["pairs"][:nal], chains[:nal]
    texts = [w["text"][p[0]:p[0] + p[1]] for p in pairs]
    pats = [w["pattern"][p[2]:p[2] + p[3]] for p in pairs]
    bands = chain_bands(dict(w, pairs=pairs), ch)
    x = engine.NO_XDROP if xdrop is None else xdrop
    rounds = max(3, args.rounds // 2)
    a, got = aligned_stats(engine, lambda: engine.align_pairs_affine(0, texts, pats, w["S"], go, ge, xdrop=x, chains=ch), rounds)
    b, alt = aligned_stats(engine, lambda: engine.align_pairs_affine(0, texts, pats, w["S"], go, ge, bands=bands), rounds)
    sc = engine.score_batch(0, texts, pats, w["S"], go, gap_extend=ge, xdrop=x, chains=ch)
    assert [r["score"] for r in got] == sc["score"].tolist(), "the chains aligner's scores differ from the chains scorer's"
    full = sum(64 * ((p[1] + 126) // 64) * 256 * -(-p[3] // 512) for p in pairs)
    return {"name": w["name"] + "_aligned", "pairs": nal, "gap_open": go, "gap_extend": ge, "xdrop": xdrop, "chains": a, "band_at": b,
            "full_rectangle_dir_bytes": full, "equal_scores": int(sum(r["score"] == q["score"] for r, q in zip(got, alt))),
            "equal_strings": int(sum(r["aligned_text"] == q["aligned_text"] and r["aligned_pattern"] == q["aligned_pattern"] for r, q in zip(got, alt))),
            "chains_over_band_at_wall": round(a["end_to_end_wall"]["median_ms"] / b["end_to_end_wall"]["median_ms"], 4),
            "chains_over_band_at_arena": round(a["arena_bytes"] / max(b["arena_bytes"], 1), 4)}


def chaining_call(engine, anchors, cp: dict):
    """The raw C calls of --mode chaining on anchors packed once: (device, host), each returning (results, flat
    seeds, offsets) of one call, the chain set destroyed."""
    import ctypes
    n = len(anchors)
    flat = np.ascontiguousarray(np.concatenate(list(anchors) + [np.zeros((1, 3), np.int64)]).astype(np.uint64))
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(a) for a in anchors], dtype=np.uint64)
    params = engine.SaChainParams(cp["match"], cp["gap_open"], cp["gap_extend"], cp["skip"], cp["max_gap"], cp["max_diag"], cp["lookback"])
    res = (engine.SaChainResult * max(1, n))()

    def call(host: bool):
        handle = ctypes.c_void_p()
        head = (ctypes.byref(params), flat.ctypes.data, off.ctypes.data, n)
        rc = engine.lib.sa_chain_anchors_host(*head, res, ctypes.byref(handle)) if host else engine.lib.sa_chain_anchors(*head, 0, res, ctypes.byref(handle))
        if rc != 0:
            raise engine.SaError(rc, engine.lib.sa_last_error().decode())
        return handle

    def fetch(handle):
        rows = np.frombuffer(res, dtype=engine.CHAIN_DTYPE, count=n).copy()
        coff = np.ctypeslib.as_array(ctypes.cast(engine.lib.sa_chain_set_off(handle), ctypes.POINTER(ctypes.c_uint64)), (n + 1,)).copy()
        addr = engine.lib.sa_chain_set_seeds(handle)
        seeds = np.ctypeslib.as_array(ctypes.cast(addr, ctypes.POINTER(ctypes.c_uint64)), (int(coff[n]), 3)).copy() if addr else np.zeros((0, 3), np.uint64)
        engine.lib.sa_chain_set_destroy(handle)
        return rows, seeds, coff
    return call, fetch, engine.lib.sa_chain_set_destroy


def chaining_rows(args, engine, name: str, anchors, cp: dict) -> dict:
    """(a) of --mode chaining: sa_chain_anchors end to end (the C call: validation, upload, both kernels, the copies
    back) with its dp_ms and walk_ms, against sa_chain_anchors_host on the same anchors, alternated round by round."""
    call, fetch, destroy = chaining_call(engine, anchors, cp)
    dev, host = fetch(call(False)), fetch(call(True))  # warm-up, and (K2) on the workload
    assert all((a == b).all() for a, b in zip(dev, host)), "the device chains differ from the host function's"
    counts = np.array([len(a) for a in anchors])
    row = {"name": name, "pairs": len(anchors), "params": cp, "anchors_per_pair": round(float(counts.mean()), 1), "anchors_max": int(counts.max()),
           "seeds_per_pair": round(float(dev[0]["num_seeds"].mean()), 1), "device_equals_host": True}
    ms = {"device": [], "host": [], "dp": [], "walk": []}
    for _ in range(args.rounds):
        for key in ("device", "host"):
            t0 = time.perf_counter()
            handle = call(key == "host")
            ms[key].append((time.perf_counter() - t0) * 1e3)
            destroy(handle)
            if key == "device":
                st = engine.chain_last_stats()
                ms["dp"].append(st["dp_ms"]), ms["walk"].append(st["walk_ms"])
                row["device_bytes"] = st["device_bytes"]
    row.update({"device_end_to_end_wall": stats(ms["device"]), "host_wall": stats(ms["host"]), "dp_kernel": stats(ms["dp"]), "walk_kernel": stats(ms["walk"])})
    row["device_over_host"] = round(statistics.median(ms["device"]) / statistics.median(ms["host"]), 4)
    return row


def chaining_scores_row(args, engine, w, chained, derived, go: int, ge: int, xdrop, k: int) -> dict:
    """(b) of --mode chaining: the chains scorer on the chains of sa_chain_anchors and on the alignment-derived ones of
    exact_match_chains, pair by pair. A pair whose chain is empty is left out of both calls."""
    keep = [i for i, c in enumerate(chained) if len(c)]
    pairs = [w["pairs"][i] for i in keep]
    texts = [w["text"][p[0]:p[0] + p[1]] for p in pairs]
    pats = [w["pattern"][p[2]:p[2] + p[3]] for p in pairs]
    x = engine.NO_XDROP if xdrop is None else xdrop
    a = engine.score_batch(0, texts, pats, w["S"], go, gap_extend=ge, xdrop=x, chains=[chained[i] for i in keep])["score"].astype(np.int64)
    b = engine.score_batch(0, texts, pats, w["S"], go, gap_extend=ge, xdrop=x, chains=[derived[i] for i in keep])["score"].astype(np.int64)
    return {"name": f"{w['name']}_chains_scores_k{k}", "pairs": len(keep), "pairs_without_a_chain": len(chained) - len(keep), "gap_open": go, "gap_extend": ge,
            "xdrop": xdrop, "equal": int((a == b).sum()), "chained_higher": int((a > b).sum()), "chained_lower": int((a < b).sum()),
            "largest_deficit": int(max(0, (b - a).max())), "largest_surplus": int(max(0, (a - b).max())),
            "seeds_per_pair_chained": round(float(np.mean([len(chained[i]) for i in keep])), 1),
            "seeds_per_pair_derived": round(float(np.mean([len(derived[i]) for i in keep])), 1)}


def next_profile_dir() -> str:
    """The next unused profiles/rNN."""
    taken = [int(d[1:]) for d in os.listdir(os.path.join(ROOT, "profiles")) if d[0] == "r" and d[1:].isdigit()]
    return f"r{max(taken, default=0) + 1:02d}"


def cigar_row(args, engine, name: str, texts, pats, S, go: int, ge: int, kw: dict) -> dict:
    """--mode cigar: align_pairs_affine with strings and align_pairs_cigar on the same pairs and keywords, alternated
    round by round in this process after one warm-up each: wall time end to end (host arrays in, Python dicts out),
    the device times of the fill, the walks and the encoder, and the bytes each call copies to the host beside its
    per-pair records. The CIGARs are checked against cigar_from_strings of the string call's strings first."""
    import time
    strings = lambda: engine.align_pairs_affine(0, texts, pats, S, go, ge, **kw)  # noqa: E731
    cigars = lambda: engine.align_pairs_cigar(0, texts, pats, S, go, ge, **kw)  # noqa: E731
    want, got = strings(), cigars()
    for w_, g in zip(want, got):
        ref = engine.cigar_from_strings(w_["aligned_text"], w_["aligned_pattern"])
        assert g["cigar_string"] == ref["cigar_string"] and g["score"] == w_["score"], "a device CIGAR differs from its strings'"
    ms = {k: {"wall": [], "fill": [], "walk": [], "encode": []} for k in ("strings", "cigar")}
    st = {}
    for _ in range(args.rounds):
        for k, call in (("strings", strings), ("cigar", cigars)):
            t0 = time.perf_counter()
            call()
            ms[k]["wall"].append((time.perf_counter() - t0) * 1e3)
            a = engine.affine_last_stats()
            ms[k]["fill"].append(a["fill_ms"]), ms[k]["walk"].append(a["walk_ms"])
            if k == "cigar":
                st = engine.cigar_last_stats()
                ms[k]["encode"].append(st["encode_ms"])
    row = {"name": name, "pairs": len(texts), "gap_open": go, "gap_extend": ge, "keywords": sorted(kw), "cigars_equal_the_strings": True,
           "mean_letters": round(float(np.mean([len(t) + len(p) for t, p in zip(texts, pats)])) / 2, 1),
           "mean_ops": round(float(np.mean([g["num_ops"] for g in got])), 1)}
    for k in ms:
        row[k] = {"end_to_end_wall": stats(ms[k]["wall"]), "fill": stats(ms[k]["fill"]), "walk": stats(ms[k]["walk"])}
        row[k]["non_device_ms"] = round(row[k]["end_to_end_wall"]["median_ms"] - row[k]["fill"]["median_ms"] - row[k]["walk"]["median_ms"], 3)
    row["cigar"]["encode"] = stats(ms["cigar"]["encode"])
    row["cigar"]["non_device_ms"] = round(row["cigar"]["non_device_ms"] - row["cigar"]["encode"]["median_ms"], 3)
    row["strings"]["string_bytes_to_host"] = st["string_bytes_not_copied"]
    row["cigar"]["ops_bytes_to_host"] = st["ops_bytes"]
    row["cigar"]["string_bytes_not_copied"] = st["string_bytes_not_copied"]
    row["cigar_over_strings_wall"] = round(row["cigar"]["end_to_end_wall"]["median_ms"] / row["strings"]["end_to_end_wall"]["median_ms"], 4)
    return row


def width_model_cost(pairs, width: int, R: int, local: bool) -> int:
    """The planner's instruction count of a banded pair (sa_score_plan.h: band_ext, band_window_at): the affine
    step of the local (an extension) or the global program, charged jmax - jmin + 64 times per strip that holds
    an in-band cell."""
    step, rows, total = 18 + R * (14 if local else 10), 64 * R, 0
    for _, n, _, m in pairs:
        if n == 0 or m == 0:
            continue
        lo, hi = max(-width, -m), min(width, n)
        for first in range(1, m + 1, rows):
            ia, ib = max(first, 1 - hi), min(m, first + rows - 1, n - lo)
            if ia <= ib:
                total += (min(n, ib + hi) - max(1, ia + lo) + 64) * step
    return total


def aligned_stats(engine, call, rounds: int) -> dict:
    """One aligner call, `rounds` times after a warm-up: wall time end to end and sa_affine_last_stats."""
    import time
    wall, fill, walk, st = [], [], [], {}
    for rnd in range(rounds + 1):
        t0 = time.perf_counter()
        got = call()
        ms = (time.perf_counter() - t0) * 1e3
        st = engine.affine_last_stats()
        if rnd:
            wall.append(ms), fill.append(st["fill_ms"]), walk.append(st["walk_ms"])
    return {"end_to_end_wall": stats(wall), "fill": stats(fill), "walk": stats(walk), "arena_bytes": st["arena_bytes"],
            "num_chunks": st["num_chunks"]}, got


def extend_band_rows(args, engine, w, dt, dp, go: int, ge: int, xdrop) -> dict:
    """The unbanded extension scorer, and per width the banded extension scorer and the band-at global scorer
    on {-w, w}, at one X-drop (None: no drop); alternated."""
    pairs, cells = w["pairs"], sum(p[1] * p[3] for p in w["pairs"])
    x = engine.NO_XDROP if xdrop is None else xdrop
    sc = {"extend": engine.Scorer(0, w["S"], go, pairs, gap_extend=ge, xdrop=x)}
    for wd in args.width:
        sc[f"extend_band_{wd}"] = engine.Scorer(0, w["S"], go, pairs, gap_extend=ge, xdrop=x, width=wd)
        sc[f"band_at_global_{wd}"] = engine.Scorer(0, w["S"], go, pairs, gap_extend=ge, bands=[(-wd, wd)] * len(pairs))
    row = {"name": w["name"] + ("_xdrop" if xdrop is not None else "_no_xdrop"), "pairs": len(pairs), "cells": cells, "gap_open": go,
           "gap_extend": ge, "xdrop": xdrop, "widths": list(args.width), "scorers": {k: s.info() for k, s in sc.items()}}
    res = {}
    for _ in range(2):  # warm-up, and the results
        for k, s in sc.items():
            s.run(dt.data_ptr(), dp.data_ptr())
            res[k] = s.results().copy()
    ms = {k: [] for k in sc}
    for _ in range(args.rounds):
        for k, s in sc.items():
            ms[k].append(timed(lambda: s.run(dt.data_ptr(), dp.data_ptr()), lambda: s.results()))
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k, s in sc.items():
        row[k + "_run"] = stats(ms[k])
        s.close()
    Rf = row["scorers"]["extend"]["rows_per_lane"]
    full_model = model_cost(pairs, Rf, True, True)
    for wd in args.width:
        b, a = f"extend_band_{wd}", f"band_at_global_{wd}"
        Rb, Ra = row["scorers"][b]["rows_per_lane"], row["scorers"][a]["rows_per_lane"]
        assert (res[b]["score"] <= res["extend"]["score"]).all() or xdrop is not None, "a banded score exceeds the unbanded one (W3)"
        row[f"width_{wd}"] = {
            "band_over_unbanded": round(med[b] / med["extend"], 4),
            "model_band_over_unbanded": round(width_model_cost(pairs, wd, Rb, True) / full_model, 4),
            "band_over_band_at_global": round(med[b] / med[a], 4),
            "model_band_over_band_at_global": round(width_model_cost(pairs, wd, Rb, True) / width_model_cost(pairs, wd, Ra, False), 4),
            "scores_equal_the_unbanded": int((res[b]["score"] == res["extend"]["score"]).sum()),
            "cells_equal_the_unbanded": int(((res[b]["score"] == res["extend"]["score"]) & (res[b]["end_text"] == res["extend"]["end_text"]) &
                                             (res[b]["end_pattern"] == res["extend"]["end_pattern"])).sum())}
    # aligned: the first pairs end to end, unbanded and at each width
    nal = min(len(pairs), 16 if args.small else 64)
    texts = [w["text"][p[0]:p[0] + p[1]] for p in pairs[:nal]]
    pats = [w["pattern"][p[2]:p[2] + p[3]] for p in pairs[:nal]]
    rounds = max(3, args.rounds // 2)
    row["aligned"] = {"pairs": nal}
    row["aligned"]["unbanded"], full = aligned_stats(engine, lambda: engine.align_pairs_affine(0, texts, pats, w["S"], go, ge, xdrop=x), rounds)
    for wd in args.width:
        st, got = aligned_stats(engine, lambda: engine.align_pairs_affine(0, texts, pats, w["S"], go, ge, xdrop=x, width=wd), rounds)
        assert [g["score"] for g in got] == res[f"extend_band_{wd}"]["score"][:nal].tolist(), "the banded aligner and scorer differ"
        same = [k for k in range(nal) if got[k]["score"] == full[k]["score"] and got[k]["num_bytes"] == full[k]["num_bytes"]]
        assert all(got[k] == full[k] for k in same), "equal scores with different strings"
        st["scores_equal_the_unbanded"] = len(same)
        row["aligned"][f"width_{wd}"] = st
    return row


def seeds_band_rows(args, engine, w, seeds, wc, seeds_c, gap: int, gap_extend: int, xdrop) -> dict:
    """The unbanded seeds scorer on the whole windows and on the clipped ones, and per width the banded seeds
    scorer on the whole windows; alternated."""
    import torch
    x = engine.NO_XDROP if xdrop is None else xdrop
    dev = {k: (torch.from_numpy(v["text"]).cuda(), torch.from_numpy(v["pattern"]).cuda()) for k, v in (("w", w), ("c", wc))}
    sc = {"seeds": engine.Scorer(0, w["S"], gap, w["pairs"], gap_extend=gap_extend, xdrop=x, seeds=seeds),
          "seeds_clipped": engine.Scorer(0, w["S"], gap, wc["pairs"], gap_extend=gap_extend, xdrop=x, seeds=seeds_c)}
    ptr = {"seeds": dev["w"], "seeds_clipped": dev["c"]}
    for wd in args.width:
        sc[f"seeds_band_{wd}"] = engine.Scorer(0, w["S"], gap, w["pairs"], gap_extend=gap_extend, xdrop=x, seeds=seeds, width=wd)
        ptr[f"seeds_band_{wd}"] = dev["w"]
    run = {k: (lambda k=k: sc[k].run(ptr[k][0].data_ptr(), ptr[k][1].data_ptr())) for k in sc}
    row = {"name": w["name"] + "_seeds_band" + ("_xdrop" if xdrop is not None else "_no_xdrop"), "pairs": len(w["pairs"]),
           "cells": sum(p[1] * p[3] for p in w["pairs"]), "clipped_cells": sum(p[1] * p[3] for p in wc["pairs"]), "gap": gap,
           "gap_extend": gap_extend, "xdrop": xdrop, "widths": list(args.width), "scorers": {k: s.info() for k, s in sc.items()}}
    res = {}
    for _ in range(2):
        for k in sc:
            run[k]()
            res[k] = sc[k].results().copy()
    ms = {k: [] for k in sc}
    for _ in range(args.rounds):
        for k in sc:
            ms[k].append(timed(run[k], lambda: sc[k].results()))
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k, s in sc.items():
        row[k + "_run"] = stats(ms[k])
        s.close()
    left, right = halves_workloads(w, seeds)
    items = [(0, n, 0, m) for _, n, _, m in left["pairs"] + right["pairs"]]
    full_model = model_cost(items, row["scorers"]["seeds"]["rows_per_lane"], True, gap != gap_extend)
    for wd in args.width:
        b = f"seeds_band_{wd}"
        row[f"width_{wd}"] = {
            "band_over_whole_windows": round(med[b] / med["seeds"], 4),
            "model_band_over_whole_windows": round(width_model_cost(items, wd, row["scorers"][b]["rows_per_lane"], True) / full_model, 4),
            "band_over_clipped_windows": round(med[b] / med["seeds_clipped"], 4),
            "share_of_scores_equal_the_whole_windows": round(float((res[b]["score"] == res["seeds"]["score"]).mean()), 4)}
    row["share_of_clipped_scores_equal_the_whole_windows"] = round(float((res["seeds_clipped"]["score"] == res["seeds"]["score"]).mean()), 4)
    # aligned: the first reads end to end
    nal = min(len(w["pairs"]), 4000)
    texts = [w["text"][p[0]:p[0] + p[1]] for p in w["pairs"][:nal]]
    pats = [w["pattern"][p[2]:p[2] + p[3]] for p in w["pairs"][:nal]]
    sd = seeds[:nal]
    rounds = max(3, args.rounds // 2)
    row["aligned"] = {"pairs": nal}
    row["aligned"]["unbanded"], full = aligned_stats(engine, lambda: engine.align_pairs_affine(0, texts, pats, w["S"], gap, gap_extend, xdrop=x, seeds=sd), rounds)
    for wd in args.width:
        st, got = aligned_stats(engine, lambda: engine.align_pairs_affine(0, texts, pats, w["S"], gap, gap_extend, xdrop=x, seeds=sd, width=wd), rounds)
        assert [g["score"] for g in got] == res[f"seeds_band_{wd}"]["score"][:nal].tolist(), "the banded seeds aligner and scorer differ"
        st["alignments_equal_the_unbanded"] = sum(a == b for a, b in zip(got, full))
        row["aligned"][f"width_{wd}"] = st
    return row


def fit_rows(args, engine, w, dt, dp, gap: int, gap_extend) -> dict:
    """The fit, global and local scorers of one gap model on the mapping workload, alternated."""
    cells = sum(p[1] * p[3] for p in w["pairs"])
    affine = gap_extend is not None
    sc = {k: engine.Scorer(m, w["S"], gap, w["pairs"], gap_extend=gap_extend) for k, m in MODES.items()}
    row = {"name": w["name"] + ("_affine" if affine else "_linear"), "pairs": len(w["pairs"]), "cells": cells, "gap": gap,
           "gap_extend": gap_extend, "scorers": {k: s.info() for k, s in sc.items()}}
    res = {}
    for k, s in sc.items():  # warm-up
        s.run(dt.data_ptr(), dp.data_ptr())
        res[k] = s.results()
    assert (res["global"]["score"] <= res["fit"]["score"]).all() and (res["fit"]["score"] <= res["local"]["score"]).all()
    ms = {k: [] for k in sc}
    for _ in range(args.rounds):
        for k, s in sc.items():
            ms[k].append(timed(lambda: s.run(dt.data_ptr(), dp.data_ptr()), lambda: s.results()))
    for k, s in sc.items():
        row[k + "_run"] = stats(ms[k])
        row[k + "_gcups"] = round(cells / statistics.median(ms[k]) / 1e6, 1)
        s.close()
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = max(ms["local"]) - min(ms["local"])
    model = {k: model_cost(w["pairs"], row["scorers"][k]["rows_per_lane"], k == "local", affine, k == "fit") for k in sc}
    row["fit_over_global"] = round(med["fit"] / med["global"], 3)
    row["model_fit_over_global"] = round(model["fit"] / model["global"], 3)
    row["fit_over_local"] = round(med["fit"] / med["local"], 3)
    row["model_fit_over_local"] = round(model["fit"] / model["local"], 3)
    row["local_spread_ms"] = round(spread, 3)
    row["fit_within_local_plus_spread"] = bool(med["fit"] <= med["local"] + spread)
    sweep = {}
    for R in (1, 2, 4, 8):
        s = engine.Scorer(2, w["S"], gap, w["pairs"], rows_per_lane=R, gap_extend=gap_extend)
        s.run(dt.data_ptr(), dp.data_ptr())
        assert s.results().tolist() == res["fit"].tolist(), f"fit R = {R} results differ"
        t = [timed(lambda: s.run(dt.data_ptr(), dp.data_ptr()), lambda: s.results()) for _ in range(max(3, args.rounds))]
        sweep[str(R)] = dict(stats(t), num_waves=s.info()["num_waves"], model=model_cost(w["pairs"], R, False, affine, True))
        s.close()
    row["fit_rows_per_lane_sweep"] = sweep
    return row


def fit_hits_row(args, engine, w) -> dict:
    """search(k) in fit and in local mode on the search workload under gap open / gap extend: end to
    end (wall clock) with the device time of the traced fill and of the walk of the hits."""
    import time
    texts = [w["text"][o:o + n] for o, n, _, _ in w["pairs"]]
    q, k, ge = w["pattern"], args.hits or 100, args.gap_extend if args.gap_extend is not None else 2
    row = {"name": w["name"] + "_fit_hits", "pairs": len(w["pairs"]), "hits": k, "gap_open": args.gap_open, "gap_extend": ge}
    runs = {name: (lambda m=m: engine.search(m, q, texts, w["S"], args.gap_open, k, gap_extend=ge)) for name, m in
            (("fit", 2), ("local", 1))}
    out = {name: {"wall": [], "fill": [], "walk": []} for name in runs}
    for name, run in runs.items():
        _, hits = run()
        row[name + "_hit_cells"] = sum(len(texts[h["index"]]) * len(q) for h in hits)
    for _ in range(args.rounds):
        for name, run in runs.items():
            t0 = time.perf_counter()
            run()
            out[name]["wall"].append((time.perf_counter() - t0) * 1e3)
            st = engine.affine_last_stats()
            out[name]["fill"].append(st["fill_ms"])
            out[name]["walk"].append(st["walk_ms"])
            row[name + "_direction_arena_bytes"] = st["arena_bytes"]
    for name in runs:
        row[name + "_traced_fill_of_hits"] = stats(out[name]["fill"])
        row[name + "_walk_of_hits"] = stats(out[name]["walk"])
        row[name + "_search_end_to_end"] = stats(out[name]["wall"])
    return row


def affine_rows(args, engine, w, dt, dp) -> dict:
    """Linear against affine Scorer.run on one workload, alternated; then the affine forced-R sweep."""
    cells = sum(p[1] * p[3] for p in w["pairs"])
    local = w["mode"] == 1
    lin = engine.Scorer(w["mode"], w["S"], w["gap"], w["pairs"])
    aff = engine.Scorer(w["mode"], w["S"], args.gap_open, w["pairs"], gap_extend=args.gap_extend)
    row = {"name": w["name"], "pairs": len(w["pairs"]), "cells": cells, "gap": w["gap"], "gap_open": args.gap_open,
           "gap_extend": args.gap_extend, "linear": lin.info(), "affine": aff.info()}
    run_l = lambda: lin.run(dt.data_ptr(), dp.data_ptr())  # noqa: E731
    run_a = lambda: aff.run(dt.data_ptr(), dp.data_ptr())  # noqa: E731
    run_l()
    lin.results()
    run_a()
    a_scores = aff.results()["score"].copy()
    tl, ta = [], []
    for _ in range(args.rounds):
        tl.append(timed(run_l, lambda: lin.results()))
        ta.append(timed(run_a, lambda: aff.results()))
    row["linear_run"], row["affine_run"] = stats(tl), stats(ta)
    row["linear_gcups"] = round(cells / statistics.median(tl) / 1e6, 1)
    row["affine_gcups"] = round(cells / statistics.median(ta) / 1e6, 1)
    row["affine_over_linear"] = round(statistics.median(ta) / statistics.median(tl), 3)
    row["model_affine_over_linear"] = round(model_cost(w["pairs"], row["affine"]["rows_per_lane"], local, True) /
                                            model_cost(w["pairs"], row["linear"]["rows_per_lane"], local, False), 3)
    lin.close()
    aff.close()
    sweep = {}
    for R in (1, 2, 4, 8):
        s = engine.Scorer(w["mode"], w["S"], args.gap_open, w["pairs"], rows_per_lane=R, gap_extend=args.gap_extend)
        s.run(dt.data_ptr(), dp.data_ptr())
        assert (s.results()["score"] == a_scores).all(), f"{w['name']}: affine R = {R} scores differ"
        ms = [timed(lambda: s.run(dt.data_ptr(), dp.data_ptr()), lambda: s.results()) for _ in range(max(3, args.rounds))]
        sweep[str(R)] = dict(stats(ms), num_waves=s.info()["num_waves"], model=model_cost(w["pairs"], R, local, True))
        s.close()
    row["affine_rows_per_lane_sweep"] = sweep
    return row


def hits_row(args, engine, w, dt, dp) -> dict:
    """--hits K on the search workload: the affine Scorer.run alone (device events), and
    search(k=K, gap_extend=) end to end (wall clock, from host arrays to host strings) with the device
    time of its traced fill and of its walk (sa_affine_last_stats), beside the linear search(k=K) of the
    same data; alternated round by round after a warm-up. Without --gap-extend the linear search alone
    (with --tree: that of another checkout's library, e.g. the parent commit's)."""
    import time
    texts = [w["text"][o:o + n] for o, n, _, _ in w["pairs"]]
    q = w["pattern"]
    if args.gap_extend is None:
        run = lambda: engine.search(w["mode"], q, texts, w["S"], w["gap"], args.hits)  # noqa: E731
        _, hits = run()
        ms = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            run()
            ms.append((time.perf_counter() - t0) * 1e3)
        return {"name": w["name"] + "_hits_linear", "pairs": len(w["pairs"]), "hits": len(hits), "linear_gap": w["gap"],
                "hit_cells": sum(len(texts[h["index"]]) * len(q) for h in hits), "library_build_id": engine.lib.sa_build_id().decode(),
                "search_linear_end_to_end": stats(ms)}
    aff = engine.Scorer(w["mode"], w["S"], args.gap_open, w["pairs"], gap_extend=args.gap_extend)
    run_a = lambda: aff.run(dt.data_ptr(), dp.data_ptr())  # noqa: E731

    def wall(fn):
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    search_a = lambda: engine.search(w["mode"], q, texts, w["S"], args.gap_open, args.hits, gap_extend=args.gap_extend)  # noqa: E731
    search_l = lambda: engine.search(w["mode"], q, texts, w["S"], w["gap"], args.hits)  # noqa: E731
    run_a()
    a_scores = aff.results()["score"].copy()
    scores, hits = search_a()
    assert (scores["score"] == a_scores).all(), "search and scorer scores differ"
    assert all(h["score"] == int(a_scores[h["index"]]) for h in hits), "a hit's alignment score is not its rank score"
    search_l()
    t_run, t_sa, t_sl, t_fill, t_walk = [], [], [], [], []
    st = {}
    for _ in range(args.rounds):
        t_run.append(timed(run_a, lambda: aff.results()))
        t_sa.append(wall(search_a)[0])
        st = engine.affine_last_stats()
        t_fill.append(st["fill_ms"])
        t_walk.append(st["walk_ms"])
        t_sl.append(wall(search_l)[0])
    aff.close()
    hit_cells = sum(len(texts[h["index"]]) * len(q) for h in hits)
    return {"name": w["name"] + "_hits", "pairs": len(w["pairs"]), "hits": len(hits), "gap_open": args.gap_open,
            "gap_extend": args.gap_extend, "linear_gap": w["gap"], "hit_cells": hit_cells,
            "direction_arena_bytes": st.get("arena_bytes"), "chunks": st.get("num_chunks"),
            "affine_scorer_run": stats(t_run), "traced_fill_of_hits": stats(t_fill), "walk_of_hits": stats(t_walk),
            "search_affine_end_to_end": stats(t_sa), "search_linear_end_to_end": stats(t_sl)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="profiles/r09/score_bench.json; --mode fit: profiles/r13/score_fit_bench.json")
    ap.add_argument("--rounds", type=int, default=None, help="timed rounds: 5, --mode extend 7")
    ap.add_argument("--small", action="store_true", help="a sixteenth of the batch, a tenth of the texts")
    ap.add_argument("--gap-extend", type=int, default=None, help="compare the affine scorer with the linear one")
    ap.add_argument("--gap-open", type=int, default=11, help="gap-open penalty of the affine scorer")
    ap.add_argument("--hits", type=int, default=None,
                    help="time search(k=HITS) on the search workload; with --gap-extend also its traced fill and its walk")
    ap.add_argument("--exit-gap", type=int, nargs=2, default=[16, 4], metavar=("OPEN", "EXTEND"),
                    help="--mode extend: the penalties of the early-exit comparison")
    ap.add_argument("--xdrop", type=int, default=100, help="--mode extend: the X-drop of the early-exit comparison")
    ap.add_argument("--mode", choices=["fit", "ends", "mapped", "extend", "seeds", "chain", "cigar", "chaining"], default=None,
                    help="fit: the fit scorers against the global and local ones on a read-mapping workload; "
                         "ends: the ends-free scorers against the fit and global ones on it and on an overlap workload; "
                         "mapped: the band-at fit scorer around each read's true offset against the unbanded fit scorer "
                         "(profiles/r16/score_mapped_bench.json); "
                         "extend: the extension scorers against the local ones, with and without an X-drop "
                         "(profiles/r17/score_extend_bench.json); "
                         "seeds: the seeds scorer and aligner against two extension calls on host-reversed halves and "
                         "against the fit scorer (profiles/r18/score_seeds_bench.json); "
                         "chain: the chains scorer and aligner on 10000-letter reads against the composition of existing calls "
                         "and against the band-at global scorer (profiles/r22/score_chain_bench.json); "
                         "cigar: align_pairs_cigar against align_pairs_affine with strings on the chain workload (all its reads, "
                         "and the first 64) and on 4000 reads of the seeds workload (profiles/r23/score_cigar_bench.json); "
                         "chaining: sa_chain_anchors against sa_chain_anchors_host on the k-mer anchors of the long reads, and the chains "
                         "scorer on its chains against the alignment-derived ones (the next unused profiles/rNN/score_chaining_bench.json)")
    ap.add_argument("--band", type=int, nargs="+", default=None,
                    help="half-widths: the banded scorer and aligner against the unbanded ones on related 20000-letter pairs")
    ap.add_argument("--width", type=int, nargs="+", default=None,
                    help="--mode extend, --mode seeds: the banded extension and the banded seeds functions at these half-widths "
                         "(profiles/r21/score_extend_band_bench.json, profiles/r21/score_seeds_band_bench.json)")
    ap.add_argument("--tree", default=None,
                    help="take the sa_amd package and its library from this checkout (e.g. one of the parent commit, built)")
    args = ap.parse_args()
    if args.rounds is None:
        args.rounds = 7 if args.mode in ("extend", "seeds", "chain", "cigar", "chaining") else 5
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", *(("r14", "score_band_bench.json") if args.band else
                                                    ("r13", "score_fit_bench.json") if args.mode == "fit" else
                                                    ("r15", "score_ends_bench.json") if args.mode == "ends" else
                                                    ("r16", "score_mapped_bench.json") if args.mode == "mapped" else
                                                    ("r21", "score_extend_band_bench.json") if args.mode == "extend" and args.width else
                                                    ("r21", "score_seeds_band_bench.json") if args.mode == "seeds" and args.width else
                                                    ("r22", "score_chain_bench.json") if args.mode == "chain" else
                                                    ("r23", "score_cigar_bench.json") if args.mode == "cigar" else
                                                    (next_profile_dir(), "score_chaining_bench.json") if args.mode == "chaining" else
                                                    ("r17", "score_extend_bench.json") if args.mode == "extend" else
                                                    ("r18", "score_seeds_bench.json") if args.mode == "seeds" else ("r09", "score_bench.json")))
    if args.tree:
        sys.path.insert(0, os.path.join(os.path.abspath(args.tree), "sequence-alignment-gpu_amd", "python"))
    import torch
    if not torch.cuda.is_available():
        print("score_bench: no GPU", file=sys.stderr)
        return 1
    from sa_amd import engine
    report = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "library": "another checkout (--tree)" if args.tree else "this tree",
              "workloads": []}
    if args.band:
        w = related_workload(args.small)
        dt, dp = torch.from_numpy(w["text"]).cuda(), torch.from_numpy(w["pattern"]).cuda()
        row = band_rows(args, engine, w, dt, dp)
        report["workloads"].append(row)
        print(json.dumps(row), flush=True)
        del dt, dp
    elif args.mode == "fit":
        w = mapping_workload(args.small)
        dt, dp = torch.from_numpy(w["text"]).cuda(), torch.from_numpy(w["pattern"]).cuda()
        for gap, ge in ((5, None), (args.gap_open, args.gap_extend if args.gap_extend is not None else 2)):
            row = fit_rows(args, engine, w, dt, dp, gap, ge)
            report["workloads"].append(row)
            print(json.dumps(row), flush=True)
        del dt, dp
        row = fit_hits_row(args, engine, next(workloads(args.small, search_only=True)))
        report["workloads"].append(row)
        print(json.dumps(row), flush=True)
    elif args.mode == "mapped":
        w = mapped_workload(args.small)
        dt, dp = torch.from_numpy(w["text"]).cuda(), torch.from_numpy(w["pattern"]).cuda()
        for gap, ge in ((5, None), (args.gap_open, args.gap_extend if args.gap_extend is not None else 2)):
            row = mapped_rows(args, engine, w, dt, dp, gap, ge)
            report["workloads"].append(row)
            print(json.dumps(row), flush=True)
        del dt, dp
    elif args.mode == "extend" and args.width:
        w = chimeric_workload(args.small)
        dt, dp = torch.from_numpy(w["text"]).cuda(), torch.from_numpy(w["pattern"]).cuda()
        for xdrop in (None, args.xdrop):
            row = extend_band_rows(args, engine, w, dt, dp, args.exit_gap[0], args.exit_gap[1], xdrop)
            report["workloads"].append(row)
            print(json.dumps(row), flush=True)
        del dt, dp
    elif args.mode == "seeds" and args.width:
        w = mapped_workload(args.small)
        ge = args.gap_extend if args.gap_extend is not None else 2
        seeds, spans = longest_match_seeds(engine, w, args.gap_open, ge)
        wc, seeds_c = clip_workload(w, seeds, spans)
        for xdrop in (None, args.xdrop):
            row = seeds_band_rows(args, engine, w, seeds, wc, seeds_c, args.gap_open, ge, xdrop)
            report["workloads"].append(row)
            print(json.dumps(row), flush=True)
    elif args.mode == "extend":
        w = mapping_workload(args.small)
        dt, dp = torch.from_numpy(w["text"]).cuda(), torch.from_numpy(w["pattern"]).cuda()
        for gap, ge in ((5, None), (args.gap_open, args.gap_extend if args.gap_extend is not None else 2)):
            row = extend_same_work_rows(args, engine, w, dt, dp, gap, ge)
            report["workloads"].append(row)
            print(json.dumps(row), flush=True)
        del dt, dp
        w = chimeric_workload(args.small)
        dt, dp = torch.from_numpy(w["text"]).cuda(), torch.from_numpy(w["pattern"]).cuda()
        row = extend_early_exit_row(args, engine, w, dt, dp, args.exit_gap[0], args.exit_gap[1], args.xdrop)
        report["workloads"].append(row)
        print(json.dumps(row), flush=True)
        del dt, dp
    elif args.mode == "seeds":
        w = mapped_workload(args.small)
        ge = args.gap_extend if args.gap_extend is not None else 2
        seeds, spans = longest_match_seeds(engine, w, args.gap_open, ge)
        report["seed_length"] = {"mean": round(float(np.mean([s[2] for s in seeds])), 1), "min": int(min(s[2] for s in seeds)),
                                 "max": int(max(s[2] for s in seeds))}
        wc, seeds_c = clip_workload(w, seeds, spans)
        for ww, sd in ((w, seeds), (wc, seeds_c)):
            for gap, gx in ((5, 5), (args.gap_open, ge)):
                for xdrop in (None, args.xdrop):
                    row = seeds_rows(args, engine, ww, sd, gap, gx, xdrop)
                    report["workloads"].append(row)
                    print(json.dumps(row), flush=True)
        row = seeds_aligned_row(args, engine, w, seeds, args.gap_open, ge, args.xdrop)
        report["workloads"].append(row)
        print(json.dumps(row), flush=True)
    elif args.mode == "chain":
        w = chain_workload(args.small)
        ge = args.gap_extend if args.gap_extend is not None else 2
        chains = exact_match_chains(engine, w, args.gap_open, ge)
        for xdrop in (None, args.xdrop):
            row = chain_rows(args, engine, w, chains, args.gap_open, ge, xdrop)
            report["workloads"].append(row)
            print(json.dumps(row), flush=True)
        row = chain_aligned_row(args, engine, w, chains, args.gap_open, ge, args.xdrop)
        report["workloads"].append(row)
        print(json.dumps(row), flush=True)
    elif args.mode == "cigar":
        ge = args.gap_extend if args.gap_extend is not None else 2
        x = engine.NO_XDROP if args.xdrop is None else args.xdrop
        w = chain_workload(args.small)
        chains = exact_match_chains(engine, w, args.gap_open, ge)
        texts = [w["text"][p[0]:p[0] + p[1]] for p in w["pairs"]]
        pats = [w["pattern"][p[2]:p[2] + p[3]] for p in w["pairs"]]
        for count in (len(texts), 64):
            row = cigar_row(args, engine, f"long_reads_chains_{count}", texts[:count], pats[:count], w["S"], args.gap_open, ge,
                            {"xdrop": x, "chains": chains[:count]})
            report["workloads"].append(row)
            print(json.dumps(row), flush=True)
        w = mapped_workload(args.small)
        w = dict(w, pairs=w["pairs"][:4000])
        seeds, _ = longest_match_seeds(engine, w, args.gap_open, ge)
        texts = [w["text"][p[0]:p[0] + p[1]] for p in w["pairs"]]
        pats = [w["pattern"][p[2]:p[2] + p[3]] for p in w["pairs"]]
        row = cigar_row(args, engine, "mapped_seeds_4000", texts, pats, w["S"], args.gap_open, ge, {"xdrop": x, "seeds": seeds})
        report["workloads"].append(row)
        print(json.dumps(row), flush=True)
    elif args.mode == "chaining":
        from sa_amd import synthetic
        ge = args.gap_extend if args.gap_extend is not None else 2
        w = chain_workload(args.small)
        cp = {"match": 5, "gap_open": args.gap_open, "gap_extend": ge, "skip": 0, "max_gap": engine.NO_LIMIT, "max_diag": 500, "lookback": 64}
        report["conditions"] = {"timing": "time.perf_counter around the C call, device and host alternated round by round in one process",
                                "library_build_id": engine.lib.sa_build_id().decode(), "host_cpus": os.cpu_count()}
        derived = exact_match_chains(engine, w, args.gap_open, ge)
        for k in (11, 15):
            anchors = [synthetic.kmer_anchors(w["text"][p[0]:p[0] + p[1]], w["pattern"][p[2]:p[2] + p[3]], k) for p in w["pairs"]]
            for count in (len(anchors), 64):
                row = chaining_rows(args, engine, f"{w['name']}_k{k}_{count}", anchors[:count], cp)
                report["workloads"].append(row)
                print(json.dumps(row), flush=True)
            _, chained = engine.chain_anchors(anchors, sort=False, **cp)
            row = chaining_scores_row(args, engine, w, chained, derived, args.gap_open, ge, None, k)
            report["workloads"].append(row)
            print(json.dumps(row), flush=True)
    elif args.mode == "ends":
        report["library_build_id"] = engine.lib.sa_build_id().decode()
        for w in (mapping_workload(args.small), overlap_workload(args.small)):
            dt, dp = torch.from_numpy(w["text"]).cuda(), torch.from_numpy(w["pattern"]).cuda()
            for gap, ge in ((5, None), (args.gap_open, args.gap_extend if args.gap_extend is not None else 2)):
                row = ends_rows(args, engine, w, dt, dp, gap, ge)
                report["workloads"].append(row)
                print(json.dumps(row), flush=True)
            del dt, dp
    for w in ([] if args.mode or args.band else workloads(args.small, search_only=args.hits is not None)):
        dt, dp = torch.from_numpy(w["text"]).cuda(), torch.from_numpy(w["pattern"]).cuda()
        if args.hits is not None:
            row = hits_row(args, engine, w, dt, dp)
            report["workloads"].append(row)
            print(json.dumps(row), flush=True)
            continue
        if args.gap_extend is not None:
            row = affine_rows(args, engine, w, dt, dp)
            report["workloads"].append(row)
            print(json.dumps(row), flush=True)
            continue
        cells = sum(p[1] * p[3] for p in w["pairs"])
        row = {"name": w["name"], "pairs": len(w["pairs"]), "cells": cells}
        sc = engine.Scorer(w["mode"], w["S"], w["gap"], w["pairs"])
        row["scorer"] = sc.info()
        run_a = lambda: sc.run(dt.data_ptr(), dp.data_ptr())  # noqa: E731
        try:
            pl = engine.Plan(w["mode"], w["S"], w["gap"], w["pairs"])
        except engine.SaError as e:
            pl = None
            row["plan"] = {"error": str(e)}
        run_a()
        a_scores = sc.results()["score"].copy()
        ta, tf, tft = [], [], []
        if pl is not None:
            row["plan"] = pl.info()
            pl.fill(dt.data_ptr(), dp.data_ptr())
            pl.traceback()
            b_scores = pl.results_array()["score"]
            assert (a_scores == b_scores).all(), f"{w['name']}: scorer and plan scores differ"
            row["scores_agree"] = True
        for _ in range(args.rounds):
            ta.append(timed(run_a, lambda: sc.results()))
            if pl is not None:
                tf.append(timed(lambda: pl.fill(dt.data_ptr(), dp.data_ptr()), torch.cuda.synchronize))

                def both():
                    pl.fill(dt.data_ptr(), dp.data_ptr())
                    pl.traceback()
                tft.append(timed(both, lambda: pl.results_array()))
        row["scorer_run"] = stats(ta)
        row["scorer_gcups"] = round(cells / statistics.median(ta) / 1e6, 1)
        if pl is not None:
            row["plan_fill"] = stats(tf)
            row["plan_fill_traceback"] = stats(tft)
            pl.close()
        sc.close()
        # the forced rows-per-lane sweep behind the automatic rule
        sweep = {}
        for R in (1, 2, 4, 8):
            s = engine.Scorer(w["mode"], w["S"], w["gap"], w["pairs"], rows_per_lane=R)
            s.run(dt.data_ptr(), dp.data_ptr())
            assert (s.results()["score"] == a_scores).all(), f"{w['name']}: R = {R} scores differ"
            ms = [timed(lambda: s.run(dt.data_ptr(), dp.data_ptr()), lambda: s.results()) for _ in range(max(3, args.rounds))]
            sweep[str(R)] = dict(stats(ms), num_waves=s.info()["num_waves"])
            s.close()
        row["rows_per_lane_sweep"] = sweep
        report["workloads"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
