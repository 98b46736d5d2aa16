"""The band fill with three-row bands (sa_fill.hip process_band3, fill_kernel_band3): 192-row score
strips (three rows per lane) run ahead on their own workgroups and feed the 64-row strips, which run
in groups of three. Checked in subprocesses (the engine reads its knobs once per process) with
SA_BAND_R=3 and once with SA_BAND_R=2, cell by cell against the oracle's DIRECTION matrix
(oracle.fill_only) and the full alignment (oracle.align), the way test_band_fill.py checks two rows:
  * m in {193, 385, 450, 769, 1100, 2900}: one band; a last strip group of one, two and three strips;
    five and more bands (a band group boundary, so a cross-group granule hand-off between bands);
    rows past m inside the last strips; n in {700, 2100, 4500}: below one ring lap (2048 columns),
    just past one, past two, none a multiple of 16; global gaps 5 / 0 / -3, local gaps 5 / 0;
  * the plans report the band height they run (sa_plan_fill_kind through Plan.info());
  * BLOSUM50: alphabets larger than 4 have no three-row kernels (they read copy 0 of their text
    profiles, kArr8A), so SA_BAND_R=3 must leave them on the two-row bands, still exact;
  * several chained pairs whose heights are multiples of 192 (every first strip a multiple of 3: band
    and strip groups span pair boundaries), and a plan where a first strip is no multiple of 3, which
    must fall back to the two-row bands and stay exact;
  * SA_MAX_CUS=16 on a 2048 x 4096 pair: more band and strip groups than CUs, persistent workers with
    the new group widths;
  * the 32768^2 headline in a fresh process at the default knobs against large.json (score 25141)."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEAD = r'''
import sys, json, numpy as np
sys.path[:0] = [sys.argv[1] + "/sequence-alignment-gpu_amd/python", sys.argv[1] + "/oracle"]
import oracle
from sa_amd import engine, synthetic
from sa_amd.batch import DeviceBatch
S = synthetic.blast_matrix()
KIND = sys.argv[2]  # the fill kernel the DNA plans below must report
bad = []
def check(mode, n, m, gap, seed, related, S=S, kind=KIND):
    A = S.shape[0]
    t = synthetic.random_sequence(seed, n, A)
    p = synthetic.mutate(t, seed + 1, A, m) if related else synthetic.random_sequence(seed + 2, m, A)
    b = DeviceBatch(mode, S, gap, [t], [p], rows_per_lane=1)
    if b.plan.info()["fill_kernel"] != kind:
        bad.append(("kind", mode, n, m, gap, b.plan.info()["fill_kernel"]))
    b.fill()
    got = b.directions(0)
    b.close()
    exp = np.empty((m + 1) * (n + 1), np.uint8)
    oracle.fill_only(mode, t, p, S, gap, exp)  # (the reference's M, STOP included)
    nbad = int((got != exp).sum())
    if nbad:
        bad.append(("dirs", mode, n, m, gap, nbad))
    r = engine.align_pair(mode, t, p, S, gap, device=0)
    r.pop("fill_us")
    if r != oracle.align(mode, t, p, S, gap):
        bad.append(("align", mode, n, m, gap))
def batch(mode, ts, ps, kind):
    b = DeviceBatch(mode, S, 5, ts, ps, rows_per_lane=1)
    if b.plan.info()["fill_kernel"] != kind:
        bad.append(("kind", mode, "batch", b.plan.info()["fill_kernel"]))
    b.fill()
    for k, (t, p) in enumerate(zip(ts, ps)):
        exp = np.empty((len(p) + 1) * (len(t) + 1), np.uint8)
        oracle.fill_only(mode, t, p, S, 5, exp)
        if int((b.directions(k) != exp).sum()):
            bad.append(("batch dirs", mode, k))
    b.close()
    got = engine.align_batch(mode, ts, ps, S, 5, num_gpus=1)
    for k in range(len(ts)):
        if got[k] != oracle.align(mode, ts[k], ps[k], S, 5):
            bad.append(("batch align", mode, k))
'''

SMALL = HEAD + r'''
cases = [(700, 193, 5), (2100, 385, 0), (4500, 450, -3), (2100, 769, 5), (700, 1100, 0), (4500, 2900, 5), (2100, 1100, -3)]
for k, (n, m, gap) in enumerate(cases):
    check(0, n, m, gap, 2800 + 10 * k, k % 2 == 0)
    if gap >= 0:  # (local with g < 0 has no byte-sized differences: the one-wave kArr fill, no bands)
        check(1, n, m, gap, 2805 + 10 * k, k % 2 == 0)
# 23 letters: no three-row kernels, the two-row bands whatever SA_BAND_R says
B50 = np.array(json.load(open(sys.argv[1] + "/tests/golden/matrices.json"))["blosum50"], np.int32).reshape(23, 23)
check(0, 2100, 769, 5, 2900, True, S=B50, kind="band")
print("BAND3_OK" if not bad else "BAND3_BAD %r" % (bad,))
'''

PLANS = HEAD + r'''
# heights that are multiples of 192: every pair's first strip is a multiple of 3
ts = [synthetic.random_sequence(3000 + k, 1800 + 97 * k, 4) for k in range(4)]
ps = [synthetic.mutate(t, 3100 + k, 4, 192 * (2 + 2 * k)) for k, t in enumerate(ts)]
for mode in (0, 1):
    batch(mode, ts, ps, KIND)
# the second pair's first strip is 4: no multiple of 3, so the plan takes the two-row bands
ps = [synthetic.mutate(t, 3200 + k, 4, 256 * (1 + k)) for k, t in enumerate(ts)]
for mode in (0, 1):
    batch(mode, ts, ps, "band")
print("BAND3_OK" if not bad else "BAND3_BAD %r" % (bad,))
'''

# 64 strips: 22 strip groups of three and 6 band groups on 16 CUs (5 band and 11 strip workers)
PERSIST = HEAD + r'''
for mode in (0, 1):
    check(mode, 2048, 4096, 5, 5200 + mode, False)
print("BAND3_OK" if not bad else "BAND3_BAD %r" % (bad,))
'''

LARGE = r'''
import sys, json
sys.path[:0] = [sys.argv[1] + "/sequence-alignment-gpu_amd/python", sys.argv[1] + "/tests"]
from sa_amd import engine, synthetic
from conftest import matrix, same_result
c = {c["name"]: c for c in json.load(open(sys.argv[1] + "/tests/golden/large.json"))}["headline_dna_global_32768_uniform"]
A = c["letters"]
t = synthetic.random_sequence(c["text_seed"], c["n"], A)
p = (synthetic.random_sequence(c["pattern_seed"], c["m"], A) if c["pattern_kind"] == "rand"
     else synthetic.mutate(t, c["pattern_seed"], A, c["m"]))
S = matrix(c["matrix"], 4 if c["matrix"] == "blast" else 23)
plan = engine.Plan(c["mode"], S, c["gap"], [(0, c["n"], 0, c["m"])], device=0)
kind = plan.info()["fill_kernel"]
plan.close()
got = engine.align_pair(c["mode"], t, p, S, c["gap"], device=0)
ok = same_result(got, c["result"]) and got["score"] == 25141 and kind == sys.argv[2]
print("BAND3_OK" if ok else "BAND3_BAD %r %r" % (got["score"], kind))
'''


def _run(script, kind, **env):
    e = dict(os.environ, SA_HANDOFF_TIMEOUT_S="10", **env)
    out = subprocess.run([sys.executable, "-c", script, ROOT, kind], env=e, capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "BAND3_OK" in out.stdout, out.stdout[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ["3", "2"])
def test_band3_fill_vs_oracle(rows):
    _run(SMALL, "band3" if rows == "3" else "band", SA_BAND_R=rows)


@pytest.mark.gpu
def test_band3_chained_pairs_and_fallback_vs_oracle():
    _run(PLANS, "band3", SA_BAND_R="3")


@pytest.mark.gpu
def test_band3_persistent_workers_vs_oracle():
    _run(PERSIST, "band3", SA_BAND_R="3", SA_MAX_CUS="16")


@pytest.mark.gpu
def test_band3_headline_default_fresh_process():
    """The default plan of the 32768^2 DNA global headline: every band and strip group resident, so
    three-row bands (43 band groups + 171 strip groups), and the reference's recorded result."""
    e = {k: v for k, v in os.environ.items() if k not in ("SA_BAND_R", "SA_BAND")}
    out = subprocess.run([sys.executable, "-c", LARGE, ROOT, "band3"], env=dict(e, SA_HANDOFF_TIMEOUT_S="10"),
                         capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "BAND3_OK" in out.stdout, out.stdout[-2000:]


def test_band3_large_fixture():
    """(CPU) the fixture the headline test reads exists and records the score the issue names."""
    c = {c["name"]: c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "large.json")))}
    assert c["headline_dna_global_32768_uniform"]["result"]["score"] == 25141
