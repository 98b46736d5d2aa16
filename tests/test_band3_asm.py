"""(CPU) The three-row bands' generated score steps (sa_fill_steps.inc band3_steps_asm,
tools/gen_fill_asm.py band_block(rows = 3)) interpreted over 64 lanes the way process_band3 drives
them (tools/sim_band.py): lane k owns rows 3k .. 3k + 2 of a 192-row band, and every band's published
bottom row must equal a direct DP of the same rows, global (shifted domain) with gaps 5 / 0 / -3 and
local with gaps 5 / 0, text lengths that are no multiple of 16, with a feed from the band above and
without one. On the generated text: every DPP stands behind the writes of the registers it reads
with at least two other instructions in between, a 16-step body returns every value to its register,
and the generator still emits the committed file (the two-row and one-wave blocks included)."""
from __future__ import annotations

import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

INC = os.path.join(ROOT, "sequence-alignment-gpu_amd", "csrc", "sa_fill_steps.inc")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


sim = _tool("sim_band")
gen = _tool("gen_fill_asm")


def _pair(n, m, seed):
    from sa_amd import synthetic
    t = synthetic.random_sequence(seed, n, 4)
    return t, synthetic.mutate(t, seed + 1, 4, m), synthetic.blast_matrix()


# (mode, n, m, gap): two or three bands per case, m in each third of the last band
CASES = [(0, 150, 577, 5), (0, 97, 450, 0), (0, 121, 385, -3), (1, 150, 600, 5), (1, 90, 449, 0), (0, 33, 390, 5)]


@pytest.mark.parametrize("mode,n,m,g", CASES)
def test_band3_published_rows_vs_dp(mode, n, m, g):
    assert n % 16 != 0
    t, p, S = _pair(n, m, 40 + n)
    F = sim.dp(mode, t, p, S, g)
    got = sim.bands(mode, t, p, S, g, rows=3)
    assert len(got) == (m + 191) // 192 - 1 >= 2
    for b, row in enumerate(got):
        assert (row[1:] == F[192 * (b + 1), 1:]).all(), (b, int(np.argmax(row[1:] != F[192 * (b + 1), 1:])) + 1)


@pytest.mark.parametrize("mode,g", [(0, 5), (0, -3), (1, 5)])
def test_band3_without_feed_vs_dp_of_its_own_rows(mode, g):
    """No band above (HP = false): band b's published row is the DP of pattern rows 192 b .. 192 b + 191
    alone under the row-0 boundary, as for a pair's first band."""
    n, m = 109, 500
    t, p, S = _pair(n, m, 77)
    got = sim.bands(mode, t, p, S, g, rows=3, fed=False)
    assert len(got) == 2
    for b, row in enumerate(got):
        F = sim.dp(mode, t, p[192 * b:192 * (b + 1)], S, g)
        assert (row[1:] == F[192, 1:]).all(), b


def _ops(ins):
    """(destination, registers read) of one instruction of the band block."""
    op = ins.split()[0]
    regs = re.findall(r"%\[\w+\]", ins)
    if op in ("s_nop", "s_waitcnt"):
        return None, []
    if op == "ds_write_b32":
        return None, regs
    if op == "v_mov_b32_dpp":
        return regs[0], regs  # the destination's other lanes are kept: `old` is read
    return regs[0], regs[1:]


@pytest.mark.parametrize("local", [False, True])
@pytest.mark.parametrize("hn", [False, True])
@pytest.mark.parametrize("hp", [False, True])
def test_band3_dpp_distance_and_round_trip(local, hn, hp):
    lines = sim.band_asm(local, hn, hp, rows=3)
    assert lines == gen.band_block(local, hn, hp, 3).split("\\n\\t")
    assert lines[0] == "s_nop 1"  # covers the compiler's writes right before the block
    last_write = {}
    for i, ins in enumerate(lines):
        dst, reads = _ops(ins)
        if ins.startswith("v_mov_b32_dpp"):
            for r in reads:
                assert i - last_write.get(r, -10) >= 3, (i, ins, r)
        if dst:
            last_write[dst] = i
    # steps: each begins with row 0's add; VALU count per step; register use has period 8 (so 16 steps
    # return every value to its register)
    starts = [i for i, ins in enumerate(lines) if ins.startswith("v_add_u32_sdwa") and "%[ta" in ins]
    assert len(starts) == 16
    steps = [lines[a:b] for a, b in zip(starts, starts[1:] + [None])]
    valu = [[x for x in st if x.startswith("v_") and "%[p" in x.split(",")[0]] for st in steps]
    for k in range(15):
        assert len([x for x in steps[k] if x.startswith("v_")]) == (11 if local else 8), k
    use = [[re.findall(r"%\[p\d\]", x) for x in st[:11 if local else 8]] for st in valu]
    for k in range(8):
        assert use[k] == use[k + 8], k
        if k:
            rot = [[f"%[p{(int(r[3]) + k) % 8}]" for r in x] for x in use[0]]
            assert use[k] == rot, k
    # entry / exit state registers (band_operands): Q = p7, diag = p6, F0 = p5, F1 = p3, F2 = p1
    outs, _ = gen.band_operands(local, hn, hp, 3)
    assert outs[:5] == ['[p7] "+v"(r.Q)', '[p6] "+v"(r.diag)', '[p5] "+v"(r.F0)', '[p3] "+v"(r.F1)', '[p1] "+v"(r.F2)']


def test_generator_reproduces_committed_file(tmp_path):
    out = tmp_path / "steps.inc"
    env = dict(os.environ, SA_GEN_FILL_OUT=str(out))
    for k in ("SA_GEN_PF_STEP", "SA_GEN_BAND_PF_STEP", "SA_GEN_EXP_FEED"):
        env.pop(k, None)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_fill_asm.py")], env=env, check=True,
                   capture_output=True, timeout=120)
    committed = open(INC).read()
    assert out.read_text() == committed
    # the existing blocks: the two-row band steps and the one-wave steps as their functions emit them
    for local in (False, True):
        for hn in (False, True):
            for hp in (False, True):
                assert f'asm volatile("{gen.band_block(local, hn, hp)}"' in committed
                assert gen.band_block(local, hn, hp) == gen.band_block(local, hn, hp, 2)
                for half in (0, 1):
                    assert f'asm volatile("{gen.block(local, hn, hp, half)}"' in committed
    # and they precede the three-row section, which is appended
    assert committed.index("band3_steps_asm<false, false, false>") > committed.index("merge_asm<true>")
