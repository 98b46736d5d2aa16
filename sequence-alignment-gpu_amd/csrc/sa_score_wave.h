// The wave program of the score-only path (sa_score.hip) and of the traced fill of the affine aligners
// (sa_affine_walk.hip): score_wave<R, MODE, SMALL, F>, every instance of it the kernel
// wave_kernel<R, MODE, SMALL, F>. R is the rows per lane, MODE the program (SA_GLOBAL, SA_LOCAL or SA_FIT),
// SMALL an alphabet of at most four letters, and F the variant, a mask of the kWave* flags below. The
// variants that exist, the programs they run and what they read from the kernel argument (WaveArgs;
// traced, TracedWaveArgs with the direction arena `tr`):
//
//   variant            flags                           programs             reads
//   kVarLinear         -                               global, local, fit   -
//   kVarAffine         Affine                          global, local, fit   gap_extend
//   kVarBand           Affine Band                     global, local        gap_extend, band
//   kVarEnds           Ends                            global, fit          ends
//   kVarAffineEnds     Affine Ends                     global, fit          gap_extend, ends
//   kVarBandAtLocal    Affine Band BandAt              local                gap_extend, bands
//   kVarBandAt         Affine Band BandAt Ends         global, fit          gap_extend, ends, bands
//   kVarExtend         Extend                          global               xdrop
//   kVarAffineExtend   Affine Extend                   global               gap_extend, xdrop
//   kVarSeeds          Extend Seed                     global               xdrop, items
//   kVarAffineSeeds    Affine Extend Seed              global               gap_extend, xdrop, items
//   kVarExtendBand     Affine Band BandAt Extend       global               gap_extend, xdrop, width
//   kVarSeedsBand      Affine Band BandAt Extend Seed  global               gap_extend, xdrop, width, items
//   kVarItems          Seed                            global               items
//   kVarAffineItems    Affine Seed                     global               gap_extend, items
//
// Untraced, every row exists at R = 1, 2, 4, 8; with Trace added, the affine rows exist at R = 8. The
// static_asserts of score_wave are the rule for a legal combination, the table of sa_wave_launch.h is the
// set that is instantiated, and the sections below say what each flag does (AFFINE, TRACE, BAND, ENDS, BAT,
// EXT and SEED are the names the program gives its flags).
//
// The kernels are persistent with one wave per workgroup. A wave draws the next pair of the work
// order (sa_score_plan.cpp: most cells first) with one atomicAdd and runs the pair's strips of 64 R
// rows one after another; no wave ever waits for another wave. Lane l owns rows
// 64R s + R l + 1 .. + R of strip s and computes, at step t, its R cells of column t - l + 1; H of the
// row above its first row and the text letter come from lane l - 1 by a DPP shift, everything else
// stays in registers. The strip's top row H[64R s][1..n] is read from the wave's own row buffer in
// 64-column bodies (one coalesced access per lane per 64 steps, shifted to lane 0 one lane per step)
// and its bottom row is collected from lane 63 the same way and written back in place: the writes
// trail the reads by at least 63 columns. The linear recurrence is the reference's
// (alignSequenceCPU.cpp:175-192, :259-273) in int32; the local result is the first maximum in
// row-major order, taken as the maximum of the key (H, ~row, ~col) over rows, lanes and strips.
//
// AFFINE is Gotoh's three-state recurrence, a gap of k cells costing gap_open + (k - 1) gap_extend:
//
//   E[i][j] = max(E[i][j-1] - ge, H[i][j-1] - go)      gap run along the row
//   F[i][j] = max(F[i-1][j] - ge, H[i-1][j] - go)      gap run along the column
//   H[i][j] = max(H[i-1][j-1] + S[p[i-1]][t[j-1]], E[i][j], F[i][j])      local: max(0, .)
//
// Per row a lane also keeps E[row][column - 1]; F runs down the lane's R rows inside a step, and the
// lane above hands down H and F of its bottom row (two DPP shifts where the linear kernel has one).
// The boundary row then holds (H, F) of the strip's bottom row, two ints per column, read and
// written as one 8-byte access under the same in-place rule. The borders need no minus infinity:
// E[i][0] := H[i][0] - go + ge and F[0][j] := H[0][j] - go + ge make the first step of a run yield
// H - go from both branches.
//
// MODE is SA_GLOBAL, SA_LOCAL or SA_FIT. SA_FIT (semi-global: the whole pattern inside the text, the
// text free at both ends; sa_hip.h has the definition) is the global program with three changes, all
// under `if constexpr (FIT)`: the top row fed to strip 0 is H[0][j] = 0 (its F stand-in derived from
// it as above; column 0 stays global, -i g or -(go + (i - 1) ge)); the result is the leftmost maximum
// of H[m][1..n]; and an empty pattern scores 0 at (0, 0), an empty text one run of m gaps at (m, 0).
// Row m lies in one lane of the last strip (lane flm, its row frm), so there is no key and no merge
// over lanes: every lane selects its row frm once per step and keeps one running best (value and
// step; strictly greater keeps the first column), started below any score at every strip, and lane
// flm's pair after the last strip is the result. A lane outside columns 1..n (ramp-up: it still holds
// H[row][0]; ramp-down: H[row][n]) registers nothing, so column 0 is never reported.
// DESIGN.md §3.4 has the resource usage of the instances, the rule for R and the step costs the
// planner uses.
//
// TRACE (AFFINE, R = 8: the instances of sa_affine_walk.hip) also records, per cell, where H came
// from and whether E and F extend a run: a nibble per row, so a lane's eight rows are one dword per
// step, stored at dirs[(strip * steps + t) * 64 + lane] of the pair's directions, steps = 64 nbodies.
// Every step stores, the predicated ones too; the words of lanes outside columns 1..n and the nibbles
// of rows past m are never read. DESIGN.md §3.5 has the nibble and the walk that reads it.
//
// BAND (AFFINE, global or local: kVarBand) keeps to the diagonal band of
// sa_hip.h: cell (i, j) is in band iff lo <= j - i <= hi, and H, E and F of every other cell are
// kBandSentinel. Everything banded is under `if constexpr (BAND)` or MASK; the other instances compile
// to what they were. A strip runs only the bodies of its window (band_window, sa_score_plan.h), with
// the step numbers and the lane skew of the whole strip, so a cell's step, its column and the local
// key do not change.
//  - Start. In body 0 a border cell (i, 0) is real down to row -lo and the sentinel below it. A window
//    that starts at body b0 >= 1 has every lane's first cell left of the band, so hl, el and upprev
//    start at the sentinel; only lane 0's upprev, the cell (64R s, 64 b0) of the row above the strip,
//    can be the band's left edge, and is read from the row buffer under the mask.
//  - Top row. A column of the row above the strip is taken from the row buffer (strip 0: from the
//    border formula) only if it is in band for that row; any other column reads as the sentinel,
//    whatever the buffer holds there from an earlier strip or from the pair this wave scored before.
//  - Bottom row. The write-back covers the columns lane 63 met in the window's bodies, 64 b0 - 62 ..
//    64 (b1 - 1) + 1. Inside a window the writes trail the reads by 63 columns as before. Between
//    strips: the in-band columns of row 64R (s + 1) lie between the jmin and the jmax of strip s,
//    whose window spans them (band_window takes jmax from the strip's last row), so strip s wrote
//    each of them after strip s read it, and strip s + 1 trusts no other column. What strip s + 1
//    writes lies at or left of columns it has read or masks.
//  - Cells. A body whose diagonals all lie in the band (and whose columns all lie in 1..n) runs the
//    plain step. Any other body runs the MASK step: after the recurrence and the local clamp an
//    out-of-band cell becomes the sentinel in H, E and F, so it never exceeds a local best and hands
//    exactly the sentinel on; a lane outside columns 1..n keeps its state as in the unbanded program.
//  - Values. An in-band cell's diagonal neighbour is in band, so its H is a real score. Its E (F) is
//    sentinel-derived only when the cell to its left (above) is out of band: the sentinel minus one
//    penalty; the next cell's E (F) takes the real H - go instead. Under the planner's limit
//    (kBandScoreLimit) such a value stays below every real score minus a penalty and inside int32, so
//    it never wins a maximum, never ties, and no direction nibble that is read points out of band.
//  - TRACE stores a word only for the steps the strip runs: the pair's directions are the strips'
//    windows one after another, 64 (b1 - b0) steps of 64 words each (trace_band_dir_bytes).
//
// ENDS (MODE SA_GLOBAL or SA_FIT; kVarEnds, kVarAffineEnds) is
// ends-free alignment, sa_hip.h SA_ENDS_FREE: `ends` holds the flags, TB, TE, PB and PE for short.
// TE decides the program: unset it is the global program, set it is the fit program (the running best
// of row m), and the host launches MODE accordingly. The other three flags are wave-uniform values and
// cost nothing per step; everything of ENDS is under `if constexpr (ENDS)`, so the other instances
// compile to what they were.
//  - TB, PB: the border values. H[0][j] (the top row fed to strip 0) is 0 under TB and H[i][0] (hl, el
//    and upprev at the start of a strip) is 0 under PB; the stand-ins for E and F follow from them.
//  - PE: after a strip hl[r] is H[row][n], so every lane folds its rows <= m into one running best of
//    the last column (strictly greater keeps the earlier row, within the lane and across strips), and
//    after the last strip one wave maximum of the key (value + 2^30, ~row) gives the lowest row of the
//    maximum: the planner keeps |H| below 2^30.
//  - The result: lane 0 compares the best of row m (TE unset: H[m][n]), the best of the last column
//    and the closed-form border candidates H[0][n] and H[m][0] in the tie order of sa_hip.h.
//  - An empty side: every candidate is a border cell; the early-out compares the border values at
//    0, 1 and the side's length, as a gap's cost need not grow with its length.
//
// BAT (BAND; MODE SA_LOCAL, or ENDS with the global or the fit program: kVarBandAtLocal, kVarBandAt) is the band program on a band of the caller's, sa_hip.h sa_band: `bands` holds
// one (lo, hi) per pair, clipped to [-m, n] by the planner and read once per pair as a wave-uniform
// value. Neither lo <= 0 <= hi nor "every row has an in-band cell" holds any more; the planner admits
// only pairs with an alignment inside their band (sa_band_reachable), and in such a pair every in-band
// cell, border cells included, is a real score: an in-band border cell that costs implies an in-band
// origin, and every in-band cell lies on a diagonal that starts in a real border cell. Everything of
// BAT is under `if constexpr (BAT)`; the other instances compile to what they were.
//  - Windows. band_window_at may be empty (b0 == b1): the strip runs no body, stores no direction word
//    and leaves the row buffer alone. The strip after it masks the whole row above it (an empty strip's
//    last row holds no in-band column in 1..n), so the buffer's stale content is never read; the
//    between-strips argument of "Bottom row" holds between two strips that both ran as it stands.
//  - Borders. (row, 0) is real iff in band, -hi <= row <= -lo, and (0, j) iff lo <= j <= hi. Strip 0
//    under lo > 0 starts past body 0: lane 0's upprev is then the border H[0][64 b0], not a row-buffer word.
//  - Result. PE folds a row only if (row, n) is in band: only then did the strip's window reach column n
//    and hl[r] is H[row][n]. The running best of row m sees sentinels (out-of-band columns) before or
//    after real values; a real value is above -2^29 under the planner's limit and the sentinel never
//    ties one, so the best is the leftmost real maximum, or at most -2^29 when row m has no in-band
//    column in 1..n. Lane 0 drops a row-m candidate that is not real ((m, n) out of band without TE) and
//    counts H[0][n] and H[m][0] only in band; reachability leaves at least one candidate.
//  - An empty side: the candidates are the border's in-band cells.
//
// EXT (MODE SA_GLOBAL, no band, no free ends: kVarExtend, kVarAffineExtend) is extension alignment, sa_hip.h sa_score_batch_extend: the start anchored at the
// origin, the end at the best interior cell of the rows before the stop row i*, `xdrop` a wave-uniform
// kernel argument. It is the local program's result on the global program's cells; everything of EXT is
// under `if constexpr (EXT)` or a constant condition, so the other instances compile to what they were.
//  - Cells. The borders, the recurrence and the traced nibble are global's: no clamp, no STOP nibble.
//  - Per-row best. best[r] starts below any score at every strip and a lane outside columns 1..n
//    registers nothing (the fit step's `valid` test): H[row][0] may exceed the row's real cells, which the
//    local step never sees as its values are >= 0. After a strip best[r] is r(row) for every row <= m, as
//    every strip runs all columns. The key and its `best > 0` condition are local's: without a positive
//    row the wave maximum is 0, the empty extension at (0, 0).
//  - Drop test, after every strip, outside the step. Row i drops iff B(i - 1) - r(i) > xdrop. B(i - 1) is
//    the maximum of B carried from the strips before (a scalar, 0 at the start: the origin), of the lanes
//    before this one (an inclusive prefix maximum of the lanes' strip maxima, wave_prefix_max, shifted by
//    one lane) and of the lane's rows before. A ballot finds the first lane that holds a dropping row and
//    a readlane its first such row: i*, wave-uniform. Rows past m neither raise B nor drop.
//  - Exit. Without a drop B is carried on. With one, only rows < i* fold into the key and the strip loop
//    ends (a uniform break): the strips below run no body, store no direction word and leave the
//    boundary row as strip s wrote it. That row is stale for this pair's shape, and harmless: strip 0 of
//    the wave's next pair reads its top row from the border formula, never from the buffer, and every
//    later strip reads only columns the strip before it wrote (the BAT argument above, without windows).
//    The walk starts at a cell of a row < i*, rows only fall along it, and those rows' strips stored
//    every word: it never reads a word of a strip that did not run.
//  - xdrop SA_NO_XDROP skips the test: every row counts, as with a drop that no score can reach.
//
// BAND + EXT (AFFINE, BAT: kVarExtendBand, with SEED kVarSeedsBand) is extension alignment inside a width of the
// anchor's diagonal, sa_hip.h sa_score_batch_extend_band: the band-at program's cells with EXT's result. The
// band is computed, not loaded: band_ext(n, m, width) of the pair or item the wave drew, from the wave-uniform
// kernel argument `width`, so lo <= 0 <= hi, the origin is in band, every in-band cell lies on a diagonal that
// starts in an in-band border cell of the global borders, and BAT's "every in-band cell is a real score" holds
// with no reachability test. Everything of it is under `if constexpr (BAND && EXT)` or inside BAT's and EXT's
// own sections; the other instances compile to what they were.
//  - Cells. BAT's borders ((row, 0) real iff row <= -lo, (0, j) iff j <= hi), band_window_at windows and the
//    MASK step, on global's recurrence: no clamp.
//  - Per-row best. best[r] starts at the sentinel, not at INT32_MIN: a masked cell registers the sentinel (it is
//    `valid`, and never above the start value), a real cell is above -2^29 and always registers, and a row the
//    window never meets, or a row of a strip without a window, keeps the start value. So after a strip best[r]
//    is r(row) on the banded matrix, with the sentinel standing for minus infinity.
//  - Drop test. 0 <= B < 2^29 (kBandScoreLimit) and best[r] >= -2^30, so B - best[r] < 2^31 stays inside int32,
//    and for a row without an in-band cell it is >= 2^30 > xdrop: the row drops under every xdrop >= 0 by the
//    test as it stands. lm and pm[] take maxima only. Under SA_NO_XDROP nothing is tested and such a row
//    holds no candidate, as best[r] > 0 fails.
//  - Empty strips end the pair. Rows with an in-band column are 1 .. n - lo, a prefix: once a strip's window is
//    empty every later one is, none holds a candidate, and a finite drop fired at the latest in the first row
//    past n - lo. The strip loop ends there, before any of the strip's work.
//  - The row buffer. Strip s + 1 reads only the in-band columns of row 64R (s + 1), which strip s wrote after
//    reading them (BAT, "Windows" and BAND, "Bottom row"); after a drop or an empty strip the boundary row is
//    stale and harmless by EXT's "Exit": the wave's next pair starts from the border formulas.
//  - TRACE. The strips that run store their windows' words one after another (trace_band_at_dir_bytes of the
//    band sizes the pair); a strip past the stop row or without a window stores none, and the walk, which
//    starts in a row < i*, steps over strips that ran only.
//
// SEED (EXT: kVarSeeds, kVarAffineSeeds, kVarSeedsBand) is seed extension, sa_hip.h
// sa_score_batch_seeds: the wave draws work items (SeedItem, sa_score_plan.h), a pair's left half or its
// right half, where the other instances draw pairs, and `order`, `np`, `out` and TRACE's dir_off speak of
// items. An item is an extension pair whose letter k lies at base[dir * k], base the address of the half's
// first-read letter: the right half reads forwards from the seed's end, the left half backwards from the
// letter before the seed, so column j of its matrix is t[ts - j] and row i is p[ps - i], the reversed
// prefixes of sa_hip.h, with nothing reversed or copied. Only the two loads differ, text[dir * c0] per
// body and pattern[dir * (row1 + r)] per strip; no step changes. Everything of SEED is under
// `if constexpr (SEED)` or a constant condition, so the other instances compile to what they were. The
// planner makes no item of an empty half, and the guards c0 < n and row1 + r < m keep a backward read at
// or after the half's last letter, the pair's first.
//
// SEED without EXT (kVarItems, kVarAffineItems) is the global program on work items: the gap pieces of chained
// seeds, sa_hip.h sa_score_batch_chains, each the rectangle between two consecutive seeds of a pair. The
// addressing is SEED's two loads, here always with dir = +1; the cells, the borders, the traced nibble and the
// result, H[m][n] written to out[item], are the global program's, and no line of the program names the
// combination. The planner makes no item with an empty side.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "sa_hip.h"
#include "sa_score_plan.h"
#include "sa_wave.h"

namespace sa {

struct ScorePair {
    uint64_t text_off, pattern_off;
    uint32_t n, m;
};
static_assert(sizeof(ScorePair) == 24, "the planner counts 24 bytes per descriptor");

struct ScoreArgs {
    const int8_t *text, *pattern;
    const ScorePair *pairs;
    const int32_t *order;   // work order: pair indices, most cells first
    const int32_t *table;   // A x A scores, [pattern][text]
    int32_t *rows;          // one boundary row per wave: row_stride ints (affine: row_stride (H, F) pairs)
    sa_score_result *out;
    uint32_t *ctrl;         // [0] the next position of the work order, [1] bad-input flag
    int32_t np, A, gap, key_rowbits;  // gap: the linear penalty, or the affine gap-open penalty
    uint64_t row_stride;
};

struct ScoreAffineArgs {
    ScoreArgs s;
    int32_t gap_extend;
};

// TRACE: the direction arena of the launch and each pair's first word in it
struct TraceArgs {
    uint32_t *dirs = nullptr;
    const uint64_t *dir_off = nullptr;  // per pair, in words
};

// SEED: item `k` as the pair descriptor the wave program takes, and its direction
__device__ __forceinline__ ScorePair seed_item_pair(const SeedItem *items, int k, int *dir)
{
    const SeedItem it = items[k];
    *dir = uniform(it.dir);
    return ScorePair{it.text_off, it.pattern_off, it.n, it.m};
}

// direction nibble of a cell: bits 0-1 the source of H (the reference's codes), bit 2 E extends,
// bit 3 F extends
enum { kDirLeft = 0, kDirDiag = 1, kDirTop = 2, kDirStop = 3, kDirEExt = 4, kDirFExt = 8 };

// the step of a banded body that cuts a band edge: predicated as std::true_type is, and masked
struct MaskedStep : std::true_type {
};

// The variant of an instance, one bit per feature of the header comment. The legal combinations are the
// static_asserts of score_wave; the named composites are the variants that exist (sa_wave_launch.h
// has the table that instantiates them).
enum : unsigned {
    kWaveAffine = 1u << 0,
    kWaveTrace = 1u << 1,
    kWaveBand = 1u << 2,
    kWaveEnds = 1u << 3,
    kWaveBandAt = 1u << 4,
    kWaveExtend = 1u << 5,
    kWaveSeed = 1u << 6,
};
constexpr unsigned kVarLinear = 0, kVarAffine = kWaveAffine;
constexpr unsigned kVarBand = kWaveAffine | kWaveBand;
constexpr unsigned kVarEnds = kWaveEnds, kVarAffineEnds = kWaveAffine | kWaveEnds;
constexpr unsigned kVarBandAtLocal = kWaveAffine | kWaveBand | kWaveBandAt;  // the local program
constexpr unsigned kVarBandAt = kVarBandAtLocal | kWaveEnds;                 // the global and the fit program
constexpr unsigned kVarExtend = kWaveExtend, kVarAffineExtend = kWaveAffine | kWaveExtend;
constexpr unsigned kVarSeeds = kVarExtend | kWaveSeed, kVarAffineSeeds = kVarAffineExtend | kWaveSeed;
constexpr unsigned kVarExtendBand = kVarAffineExtend | kWaveBand | kWaveBandAt;  // extension inside a width
constexpr unsigned kVarSeedsBand = kVarExtendBand | kWaveSeed;
constexpr unsigned kVarItems = kWaveSeed, kVarAffineItems = kWaveAffine | kWaveSeed;  // the global program on work items

// The kernel argument of every instance: the base arguments, then (traced instances) the direction arena,
// then one int and one pointer whose meaning is the variant's, then the width of a banded extension, which has
// both of those taken (xdrop, and with kWaveSeed items). The static_asserts of score_wave make the
// union members mutually exclusive; an instance loads only the fields of its flags.
struct WaveArgs {
    ScoreAffineArgs sa;
    union {
        int32_t band;   // kWaveBand without kWaveBandAt: the half-width
        int32_t ends;   // kWaveEnds: the SA_FREE_* flags
        int32_t xdrop;  // kWaveExtend
    };
    union {
        const Band *bands;      // kWaveBandAt: per pair, clipped (ScorePlan::bands)
        const SeedItem *items;  // kWaveSeed: a.order, a.np and a.out speak of items, a.pairs is unused
    };
    int32_t width;  // kWaveExtend with kWaveBandAt: the half-width about the anchor's diagonal
};
struct TracedWaveArgs {
    ScoreAffineArgs sa;
    TraceArgs tr;
    union {
        int32_t band, ends, xdrop;
    };
    union {
        const Band *bands;
        const SeedItem *items;
    };
    int32_t width;
};
// the offsets the instances were compiled against before the variants shared one struct
static_assert(offsetof(WaveArgs, sa.gap_extend) == 88 && offsetof(WaveArgs, band) == 96 && offsetof(WaveArgs, bands) == 104 &&
                  offsetof(WaveArgs, width) == 112 && sizeof(WaveArgs) == 120,
              "untraced kernel arguments: gap_extend, the variant's int, the variant's pointer");
static_assert(offsetof(TracedWaveArgs, tr.dirs) == 96 && offsetof(TracedWaveArgs, tr.dir_off) == 104 &&
                  offsetof(TracedWaveArgs, band) == 112 && offsetof(TracedWaveArgs, bands) == 120 &&
                  offsetof(TracedWaveArgs, width) == 128 && sizeof(TracedWaveArgs) == 136,
              "traced kernel arguments: the direction arena before the variant's fields");
// (through a class template, so that a kernel's mangled name spells F and not the expression on it)
template <unsigned F>
struct WaveArgsFor {
    using type = std::conditional_t<(F & kWaveTrace) != 0, TracedWaveArgs, WaveArgs>;
};
template <unsigned F>
using ArgsOf = typename WaveArgsFor<F>::type;

// The program. `tab` is the kernel's LDS copy of the score table (SMALL: unused, the four scores of a row
// sit in registers). The variant's values arrive as function arguments, unpacked by wave_kernel below,
// its only caller, and not as loads from the argument struct inside the body: the optimizer ranks an
// argument and a loaded value differently when it orders operands, and one more level of inlining moves
// code as well; the instances are to stay what they were (profiles/r19/score_disasm_compare.md). A banded
// extension's width arrives as `band`, which no other band-at instance reads.
template <int R, int MODE, bool SMALL, unsigned F>
__device__ __forceinline__ void score_wave(const ScoreArgs &a, int gap_extend, int32_t *tab, const TraceArgs &tr, int band, int ends,
                                           const Band *bands, int xdrop, const SeedItem *items)
{
    // static: the generic lambda `step` below would capture an automatic variable that it names in an
    // expression depending on its parameter, and one more capture reorders the instances' code
    static constexpr bool AFFINE = (F & kWaveAffine) != 0, TRACE = (F & kWaveTrace) != 0, BAND = (F & kWaveBand) != 0, ENDS = (F & kWaveEnds) != 0,
                          BAT = (F & kWaveBandAt) != 0, EXT = (F & kWaveExtend) != 0, SEED = (F & kWaveSeed) != 0;
    static_assert(!TRACE || (AFFINE && R == 8), "traced instances: affine, eight rows per lane");
    static_assert(MODE == SA_GLOBAL || MODE == SA_LOCAL || MODE == SA_FIT, "one of the three modes");
    static_assert(!BAND || (AFFINE && (BAT || MODE != SA_FIT)), "banded instances: affine; on the half-width, global or local");
    static_assert(!ENDS || (MODE != SA_LOCAL && (BAT || !BAND)), "ends-free instances: the global or the fit program, no band but the caller's");
    static_assert(!BAT || (BAND && (ENDS || MODE == SA_LOCAL || EXT)),
                  "band-at instances: banded; local, ends-free (global and fit are two of its flag sets), or an extension inside its width");
    static_assert(!EXT || (MODE == SA_GLOBAL && (!BAND || BAT) && !ENDS), "extension instances: the global borders, no band but its width's, no free ends");
    static_assert(!SEED || EXT || (MODE == SA_GLOBAL && !BAND && !ENDS),
                  "work items: extension alignment of a seed's half, or the plain global program on a chain's gap piece");
    constexpr bool LOCAL = MODE == SA_LOCAL, FIT = MODE == SA_FIT;
    constexpr bool BEST = LOCAL || EXT;  // the result is the best cell: per-row running best and the key
    constexpr int SENT = kBandSentinel;
    using Col = std::conditional_t<AFFINE, int2, int32_t>;  // a column of the boundary row
    const int lane = threadIdx.x;
    const int A = a.A, g = a.gap, ge = gap_extend;
    if (!SMALL)
    {
        for (int e = lane; e < A * A; e += kWave) tab[e] = a.table[e];
        __syncthreads();
    }
    Col *const rowbuf = (Col *)a.rows + (uint64_t)blockIdx.x * a.row_stride;
    const int kb = a.key_rowbits;
    const uint32_t kmask = (1u << kb) - 1u;
    bool bad = false;
    // ENDS: the free ends but TE, which is FIT; gapc(k), the cost of a border gap of k >= 1 cells
    const bool etb = ENDS && (ends & SA_FREE_TEXT_BEGIN), epb = ENDS && (ends & SA_FREE_PATTERN_BEGIN),
               epe = ENDS && (ends & SA_FREE_PATTERN_END);
    auto gapc = [&](int k) { return AFFINE ? g + (k - 1) * ge : g * k; };
    for (;;)
    {
        int w = 0;
        if (lane == 0) w = (int)atomicAdd(&a.ctrl[0], 1u);
        w = uniform(w);
        if (w >= a.np) break;
        const int pi = uniform(a.order[w]);
        int sdir = 1;  // SEED: the item's direction, -1 for a left half
        const ScorePair pd = SEED ? seed_item_pair(items, pi, &sdir) : a.pairs[pi];
        const int n = uniform((int)pd.n), m = uniform((int)pd.m);
        if constexpr (ENDS)
        {
            if (n == 0 || m == 0)
            {
                // the candidates are cells of the other side's border, 0 .. k: cell k, or under the
                // side's free end the first maximum, which lies at 0, 1 or k
                if (lane == 0)
                {
                    const bool rows = n == 0;  // the border is column 0 (both sides empty: its cell 0)
                    const int k = rows ? m : n;
                    const bool zero = rows ? epb : etb, anywhere = rows ? epe : FIT;
                    auto bval = [&](int c) { return c == 0 || zero ? 0 : -gapc(c); };
                    int bc = k, bv = bval(k);
                    if constexpr (BAT)
                    {
                        // only the border's in-band cells count: (c, 0) for -hi <= c <= -lo, (0, c) for
                        // lo <= c <= hi. The planner admitted the pair, so there is one, cell k is one
                        // unless any will do, and a border that costs has the origin in band. bval is
                        // linear from 1 on: the first maximum lies at ca, at 1 after 0, or at cb
                        const Band bd = bands[pi];
                        const int ca = max(0, rows ? -bd.hi : bd.lo), cb = min(k, rows ? -bd.lo : bd.hi);
                        if (anywhere)
                        {
                            bc = ca, bv = bval(ca);
                            if (ca == 0 && cb >= 1 && bval(1) > bv) bc = 1, bv = bval(1);
                            if (cb > bc && bval(cb) > bv) bc = cb, bv = bval(cb);
                        }
                    }
                    else if (anywhere)
                    {
                        bc = 0, bv = 0;
                        if (k >= 1 && bval(1) > bv) bc = 1, bv = bval(1);
                        if (k >= 2 && bval(k) > bv) bc = k, bv = bval(k);
                    }
                    sa_score_result r;
                    r.score = bv;
                    r.status = SA_OK;
                    r.end_text = rows ? 0 : (uint64_t)bc;
                    r.end_pattern = rows ? (uint64_t)bc : 0;
                    a.out[pi] = r;
                }
                continue;
            }
        }
        else if (n == 0 || m == 0)
        {
            // H[m][n] of an empty side is one run of max(n, m) gaps (alignSequenceCPU.cpp:232-236, :247-248)
            if (lane == 0)
            {
                const int k = FIT ? m : max(n, m);  // FIT: the text is free, only the pattern costs
                sa_score_result r;
                if constexpr (AFFINE) r.score = BEST || k == 0 ? 0 : -(g + (k - 1) * ge);
                else r.score = BEST ? 0 : -g * k;
                r.status = SA_OK;
                r.end_text = BEST || (FIT && m == 0) ? 0 : (uint64_t)n;
                r.end_pattern = BEST ? 0 : (uint64_t)m;
                a.out[pi] = r;
            }
            continue;
        }
        const int8_t *const text = a.text + pd.text_off;
        const int8_t *const pattern = a.pattern + pd.pattern_off;
        const int nstrips = (m + 64 * R - 1) / (64 * R);
        const int nbodies = (n + 63 + 63) / 64;  // steps 0 .. n + 62
        int hl[R];  // H[row][column - 1] of the lane's rows; after a strip, H[row][n]
        uint64_t lanekey = 0;
        // FIT: row m is row `frm` of lane `flm` of the last strip; fbest is the first maximum of the
        // lane's row frm over the strip's columns and fbestt the step it was met at
        const int flast = m - 1 - (nstrips - 1) * 64 * R;
        const int frm = flast % R, flm = flast / R;
        int fbest = INT32_MIN, fbestt = 0;
        // ENDS: the lane's first maximum of H[row][n] over its rows <= m of the strips so far, started
        // below any score, and its row
        int pebest = -(1 << 30), perow = 0;
        int bcarry = 0;  // EXT: B of the last row of the strips so far; B(0) = 0, the origin
        uint32_t *dlane = nullptr;  // TRACE: the lane's word of step 0 of the pair's first strip
        if constexpr (TRACE) dlane = tr.dirs + uniform64(tr.dir_off[pi]) + lane;
        // BAND: cell (i, j) is in band iff (unsigned)(j - i - blo) <= bspan
        int blo = 0;
        uint32_t bspan = 0;
        if constexpr (BAT && EXT)
        {
            // the band of the width about the anchor's diagonal, for this pair's or item's shape: wave-uniform
            const Band bd = band_ext(n, m, band);
            blo = bd.lo;
            bspan = (uint32_t)(bd.hi - bd.lo);
        }
        else if constexpr (BAT)
        {
            // the caller's band of this pair, clipped by the planner (band_clip): wave-uniform
            const Band bd = bands[pi];
            blo = uniform(bd.lo);
            bspan = (uint32_t)(uniform(bd.hi) - blo);
        }
        else if constexpr (BAND)
        {
            const Band bd = band_of(n, m, band);
            blo = bd.lo;
            bspan = (uint32_t)(bd.hi - bd.lo);
        }
        auto inb = [&](int i, int j) { return (uint32_t)(j - i - blo) <= bspan; };  // BAND: cell (i, j) is in band
        for (int s = 0; s < nstrips; ++s)
        {
            const int row1 = s * 64 * R + R * lane;  // rows row1 + 1 .. row1 + R
            // the strip's bodies: all of them, or (BAND) its window's
            BandWindow bw = {};
            if constexpr (BAT) bw = band_window_at(n, m, 64 * R, s, Band{blo, blo + (int)bspan});  // may be empty: no body
            else if constexpr (BAND) bw = band_window(n, m, 64 * R, s, Band{blo, blo + (int)bspan});
            const int bfirst = BAND ? bw.b0 : 0, bend = BAND ? bw.b1 : nbodies;
            if constexpr (BAND && EXT)
            {
                if (bfirst == bend) break;  // uniform: no row from here on holds an in-band cell
            }
            int s0[R], s1[R], s2[R], s3[R];  // S[pattern letter of the row][0..3] (SMALL)
            int prow[R];               // A * pattern letter of the row (LDS table row)
            int el[R];                 // AFFINE: E[row][column - 1]
            int best[R], bestt[R];
#pragma unroll
            for (int r = 0; r < R; ++r)
            {
                int c = 0;
                if (row1 + r < m)
                {
                    c = SEED ? pattern[(row1 + r) * sdir] : pattern[row1 + r];
                    bad = bad || c < 0 || c >= A;
                    c = min(max(c, 0), A - 1);
                }
                prow[r] = c * A;
                if constexpr (SMALL)
                {
                    s0[r] = a.table[c * A];
                    s1[r] = 1 < A ? a.table[c * A + 1] : 0;
                    s2[r] = 2 < A ? a.table[c * A + 2] : 0;
                    s3[r] = 3 < A ? a.table[c * A + 3] : 0;
                }
                // H[row][0], row = row1 + r + 1
                if constexpr (AFFINE)
                {
                    hl[r] = LOCAL ? 0 : -(g + (row1 + r) * ge);
                    el[r] = hl[r] - g + ge;  // stands for E[row][0] = -infinity
                }
                else hl[r] = LOCAL ? 0 : -(row1 + r + 1) * g;
                if constexpr (ENDS)
                {
                    hl[r] = epb ? 0 : hl[r];
                    if constexpr (AFFINE) el[r] = hl[r] - g + ge;
                }
                if constexpr (BAND)
                {
                    // a window past body 0 starts left of the band in every row; in body 0 the border
                    // cell (row, 0) is in band down to row -lo
                    // (BAT: from row -hi on, too)
                    const bool in = bfirst == 0 && (BAT ? inb(row1 + r + 1, 0) : row1 + r + 1 <= -blo);
                    hl[r] = in ? hl[r] : SENT;
                    el[r] = in ? el[r] : SENT;
                }
                // EXT: below any score, so that after the strip it is r(row); in a band the sentinel, which keeps
                // the drop test of a row without an in-band cell inside int32
                best[r] = EXT ? (BAND ? SENT : INT32_MIN) : 0;
                bestt[r] = 0;
            }
            if constexpr (FIT)
            {
                fbest = INT32_MIN;  // below any score: a row of negative values still has a first maximum
                fbestt = 0;
            }
            int upprev;  // H[row1][column - 1]
            if constexpr (AFFINE) upprev = LOCAL || row1 == 0 ? 0 : -(g + (row1 - 1) * ge);
            else upprev = LOCAL ? 0 : -row1 * g;
            if constexpr (ENDS) upprev = epb ? 0 : upprev;
            if constexpr (BAND)
            {
                if (bfirst == 0) upprev = (BAT ? inb(row1, 0) : row1 <= -blo) ? upprev : SENT;
                else
                {
                    // the cell left of the window in the row above: out of band for every lane but 0,
                    // whose row above is the previous strip's last and may have its band edge there
                    const int col = 64 * bfirst;  // >= 64 and < n; the previous strip's window holds it
                    const bool in = lane == 0 && (uint32_t)(col - row1 - blo) <= bspan;
                    if constexpr (BAT)
                    {
                        // a band with lo > 0 starts strip 0 past body 0: the row above is the border
                        // H[0][col]. After an empty strip `in` is false: its last row holds no in-band column
                        int v = SENT;
                        if (in) v = s == 0 ? (LOCAL || etb ? 0 : -gapc(col)) : rowbuf[col - 1].x;
                        upprev = v;
                    }
                    else upprev = in ? rowbuf[col - 1].x : SENT;
                }
            }
            int tl = 0, tfeed = 0, feed = 0, ofeed = 0;
            int fb = 0;                  // AFFINE: F[row1 + R][column] of the lane's last step,
            int feedf = 0, ofeedf = 0;   // and the F halves of the top-row feed and the bottom-row collection
            uint32_t *dstrip = nullptr;  // TRACE: the lane's word of step 0 of this strip
            if constexpr (TRACE)
            {
                if constexpr (BAND) dstrip = dlane;  // advanced past each strip's window below
                else dstrip = dlane + (uint64_t)s * (uint64_t)nbodies * (64 * 64);
            }
            auto step = [&](auto predc, const int t) {
                constexpr bool PRED = decltype(predc)::value;
                constexpr bool MASK = BAND && std::is_same<decltype(predc), MaskedStep>::value;  // a body that cuts a band edge
                const int up = dpp_shr1(feed, hl[R - 1]);  // lane 0: the top row's next column
                int upf = 0;
                if constexpr (AFFINE) upf = dpp_shr1(feedf, fb);  // and its F
                tl = dpp_shr1(tfeed, tl);                  // lane 0: the next text letter
                feed = dpp_shl1(feed, feed);
                if constexpr (AFFINE) feedf = dpp_shl1(feedf, feedf);
                tfeed = dpp_shl1(tfeed, tfeed);
                // ramp-up and ramp-down bodies: a lane outside columns 1..n keeps its state
                const bool valid = !PRED || (unsigned)(t - lane) < (unsigned)n;
                const bool b0 = (tl & 1) != 0, b1 = (tl & 2) != 0;
                int d = upprev, u = up, uf = upf;
                uint32_t word = 0;  // TRACE: the direction nibbles of the lane's rows
                // MASK: row r's cell lies qq - r diagonals above the band's lower edge
                int qq = 0;
                if constexpr (BAND)  // outside the test of MASK: an unbanded instance's step captures nothing more
                {
                    if constexpr (MASK) qq = t - lane - row1 - blo;
                }
#pragma unroll
                for (int r = 0; r < R; ++r)
                {
                    int sv;
                    if constexpr (SMALL)
                    {
                        const int x0 = s0[r], x1 = s1[r], x2 = s2[r], x3 = s3[r];
                        sv = b1 ? (b0 ? x3 : x2) : (b0 ? x1 : x0);
                    }
                    else sv = tab[prow[r] + tl];
                    int h, e = 0, f = 0;
                    if constexpr (AFFINE)
                    {
                        e = max(el[r] - ge, hl[r] - g);
                        f = max(uf - ge, u - g);
                        h = max(d + sv, max(e, f));
                        if constexpr (TRACE)
                        {
                            // the reference's tie rule with left := E, up := F; a run extends only when
                            // extending is strictly better than opening
                            uint32_t nib = d + sv > max(e, f) ? kDirDiag : e >= f ? kDirLeft : kDirTop;
                            if (LOCAL) nib = h <= 0 ? kDirStop : nib;
                            nib |= el[r] - ge > hl[r] - g ? kDirEExt : 0;
                            nib |= uf - ge > u - g ? kDirFExt : 0;
                            word |= nib << (4 * r);
                        }
                    }
                    else h = max(d + sv, max(hl[r] - g, u - g));
                    if (LOCAL) h = max(h, 0);
                    d = hl[r];
                    if constexpr (BAND)
                    {
                        if constexpr (MASK)
                        {
                            // an out-of-band cell is the sentinel in all three states, after the clamp
                            const bool in = (uint32_t)(qq - r) <= bspan;
                            h = in ? h : SENT;
                            e = in ? e : SENT;
                            f = in ? f : SENT;
                        }
                    }
                    if (PRED)
                    {
                        h = valid ? h : hl[r];
                        if constexpr (AFFINE) e = valid ? e : el[r];
                    }
                    if (BEST)
                    {
                        // a row meets its columns in ascending order: strictly greater keeps the first.
                        // EXT: H[row][0] (or H[row][n] again) may exceed the row's cells and is no candidate
                        const bool better = EXT ? valid && h > best[r] : h > best[r];
                        best[r] = better ? h : best[r];
                        bestt[r] = better ? t : bestt[r];
                    }
                    hl[r] = h;
                    u = h;
                    if constexpr (AFFINE)
                    {
                        el[r] = e;
                        uf = f;
                    }
                }
                if constexpr (FIT)
                {
                    // one value per lane and step instead of the local instances' R: the lane's row frm.
                    // A lane outside columns 1..n still (or again) holds H[row][0] (or H[row][n]): no column
                    int v = hl[0];
#pragma unroll
                    for (int r = 1; r < R; ++r) v = r == frm ? hl[r] : v;
                    const bool better = valid && v > fbest;
                    fbest = better ? v : fbest;
                    fbestt = better ? t : fbestt;
                }
                upprev = valid ? up : upprev;
                // lane 63's bottom-row value enters, the rest move down
                ofeed = dpp_shl1(hl[R - 1], ofeed);
                if constexpr (AFFINE)
                {
                    fb = valid ? uf : fb;
                    ofeedf = dpp_shl1(fb, ofeedf);
                }
                if constexpr (TRACE && BAND) dstrip[(uint32_t)(t - 64 * bfirst) * 64u] = word;
                else if constexpr (TRACE) dstrip[(uint32_t)t * 64u] = word;
            };
            for (int b = bfirst; b < bend; ++b)
            {
                const int c0 = 64 * b + lane;  // text index of tfeed; feed holds column c0 + 1
                tfeed = 0;
                if (c0 < n)
                {
                    const int c = SEED ? text[c0 * sdir] : text[c0];
                    bad = bad || c < 0 || c >= A;
                    tfeed = min(max(c, 0), A - 1);
                }
                if constexpr (AFFINE)
                {
                    if (s == 0)
                    {
                        if constexpr (ENDS) feed = etb ? 0 : -(g + c0 * ge);
                        else feed = LOCAL || FIT ? 0 : -(g + c0 * ge);  // H[0][c0 + 1]
                        feedf = feed - g + ge;              // stands for F[0][c0 + 1] = -infinity
                    }
                    else
                    {
                        const int2 v = c0 < n ? rowbuf[c0] : make_int2(0, 0);
                        feed = v.x;
                        feedf = v.y;
                    }
                    if constexpr (BAND)
                    {
                        // column c0 + 1 of the row above the strip: past the band's edge the row buffer
                        // holds what an earlier strip or pair left there, and strip 0's border has no end
                        const bool in = c0 < n && (uint32_t)(c0 + 1 - s * 64 * R - blo) <= bspan;
                        feed = in ? feed : SENT;
                        feedf = in ? feedf : SENT;
                    }
                }
                else
                {
                    if (s == 0)
                    {
                        if constexpr (ENDS) feed = etb ? 0 : -(c0 + 1) * g;
                        else feed = LOCAL || FIT ? 0 : -(c0 + 1) * g;
                    }
                    else feed = c0 < n ? rowbuf[c0] : 0;
                }
                // BAND: the body's diagonals j - i run from lane 63's last row at its first step to lane
                // 0's first row at its last step; a body that holds one outside the band masks its cells
                if constexpr (BAND)
                {
                    const int dmin = 64 * b - 64 * R * s - 64 * R - 62, dmax = 64 * b + 63 - 64 * R * s;
                    if (dmin < blo || dmax > blo + (int)bspan)
                    {
#pragma unroll 2
                        for (int k = 0; k < 64; ++k) step(MaskedStep{}, 64 * b + k);
                    }
                    else if (b == 0 || 64 * b + 64 > n)
                    {
#pragma unroll 2
                        for (int k = 0; k < 64; ++k) step(std::true_type{}, 64 * b + k);
                    }
                    else
                    {
#pragma unroll 4
                        for (int k = 0; k < 64; ++k) step(std::false_type{}, 64 * b + k);
                    }
                }
                else if (b == 0 || 64 * b + 64 > n)
                {
#pragma unroll 2
                    for (int k = 0; k < 64; ++k) step(std::true_type{}, 64 * b + k);
                }
                else
                {
#pragma unroll 4
                    for (int k = 0; k < 64; ++k) step(std::false_type{}, 64 * b + k);
                }
                // the 64 values lane 63 produced in this body: columns 64 b - 62 .. 64 b + 1, all read before
                if (s + 1 < nstrips)
                {
                    const int col = 64 * b - 62 + lane;
                    if (col >= 1 && col <= n)
                    {
                        if constexpr (AFFINE) rowbuf[col - 1] = make_int2(ofeed, ofeedf);
                        else rowbuf[col - 1] = ofeed;
                    }
                }
            }
            if constexpr (TRACE && BAND) dlane += (uint64_t)(bend - bfirst) * (64 * 64);
            if constexpr (ENDS)
            {
#pragma unroll
                for (int r = 0; r < R; ++r)
                {
                    const int row = row1 + r + 1;
                    // BAT: hl[r] is H[row][n] only where (row, n) is in band: the strip's window then reached
                    // column n; an empty strip and one that ends left of n fold nothing
                    const bool better = row <= m && (!BAT || inb(row, n)) && hl[r] > pebest;
                    pebest = better ? hl[r] : pebest;
                    perow = better ? row : perow;
                }
            }
            // EXT: rows from `stop` on count for nothing; a strip that holds row i* is the last one run
            int stop = INT32_MAX;
            if constexpr (EXT)
            {
                if (xdrop >= 0)  // wave-uniform
                {
                    // row i drops iff B(i - 1) - r(i) > xdrop, B(i - 1) the maximum of the carried B, of the
                    // lanes before (their rows come first) and of the lane's rows before
                    int lm = INT32_MIN, pm[R];
#pragma unroll
                    for (int r = 0; r < R; ++r)
                    {
                        pm[r] = lm;
                        lm = row1 + r < m ? max(lm, best[r]) : lm;
                    }
                    const int inc = wave_prefix_max(lm);
                    const int before = max(bcarry, dpp_shr1(INT32_MIN, inc));
                    int fr = R;  // the lane's first dropping row
#pragma unroll
                    for (int r = R - 1; r >= 0; --r)
                    {
                        // |H| < 2^30 and 0 <= B < 2^30 (planner): the difference stays inside int32
                        // (BAND: B < 2^29 and best[r] >= -2^30, the sentinel of a row without an in-band cell)
                        const bool drop = row1 + r < m && max(before, pm[r]) - best[r] > xdrop;
                        fr = drop ? r : fr;
                    }
                    const uint64_t dl = ballot(fr < R);
                    if (dl)
                    {
                        const int l0 = __builtin_ctzll(dl);
                        stop = s * 64 * R + R * l0 + __builtin_amdgcn_readlane(fr, l0) + 1;
                    }
                    else bcarry = max(bcarry, __builtin_amdgcn_readlane(inc, kWave - 1));
                }
            }
            if (BEST)
            {
#pragma unroll
                for (int r = 0; r < R; ++r)
                {
                    const int row = row1 + r + 1, col = bestt[r] - lane + 1;
                    const uint64_t key = ((uint64_t)(uint32_t)best[r] << (2 * kb)) |
                                         ((uint64_t)(~(uint32_t)row & kmask) << kb) | (uint64_t)(~(uint32_t)col & kmask);
                    if (row <= m && (!EXT || row < stop) && best[r] > 0 && key > lanekey) lanekey = key;
                }
            }
            if constexpr (EXT)
            {
                if (stop != INT32_MAX) break;  // uniform: the strips below run no body and store nothing
            }
        }
        sa_score_result res;
        res.status = SA_OK;
        if (BEST)
        {
            const uint64_t key = wave_max_u64(lanekey);
            const uint32_t H = (uint32_t)(key >> (2 * kb));
            res.score = (int32_t)H;
            res.end_pattern = H ? (uint64_t)(~(uint32_t)(key >> kb) & kmask) : 0;
            res.end_text = H ? (uint64_t)(~(uint32_t)key & kmask) : 0;
        }
        else if constexpr (FIT)
        {
            // the last strip's values of lane flm; every row has columns 1..n, so the lane met one
            res.score = __builtin_amdgcn_readlane(fbest, flm);
            res.end_text = (uint64_t)(__builtin_amdgcn_readlane(fbestt, flm) - flm + 1);
            res.end_pattern = (uint64_t)m;
        }
        else
        {
            const int last = m - 1 - (nstrips - 1) * 64 * R;  // row m inside the last strip
            const int rm = last % R;
            int v = hl[0];
#pragma unroll
            for (int r = 1; r < R; ++r) v = r == rm ? hl[r] : v;
            res.score = __builtin_amdgcn_readlane(v, last / R);
            res.end_text = (uint64_t)n;
            res.end_pattern = (uint64_t)m;
        }
        if constexpr (ENDS)
        {
            // res is the candidate of row m; the lowest row of the last column's maximum beats it when
            // it is no smaller and lies above row m (it is then at least H[m][n]); a border candidate,
            // (0, n) before (m, 0), wins only when it is strictly greater
            int bv = res.score;
            if constexpr (BAT)
            {
                // only in-band candidates count; the planner admitted the pair, so one of them does, and
                // in such a pair every in-band cell, border cells included, holds a real score (it lies
                // on a diagonal that starts in a permitted, in-band border cell). Row m: the running
                // best took the sentinel of an out-of-band column only until a real value came, which
                // is above -2^29 under the planner's limit and never ties it; a row m without an in-band
                // column in 1..n (or a last strip that ran no body) leaves something below. TE unset:
                // hl is H[m][n] only if (m, n) is in band
                const bool rowm = FIT ? bv > -(1 << 29) : inb(m, n);
                bv = rowm ? bv : SENT;
            }
            if (epe)
            {
                const uint64_t key = wave_max_u64(((uint64_t)(uint32_t)(pebest + (1 << 30)) << 32) | (uint64_t)~(uint32_t)perow);
                const int vc = (int)(uint32_t)(key >> 32) - (1 << 30), rc = (int)~(uint32_t)key;
                if ((!BAT || vc > SENT) && vc >= bv && rc < m)  // BAT: no fold at all leaves the start value
                {
                    bv = vc;
                    res.end_pattern = (uint64_t)rc;
                    res.end_text = (uint64_t)n;
                }
                const int h0n = etb ? 0 : -gapc(n);
                if ((!BAT || inb(0, n)) && h0n > bv)
                {
                    bv = h0n;
                    res.end_pattern = 0;
                    res.end_text = (uint64_t)n;
                }
            }
            if constexpr (FIT)
            {
                const int hm0 = epb ? 0 : -gapc(m);
                if ((!BAT || inb(m, 0)) && hm0 > bv)
                {
                    bv = hm0;
                    res.end_pattern = (uint64_t)m;
                    res.end_text = 0;
                }
            }
            res.score = bv;
        }
        if (lane == 0) a.out[pi] = res;
    }
    if (bad) __hip_atomic_store(&a.ctrl[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Every instance of the program as a kernel, one wave per workgroup, and the one place that unpacks the
// kernel argument: a variant's field is read only where its flag is set. sa_score.hip instantiates the
// untraced instances and sa_affine_walk.hip the traced ones, both through the table of sa_wave_launch.h.
template <int R, int MODE, bool SMALL, unsigned F>
__global__ __launch_bounds__(64) void wave_kernel(ArgsOf<F> w)
{
    __shared__ int32_t tab[SMALL ? 1 : 32 * 32];
    constexpr bool BAT = (F & kWaveBandAt) != 0;
    const int gap_extend = F & kWaveAffine ? w.sa.gap_extend : 0;
    constexpr bool EXTBAND = BAT && (F & kWaveExtend) != 0;
    const int band = (F & kWaveBand) && !BAT ? w.band : EXTBAND ? w.width : 0, ends = F & kWaveEnds ? w.ends : 0, xdrop = F & kWaveExtend ? w.xdrop : SA_NO_XDROP;
    const Band *const bands = BAT && !EXTBAND ? w.bands : nullptr;
    const SeedItem *const items = F & kWaveSeed ? w.items : nullptr;
    if constexpr ((F & kWaveTrace) != 0) score_wave<R, MODE, SMALL, F>(w.sa.s, gap_extend, tab, w.tr, band, ends, bands, xdrop, items);
    else score_wave<R, MODE, SMALL, F>(w.sa.s, gap_extend, tab, TraceArgs(), band, ends, bands, xdrop, items);
}

}  // namespace sa
