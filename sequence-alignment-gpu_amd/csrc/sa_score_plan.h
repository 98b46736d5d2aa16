// The score-only planner: everything a scorer (sa_scorer_*, sa_score_batch, sa_search) decides before
// its first HIP call, as one pure function of (params, pair shapes, CU count, knobs). No HIP here:
// sa_score_plan.cpp builds into libsa_hip.so and, with the plain host compiler, into
// bin/sa_score_plan_check (csrc/host/score_plan_check.cpp), which tests/test_score_plan.py runs
// without a GPU. DESIGN.md §3.4 has the kernel and the rule for R.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "sa_hip.h"

namespace sa {

// Environment knobs of the scorer (tuning and tests), read once per process.
struct ScoreKnobs {
    int rows_per_lane = 0;   // SA_SCORE_ROWS_PER_LANE: force R (1, 2, 4, 8)
    int waves_per_simd = 0;  // SA_SCORE_WAVES: resident waves per SIMD the grid is sized for
    int max_cus = 0;         // SA_MAX_CUS: plan as if the device had at most this many CUs
};
const ScoreKnobs &score_knobs();

// Instruction counts of the linear instances' steady loop (wave_kernel, kVarLinear; counted in the gfx950 assembly;
// DESIGN.md §3.4): one step of a wave costs kScoreStepBase + R * kScoreStepRow* instructions (the
// lane shifts and the loop; per row the score, the three-way maximum and, for local pairs, the
// clamp at zero and the running best) and advances 64 R cells.
constexpr int kScoreStepBase = 14;
constexpr int kScoreStepRowGlobal = 6;
constexpr int kScoreStepRowLocal = 10;
// The same of the affine instances' steady loop (kVarAffine): eight lane shifts where the
// linear instances have five, and per row the two extra states E and F (two subtractions and a maximum
// each, where the linear row has two subtractions).
constexpr int kScoreAffineStepBase = 18;
constexpr int kScoreAffineStepRowGlobal = 10;
constexpr int kScoreAffineStepRowLocal = 14;
// A fit instance (SA_FIT) is the global one of its kernel plus, per step, the best of row m:
// kScoreFitStepBest for the running best (the compare, the selects of the value and its step, the
// step number) and kScoreFitStepSelect for each of the R - 1 conditional moves that pick the lane's
// row among its R. Counted in the steady loops of both kernels: 5, 5 to 6, 7 to 8 and 10.5 to 13
// instructions per step above the global instance at R = 1, 2, 4, 8.
constexpr int kScoreFitStepBest = 5;
constexpr int kScoreFitStepSelect = 1;

// What a call asks of the wave program (sa_score_wave.h) beyond its sa_params: the variant, as a value. The
// C ABI functions build one, the planners check it against the mode and the pairs, the plan records the
// one it runs, and the launch table (sa_wave_launch.h) turns that into an instance.
struct WaveSpec {
    bool affine = false;           // a gap of k cells costs gap_open + (k - 1) * gap_extend, and
    int32_t gap_open = 0;          // sa_params.gap_penalty is ignored
    int32_t gap_extend = 0;
    bool banded = false;           // inside the diagonal band of one half-width (sa_hip.h)
    int32_t band = 0;
    bool band_at = false;          // inside a band of the caller's per pair (sa_hip.h sa_band)
    const sa_band *bands = nullptr;
    bool extend = false;           // extension alignment (sa_hip.h sa_score_batch_extend) under
    int32_t xdrop = SA_NO_XDROP;   // this X-drop, SA_NO_XDROP for none
    bool ext_band = false;         // an extension inside |j - i| <= width of its anchor's diagonal (sa_hip.h
    int32_t width = 0;             // sa_score_batch_extend_band): one half-width per call, both halves of a seed
    bool seeded = false;           // seed extension (sa_hip.h sa_seed, one per pair): an extension to both
    const sa_seed *seeds = nullptr;  // sides of the caller's seeds, planned by the make_seeds_* planners
    bool chained = false;          // chained seeds (sa_hip.h sa_score_batch_chains; with seeded): pair k owns
    const uint64_t *chain_off = nullptr;  // seeds[chain_off[k] .. chain_off[k + 1]), planned by the make_chains_* planners
    bool traced = false;           // the aligners' instances: direction words, affine whatever the penalties

    static WaveSpec gaps(int32_t open, int32_t extend)
    {
        WaveSpec s;
        s.affine = true;
        s.gap_open = open;
        s.gap_extend = extend;
        return s;
    }
    WaveSpec in_band(int32_t half_width) const
    {
        WaveSpec s = *this;
        s.banded = true;
        s.band = half_width;
        return s;
    }
    WaveSpec in_bands(const sa_band *per_pair) const
    {
        WaveSpec s = *this;
        s.band_at = true;
        s.bands = per_pair;
        return s;
    }
    WaveSpec extending(int32_t x) const
    {
        WaveSpec s = *this;
        s.extend = true;
        s.xdrop = x;
        return s;
    }
    WaveSpec within(int32_t w) const
    {
        WaveSpec s = *this;
        s.ext_band = true;
        s.width = w;
        return s;
    }
    WaveSpec from_seeds(const sa_seed *per_pair) const
    {
        WaveSpec s = *this;
        s.seeded = true;
        s.seeds = per_pair;
        return s;
    }
    WaveSpec from_chains(const sa_seed *flat, const uint64_t *off) const
    {
        WaveSpec s = from_seeds(flat);
        s.chained = true;
        s.chain_off = off;
        return s;
    }
};

#if defined(__HIPCC__)
#define SA_BAND_FN __host__ __device__ inline
#else
#define SA_BAND_FN inline
#endif

// The diagonal band of a pair (sa_hip.h has the definition): cell (i, j) is in band iff
// lo <= j - i <= hi. A half-width above max(n, m) admits every cell already and is cut to it, so
// everything below stays inside 32 bits for the lengths the planner admits (n, m < 2^24).
struct Band {
    int32_t lo, hi;
};
SA_BAND_FN Band band_of(int64_t n, int64_t m, int64_t w)
{
    const int64_t d = n - m, big = n > m ? n : m, ww = w < big ? w : big;
    return Band{(int32_t)((d < 0 ? d : 0) - ww), (int32_t)((d > 0 ? d : 0) + ww)};
}
// The window of strip s of `rows` rows (rows * s + 1 .. min(m, rows * (s + 1))): its in-band columns
// jmin .. jmax, never empty. Lane 0 meets column jmin at step jmin - 1 and lane 63 column jmax at step
// jmax + 62, so the strip runs the 64-step bodies b0 .. b1 - 1, and jmax - jmin + 64 of their steps
// touch the band. With every cell in band that is 0 .. nbodies - 1 and n + 63, the unbanded strip.
struct BandWindow {
    int32_t jmin, jmax, b0, b1;
};
SA_BAND_FN BandWindow band_window(int64_t n, int64_t m, int64_t rows, int64_t s, Band bd)
{
    const int64_t first = rows * s + 1, last = m < rows * (s + 1) ? m : rows * (s + 1);
    const int64_t jmin = first + bd.lo > 1 ? first + bd.lo : 1, jmax = last + bd.hi < n ? last + bd.hi : n;
    return BandWindow{(int32_t)jmin, (int32_t)jmax, (int32_t)((jmin - 1) / 64), (int32_t)((jmax + 62) / 64 + 1)};
}
// Cells (i, j), 1 <= i <= m, 1 <= j <= n, inside the band, for any lo <= hi: the sum over the rows
// ia .. ib that hold an in-band column (i + hi >= 1 and i + lo <= n) of
// min(n, i + hi) - max(1, i + lo) + 1, in closed form.
inline uint64_t band_cells(uint64_t n_, uint64_t m_, Band bd)
{
    const int64_t n = (int64_t)n_, m = (int64_t)m_, lo = bd.lo, hi = bd.hi;
    if (n == 0 || m == 0 || lo > hi) return 0;
    const int64_t ia = std::max<int64_t>(1, 1 - hi), ib = std::min<int64_t>(m, n - lo);
    if (ia > ib) return 0;
    auto tri = [](int64_t a, int64_t b) { return b < a ? 0 : (a + b) * (b - a + 1) / 2; };  // a + .. + b
    const int64_t k = std::min(std::max<int64_t>(n - hi, ia - 1), ib);   // rows ia .. k end at column i + hi
    const int64_t right = tri(ia, k) + (k - ia + 1) * hi + (ib - k) * n;
    const int64_t k2 = std::min(std::max<int64_t>(1 - lo, ia - 1), ib);  // rows ia .. k2 start at column 1
    const int64_t left = (k2 - ia + 1) + tri(k2 + 1, ib) + (ib - k2) * lo;
    return (uint64_t)(right - left + (ib - ia + 1));
}

// A caller's band (sa_hip.h sa_band, one per pair: the band-at functions) as the kernels take it: both
// limits brought into [-m, n], which changes no in-band cell of a reachable pair. A band with no cell
// at all (lo > n or hi < -m; only a local pair gets this far) becomes {n, n} or {-m, -m}: one border
// cell, no interior cell.
SA_BAND_FN Band band_clip(int64_t n, int64_t m, int64_t lo, int64_t hi)
{
    const int64_t l = lo < -m ? -m : lo > n ? n : lo, h = hi < -m ? -m : hi > n ? n : hi;
    return Band{(int32_t)l, (int32_t)h};
}
// The band of a banded extension (sa_hip.h sa_score_batch_extend_band) of half-width w >= 0 about the
// diagonal of its anchor, the origin of the extension matrix, clipped as band_clip clips: a wider w
// admits no further cell. The planner, the kernels and the walks all derive it from (n, m, w); for a
// seed's half, from the half's own shape.
SA_BAND_FN Band band_ext(int64_t n, int64_t m, int64_t w)
{
    return Band{(int32_t)(w < m ? -w : -m), (int32_t)(w < n ? w : n)};
}
// band_window for any lo <= hi. Rows of the strip with an in-band column in 1..n are those from 1 - hi
// to n - lo; their windows shift right row by row, so the strip's in-band columns run from the first
// such row's to the last such row's. A strip without one is empty: b0 == b1, jmax < jmin, no body runs
// and no direction word is stored. With lo <= min(0, n - m) and hi >= max(0, n - m) (band_of) every row
// has one and the result is band_window's.
SA_BAND_FN BandWindow band_window_at(int64_t n, int64_t m, int64_t rows, int64_t s, Band bd)
{
    const int64_t first = rows * s + 1, last = m < rows * (s + 1) ? m : rows * (s + 1);
    const int64_t ia = first > 1 - bd.hi ? first : 1 - bd.hi, ib = last < n - bd.lo ? last : n - bd.lo;
    if (ia > ib) return BandWindow{1, 0, 0, 0};
    const int64_t jmin = ia + bd.lo > 1 ? ia + bd.lo : 1, jmax = ib + bd.hi < n ? ib + bd.hi : n;
    return BandWindow{(int32_t)jmin, (int32_t)jmax, (int32_t)((jmin - 1) / 64), (int32_t)((jmax + 62) / 64 + 1)};
}

// The value of H, E and F of every out-of-band cell, and the limit of the banded planner: with
// (max|S| + G)(n + m) + G (n + m) < kBandScoreLimit (G the larger of |gap open| and |gap extend|) no
// score falls below -2^29 + G, and a value derived from the sentinel, at most two penalties above
// it, stays below that and inside int32.
constexpr int32_t kBandSentinel = -(1 << 30);
constexpr uint64_t kBandScoreLimit = 1ull << 29;

struct ScorePlan {
    int mode = 0, A = 0, gap = 0, R = 1, key_rowbits = 1;  // gap: the linear penalty, or gap open
    WaveSpec spec;                 // the variant the scorer runs: the call's, but affine false where the linear
                                   // instances serve (an extension with gap open == gap extend), bands and seeds null
    std::vector<Band> bands;       // band-at scorer: every pair's band, clipped (band_clip)
    int num_cu = 0, waves_per_simd = 0, grid = 0;
    int64_t num_pairs = 0;
    uint64_t max_text = 0;         // longest text
    uint64_t row_stride = 0;       // columns of one wave's boundary row (max_text plus padding): an int
                                   // each, affine an (H, F) pair of ints each
    uint64_t input_bytes = 0;      // text and pattern letters of every pair (the caller's arenas)
    uint64_t device_bytes = 0;     // inputs, descriptors, results, row buffers, constants
    uint64_t padded_cells = 0;     // sum of n * ceil(m / 64R) * 64R; banded: of each strip's in-band columns * 64R
    uint64_t band_cells = 0;       // banded: cells inside the bands of all pairs
    uint64_t cost[4] = {0, 0, 0, 0};  // the model's cost of R = 1, 2, 4, 8 (instructions per wave)
    std::vector<int32_t> order;    // pair indices, most cells (banded: band cells) first, ties by index
};

// Plans `np` pairs for a device of `num_cu` compute units. Returns SA_OK, or the SA_ERR_* code with
// its message in *err. `spec` says what the call asks for:
//  - affine false: the linear gap P->gap_penalty; else the affine gap model.
//  - banded: the banded scorer of that half-width (affine only, global or local): a strip is charged the
//    steps of its window, the work order and padded_cells count band cells, and the score limit is
//    kBandScoreLimit.
//  - band_at (and not banded): the band-at scorer (sa_hip.h sa_score_batch_band_at), bands[p] the band of pair
//    p, in every mode: lo > hi and a pair that sa_band_reachable denies are SA_ERR_INVALID, the message
//    naming the pair; the rest as with `banded`, on the clipped bands (ScorePlan::bands), and the
//    descriptors count 8 more bytes per pair. `bands` may be null when there is no pair.
//  - extend: the extension scorer (sa_hip.h sa_score_batch_extend), which takes the affine gap model, the mode
//    SA_GLOBAL and an xdrop of SA_NO_XDROP .. 2^30 - 1 (else SA_ERR_INVALID) and no band of either kind
//    (SA_ERR_UNSUPPORTED). Cost, R, grid and bytes are the local program's, the linear one when gap open
//    equals gap extend (unless `traced`); xdrop changes nothing, the stop rows are not known beforehand. The
//    limits are the int32 one and the local best-cell key's.
//  - ext_band (with extend): the banded extension scorer (sa_hip.h sa_score_batch_extend_band). width < 0 is
//    SA_ERR_INVALID. A pair is planned on band_ext(n, m, width) as a band-at pair is on its band: a strip is
//    charged its band_window_at steps at the local step cost, the order and padded_cells count band cells, and
//    kBandScoreLimit applies. The instance is affine whatever the penalties; no bands are kept, the kernel
//    computes each from the width.
//  - seeded: SA_ERR_INVALID. Seeds are planned as work items, by make_seeds_score_plan.
int make_score_plan(const sa_params *P, const WaveSpec &spec, const sa_pair *pairs, int64_t np, int num_cu, const ScoreKnobs &kn,
                    ScorePlan *out, std::string *err);

// Seed extension (sa_hip.h sa_score_batch_seeds): a pair becomes up to two work items, the extension of
// its left half read backwards and of its right half read forwards; an empty half is no item. The
// kernels draw items, not pairs. text_off and pattern_off address the half's first-read letters in the
// arenas: letter k of the half's text is arena[text_off + dir * k].
struct SeedItem {
    uint64_t text_off, pattern_off;
    uint32_t n, m;   // columns and rows of the half
    int32_t dir;     // +1 the right half, -1 the left half
    int32_t pair;
};
// One pair of a seeds call as the combine and walk kernels take it: the arena offsets of the seed's first
// letters, the seed, and the pair's items (-1: that half is empty).
struct SeedPair {
    uint64_t text_seed, pattern_seed;
    uint64_t ts, ps, len;
    int32_t left, right;
};
struct SeedItems {
    std::vector<SeedItem> items;  // pair by pair, left before right
    std::vector<SeedPair> pairs;
};

// Plans the seeds scorer (`spec` an extension's, seeded or not; the plan's is): `seeds` null with pairs, ts + L > n and ps + L > m are SA_ERR_INVALID, the
// message naming the first such pair; the mode, the xdrop and the limits are make_score_plan's for the
// extension scorer on the whole pairs' (n, m). The plan is then make_score_plan's for the items as
// extension pairs: costed by the local step model, ordered by cells (plan->order holds item indices and
// plan->num_pairs the number of items). input_bytes is the whole pairs'; device_bytes adds the items'
// 8 bytes above a pair descriptor and, per pair, a SeedPair and a sa_seed_result.
int make_seeds_score_plan(const sa_params *P, const WaveSpec &spec, const sa_pair *pairs, const sa_seed *seeds, int64_t np, int num_cu,
                          const ScoreKnobs &kn, ScorePlan *out, SeedItems *items, std::string *err);

// Chained seeds (sa_hip.h sa_score_batch_chains): a pair becomes its two end items, the left half of its first
// seed and the right half of its last (SeedItem, as the seeds scorer has them), and one gap item per rectangle
// between two consecutive seeds, a SeedItem with dir +1 that the global program fills (kVarItems,
// kVarAffineItems). A piece with an empty side is no item: an empty end scores 0 as ever, and an empty-side gap is
// one gap run whose closed-form score and length go into the pair's record.
struct ChainSeed {
    uint64_t text_off, pattern_off, len;  // the arena offsets of the seed's first letters
    int32_t gap, pad;                     // the gap item between this seed and the next, -1: none, or one with an empty side
};
// One pair of a chains call as the combine, walk and join kernels take it.
struct ChainPair {
    uint64_t text_base, pattern_base;  // the arena offsets of the pair's first letters
    uint64_t ts, ps;                 // the first seed's position in the pair
    uint64_t te, pe;                 // the last seed's end
    int32_t seed_begin, seed_end;    // the pair's seeds in ChainItems::seeds (the caller's chain_off)
    int32_t gap_begin, gap_end;      // its gap items in ChainItems::gaps, in chain order
    int32_t left, right;             // its end items in ChainItems::ends, -1: that end is empty
    int32_t closed_score;            // the sum of its empty-side gaps' scores, -(gap_open + (k - 1) gap_extend) each
    uint32_t closed_cols;            // and of their lengths k
};
struct ChainItems {
    std::vector<SeedItem> ends;      // pair by pair, left before right
    std::vector<SeedItem> gaps;      // pair by pair, in chain order
    std::vector<ChainSeed> seeds;
    std::vector<ChainPair> pairs;
};
// The chains scorer's plan: two launches on one stream, each with its own R, grid, boundary rows and work order.
// `ends` is the seeds scorer's plan of the end items (spec.seeded and spec.chained set), `gaps` the global
// scorer's plan of the gap items (spec.seeded set and spec.extend not: the items variants; linear when gap open
// equals gap extend, unless traced). ends.input_bytes is the whole pairs'; device_bytes is the sum of both
// launches' and of the per-pair records, seeds and results.
struct ChainsScorePlan {
    ScorePlan ends, gaps;
    ChainItems items;
    uint64_t device_bytes = 0;
};
// Plans the chains scorer; `spec` is an extension's with from_chains(). SA_ERR_INVALID, the message naming the
// pair and (where one is at fault) the seed's index in its chain, for: seeds or chain_off null with pairs,
// chain_off[0] != 0, chain_off decreasing, a pair without a seed, a seed outside its pair, and a seed that
// begins before the one before it ends, on either side. A width (ext_band) is SA_ERR_UNSUPPORTED, as a band of
// either kind is for every extension. The mode, the xdrop and the limits are make_score_plan's for the extension
// scorer on the whole pairs' (n, m).
int make_chains_score_plan(const sa_params *P, const WaveSpec &spec, const sa_pair *pairs, int64_t np, int num_cu, const ScoreKnobs &kn,
                           ChainsScorePlan *out, std::string *err);

// Resident waves per SIMD the grid is sized for at R rows per lane (register budget of the
// instances).
int score_waves_per_simd(int R);
int score_affine_waves_per_simd(int R);
int score_ext_band_waves_per_simd(int R);  // the banded extension and banded seeds instances

}  // namespace sa
