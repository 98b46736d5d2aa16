// The planner of the affine alignment path (sa_align_pairs_affine, sa_search_affine): what the traced
// Gotoh fill and its traceback need before the first HIP call, as one pure function of (params, gap
// open, gap extend, pair shapes, CU count, knobs, arena budget). No HIP here: sa_trace_plan.cpp builds
// into libsa_hip.so and, with the plain host compiler, into bin/sa_trace_plan_check
// (csrc/host/trace_plan_check.cpp), which tests/test_trace_plan.py runs without a GPU. DESIGN.md §3.5
// has the direction words, the walk and the chunking.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "sa_hip.h"
#include "sa_score_plan.h"

namespace sa {

// The traced fill runs strips of 64 lanes x 8 rows and writes one dword (eight direction nibbles) per
// lane and step: a strip is 512 rows, a step of a strip 256 bytes.
constexpr int kTraceRows = 8;
constexpr uint64_t kTraceStripRows = 64 * kTraceRows;
constexpr uint64_t kTraceStepBytes = 64 * 4;
constexpr uint64_t kTraceArenaDefault = 2ull << 30;
// Resident waves per SIMD the grid is sized for: the traced instances take 154 to 226 VGPRs
// (DESIGN.md §3.5), two waves of the SIMD's 512 in three of the four.
constexpr int kTraceWavesPerSimd = 2;

// SA_TRACE_ARENA_BYTES: the budget of the direction arena, read once per process.
uint64_t trace_arena_budget();

// Strips, steps and direction bytes of an m-row, n-column pair: ceil(m / 512) strips of
// 64 nbodies steps, nbodies = (n + 126) / 64 rounded down as in score_wave (steps 0 .. n + 62 in whole
// 64-step bodies). A pair with an empty side has no cells and no directions.
inline uint64_t trace_strips(uint64_t m) { return (m + kTraceStripRows - 1) / kTraceStripRows; }
inline uint64_t trace_steps(uint64_t n) { return 64 * ((n + 126) / 64); }
inline uint64_t trace_dir_bytes(uint64_t n, uint64_t m)
{
    return n == 0 || m == 0 ? 0 : trace_strips(m) * trace_steps(n) * kTraceStepBytes;
}

// The same of a banded pair (sa_hip.h; band_of and band_window in sa_score_plan.h): a strip stores
// only the steps of its window, 64 (b1 - b0) of them, and the strips' windows follow one another. The
// planner sizes the pair with it, the traced fill advances by it strip after strip, and the walk
// finds a strip's first word with it. With every cell in band it is trace_dir_bytes.
SA_BAND_FN uint64_t trace_band_strip_words(int64_t n, int64_t m, int64_t s, Band bd)
{
    const BandWindow bw = band_window(n, m, (int64_t)kTraceStripRows, s, bd);
    return (uint64_t)(bw.b1 - bw.b0) * (64 * 64);
}
inline uint64_t trace_band_dir_bytes(uint64_t n, uint64_t m, int64_t band)
{
    if (n == 0 || m == 0) return 0;
    const Band bd = band_of((int64_t)n, (int64_t)m, band);
    uint64_t words = 0;
    for (uint64_t s = 0; s < trace_strips(m); ++s) words += trace_band_strip_words((int64_t)n, (int64_t)m, (int64_t)s, bd);
    return words * 4;
}

// The same for a band of the caller's (any lo <= hi, clipped: band_clip): band_window_at, whose empty
// strips store nothing. On the bands of band_of both give the figures above.
SA_BAND_FN uint64_t trace_band_at_strip_words(int64_t n, int64_t m, int64_t s, Band bd)
{
    const BandWindow bw = band_window_at(n, m, (int64_t)kTraceStripRows, s, bd);
    return (uint64_t)(bw.b1 - bw.b0) * (64 * 64);
}
inline uint64_t trace_band_at_dir_bytes(uint64_t n, uint64_t m, Band bd)
{
    if (n == 0 || m == 0) return 0;
    uint64_t words = 0;
    for (uint64_t s = 0; s < trace_strips(m); ++s) words += trace_band_at_strip_words((int64_t)n, (int64_t)m, (int64_t)s, bd);
    return words * 4;
}

struct TracePlan {
    ScorePlan score;                  // validation, work order, key bits, grid and boundary rows (R = 8, affine)
    uint64_t budget = 0;              // direction bytes one chunk may hold
    std::vector<uint64_t> dir_bytes;  // per pair
    std::vector<uint64_t> dir_off;    // per pair: byte offset of its directions in its chunk's arena
    std::vector<uint64_t> slot_off;   // per pair: byte offset of its text_len + pattern_len string slot
    std::vector<int64_t> chunk_begin; // chunk c is positions chunk_begin[c] .. chunk_begin[c + 1] - 1 of score.order
    uint64_t arena_bytes = 0;         // direction bytes of the largest chunk: the arena's size
    uint64_t total_dir_bytes = 0;     // of all pairs
    uint64_t string_bytes = 0;        // of each of the two string arenas
    int64_t num_chunks() const { return (int64_t)chunk_begin.size() - 1; }
};

// Plans `np` pairs for `spec`, the call's WaveSpec with its gap model (the planner sets `traced`). Returns
// SA_OK, or the SA_ERR_* code with its message in *err: make_score_plan's for the spec, or
// SA_ERR_UNSUPPORTED for a pair whose directions exceed `budget`.
//  - banded: the banded aligner; a pair's directions are its band's (trace_band_dir_bytes), the chunks are
//    cut by them, and a pair is refused only when its band exceeds the budget.
//  - band_at: the band-at aligner, bands[p] the band of pair p (make_score_plan's checks;
//    trace_band_at_dir_bytes of the clipped band).
//  - extend: the extension aligner (sa_hip.h sa_align_pairs_extend; make_score_plan's checks). A pair is
//    planned with the directions of a global pair: where its fill stops is not known beforehand.
//  - ext_band (with extend): the banded extension aligner (sa_align_pairs_extend_band): a pair's directions are
//    trace_band_at_dir_bytes of band_ext(n, m, width), whatever its fill's stop row.
int make_trace_plan(const sa_params *P, const WaveSpec &spec, const sa_pair *pairs, int64_t np, int num_cu, const ScoreKnobs &kn,
                    uint64_t budget, TracePlan *out, std::string *err);

// The seeds aligner (sa_hip.h sa_align_pairs_seeds): the traced fill draws work items (SeedItems), the walk
// pairs. dir_bytes and dir_off are per item, each half traced as a global pair of its shape, ps x ts and
// (m - ps - L) x (n - ts - L), never the pair's n x m; slot_off is per pair, its text_len + pattern_len
// bytes. The chunks are cut over the pairs, ordered by the cells of both halves together, so that a
// pair's halves share a chunk: chunk c walks positions pair_chunk_begin[c] .. of pair_order and fills
// positions chunk_begin[c] .. of score.order, that chunk's items, most cells first. A pair is
// SA_ERR_UNSUPPORTED only when its two halves together exceed `budget`. Under a width (spec.ext_band) each half
// is traced inside band_ext of its own shape: two banded rectangles, and the orders count their band cells.
struct SeedTracePlan : TracePlan {
    SeedItems seeds;
    std::vector<int32_t> pair_order;
    std::vector<int64_t> pair_chunk_begin;
    int64_t num_pairs = 0;
};
int make_seeds_trace_plan(const sa_params *P, const WaveSpec &spec, const sa_pair *pairs, const sa_seed *seeds, int64_t np, int num_cu,
                          const ScoreKnobs &kn, uint64_t budget, SeedTracePlan *out, std::string *err);

// The chains aligner (sa_hip.h sa_align_pairs_chains): two traced fills per chunk, of the chunk's end items
// (`score`, its order cut by chunk_begin; dir_bytes and dir_off per end item) and of its gap items (`gaps`, cut by
// gap_chunk_begin; gap_dir_bytes and gap_dir_off per gap item), into one arena. Every piece is charged
// trace_dir_bytes of its own rectangle, never of n x m; a piece with an empty side has no item and no bytes. The
// chunks are cut over the pairs, ordered by the cells of all their pieces, so that a pair's pieces share a chunk;
// inside a chunk each launch's items are ordered by cells. A pair is SA_ERR_UNSUPPORTED only when its pieces
// together exceed `budget`. slot_off is per pair, its text_len + pattern_len bytes.
struct ChainTracePlan : TracePlan {
    ScorePlan gaps;
    ChainItems items;
    std::vector<uint64_t> gap_dir_bytes, gap_dir_off;
    std::vector<int64_t> gap_chunk_begin;
    std::vector<int32_t> pair_order;
    std::vector<int64_t> pair_chunk_begin;
    int64_t num_pairs = 0;
};
int make_chains_trace_plan(const sa_params *P, const WaveSpec &spec, const sa_pair *pairs, int64_t np, int num_cu, const ScoreKnobs &kn,
                           uint64_t budget, ChainTracePlan *out, std::string *err);

}  // namespace sa
