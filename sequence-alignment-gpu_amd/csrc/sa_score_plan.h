// The score-only planner: everything a scorer (sa_scorer_*, sa_score_batch, sa_search) decides before
// its first HIP call, as one pure function of (params, pair shapes, CU count, knobs). No HIP here:
// sa_score_plan.cpp builds into libsa_hip.so and, with the plain host compiler, into
// bin/sa_score_plan_check (csrc/host/score_plan_check.cpp), which tests/test_score_plan.py runs
// without a GPU. DESIGN.md §3.4 has the kernel and the rule for R.
#pragma once
#include <stdint.h>

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

// Instruction counts of score_kernel's steady loop (sa_score.hip, counted in the gfx950 assembly;
// DESIGN.md §3.4): one step of a wave costs kScoreStepBase + R * kScoreStepRow* instructions (the
// lane shifts and the loop; per row the score, the three-way maximum and, for local pairs, the
// clamp at zero and the running best) and advances 64 R cells.
constexpr int kScoreStepBase = 14;
constexpr int kScoreStepRowGlobal = 6;
constexpr int kScoreStepRowLocal = 10;
// The same of score_affine_kernel's steady loop (sa_score_affine.hip): eight lane shifts where the
// linear kernel has five, and per row the two extra states E and F (two subtractions and a maximum
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

// The affine gap model of a scorer: a gap of k cells costs open + (k - 1) * extend. With it,
// sa_params.gap_penalty is ignored.
struct ScoreGap {
    int32_t open, extend;
};

struct ScorePlan {
    int mode = 0, A = 0, gap = 0, R = 1, key_rowbits = 1;  // gap: the linear penalty, or gap open
    bool affine = false;           // score_affine_kernel: gap, gap_extend
    int gap_extend = 0;
    int num_cu = 0, waves_per_simd = 0, grid = 0;
    int64_t num_pairs = 0;
    uint64_t max_text = 0;         // longest text
    uint64_t row_stride = 0;       // columns of one wave's boundary row (max_text plus padding): an int
                                   // each, affine an (H, F) pair of ints each
    uint64_t input_bytes = 0;      // text and pattern letters of every pair (the caller's arenas)
    uint64_t device_bytes = 0;     // inputs, descriptors, results, row buffers, constants
    uint64_t padded_cells = 0;     // sum of n * ceil(m / 64R) * 64R
    uint64_t cost[4] = {0, 0, 0, 0};  // the model's cost of R = 1, 2, 4, 8 (instructions per wave)
    std::vector<int32_t> order;    // pair indices, most cells first, ties by index
};

// Plans `np` pairs for a device of `num_cu` compute units. Returns SA_OK, or the SA_ERR_* code with
// its message in *err. `affine` null: the linear gap P->gap_penalty; else the affine gap model.
int make_score_plan(const sa_params *P, const sa_pair *pairs, int64_t np, int num_cu, const ScoreKnobs &kn,
                    ScorePlan *out, std::string *err, const ScoreGap *affine = nullptr);

// Resident waves per SIMD the grid is sized for at R rows per lane (register budget of the
// instances).
int score_waves_per_simd(int R);
int score_affine_waves_per_simd(int R);

}  // namespace sa
