// Kernel arguments of the score-only kernels: score_kernel (sa_score.hip, linear gap) and
// score_affine_kernel (sa_score_affine.hip, gap open / gap extend). The host side of both is in
// sa_score.hip; the affine kernel is launched through launch_score_affine.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "sa_hip.h"

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

// score_affine_kernel<R, LOCAL, SMALL> on `grid` one-wave workgroups (sa_score_affine.hip). R is 1, 2,
// 4 or 8; a.gap is the gap-open penalty.
void launch_score_affine(const ScoreArgs &a, int gap_extend, int R, bool local, bool small, int grid, hipStream_t st);

}  // namespace sa
