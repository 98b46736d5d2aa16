// The affine alignment path inside the library (sa_affine_walk.hip): what sa_align_pairs_affine and
// sa_search_affine (sa_score.hip) share. Host only.
#pragma once
#include <stdint.h>

#include "sa_hip.h"
#include "sa_score_plan.h"

namespace sa {

struct CigarSink;  // sa_cigar.h

// Aligns `np` pairs addressed in the device arenas d_text / d_pattern (alphabet indices) on `device`
// under the gap model of `spec`: the traced Gotoh fill and the walk, chunk by chunk of the work order
// (sa_trace_plan.h), on the null stream; synchronous. results: np entries. aligned_text /
// aligned_pattern: both null, or np host buffers of at least text_len + pattern_len bytes each.
// `spec` banded: inside the diagonal band of that half-width (sa_align_pairs_banded); band_at: inside
// bands[p] for pair p (sa_align_pairs_band_at; null bands with pairs is SA_ERR_INVALID); extend: extension
// alignment under that X-drop (sa_align_pairs_extend); seeded: align_seeds_device below.
// `cigar` (sa_align_pairs_cigar; aligned_text and aligned_pattern are then null): the strings are made on the device
// as for a call that takes them, stay there, and are encoded into the sink's ops and counts before the call returns.
int align_affine_device(const sa_params *P, const WaveSpec &spec, const sa_pair *pairs, int64_t np, int device, const void *d_text,
                        const void *d_pattern, sa_result *results, char *const *aligned_text, char *const *aligned_pattern,
                        CigarSink *cigar = nullptr);

// Every sa_align_pairs_*: the host pairs packed into two arenas and uploaded, then align_affine_device.
int align_host_pairs(const sa_params *P, const WaveSpec &spec, const sa_host_pair *pairs, int64_t np, int device, sa_result *results,
                     char *const *aligned_text, char *const *aligned_pattern, CigarSink *cigar = nullptr);

// Seed extension (sa_hip.h sa_score_batch_seeds): seeds_combine_kernel (sa_score.hip), one wave per pair
// after the items' fill, shared by the seeds scorer and the seeds aligner. It sums the seed's scores, flags
// a seed letter outside the alphabet in ctrl[1] and writes the pair's sa_seed_result from the results of
// its items. `stream` is a hipStream_t.
struct SeedsCombineArgs {
    const int8_t *text, *pattern;
    const SeedPair *pairs;
    const int32_t *order;              // workgroup w combines pair order[w]; null: pair w
    const int32_t *table;              // A x A scores, [pattern][text]
    const sa_score_result *item_out;   // the fill's result of every item
    sa_seed_result *out;
    uint32_t *ctrl;
    int32_t A;
};
void launch_seeds_combine(const SeedsCombineArgs &a, int64_t np, void *stream);

// Chained seeds (sa_hip.h sa_score_batch_chains): chains_combine_kernel (sa_score.hip), one wave per pair after
// the two fills, shared by the chains scorer and the chains aligner. It sums the substitution scores of all the
// pair's seed columns and the scores of its gap items, adds the closed-form gaps, flags a seed letter outside the
// alphabet in ctrl[1] and writes the pair's sa_seed_result from these and its two end items.
struct ChainsCombineArgs {
    const int8_t *text, *pattern;
    const ChainPair *pairs;
    const ChainSeed *seeds;
    const int32_t *order;              // workgroup w combines pair order[w]; null: pair w
    const int32_t *table;              // A x A scores, [pattern][text]
    const sa_score_result *end_out;    // the extension fill's result of every end item
    const sa_score_result *gap_out;    // the global fill's result of every gap item
    sa_seed_result *out;
    uint32_t *ctrl;
    int32_t A;
};
void launch_chains_combine(const ChainsCombineArgs &a, int64_t np, void *stream);

// sa_align_pairs_seeds on device arenas: the traced fill of the work items, the combine and the seeded walk,
// chunk by chunk (sa_trace_plan.h SeedTracePlan); arguments as align_affine_device, the seeds are spec.seeds.
int align_seeds_device(const sa_params *P, const WaveSpec &spec, const sa_pair *pairs, int64_t np, int device, const void *d_text,
                       const void *d_pattern, sa_result *results, char *const *aligned_text, char *const *aligned_pattern,
                       CigarSink *cigar = nullptr);

// sa_align_pairs_chains on device arenas: per chunk (sa_trace_plan.h ChainTracePlan) the traced fills of the gap
// items and of the end items, the combine, the walk of every item at once and the join of the pairs; arguments as
// align_affine_device, the chains are spec.seeds and spec.chain_off.
int align_chains_device(const sa_params *P, const WaveSpec &spec, const sa_pair *pairs, int64_t np, int device, const void *d_text,
                        const void *d_pattern, sa_result *results, char *const *aligned_text, char *const *aligned_pattern,
                        CigarSink *cigar = nullptr);

}  // namespace sa
