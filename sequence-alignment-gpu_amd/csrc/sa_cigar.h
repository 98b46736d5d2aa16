// CIGAR output inside the library (sa_hip.h sa_align_pairs_cigar): the sink that traced_run (sa_affine_walk.hip)
// hands a call's device strings to, and the encoder behind it (sa_cigar.hip). Host only.
#pragma once
#include <stdint.h>

#include <vector>

#include "sa_hip.h"

namespace sa {

// What a call with a CIGAR sink asks for and gets back. With a sink set, traced_run allocates the string arenas
// as for a call with strings, copies neither to the host and calls cigar_encode once every walk has ended well.
struct CigarSink {
    int32_t flags = SA_CIGAR_M;
    sa_cigar_result *results = nullptr;  // np entries: the encoder sets ops_off, num_ops and the five counts
    std::vector<uint32_t> ops;           // the call's op array, pair after pair
};

// Where the encoder finds a pair's columns: its slot of `cap` = text_len + pattern_len bytes in each arena.
struct CigarSlot {
    uint64_t off, cap;
};

// Encodes np pairs on `stream` (a hipStream_t), after the call's last walk or join: pair p's strings are the
// head piece at the start of its slot and the tail piece at the slot's end, of the lengths the host loop of
// traced_run derives from d_results[p].num_alignment_bytes and d_tail[p] (d_tail null: every string is all
// tail). Pass 1 of cigar_encode_kernel counts, the host sums the counts into ops_off, pass 2 writes into a
// buffer of the counted size, and one copy of 4 * total bytes fills sink->ops. Synchronous; records what
// sa_cigar_last_stats reports, `string_bytes` being the size of each arena.
int cigar_encode(void *stream, const char *d_text, const char *d_pattern, uint64_t string_bytes, const sa_result *d_results,
                 const uint64_t *d_tail, const std::vector<CigarSlot> &slots, char gap_letter, CigarSink *sink);

// The statistics of a call that failed before its encoder ran: all zero.
void cigar_reset_stats();

}  // namespace sa
