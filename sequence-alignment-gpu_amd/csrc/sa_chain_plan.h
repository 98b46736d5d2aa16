// Chaining (sa_hip.h sa_chain_anchors): the host side that needs no device. chain_plan validates a call and
// turns its anchors into the structure-of-arrays form both implementations read; chain_host is the definition
// itself, anchor by anchor, which sa_chain_anchors_host returns and the device kernels (sa_chain.hip) must equal
// bit for bit. Plain C++14, no HIP (also bin/sa_chain_plan_check).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "sa_hip.h"

namespace sa {

constexpr int32_t kChainMaxMatch = 1024, kChainMaxCost = 1 << 20, kChainMaxLookback = 1024;
constexpr int64_t kChainScoreLimit = 1ll << 30;       // f < 2^30: match sum(L) of a pair stays below it
constexpr uint64_t kChainCoordLimit = 2147483647ull;  // x + L and y + L stay below 2^31 - 1

// A validated call. Anchor a of the flat array is (ex[a], ey[a], len[a]); pair k owns off[k] .. off[k + 1).
struct ChainPlan {
    sa_chain_params cp;
    int64_t num_pairs = 0;
    std::vector<int32_t> ex, ey, len;
    std::vector<uint64_t> off;    // num_pairs + 1 entries
    std::vector<uint32_t> order;  // the pairs, most anchors first (ties: lower index first): the device's draw order
    uint64_t max_anchors = 0;     // of one pair
};

// What the recurrence leaves per anchor (pred -1: the chain starts here; cut = o of the transition taken) and per pair
struct ChainHead {
    int32_t score;
    uint32_t last, num_seeds, pad;
};

// Every refusal of sa_hip.h, in its order; `fn` starts the message. Returns SA_OK or the status with *err set.
int chain_plan(const char *fn, const sa_chain_params *cp, const sa_seed *anchors, const uint64_t *anchor_off, int64_t num_pairs,
               ChainPlan *out, std::string *err);

// The recurrence of one pair (anchors first .. first + count of the plan): pred and cut get `count` entries.
ChainHead chain_host_pair(const ChainPlan &plan, uint64_t first, uint64_t count, int32_t *pred, int32_t *cut);

// The walk of one pair: head.num_seeds seeds in forward order into `seeds`.
void chain_walk_pair(const ChainPlan &plan, uint64_t first, uint64_t count, const ChainHead &head, const int32_t *pred,
                     const int32_t *cut, sa_seed *seeds);

// The whole call on the host: results (num_pairs entries), the seeds and their num_pairs + 1 offsets.
void chain_host(const ChainPlan &plan, sa_chain_result *results, std::vector<sa_seed> *seeds, std::vector<uint64_t> *seeds_off);

}  // namespace sa
