// --chain of bin/sa_score_plan_check and bin/sa_trace_plan_check: the chains of a chained-seeds call
// (sa_hip.h sa_score_batch_chains) from the command line, and the planners' work items as JSON.
//   --chain TS:PS:L,TS:PS:L,...   once for all pairs, or once per shape argument, in their order; "" is a chain
//                                 without a seed, "null" passes seeds == NULL
//   --chain-off A,B,...|null      chain_off as given (or NULL) in the place of the one the chains imply: for the
//                                 refusals only
#pragma once
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "sa_score_plan.h"

namespace sa {

struct ChainArgs {
    std::vector<std::vector<sa_seed>> shape_chains;  // one per --chain
    bool seeds_null = false, off_given = false, off_null = false;
    std::vector<uint64_t> off_as_given;
    // what the planner is called with
    std::vector<sa_seed> seeds;
    std::vector<uint64_t> off;
    bool given() const { return !shape_chains.empty() || seeds_null; }
    const sa_seed *seeds_ptr() const { return seeds_null ? nullptr : seeds.data(); }
    const uint64_t *off_ptr() const { return off_null ? nullptr : off.data(); }

    bool parse_chain(const char *v)
    {
        if (std::string(v) == "null")
        {
            seeds_null = true;
            return true;
        }
        std::vector<sa_seed> chain;
        for (const char *s = v; *s;)
        {
            unsigned long long ts = 0, ps = 0, len = 0;
            int used = 0;
            if (std::sscanf(s, "%llu:%llu:%llu%n", &ts, &ps, &len, &used) != 3) return false;
            chain.push_back(sa_seed{ts, ps, len});
            s += used;
            if (*s == ',') ++s;
            else if (*s) return false;
        }
        shape_chains.push_back(chain);
        return true;
    }
    void parse_off(const char *v)
    {
        off_given = true;
        if (std::string(v) == "null")
        {
            off_null = true;
            return;
        }
        for (const char *s = v; *s;)
        {
            char *end = nullptr;
            const unsigned long long o = std::strtoull(s, &end, 10);
            if (end == s) break;
            off_as_given.push_back(o);
            s = *end == ',' ? end + 1 : end;
        }
    }
    // the flat seeds and chain_off of `shape_of.size()` pairs; false: --chain neither once nor once per shape
    bool resolve(const std::vector<size_t> &shape_of, size_t num_shapes)
    {
        if (!seeds_null && shape_chains.size() != 1 && shape_chains.size() != num_shapes) return false;
        off.assign(1, 0);
        for (size_t i = 0; i < shape_of.size(); ++i)
        {
            if (!seeds_null)
            {
                const std::vector<sa_seed> &c = shape_chains[shape_chains.size() == 1 ? 0 : shape_of[i]];
                seeds.insert(seeds.end(), c.begin(), c.end());
            }
            off.push_back(seeds_null ? i + 1 : seeds.size());
        }
        if (off_given && !off_null) off = off_as_given;
        seeds.push_back(sa_seed{0, 0, 0});  // so that an empty list still has an address
        return true;
    }
};

inline void print_items(const char *name, const std::vector<SeedItem> &items, const std::vector<uint64_t> *dir_bytes = nullptr,
                        const std::vector<uint64_t> *dir_off = nullptr)
{
    std::printf(", \"%s\": [", name);
    for (size_t k = 0; k < items.size() && k < 512; ++k)
    {
        const SeedItem &it = items[k];
        std::printf("%s{\"pair\": %d, \"dir\": %d, \"text_off\": %llu, \"pattern_off\": %llu, \"n\": %u, \"m\": %u", k ? ", " : "", it.pair, it.dir,
                    (unsigned long long)it.text_off, (unsigned long long)it.pattern_off, it.n, it.m);
        if (dir_bytes) std::printf(", \"dir_bytes\": %llu, \"dir_off\": %llu", (unsigned long long)(*dir_bytes)[k], (unsigned long long)(*dir_off)[k]);
        std::printf("}");
    }
    std::printf("]");
}

// "ends", "gaps" (with the directions' bytes and offsets where given) and "chains": every pair's record
inline void print_chain_items(const ChainItems &ci, const std::vector<uint64_t> *ebytes = nullptr, const std::vector<uint64_t> *eoff = nullptr,
                              const std::vector<uint64_t> *gbytes = nullptr, const std::vector<uint64_t> *goff = nullptr)
{
    print_items("ends", ci.ends, ebytes, eoff);
    print_items("gaps", ci.gaps, gbytes, goff);
    std::printf(", \"chains\": [");
    for (size_t p = 0; p < ci.pairs.size() && p < 64; ++p)
    {
        const ChainPair &cp = ci.pairs[p];
        std::printf("%s{\"left\": %d, \"right\": %d, \"seeds\": [%d, %d], \"gap_items\": [%d, %d], \"closed_score\": %d, \"closed_cols\": %u, "
                    "\"begin\": [%llu, %llu], \"end\": [%llu, %llu], \"gap_of_seed\": [",
                    p ? ", " : "", cp.left, cp.right, cp.seed_begin, cp.seed_end, cp.gap_begin, cp.gap_end, cp.closed_score, cp.closed_cols,
                    (unsigned long long)cp.ts, (unsigned long long)cp.ps, (unsigned long long)cp.te, (unsigned long long)cp.pe);
        for (int32_t k = cp.seed_begin; k < cp.seed_end && k < cp.seed_begin + 512; ++k) std::printf("%s%d", k > cp.seed_begin ? ", " : "", ci.seeds[k].gap);
        std::printf("]}");
    }
    std::printf("]");
}

inline void print_order(const char *name, const std::vector<int32_t> &order)
{
    std::printf(", \"%s\": [", name);
    for (size_t i = 0; i < order.size() && i < 512; ++i) std::printf("%s%d", i ? ", " : "", order[i]);
    std::printf("]");
}

}  // namespace sa
