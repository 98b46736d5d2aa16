// The planner of the affine alignment path (sa_trace_plan.h): validation through the score planner,
// direction bytes and string slots per pair, and the chunks of the work order. Host only, no HIP.
#include "sa_trace_plan.h"

#include <algorithm>
#include <cstdlib>
#include <initializer_list>

namespace sa {

uint64_t trace_arena_budget()
{
    static const uint64_t b = [] {
        const char *e = std::getenv("SA_TRACE_ARENA_BYTES");
        const unsigned long long v = e ? std::strtoull(e, nullptr, 10) : 0;
        return v ? (uint64_t)v : kTraceArenaDefault;
    }();
    return b;
}

// the limits and the work order are the affine scorer's; the traced instances exist at R = 8 only.
// SA_SCORE_WAVES is tuned for the untraced kernels: here it may lower the grid, not raise it past what the
// traced instances' registers admit
static ScoreKnobs traced_knobs(const ScoreKnobs &kn)
{
    ScoreKnobs k8 = kn;
    k8.rows_per_lane = kTraceRows;
    k8.waves_per_simd = kn.waves_per_simd > 0 ? std::min(kn.waves_per_simd, kTraceWavesPerSimd) : kTraceWavesPerSimd;
    return k8;
}

int make_trace_plan(const sa_params *P, const WaveSpec &spec, const sa_pair *pairs, int64_t np, int num_cu, const ScoreKnobs &kn,
                    uint64_t budget, TracePlan *out, std::string *err)
{
    if (!out)
    {
        *err = "aligner: null argument";
        return SA_ERR_INVALID;
    }
    TracePlan &pl = *out;
    pl = TracePlan();
    WaveSpec traced = spec;
    traced.traced = true;
    if (int rc = make_score_plan(P, traced, pairs, np, num_cu, traced_knobs(kn), &pl.score, err)) return rc;
    pl.budget = budget;
    pl.dir_bytes.resize((size_t)np);
    pl.dir_off.resize((size_t)np);
    pl.slot_off.resize((size_t)np);
    for (int64_t p = 0; p < np; ++p)
    {
        const uint64_t n = pairs[p].text_len, m = pairs[p].pattern_len;
        pl.dir_bytes[p] = spec.ext_band ? trace_band_at_dir_bytes(n, m, band_ext((int64_t)n, (int64_t)m, spec.width))
                          : spec.band_at  ? trace_band_at_dir_bytes(n, m, pl.score.bands[p])
                          : spec.banded ? trace_band_dir_bytes(n, m, spec.band)
                                        : trace_dir_bytes(n, m);
        pl.total_dir_bytes += pl.dir_bytes[p];
        pl.slot_off[p] = pl.string_bytes;
        pl.string_bytes += n + m;
        if (pl.dir_bytes[p] > budget)
        {
            *err = "pair " + std::to_string(p) + " needs " + std::to_string(pl.dir_bytes[p]) +
                   " direction bytes, the arena budget is " + std::to_string(budget) + " (SA_TRACE_ARENA_BYTES)";
            return SA_ERR_UNSUPPORTED;
        }
    }
    // consecutive chunks of the work order, each as long as its directions fit the budget
    pl.chunk_begin.push_back(0);
    uint64_t used = 0;
    for (int64_t w = 0; w < np; ++w)
    {
        const int32_t p = pl.score.order[w];
        if (used + pl.dir_bytes[p] > budget)
        {
            pl.chunk_begin.push_back(w);
            used = 0;
        }
        pl.dir_off[p] = used;
        used += pl.dir_bytes[p];
        pl.arena_bytes = std::max(pl.arena_bytes, used);
    }
    if (np > 0) pl.chunk_begin.push_back(np);
    return SA_OK;
}

int make_seeds_trace_plan(const sa_params *P, const WaveSpec &spec, const sa_pair *pairs, const sa_seed *seeds, int64_t np, int num_cu,
                          const ScoreKnobs &kn, uint64_t budget, SeedTracePlan *out, std::string *err)
{
    if (!out)
    {
        *err = "aligner: null argument";
        return SA_ERR_INVALID;
    }
    SeedTracePlan &pl = *out;
    pl = SeedTracePlan();
    WaveSpec traced = spec;
    traced.traced = true;
    if (int rc = make_seeds_score_plan(P, traced, pairs, seeds, np, num_cu, traced_knobs(kn), &pl.score, &pl.seeds, err)) return rc;
    pl.budget = budget;
    pl.num_pairs = np;
    const std::vector<SeedItem> &items = pl.seeds.items;
    const int64_t ni = (int64_t)items.size();
    pl.dir_bytes.resize((size_t)ni);
    pl.dir_off.resize((size_t)ni);
    // a half's cells: under a width, those of its own band (band_ext of the half's shape)
    std::vector<uint64_t> icells((size_t)ni);
    for (int64_t k = 0; k < ni; ++k)
    {
        const uint64_t n = items[k].n, m = items[k].m;
        const Band bd = band_ext((int64_t)n, (int64_t)m, spec.width);
        pl.dir_bytes[k] = spec.ext_band ? trace_band_at_dir_bytes(n, m, bd) : trace_dir_bytes(n, m);
        icells[k] = spec.ext_band ? band_cells(n, m, bd) : n * m;
        pl.total_dir_bytes += pl.dir_bytes[k];
    }
    // per pair: the directions and the cells of both halves, and the string slot
    pl.slot_off.resize((size_t)np);
    std::vector<uint64_t> pbytes((size_t)np, 0), pcells((size_t)np, 0);
    for (int64_t p = 0; p < np; ++p)
    {
        const SeedPair &sp = pl.seeds.pairs[p];
        for (int32_t k : {sp.left, sp.right})
            if (k >= 0)
            {
                pbytes[p] += pl.dir_bytes[k];
                pcells[p] += icells[k];
            }
        pl.slot_off[p] = pl.string_bytes;
        pl.string_bytes += pairs[p].text_len + pairs[p].pattern_len;
        if (pbytes[p] > budget)
        {
            *err = "pair " + std::to_string(p) + " needs " + std::to_string(pbytes[p]) +
                   " direction bytes for its two halves, the arena budget is " + std::to_string(budget) + " (SA_TRACE_ARENA_BYTES)";
            return SA_ERR_UNSUPPORTED;
        }
    }
    pl.pair_order.resize((size_t)np);
    for (int64_t p = 0; p < np; ++p) pl.pair_order[p] = (int32_t)p;
    std::stable_sort(pl.pair_order.begin(), pl.pair_order.end(), [&](int32_t a, int32_t b) { return pcells[a] > pcells[b]; });
    // consecutive chunks of the pair order, each as long as its directions fit the budget; a chunk's items
    // in the order of their cells
    std::vector<int32_t> &order = pl.score.order;
    order.clear();
    auto by_cells = [&](int32_t a, int32_t b) { return icells[a] > icells[b]; };
    auto close_chunk = [&]() { std::stable_sort(order.begin() + pl.chunk_begin.back(), order.end(), by_cells); };
    pl.chunk_begin.push_back(0);
    pl.pair_chunk_begin.push_back(0);
    uint64_t used = 0;
    for (int64_t w = 0; w < np; ++w)
    {
        const int32_t p = pl.pair_order[w];
        if (used + pbytes[p] > budget)
        {
            close_chunk();
            pl.chunk_begin.push_back((int64_t)order.size());
            pl.pair_chunk_begin.push_back(w);
            used = 0;
        }
        const SeedPair &sp = pl.seeds.pairs[p];
        for (int32_t k : {sp.left, sp.right})
            if (k >= 0)
            {
                pl.dir_off[k] = used;
                used += pl.dir_bytes[k];
                order.push_back(k);
            }
        pl.arena_bytes = std::max(pl.arena_bytes, used);
    }
    close_chunk();
    if (np > 0)
    {
        pl.chunk_begin.push_back((int64_t)order.size());
        pl.pair_chunk_begin.push_back(np);
    }
    return SA_OK;
}

}  // namespace sa
