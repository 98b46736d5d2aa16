// The planner of the affine alignment path (sa_trace_plan.h): validation through the score planner,
// direction bytes and string slots per pair, and the chunks of the work order. Host only, no HIP.
#include "sa_trace_plan.h"

#include <algorithm>
#include <cstdlib>
#include <initializer_list>
#include <utility>

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

int make_chains_trace_plan(const sa_params *P, const WaveSpec &spec, const sa_pair *pairs, int64_t np, int num_cu, const ScoreKnobs &kn,
                           uint64_t budget, ChainTracePlan *out, std::string *err)
{
    if (!out)
    {
        *err = "aligner: null argument";
        return SA_ERR_INVALID;
    }
    ChainTracePlan &pl = *out;
    pl = ChainTracePlan();
    WaveSpec traced = spec;
    traced.traced = true;
    ChainsScorePlan sp;
    if (int rc = make_chains_score_plan(P, traced, pairs, np, num_cu, traced_knobs(kn), &sp, err)) return rc;
    pl.score = std::move(sp.ends);
    pl.gaps = std::move(sp.gaps);
    pl.items = std::move(sp.items);
    pl.budget = budget;
    pl.num_pairs = np;
    const std::vector<SeedItem> &ends = pl.items.ends, &gaps = pl.items.gaps;
    auto bytes_of = [&](const std::vector<SeedItem> &items, std::vector<uint64_t> *bytes, std::vector<uint64_t> *off) {
        bytes->resize(items.size());
        off->resize(items.size());
        for (size_t k = 0; k < items.size(); ++k)
        {
            (*bytes)[k] = trace_dir_bytes(items[k].n, items[k].m);
            pl.total_dir_bytes += (*bytes)[k];
        }
    };
    bytes_of(ends, &pl.dir_bytes, &pl.dir_off);
    bytes_of(gaps, &pl.gap_dir_bytes, &pl.gap_dir_off);
    // per pair: the directions and the cells of all its pieces, and the string slot
    pl.slot_off.resize((size_t)np);
    std::vector<uint64_t> pbytes((size_t)np, 0), pcells((size_t)np, 0);
    for (int64_t p = 0; p < np; ++p)
    {
        const ChainPair &cp = pl.items.pairs[p];
        for (int32_t k : {cp.left, cp.right})
            if (k >= 0)
            {
                pbytes[p] += pl.dir_bytes[k];
                pcells[p] += (uint64_t)ends[k].n * ends[k].m;
            }
        for (int32_t k = cp.gap_begin; k < cp.gap_end; ++k)
        {
            pbytes[p] += pl.gap_dir_bytes[k];
            pcells[p] += (uint64_t)gaps[k].n * gaps[k].m;
        }
        pl.slot_off[p] = pl.string_bytes;
        pl.string_bytes += pairs[p].text_len + pairs[p].pattern_len;
        if (pbytes[p] > budget)
        {
            *err = "pair " + std::to_string(p) + " needs " + std::to_string(pbytes[p]) +
                   " direction bytes for the pieces of its chain, the arena budget is " + std::to_string(budget) + " (SA_TRACE_ARENA_BYTES)";
            return SA_ERR_UNSUPPORTED;
        }
    }
    pl.pair_order.resize((size_t)np);
    for (int64_t p = 0; p < np; ++p) pl.pair_order[p] = (int32_t)p;
    std::stable_sort(pl.pair_order.begin(), pl.pair_order.end(), [&](int32_t a, int32_t b) { return pcells[a] > pcells[b]; });
    // consecutive chunks of the pair order, each as long as its directions fit the budget; a chunk's items of either
    // launch in the order of their cells
    std::vector<int32_t> &eorder = pl.score.order, &gorder = pl.gaps.order;
    eorder.clear();
    gorder.clear();
    auto close_chunk = [&]() {
        std::stable_sort(eorder.begin() + pl.chunk_begin.back(), eorder.end(),
                         [&](int32_t a, int32_t b) { return (uint64_t)ends[a].n * ends[a].m > (uint64_t)ends[b].n * ends[b].m; });
        std::stable_sort(gorder.begin() + pl.gap_chunk_begin.back(), gorder.end(),
                         [&](int32_t a, int32_t b) { return (uint64_t)gaps[a].n * gaps[a].m > (uint64_t)gaps[b].n * gaps[b].m; });
    };
    pl.chunk_begin.push_back(0);
    pl.gap_chunk_begin.push_back(0);
    pl.pair_chunk_begin.push_back(0);
    uint64_t used = 0;
    for (int64_t w = 0; w < np; ++w)
    {
        const int32_t p = pl.pair_order[w];
        if (used + pbytes[p] > budget)
        {
            close_chunk();
            pl.chunk_begin.push_back((int64_t)eorder.size());
            pl.gap_chunk_begin.push_back((int64_t)gorder.size());
            pl.pair_chunk_begin.push_back(w);
            used = 0;
        }
        const ChainPair &cp = pl.items.pairs[p];
        for (int32_t k : {cp.left, cp.right})
            if (k >= 0)
            {
                pl.dir_off[k] = used;
                used += pl.dir_bytes[k];
                eorder.push_back(k);
            }
        for (int32_t k = cp.gap_begin; k < cp.gap_end; ++k)
        {
            pl.gap_dir_off[k] = used;
            used += pl.gap_dir_bytes[k];
            gorder.push_back(k);
        }
        pl.arena_bytes = std::max(pl.arena_bytes, used);
    }
    close_chunk();
    if (np > 0)
    {
        pl.chunk_begin.push_back((int64_t)eorder.size());
        pl.gap_chunk_begin.push_back((int64_t)gorder.size());
        pl.pair_chunk_begin.push_back(np);
    }
    return SA_OK;
}

}  // namespace sa
