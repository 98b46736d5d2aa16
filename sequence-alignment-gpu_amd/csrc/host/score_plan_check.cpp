// bin/sa_score_plan_check: the score-only planner (sa_score_plan.cpp) as a stand-alone program. No
// GPU, no ROCm: it plans the pair shapes on its command line for a device of a given CU count, under
// the knobs of its environment, and prints the plan as one JSON object (tests/test_score_plan.py).
//   sa_score_plan_check --mode global|local|fit|<int> --alphabet A --gap G --cus N [--rows-per-lane R]
//                       [--gap-extend E] [--band W | --band-at LO:HI] [--extend X|none [--width W]] [--match M --mismatch X] NxM[xCOUNT] ...
// With --gap-extend the plan is the affine scorer's and --gap is the gap-open penalty. With --band W
// it is the banded scorer's (sa_hip.h), and the plan also prints band_cells and, for the first 8
// pairs, "bands": lo, hi, the pair's band cells and the [jmin, jmax, b0, b1] window of every strip at
// the plan's R. With --band-at LO:HI it is the band-at scorer's, the one band applied to every pair, with
// the same output ("band" is -1, lo and hi are the clipped limits, an empty strip's window is
// [1, 0, 0, 0]).
// With --extend X it is the extension scorer's (sa_score_batch_extend; "none" is SA_NO_XDROP), which takes
// --gap-extend and prints "extend": true and "xdrop".
// With --seeds TS:PS:L (once for all pairs, or once per shape argument, in their order) it is the seeds
// scorer's (sa_score_batch_seeds) under the xdrop of --extend (none without it): "items" lists the work
// items, "halves" every pair's [left, right] item (-1: empty), and "order", "num_pairs", "grid", "R" and the
// bytes are those of the items. With a band of either kind the call is refused as --extend with a band is.
// With --width W (beside --extend, with or without --seeds) it is the banded extension scorer's or the banded
// seeds scorer's (sa_score_batch_extend_band, sa_score_batch_seeds_band): the plan prints "width", "band_cells"
// and "bands" as --band-at does, for the first 8 pairs or, with --seeds, work items, each on the band of the
// width for its own shape. --band or --band-at beside --extend stays refused, with or without --width.
// With --chain TS:PS:L,TS:PS:L,... (once for all pairs, or once per shape argument; csrc/host/chain_args.h) it is the
// chains scorer's (sa_score_batch_chains) under the xdrop of --extend: the program prints the two launches' plans as
// "ends_plan" and "gaps_plan" (R, grid, num_items, the gap model, row_stride, cost, order), the work items as "ends"
// and "gaps" as --seeds prints its items, every pair's record under "chains", and the bytes. A band of either kind
// or a width beside it is refused. --chain-off is for the refusals.
// NxM is text length x pattern length; the matrix is M on the diagonal and X elsewhere (5 / -4).
// A planning error prints {"error": code, "message": text}.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "chain_args.h"
#include "sa_score_plan.h"

using namespace sa;

int main(int argc, char **argv)
{
    sa_params P;
    std::memset(&P, 0, sizeof(P));
    P.alphabet_size = 4;
    P.gap_penalty = 5;
    int cus = 256, match = 5, mismatch = -4;
    bool affine = false, banded = false, band_at = false;
    int32_t band = 0;
    sa_band at = {0, 0};
    bool extend = false;
    int32_t xdrop = SA_NO_XDROP;
    bool has_width = false;
    int32_t width = 0;
    int32_t gap_extend = 0;
    std::vector<sa_pair> pairs;
    std::vector<sa_seed> shape_seeds;  // --seeds: one per shape argument, or one for all
    std::vector<size_t> shape_of;      // the shape argument of each pair
    ChainArgs chain;                   // --chain, --chain-off
    size_t num_shapes = 0;
    for (int i = 1; i < argc; ++i)
    {
        const std::string a = argv[i];
        auto value = [&]() -> const char * { return i + 1 < argc ? argv[++i] : ""; };
        if (a == "--mode")
        {
            const std::string v = value();
            P.mode = v == "global" ? SA_GLOBAL : v == "local" ? SA_LOCAL : v == "fit" ? SA_FIT : std::atoi(v.c_str());
        }
        else if (a == "--alphabet") P.alphabet_size = std::atoi(value());
        else if (a == "--gap") P.gap_penalty = std::atoi(value());
        else if (a == "--gap-extend")
        {
            affine = true;
            gap_extend = std::atoi(value());
        }
        else if (a == "--band")
        {
            banded = true;
            band = std::atoi(value());
        }
        else if (a == "--band-at")
        {
            band_at = true;
            int lo = 0, hi = 0;
            if (std::sscanf(value(), "%d:%d", &lo, &hi) != 2)
            {
                std::fprintf(stderr, "sa_score_plan_check: --band-at takes LO:HI\n");
                return 2;
            }
            at.lo = lo;
            at.hi = hi;
        }
        else if (a == "--extend")
        {
            extend = true;
            const std::string v = value();
            xdrop = v == "none" ? SA_NO_XDROP : std::atoi(v.c_str());
        }
        else if (a == "--width")
        {
            has_width = true;
            width = std::atoi(value());
        }
        else if (a == "--seeds")
        {
            unsigned long long ts = 0, ps = 0, len = 0;
            if (std::sscanf(value(), "%llu:%llu:%llu", &ts, &ps, &len) != 3)
            {
                std::fprintf(stderr, "sa_score_plan_check: --seeds takes TS:PS:L\n");
                return 2;
            }
            shape_seeds.push_back(sa_seed{ts, ps, len});
        }
        else if (a == "--chain")
        {
            if (!chain.parse_chain(value()))
            {
                std::fprintf(stderr, "sa_score_plan_check: --chain takes TS:PS:L,TS:PS:L,...\n");
                return 2;
            }
        }
        else if (a == "--chain-off") chain.parse_off(value());
        else if (a == "--cus") cus = std::atoi(value());
        else if (a == "--rows-per-lane") P.rows_per_lane = std::atoi(value());
        else if (a == "--match") match = std::atoi(value());
        else if (a == "--mismatch") mismatch = std::atoi(value());
        else
        {
            unsigned long long n = 0, m = 0, count = 1;
            if (std::sscanf(a.c_str(), "%llux%llux%llu", &n, &m, &count) < 2)
            {
                std::fprintf(stderr, "sa_score_plan_check: bad argument %s\n", a.c_str());
                return 2;
            }
            for (unsigned long long k = 0; k < count; ++k)
            {
                sa_pair pr;
                pr.text_offset = pairs.empty() ? 0 : pairs.back().text_offset + pairs.back().text_len;
                pr.text_len = n;
                pr.pattern_offset = pairs.empty() ? 0 : pairs.back().pattern_offset + pairs.back().pattern_len;
                pr.pattern_len = m;
                pairs.push_back(pr);
                shape_of.push_back(num_shapes);
            }
            ++num_shapes;
        }
    }
    const int a = std::min(std::max(P.alphabet_size, 1), 64);
    std::vector<int32_t> S((size_t)a * a, mismatch);
    for (int c = 0; c < a; ++c) S[(size_t)c * a + c] = match;
    P.score_matrix = S.data();

    ScorePlan pl;
    std::string err;
    const std::vector<sa_band> bands(std::max<size_t>(pairs.size(), 1), at);
    // --seeds: the seeds scorer; with a band of either kind the call is the extension scorer's, refused as it is
    const bool seeded = !shape_seeds.empty() && !banded && !band_at;
    if (seeded && shape_seeds.size() != 1 && shape_seeds.size() != num_shapes)
    {
        std::fprintf(stderr, "sa_score_plan_check: --seeds once, or once per shape\n");
        return 2;
    }
    std::vector<sa_seed> seeds;
    for (size_t i = 0; seeded && i < pairs.size(); ++i) seeds.push_back(shape_seeds[shape_seeds.size() == 1 ? 0 : shape_of[i]]);
    SeedItems si;
    WaveSpec spec = affine ? WaveSpec::gaps(P.gap_penalty, gap_extend) : WaveSpec();
    if (banded) spec = spec.in_band(band);
    if (band_at) spec = spec.in_bands(bands.data());
    if (extend || !shape_seeds.empty()) spec = spec.extending(xdrop);
    if (has_width) spec = spec.within(width);
    if (chain.given())
    {
        if (!chain.resolve(shape_of, num_shapes))
        {
            std::fprintf(stderr, "sa_score_plan_check: --chain once, or once per shape\n");
            return 2;
        }
        ChainsScorePlan cp;
        const int rc = make_chains_score_plan(&P, spec.extending(xdrop).from_chains(chain.seeds_ptr(), chain.off_ptr()), pairs.data(),
                                              (int64_t)pairs.size(), cus, score_knobs(), &cp, &err);
        if (rc != SA_OK)
        {
            std::printf("{\"error\": %d, \"message\": \"%s\"}\n", rc, err.c_str());
            return 0;
        }
        std::printf("{\"chains_call\": true, \"xdrop\": %d, \"input_bytes\": %llu, \"device_bytes\": %llu", cp.ends.spec.xdrop,
                    (unsigned long long)cp.ends.input_bytes, (unsigned long long)cp.device_bytes);
        for (const ScorePlan *l : {&cp.ends, &cp.gaps})
        {
            std::printf(", \"%s_plan\": {\"R\": %d, \"grid\": %d, \"num_items\": %lld, \"affine\": %s, \"gap\": %d, \"gap_extend\": %d, \"extend\": %s, "
                        "\"max_text\": %llu, \"row_stride\": %llu, \"cost\": [%llu, %llu, %llu, %llu]",
                        l == &cp.ends ? "ends" : "gaps", l->R, l->grid, (long long)l->num_pairs, l->spec.affine ? "true" : "false", l->gap,
                        l->spec.gap_extend, l->spec.extend ? "true" : "false", (unsigned long long)l->max_text, (unsigned long long)l->row_stride,
                        (unsigned long long)l->cost[0], (unsigned long long)l->cost[1], (unsigned long long)l->cost[2], (unsigned long long)l->cost[3]);
            print_order("order", l->order);
            std::printf("}");
        }
        print_chain_items(cp.items);
        std::printf("}\n");
        return 0;
    }
    const int rc = seeded ? make_seeds_score_plan(&P, spec, pairs.data(), seeds.data(), (int64_t)pairs.size(), cus, score_knobs(), &pl, &si, &err)
                          : make_score_plan(&P, spec, pairs.data(), (int64_t)pairs.size(), cus, score_knobs(), &pl, &err);
    if (rc != SA_OK)
    {
        std::printf("{\"error\": %d, \"message\": \"%s\"}\n", rc, err.c_str());
        return 0;
    }
    std::printf("{\"mode\": %d, \"A\": %d, \"gap\": %d, \"R\": %d, \"key_rowbits\": %d, \"num_cu\": %d, \"waves_per_simd\": %d, "
                "\"grid\": %d, \"num_pairs\": %lld, \"max_text\": %llu, \"row_stride\": %llu, \"input_bytes\": %llu, "
                "\"device_bytes\": %llu, \"padded_cells\": %llu, \"cost\": [%llu, %llu, %llu, %llu], \"affine\": %s, \"gap_extend\": %d, \"order\": [",
                pl.mode, pl.A, pl.gap, pl.R, pl.key_rowbits, pl.num_cu, pl.waves_per_simd, pl.grid, (long long)pl.num_pairs,
                (unsigned long long)pl.max_text, (unsigned long long)pl.row_stride, (unsigned long long)pl.input_bytes,
                (unsigned long long)pl.device_bytes, (unsigned long long)pl.padded_cells, (unsigned long long)pl.cost[0],
                (unsigned long long)pl.cost[1], (unsigned long long)pl.cost[2], (unsigned long long)pl.cost[3],
                pl.spec.affine ? "true" : "false", pl.spec.gap_extend);
    // the order of a large batch is long: the first 64 entries
    for (size_t i = 0; i < pl.order.size() && i < 64; ++i) std::printf("%s%d", i ? ", " : "", pl.order[i]);
    std::printf("]");
    if (extend || seeded) std::printf(", \"extend\": true, \"xdrop\": %d", pl.spec.xdrop);
    if (seeded)
    {
        // the work items (the first 128): "order" above lists item indices, "num_pairs" counts items
        std::printf(", \"seeds\": true, \"num_seed_pairs\": %zu, \"items\": [", pairs.size());
        for (size_t k = 0; k < si.items.size() && k < 128; ++k)
        {
            const SeedItem &it = si.items[k];
            std::printf("%s{\"pair\": %d, \"dir\": %d, \"text_off\": %llu, \"pattern_off\": %llu, \"n\": %u, \"m\": %u}", k ? ", " : "",
                        it.pair, it.dir, (unsigned long long)it.text_off, (unsigned long long)it.pattern_off, it.n, it.m);
        }
        std::printf("], \"halves\": [");
        for (size_t p = 0; p < si.pairs.size() && p < 64; ++p) std::printf("%s[%d, %d]", p ? ", " : "", si.pairs[p].left, si.pairs[p].right);
        std::printf("]");
    }
    if (has_width && !banded && !band_at)
    {
        std::printf(", \"width\": %d, \"band_cells\": %llu, \"bands\": [", pl.spec.width, (unsigned long long)pl.band_cells);
        const size_t count = seeded ? si.items.size() : pairs.size();
        for (size_t i = 0; i < count && i < 8; ++i)
        {
            const int64_t n = seeded ? (int64_t)si.items[i].n : (int64_t)pairs[i].text_len;
            const int64_t m = seeded ? (int64_t)si.items[i].m : (int64_t)pairs[i].pattern_len, rows = 64 * pl.R;
            const Band bd = band_ext(n, m, width);
            std::printf("%s{\"lo\": %d, \"hi\": %d, \"cells\": %llu, \"windows\": [", i ? ", " : "", bd.lo, bd.hi,
                        (unsigned long long)band_cells((uint64_t)n, (uint64_t)m, bd));
            for (int64_t s = 0; n && m && s < (m + rows - 1) / rows; ++s)
            {
                const BandWindow bw = band_window_at(n, m, rows, s, bd);
                std::printf("%s[%d, %d, %d, %d]", s ? ", " : "", bw.jmin, bw.jmax, bw.b0, bw.b1);
            }
            std::printf("]}");
        }
        std::printf("]");
    }
    if (banded || band_at)
    {
        std::printf(", \"band\": %d, \"band_cells\": %llu, \"bands\": [", pl.spec.banded ? pl.spec.band : -1, (unsigned long long)pl.band_cells);
        for (size_t i = 0; i < pairs.size() && i < 8; ++i)
        {
            const int64_t n = (int64_t)pairs[i].text_len, m = (int64_t)pairs[i].pattern_len, rows = 64 * pl.R;
            const Band bd = band_at ? pl.bands[i] : band_of(n, m, band);
            std::printf("%s{\"lo\": %d, \"hi\": %d, \"cells\": %llu, \"windows\": [", i ? ", " : "", bd.lo, bd.hi,
                        (unsigned long long)band_cells((uint64_t)n, (uint64_t)m, bd));
            for (int64_t s = 0; n && m && s < (m + rows - 1) / rows; ++s)
            {
                const BandWindow bw = band_window_at(n, m, rows, s, bd);
                std::printf("%s[%d, %d, %d, %d]", s ? ", " : "", bw.jmin, bw.jmax, bw.b0, bw.b1);
            }
            std::printf("]}");
        }
        std::printf("]");
    }
    std::printf("}\n");
    return 0;
}
