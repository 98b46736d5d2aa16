// bin/sa_trace_plan_check: the planner of the affine alignment path (sa_trace_plan.cpp) as a
// stand-alone program. No GPU, no ROCm: it plans the pair shapes on its command line and prints the
// plan as one JSON object (tests/test_trace_plan.py).
//   sa_trace_plan_check --mode global|local|fit|<int> --alphabet A --gap G --gap-extend E --cus N
//                       [--budget BYTES] [--band W | --band-at LO:HI] [--extend X|none [--width W]] [--match M --mismatch X] NxM[xCOUNT] ...
// --gap is the gap-open penalty. With --band W the plan is the banded aligner's (sa_hip.h): dir_bytes
// are the band's, "steps" is the sum of the strips' window steps, and each pair also lists the
// [b0, b1] bodies of its strips' windows (the first 64 strips). With --band-at LO:HI it is the band-at
// aligner's, the one band applied to every pair, with the same output (an empty strip's window is [0, 0]). Without --budget the budget is SA_TRACE_ARENA_BYTES or the default.
// With --extend X it is the extension aligner's (sa_align_pairs_extend; "none" is SA_NO_XDROP).
// With --seeds TS:PS:L (once for all pairs, or once per shape argument, in their order) it is the seeds
// aligner's (sa_align_pairs_seeds) under the xdrop of --extend: "items" lists the work items with their
// direction bytes and offsets, "order" the items chunk by chunk ("chunk_begin"), "pair_order" and
// "pair_chunk_begin" the pairs of each chunk's walk. With a band of either kind the call is refused as
// --extend with a band is.
// With --width W (beside --extend, with or without --seeds) it is the banded extension aligner's or the banded
// seeds aligner's (sa_align_pairs_extend_band, sa_align_pairs_seeds_band): "width" is printed, every pair's or
// item's dir_bytes are those of the width's band for its shape, and a pair also lists its strips' windows as
// --band-at does. --band or --band-at beside --extend stays refused, with or without --width.
// With --chain TS:PS:L,TS:PS:L,... (once for all pairs, or once per shape argument; csrc/host/chain_args.h) it is the
// chains aligner's (sa_align_pairs_chains): "ends" and "gaps" list the work items of the two traced fills with their
// direction bytes and offsets, "order" and "gap_order" the items chunk by chunk ("chunk_begin", "gap_chunk_begin"),
// "pair_order" and "pair_chunk_begin" the pairs of each chunk, "chains" every pair's record and "slots" its slot.
// NxM is text length x pattern length; the matrix is M on the diagonal and X elsewhere (5 / -4).
// A planning error prints {"error": code, "message": text}.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "chain_args.h"
#include "sa_trace_plan.h"

using namespace sa;

int main(int argc, char **argv)
{
    sa_params P;
    std::memset(&P, 0, sizeof(P));
    P.alphabet_size = 4;
    int cus = 256, match = 5, mismatch = -4, go = 11, ge = 2;
    uint64_t budget = trace_arena_budget();
    bool banded = false, band_at = false;
    int32_t band = 0;
    sa_band at = {0, 0};
    bool extend = false;
    int32_t xdrop = SA_NO_XDROP;
    bool has_width = false;
    int32_t width = 0;
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
        else if (a == "--gap") go = std::atoi(value());
        else if (a == "--gap-extend") ge = std::atoi(value());
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
                std::fprintf(stderr, "sa_trace_plan_check: --seeds takes TS:PS:L\n");
                return 2;
            }
            shape_seeds.push_back(sa_seed{ts, ps, len});
        }
        else if (a == "--chain")
        {
            if (!chain.parse_chain(value()))
            {
                std::fprintf(stderr, "sa_trace_plan_check: --chain takes TS:PS:L,TS:PS:L,...\n");
                return 2;
            }
        }
        else if (a == "--chain-off") chain.parse_off(value());
        else if (a == "--cus") cus = std::atoi(value());
        else if (a == "--budget") budget = std::strtoull(value(), nullptr, 10);
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
                std::fprintf(stderr, "sa_trace_plan_check: --band-at takes LO:HI\n");
                return 2;
            }
            at.lo = lo;
            at.hi = hi;
        }
        else if (a == "--match") match = std::atoi(value());
        else if (a == "--mismatch") mismatch = std::atoi(value());
        else
        {
            unsigned long long n = 0, m = 0, count = 1;
            if (std::sscanf(a.c_str(), "%llux%llux%llu", &n, &m, &count) < 2)
            {
                std::fprintf(stderr, "sa_trace_plan_check: bad argument %s\n", a.c_str());
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

    std::string err;
    if (chain.given())
    {
        if (!chain.resolve(shape_of, num_shapes))
        {
            std::fprintf(stderr, "sa_trace_plan_check: --chain once, or once per shape\n");
            return 2;
        }
        ChainTracePlan cp;
        WaveSpec cspec = WaveSpec::gaps(go, ge);
        const std::vector<sa_band> cbands(std::max<size_t>(pairs.size(), 1), at);
        if (banded) cspec = cspec.in_band(band);
        if (band_at) cspec = cspec.in_bands(cbands.data());
        cspec = cspec.extending(xdrop);
        if (has_width) cspec = cspec.within(width);
        const int rc = make_chains_trace_plan(&P, cspec.from_chains(chain.seeds_ptr(), chain.off_ptr()), pairs.data(), (int64_t)pairs.size(), cus,
                                              score_knobs(), budget, &cp, &err);
        if (rc != SA_OK)
        {
            std::printf("{\"error\": %d, \"message\": \"%s\"}\n", rc, err.c_str());
            return 0;
        }
        std::printf("{\"chains_call\": true, \"xdrop\": %d, \"R\": %d, \"gap_R\": %d, \"grid\": %d, \"gap_grid\": %d, \"affine\": %s, \"gap_affine\": %s, "
                    "\"num_pairs\": %lld, \"budget\": %llu, \"arena_bytes\": %llu, \"total_dir_bytes\": %llu, \"string_bytes\": %llu, \"num_chunks\": %lld",
                    cp.score.spec.xdrop, cp.score.R, cp.gaps.R, cp.score.grid, cp.gaps.grid, cp.score.spec.affine ? "true" : "false",
                    cp.gaps.spec.affine ? "true" : "false", (long long)cp.num_pairs, (unsigned long long)cp.budget, (unsigned long long)cp.arena_bytes,
                    (unsigned long long)cp.total_dir_bytes, (unsigned long long)cp.string_bytes, (long long)cp.num_chunks());
        auto list = [](const char *name, const std::vector<int64_t> &v) {
            std::printf(", \"%s\": [", name);
            for (size_t i = 0; i < v.size(); ++i) std::printf("%s%lld", i ? ", " : "", (long long)v[i]);
            std::printf("]");
        };
        list("chunk_begin", cp.chunk_begin);
        list("gap_chunk_begin", cp.gap_chunk_begin);
        list("pair_chunk_begin", cp.pair_chunk_begin);
        print_order("order", cp.score.order);
        print_order("gap_order", cp.gaps.order);
        print_order("pair_order", cp.pair_order);
        print_chain_items(cp.items, &cp.dir_bytes, &cp.dir_off, &cp.gap_dir_bytes, &cp.gap_dir_off);
        std::printf(", \"slots\": [");
        for (size_t p = 0; p < cp.slot_off.size() && p < 64; ++p) std::printf("%s%llu", p ? ", " : "", (unsigned long long)cp.slot_off[p]);
        std::printf("]}\n");
        return 0;
    }
    // --seeds: the seeds aligner; with a band of either kind the call is the extension aligner's, refused as it is
    if (!shape_seeds.empty() && !banded && !band_at)
    {
        if (shape_seeds.size() != 1 && shape_seeds.size() != num_shapes)
        {
            std::fprintf(stderr, "sa_trace_plan_check: --seeds once, or once per shape\n");
            return 2;
        }
        std::vector<sa_seed> seeds;
        for (size_t i = 0; i < pairs.size(); ++i) seeds.push_back(shape_seeds[shape_seeds.size() == 1 ? 0 : shape_of[i]]);
        SeedTracePlan sp;
        WaveSpec sspec = WaveSpec::gaps(go, ge).extending(xdrop);
        if (has_width) sspec = sspec.within(width);
        const int rc = make_seeds_trace_plan(&P, sspec, pairs.data(), seeds.data(), (int64_t)pairs.size(), cus,
                                             score_knobs(), budget, &sp, &err);
        if (rc != SA_OK)
        {
            std::printf("{\"error\": %d, \"message\": \"%s\"}\n", rc, err.c_str());
            return 0;
        }
        std::printf("{\"mode\": %d, \"A\": %d, \"gap\": %d, \"gap_extend\": %d, \"R\": %d, \"grid\": %d, \"num_pairs\": %lld, \"num_items\": %zu, "
                    "\"budget\": %llu, \"arena_bytes\": %llu, \"total_dir_bytes\": %llu, \"string_bytes\": %llu, \"num_chunks\": %lld, "
                    "\"seeds\": true, \"xdrop\": %d, \"width\": %d, \"chunk_begin\": [",
                    sp.score.mode, sp.score.A, sp.score.gap, sp.score.spec.gap_extend, sp.score.R, sp.score.grid, (long long)sp.num_pairs,
                    sp.seeds.items.size(), (unsigned long long)sp.budget, (unsigned long long)sp.arena_bytes,
                    (unsigned long long)sp.total_dir_bytes, (unsigned long long)sp.string_bytes, (long long)sp.num_chunks(), sp.score.spec.xdrop,
                    has_width ? sp.score.spec.width : -1);
        for (size_t i = 0; i < sp.chunk_begin.size(); ++i) std::printf("%s%lld", i ? ", " : "", (long long)sp.chunk_begin[i]);
        std::printf("], \"pair_chunk_begin\": [");
        for (size_t i = 0; i < sp.pair_chunk_begin.size(); ++i) std::printf("%s%lld", i ? ", " : "", (long long)sp.pair_chunk_begin[i]);
        std::printf("], \"order\": [");
        for (size_t i = 0; i < sp.score.order.size() && i < 128; ++i) std::printf("%s%d", i ? ", " : "", sp.score.order[i]);
        std::printf("], \"pair_order\": [");
        for (size_t i = 0; i < sp.pair_order.size() && i < 64; ++i) std::printf("%s%d", i ? ", " : "", sp.pair_order[i]);
        std::printf("], \"items\": [");
        for (size_t k = 0; k < sp.seeds.items.size() && k < 128; ++k)
        {
            const SeedItem &it = sp.seeds.items[k];
            std::printf("%s{\"pair\": %d, \"dir\": %d, \"text_off\": %llu, \"pattern_off\": %llu, \"n\": %u, \"m\": %u, \"dir_bytes\": %llu, "
                        "\"dir_off\": %llu}",
                        k ? ", " : "", it.pair, it.dir, (unsigned long long)it.text_off, (unsigned long long)it.pattern_off, it.n, it.m,
                        (unsigned long long)sp.dir_bytes[k], (unsigned long long)sp.dir_off[k]);
        }
        std::printf("], \"pairs\": [");
        for (size_t p = 0; p < pairs.size() && p < 64; ++p)
            std::printf("%s{\"left\": %d, \"right\": %d, \"slot_off\": %llu}", p ? ", " : "", sp.seeds.pairs[p].left, sp.seeds.pairs[p].right,
                        (unsigned long long)sp.slot_off[p]);
        std::printf("]}\n");
        return 0;
    }
    if (!shape_seeds.empty()) extend = true;
    TracePlan pl;
    const std::vector<sa_band> bands(std::max<size_t>(pairs.size(), 1), at);
    WaveSpec spec = WaveSpec::gaps(go, ge);
    if (banded) spec = spec.in_band(band);
    if (band_at) spec = spec.in_bands(bands.data());
    if (extend) spec = spec.extending(xdrop);
    if (has_width) spec = spec.within(width);
    const bool windows = banded || band_at || has_width;
    const int rc = make_trace_plan(&P, spec, pairs.data(), (int64_t)pairs.size(), cus, score_knobs(), budget, &pl, &err);
    if (rc != SA_OK)
    {
        std::printf("{\"error\": %d, \"message\": \"%s\"}\n", rc, err.c_str());
        return 0;
    }
    std::printf("{\"mode\": %d, \"A\": %d, \"gap\": %d, \"gap_extend\": %d, \"R\": %d, \"grid\": %d, \"num_pairs\": %lld, "
                "\"budget\": %llu, \"arena_bytes\": %llu, \"total_dir_bytes\": %llu, \"string_bytes\": %llu, "
                "\"num_chunks\": %lld, \"width\": %d, \"chunk_begin\": [",
                pl.score.mode, pl.score.A, pl.score.gap, pl.score.spec.gap_extend, pl.score.R, pl.score.grid,
                (long long)pl.score.num_pairs, (unsigned long long)pl.budget, (unsigned long long)pl.arena_bytes,
                (unsigned long long)pl.total_dir_bytes, (unsigned long long)pl.string_bytes, (long long)pl.num_chunks(),
                has_width ? pl.score.spec.width : -1);
    for (size_t i = 0; i < pl.chunk_begin.size(); ++i) std::printf("%s%lld", i ? ", " : "", (long long)pl.chunk_begin[i]);
    // the lists of a large batch are long: the first 64 entries
    std::printf("], \"order\": [");
    for (size_t i = 0; i < pl.score.order.size() && i < 64; ++i) std::printf("%s%d", i ? ", " : "", pl.score.order[i]);
    std::printf("], \"pairs\": [");
    for (size_t i = 0; i < pairs.size() && i < 64; ++i)
    {
        const uint64_t strips = pl.dir_bytes[i] ? trace_strips(pairs[i].pattern_len) : 0;
        std::printf("%s{\"strips\": %llu, \"steps\": %llu, \"dir_bytes\": %llu, \"dir_off\": %llu, \"slot_off\": %llu", i ? ", " : "",
                    (unsigned long long)strips,
                    (unsigned long long)(windows ? pl.dir_bytes[i] / kTraceStepBytes : pl.dir_bytes[i] ? trace_steps(pairs[i].text_len) : 0),
                    (unsigned long long)pl.dir_bytes[i], (unsigned long long)pl.dir_off[i], (unsigned long long)pl.slot_off[i]);
        if (windows)
        {
            const int64_t n = (int64_t)pairs[i].text_len, m = (int64_t)pairs[i].pattern_len;
            const Band bd = has_width ? band_ext(n, m, width) : band_at ? pl.score.bands[i] : band_of(n, m, band);
            std::printf(", \"windows\": [");
            for (uint64_t s = 0; s < strips && s < 64; ++s)
            {
                const BandWindow bw = band_window_at(n, m, (int64_t)kTraceStripRows, (int64_t)s, bd);
                std::printf("%s[%d, %d]", s ? ", " : "", bw.b0, bw.b1);
            }
            std::printf("]");
        }
        std::printf("}");
    }
    std::printf("]}\n");
    return 0;
}
