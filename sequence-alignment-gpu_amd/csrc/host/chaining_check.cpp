// sa_chaining_check — a C++14 caller of the chaining (sa_hip.h sa_chain_anchors): <count> pairs of up to <n> anchors
// each, a noisy path of exact matches (steps along a diagonal, diagonal changes, overlaps with the anchor before,
// duplicates) with off-path hits strewn in, in canonical order, some pairs empty, through
// SequenceAlignment::chainAnchorsGPU under four parameter sets (5 / 11 / 2 with lookback 64, a skip cost with limits,
// zero costs, lookback 1). Identity K2 of sa_hip.h is checked: the score, the last anchor and every seed must be
// those of sa_chain_anchors_host on the same anchors.
//   usage: sa_chaining_check <n> <count> [device]
// Prints the first difference, or "OK <count>" as its last line; exit status 0 iff all equal.
// With --expected: the digest of the anchors and parameters and that of the host function's results (check_ref.h),
// and no device call.
#include <tuple>

#include "check_ref.h"

int main(int argc, char **argv)
{
    const bool expectedOnly = check::takeExpected(argc, argv);
    if (argc < 3)
    {
        std::cout << "usage: sa_chaining_check <n> <count> [device]\n";
        return 2;
    }
    const uint64_t maxAnchors = std::max<uint64_t>(1, std::strtoull(argv[1], nullptr, 10));
    const uint64_t count = std::strtoull(argv[2], nullptr, 10);
    const int device = argc > 3 ? std::atoi(argv[3]) : 0;
    std::vector<uint64_t> num(count), off(count + 1, 0), ts, ps, len;
    std::vector<sa_seed> anchors;
    uint64_t seed = 86420;
    for (uint64_t k = 0; k < count; ++k)
    {
        const uint64_t a = k % 7 == 3 ? 0 : 1 + check::next(seed) % maxAnchors;
        std::vector<sa_seed> one;
        uint64_t x = check::next(seed) % 50, y = check::next(seed) % 50;
        while (one.size() < a)
        {
            const uint64_t L = 1 + check::next(seed) % 24, roll = check::next(seed) % 16;
            if (roll == 0 && !one.empty()) one.push_back(one.back());  // a duplicate
            else if (roll < 3) one.push_back(sa_seed{check::next(seed) % (x + 200), check::next(seed) % (y + 200), L});  // off the path
            else
            {
                one.push_back(sa_seed{x, y, L});
                const uint64_t step = check::next(seed) % 8;
                x += L + step, y += L + step;
                if (roll == 3) x += 1 + check::next(seed) % 30;       // a diagonal change
                else if (roll == 4) y += 1 + check::next(seed) % 30;
                else if (roll == 5) x -= std::min<uint64_t>(L + step, 1 + check::next(seed) % 6), y -= std::min<uint64_t>(L + step, 1 + check::next(seed) % 6);  // an overlap
            }
        }
        std::sort(one.begin(), one.end(), [](const sa_seed &p, const sa_seed &q) {
            return std::make_tuple(p.text_pos + p.length, p.pattern_pos + p.length, p.length) <
                   std::make_tuple(q.text_pos + q.length, q.pattern_pos + q.length, q.length);
        });
        num[k] = a;
        off[k + 1] = off[k] + a;
        for (const sa_seed &s : one) ts.push_back(s.text_pos), ps.push_back(s.pattern_pos), len.push_back(s.length), anchors.push_back(s);
    }
    anchors.push_back(sa_seed{0, 0, 0});  // a call without any anchor still passes an address
    const sa_chain_params sets[4] = {{5, 11, 2, 0, SA_CHAIN_NO_LIMIT, SA_CHAIN_NO_LIMIT, 64},
                                     {3, 4, 1, 1, 40, 12, 200},
                                     {1, 0, 0, 0, SA_CHAIN_NO_LIMIT, SA_CHAIN_NO_LIMIT, 1024},
                                     {7, 2, 2, 0, SA_CHAIN_NO_LIMIT, 25, 1}};

    check::Digest sent, wanted;
    sent.numbers(num), sent.numbers(ts), sent.numbers(ps), sent.numbers(len);
    std::vector<std::vector<sa_chain_result>> want(4, std::vector<sa_chain_result>(count));
    std::vector<std::vector<sa_seed>> wantSeeds(4);
    for (int v = 0; v < 4; ++v)
    {
        const sa_chain_params &cp = sets[v];
        for (int32_t field : {cp.match, cp.gap_open, cp.gap_extend, cp.skip, cp.max_gap, cp.max_diag, cp.lookback}) sent.number(field);
        sa_chain_set *set = nullptr;
        if (sa_chain_anchors_host(&cp, anchors.data(), off.data(), (int64_t)count, want[v].data(), &set) != SA_OK)
        {
            std::cout << "error: " << sa_last_error() << "\n";
            return 1;
        }
        const uint64_t total = sa_chain_set_off(set)[count];
        if (total) wantSeeds[v].assign(sa_chain_set_seeds(set), sa_chain_set_seeds(set) + total);
        sa_chain_set_destroy(set);
        for (const sa_chain_result &r : want[v]) wanted.number(r.score), wanted.number(r.num_seeds), wanted.number(r.last_anchor), wanted.number((int64_t)r.seeds_off);
        for (const sa_seed &s : wantSeeds[v]) wanted.number((int64_t)s.text_pos), wanted.number((int64_t)s.pattern_pos), wanted.number((int64_t)s.length);
    }
    if (expectedOnly) return check::printExpected("sa_chaining_check", argc, argv, sent, &wanted);

    for (int v = 0; v < 4; ++v)
    {
        std::vector<SequenceAlignment::ChainResponse> got(count);
        if (SequenceAlignment::chainAnchorsGPU(got.data(), count, device, sets[v], num.data(), ts.data(), ps.data(), len.data())) return 1;
        for (uint64_t k = 0; k < count; ++k)
        {
            const sa_chain_result &w = want[v][k];
            const SequenceAlignment::ChainResponse &g = got[k];
            const char *field = nullptr;
            if (g.score != w.score) field = "score";
            else if (g.lastAnchor != w.last_anchor) field = "lastAnchor";
            else if (g.seedLength.size() != w.num_seeds || g.seedTextPos.size() != w.num_seeds || g.seedPatternPos.size() != w.num_seeds) field = "the number of seeds";
            for (uint32_t s = 0; !field && s < w.num_seeds; ++s)
            {
                const sa_seed &x = wantSeeds[v][w.seeds_off + s];
                if (g.seedTextPos[s] != x.text_pos || g.seedPatternPos[s] != x.pattern_pos || g.seedLength[s] != x.length) field = "a seed";
            }
            if (field)
            {
                std::cout << "pair " << k << " (" << num[k] << " anchors) under parameter set " << v << ": " << field << " differs: score " << g.score
                          << " and " << g.seedLength.size() << " seeds against " << w.score << " and " << w.num_seeds << " of the host function\n";
                return 1;
            }
        }
    }
    std::cout << "OK " << count << "\n";
    return 0;
}
