// bin/sa_chain_plan_check: the chaining planner and host function (csrc/sa_chain_plan.cpp) as a stand-alone program.
// No GPU, no ROCm. On <sets> random anchor sets of up to 9 anchors in a 30 x 30 range, under drawn parameters
// (max_diag = 0 and max_gap = 3 among them), it checks chain_host against a brute force over all index-increasing
// subsequences (K3, lookback >= the count), that every chain is a chain as sa_score_batch_chains defines one and each
// seed the tail of an input anchor (K1), that a valid chain comes back unchanged under zero costs (K4), and that a
// pair's result depends neither on its neighbours in the call nor on a shift of its anchors (K5). It also runs the
// refusals of chain_plan once each.
//   usage: sa_chain_plan_check [sets]      (default 300)
// Prints the sizes of the two structures (tests/test_chaining_plan.py compares its ctypes layouts with them), then
// the first difference, or "OK <sets>" as its last line; exit status 0 iff all hold.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <tuple>
#include <vector>

#include "sa_chain_plan.h"

using namespace sa;

namespace
{
uint64_t next(uint64_t &s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return s >> 33;
}

bool keyLess(const sa_seed &a, const sa_seed &b)
{
    return std::make_tuple(a.text_pos + a.length, a.pattern_pos + a.length, a.length) <
           std::make_tuple(b.text_pos + b.length, b.pattern_pos + b.length, b.length);
}

// value(j -> i) of sa_hip.h; false when the transition is not admissible (the lookback apart)
bool transition(const sa_chain_params &cp, const sa_seed &j, const sa_seed &i, int64_t *value, int64_t *cut)
{
    const int64_t exj = j.text_pos + j.length, eyj = j.pattern_pos + j.length, x = i.text_pos, y = i.pattern_pos, L = i.length;
    const int64_t o = std::max<int64_t>(0, std::max(exj - x, eyj - y));
    if (o >= L) return false;
    const int64_t dx = x + o - exj, dy = y + o - eyj, dd = dx > dy ? dx - dy : dy - dx;
    if (dx > cp.max_gap || dy > cp.max_gap || dd > cp.max_diag) return false;
    *value = cp.match * (L - o) - (dd ? cp.gap_open + (dd - 1) * cp.gap_extend : 0) - (int64_t)cp.skip * std::min(dx, dy);
    *cut = o;
    return true;
}

// the best score over every index-increasing subsequence with admissible consecutive transitions
int64_t bruteForce(const sa_chain_params &cp, const std::vector<sa_seed> &a)
{
    int64_t best = 0;
    const size_t n = a.size();
    for (uint32_t mask = 1; mask < (1u << n); ++mask)
    {
        int64_t score = 0, v, o;
        int last = -1;
        bool ok = true;
        for (size_t i = 0; i < n && ok; ++i)
        {
            if (!(mask >> i & 1)) continue;
            if (last < 0) score = cp.match * (int64_t)a[i].length;
            else if (transition(cp, a[(size_t)last], a[i], &v, &o)) score += v;
            else ok = false;
            last = (int)i;
        }
        if (ok) best = std::max(best, score);
    }
    return best;
}

struct Run {
    std::vector<sa_chain_result> results;
    std::vector<sa_seed> seeds;
    std::vector<uint64_t> off;
};

bool run(const sa_chain_params &cp, const std::vector<sa_seed> &anchors, const std::vector<uint64_t> &off, Run *out)
{
    ChainPlan plan;
    std::string err;
    const int64_t np = (int64_t)off.size() - 1;
    static const sa_seed none = {0, 0, 0};  // a call without any anchor still passes an address
    if (chain_plan("check", &cp, anchors.empty() ? &none : anchors.data(), off.data(), np, &plan, &err) != SA_OK)
    {
        std::printf("chain_plan refused a valid call: %s\n", err.c_str());
        return false;
    }
    out->results.assign((size_t)np, sa_chain_result{});
    chain_host(plan, out->results.data(), &out->seeds, &out->off);
    return true;
}

bool validChain(const std::vector<sa_seed> &anchors, const sa_chain_result &r, const sa_seed *seeds)
{
    for (uint32_t s = 0; s < r.num_seeds; ++s)
    {
        const sa_seed &c = seeds[s];
        if (c.length < 1) return false;
        if (s > 0 && (seeds[s - 1].text_pos + seeds[s - 1].length > c.text_pos || seeds[s - 1].pattern_pos + seeds[s - 1].length > c.pattern_pos))
            return false;
        bool tail = false;
        for (const sa_seed &a : anchors)
            tail = tail || (a.text_pos + a.length == c.text_pos + c.length && a.pattern_pos + a.length == c.pattern_pos + c.length &&
                            c.length <= a.length);
        if (!tail) return false;
    }
    if (r.num_seeds == 0) return anchors.empty();
    const sa_seed &end = anchors[r.last_anchor], &last = seeds[r.num_seeds - 1];
    return end.text_pos + end.length == last.text_pos + last.length && end.pattern_pos + end.length == last.pattern_pos + last.length;
}

bool same(const sa_seed &a, const sa_seed &b) { return a.text_pos == b.text_pos && a.pattern_pos == b.pattern_pos && a.length == b.length; }

int refusals()
{
    const sa_chain_params good = {5, 11, 2, 0, SA_CHAIN_NO_LIMIT, SA_CHAIN_NO_LIMIT, 64};
    const sa_seed two[2] = {{0, 0, 4}, {6, 6, 4}};
    const uint64_t off[2] = {0, 2};
    ChainPlan plan;
    std::string err;
    auto want = [&](int code, const char *word, const sa_chain_params *cp, const sa_seed *a, const uint64_t *o, int64_t np) {
        err.clear();
        const int rc = chain_plan("check", cp, a, o, np, &plan, &err);
        if (rc == code && err.find(word) != std::string::npos) return true;
        std::printf("refusal: status %d and \"%s\" where status %d and the word \"%s\" were due\n", rc, err.c_str(), code, word);
        return false;
    };
    bool ok = want(SA_ERR_INVALID, "params", nullptr, two, off, 1);
    sa_chain_params p = good;
    p.match = 0;
    ok = ok && want(SA_ERR_INVALID, "match", &p, two, off, 1);
    p = good, p.gap_open = (1 << 20) + 1;
    ok = ok && want(SA_ERR_INVALID, "gap_open", &p, two, off, 1);
    p = good, p.gap_extend = -1;
    ok = ok && want(SA_ERR_INVALID, "gap_extend", &p, two, off, 1);
    p = good, p.skip = -1;
    ok = ok && want(SA_ERR_INVALID, "skip", &p, two, off, 1);
    p = good, p.max_gap = -1;
    ok = ok && want(SA_ERR_INVALID, "max_gap", &p, two, off, 1);
    p = good, p.max_diag = -2;
    ok = ok && want(SA_ERR_INVALID, "max_diag", &p, two, off, 1);
    p = good, p.lookback = 1025;
    ok = ok && want(SA_ERR_INVALID, "lookback", &p, two, off, 1);
    ok = ok && want(SA_ERR_INVALID, "anchors is null", &good, nullptr, off, 1);
    ok = ok && want(SA_ERR_INVALID, "anchor_off is null", &good, two, nullptr, 1);
    const uint64_t off1[2] = {1, 2}, down[3] = {0, 2, 1};
    ok = ok && want(SA_ERR_INVALID, "anchor_off[0]", &good, two, off1, 1);
    ok = ok && want(SA_ERR_INVALID, "pair 1", &good, two, down, 2);
    const sa_seed zero[2] = {{0, 0, 4}, {6, 6, 0}}, swapped[2] = {{6, 6, 4}, {0, 0, 4}};
    ok = ok && want(SA_ERR_INVALID, "pair 0, anchor 1", &good, zero, off, 1);
    ok = ok && want(SA_ERR_INVALID, "pair 0, anchor 1", &good, swapped, off, 1);
    const sa_seed far[2] = {{0, 0, 4}, {2147483647ull - 4, 6, 4}}, farY[2] = {{0, 0, 4}, {6, 2147483647ull - 4, 4}};
    ok = ok && want(SA_ERR_UNSUPPORTED, "pair 0, anchor 1", &good, far, off, 1);
    ok = ok && want(SA_ERR_UNSUPPORTED, "pair 0, anchor 1", &good, farY, off, 1);
    p = good, p.match = 1024;
    const sa_seed heavy[2] = {{0, 0, 1 << 19}, {1 << 19, 1 << 19, 1 << 19}}, light[2] = {{0, 0, 1 << 19}, {1 << 19, 1 << 19, (1 << 19) - 1}};
    ok = ok && want(SA_ERR_UNSUPPORTED, "pair 0", &p, heavy, off, 1);
    if (ok && chain_plan("check", &p, light, off, 1, &plan, &err) != SA_OK)
    {
        std::printf("refusal: match * sum(length) = 2^30 - 1024 was refused: %s\n", err.c_str());
        ok = false;
    }
    return ok ? 0 : 1;
}
}  // namespace

int main(int argc, char **argv)
{
    const uint64_t sets = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 300;
    std::printf("sizeof sa_chain_params %zu\nsizeof sa_chain_result %zu\nsizeof sa_seed %zu\n", sizeof(sa_chain_params), sizeof(sa_chain_result),
                sizeof(sa_seed));
    if (refusals()) return 1;
    uint64_t seed = 97531;
    for (uint64_t t = 0; t < sets; ++t)
    {
        const size_t count = (size_t)(next(seed) % 10);
        std::vector<sa_seed> a(count);
        for (sa_seed &s : a)
        {
            s.length = 1 + next(seed) % 8;
            s.text_pos = next(seed) % (31 - s.length);
            // two in three near the text position, so that chains form
            s.pattern_pos = next(seed) % 3 ? std::min<uint64_t>(30 - s.length, s.text_pos + next(seed) % 4) : next(seed) % (31 - s.length);
        }
        std::sort(a.begin(), a.end(), keyLess);
        sa_chain_params cp;
        cp.match = 1 + (int32_t)(next(seed) % 6);
        cp.gap_open = (int32_t)(next(seed) % 12);
        cp.gap_extend = (int32_t)(next(seed) % 4);
        cp.skip = (int32_t)(next(seed) % 3);
        const int32_t gaps[4] = {SA_CHAIN_NO_LIMIT, 3, 10, 0}, diags[4] = {SA_CHAIN_NO_LIMIT, 0, 2, 7};
        cp.max_gap = gaps[next(seed) % 4];
        cp.max_diag = diags[next(seed) % 4];
        cp.lookback = 9 + (int32_t)(next(seed) % 3) * 500;
        // the set between two neighbours: pair 1 of three
        std::vector<sa_seed> all = {{3, 3, 5}, {9, 10, 2}};
        std::vector<uint64_t> off = {0, 2};
        all.insert(all.end(), a.begin(), a.end());
        off.push_back(all.size());
        all.push_back(sa_seed{1, 2, 3});
        off.push_back(all.size());
        Run three, alone, shifted;
        if (!run(cp, all, off, &three) || !run(cp, a, {0, a.size()}, &alone)) return 1;
        const sa_chain_result &r = alone.results[0], &in3 = three.results[1];
        const int64_t brute = bruteForce(cp, a);
        if (r.score != brute)
        {
            std::printf("set %llu: score %d, the brute force over all subsequences gives %lld (K3)\n", (unsigned long long)t, r.score, (long long)brute);
            return 1;
        }
        if (!validChain(a, r, alone.seeds.data()) || alone.off[1] != r.num_seeds || r.seeds_off != 0)
        {
            std::printf("set %llu: the output is no chain of tails of the input anchors (K1)\n", (unsigned long long)t);
            return 1;
        }
        bool k5 = in3.score == r.score && in3.num_seeds == r.num_seeds && in3.last_anchor == r.last_anchor && in3.seeds_off == three.off[1];
        for (uint32_t s = 0; k5 && s < r.num_seeds; ++s) k5 = same(three.seeds[in3.seeds_off + s], alone.seeds[s]);
        std::vector<sa_seed> moved = a;
        for (sa_seed &s : moved) s.text_pos += 1000, s.pattern_pos += 77;
        if (!run(cp, moved, {0, moved.size()}, &shifted)) return 1;
        const sa_chain_result &m = shifted.results[0];
        k5 = k5 && m.score == r.score && m.num_seeds == r.num_seeds && m.last_anchor == r.last_anchor;
        for (uint32_t s = 0; k5 && s < r.num_seeds; ++s)
            k5 = same(shifted.seeds[s], sa_seed{alone.seeds[s].text_pos + 1000, alone.seeds[s].pattern_pos + 77, alone.seeds[s].length});
        if (!k5)
        {
            std::printf("set %llu: the result changes with the pair's neighbours or with a shift of its anchors (K5)\n", (unsigned long long)t);
            return 1;
        }
        // K4: the chain just found is a valid chain; under zero costs and no limits it comes back as it is
        if (r.num_seeds > 0)
        {
            const std::vector<sa_seed> chain(alone.seeds.begin(), alone.seeds.end());
            const sa_chain_params zero = {cp.match, 0, 0, 0, SA_CHAIN_NO_LIMIT, SA_CHAIN_NO_LIMIT, 1 + (int32_t)(next(seed) % 9)};
            Run back;
            if (!run(zero, chain, {0, chain.size()}, &back)) return 1;
            uint64_t sum = 0;
            for (const sa_seed &s : chain) sum += s.length;
            bool k4 = back.results[0].score == (int64_t)(zero.match * sum) && back.seeds.size() == chain.size() &&
                      back.results[0].last_anchor == chain.size() - 1;
            for (size_t s = 0; k4 && s < chain.size(); ++s) k4 = same(back.seeds[s], chain[s]);
            if (!k4)
            {
                std::printf("set %llu: a valid chain does not come back unchanged under zero costs (K4)\n", (unsigned long long)t);
                return 1;
            }
        }
    }
    std::printf("OK %llu\n", (unsigned long long)sets);
    return 0;
}
