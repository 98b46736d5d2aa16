// Chaining on the host: validation, the structure-of-arrays form and the definition of sa_hip.h (sa_chain_plan.h).
#include "sa_chain_plan.h"

#include <algorithm>
#include <numeric>

namespace sa {

namespace {

int refuse(int code, std::string *err, const std::string &msg)
{
    if (err) *err = msg;
    return code;
}

bool limit_ok(int32_t v) { return v >= 0; }  // SA_CHAIN_NO_LIMIT is INT32_MAX: every non-negative value is a limit

}  // namespace

int chain_plan(const char *fn_name, const sa_chain_params *cp, const sa_seed *anchors, const uint64_t *anchor_off, int64_t np,
               ChainPlan *out, std::string *err)
{
    const std::string fn = std::string(fn_name) + ": ";
    if (!cp) return refuse(SA_ERR_INVALID, err, fn + "params is null");
    if (cp->match < 1 || cp->match > kChainMaxMatch) return refuse(SA_ERR_INVALID, err, fn + "match is " + std::to_string(cp->match) + ", outside 1 .. 1024");
    if (cp->gap_open < 0 || cp->gap_open > kChainMaxCost)
        return refuse(SA_ERR_INVALID, err, fn + "gap_open is " + std::to_string(cp->gap_open) + ", outside 0 .. 2^20");
    if (cp->gap_extend < 0 || cp->gap_extend > kChainMaxCost)
        return refuse(SA_ERR_INVALID, err, fn + "gap_extend is " + std::to_string(cp->gap_extend) + ", outside 0 .. 2^20");
    if (cp->skip < 0 || cp->skip > kChainMaxCost) return refuse(SA_ERR_INVALID, err, fn + "skip is " + std::to_string(cp->skip) + ", outside 0 .. 2^20");
    if (!limit_ok(cp->max_gap)) return refuse(SA_ERR_INVALID, err, fn + "max_gap is " + std::to_string(cp->max_gap) + ": >= 0, or SA_CHAIN_NO_LIMIT");
    if (!limit_ok(cp->max_diag)) return refuse(SA_ERR_INVALID, err, fn + "max_diag is " + std::to_string(cp->max_diag) + ": >= 0, or SA_CHAIN_NO_LIMIT");
    if (cp->lookback < 1 || cp->lookback > kChainMaxLookback)
        return refuse(SA_ERR_INVALID, err, fn + "lookback is " + std::to_string(cp->lookback) + ", outside 1 .. 1024");
    if (np < 0) return refuse(SA_ERR_INVALID, err, fn + "num_pairs is negative");
    if (np > 0 && !anchor_off) return refuse(SA_ERR_INVALID, err, fn + "anchor_off is null");
    if (np > 0 && !anchors) return refuse(SA_ERR_INVALID, err, fn + "anchors is null");
    if (np >= (1ll << 31)) return refuse(SA_ERR_UNSUPPORTED, err, fn + "num_pairs >= 2^31");
    if (np > 0 && anchor_off[0] != 0) return refuse(SA_ERR_INVALID, err, fn + "anchor_off[0] is " + std::to_string(anchor_off[0]) + ", not 0");
    for (int64_t k = 0; k < np; ++k)
        if (anchor_off[k + 1] < anchor_off[k])
            return refuse(SA_ERR_INVALID, err, fn + "anchor_off decreases at pair " + std::to_string(k) + ": " + std::to_string(anchor_off[k]) + " then " +
                                                   std::to_string(anchor_off[k + 1]));
    ChainPlan &plan = *out;
    plan = ChainPlan();
    plan.cp = *cp;
    plan.num_pairs = np;
    const uint64_t total = np > 0 ? anchor_off[np] : 0;
    plan.off.assign(1, 0);
    if (np > 0) plan.off.assign(anchor_off, anchor_off + np + 1);
    plan.ex.resize(total), plan.ey.resize(total), plan.len.resize(total);
    for (int64_t k = 0; k < np; ++k)
    {
        const std::string pair = "pair " + std::to_string(k);
        uint64_t sum = 0;
        for (uint64_t a = anchor_off[k]; a < anchor_off[k + 1]; ++a)
        {
            const sa_seed &s = anchors[a];
            const std::string where = pair + ", anchor " + std::to_string(a - anchor_off[k]);
            if (s.length == 0) return refuse(SA_ERR_INVALID, err, fn + where + " has length 0");
            if (s.length >= kChainCoordLimit || s.text_pos >= kChainCoordLimit || s.text_pos + s.length >= kChainCoordLimit)
                return refuse(SA_ERR_UNSUPPORTED, err, fn + where + " ends in the text at or above 2^31 - 1");
            if (s.pattern_pos >= kChainCoordLimit || s.pattern_pos + s.length >= kChainCoordLimit)
                return refuse(SA_ERR_UNSUPPORTED, err, fn + where + " ends in the pattern at or above 2^31 - 1");
            plan.ex[a] = (int32_t)(s.text_pos + s.length);
            plan.ey[a] = (int32_t)(s.pattern_pos + s.length);
            plan.len[a] = (int32_t)s.length;
            if (a > anchor_off[k])
            {
                const bool ordered = plan.ex[a - 1] != plan.ex[a]   ? plan.ex[a - 1] < plan.ex[a]
                                     : plan.ey[a - 1] != plan.ey[a] ? plan.ey[a - 1] < plan.ey[a]
                                                                    : plan.len[a - 1] <= plan.len[a];
                if (!ordered)
                    return refuse(SA_ERR_INVALID, err, fn + where + " is out of canonical order: (text end, pattern end, length) falls below that of the anchor before it");
            }
            sum += s.length;  // below 2^31 a term, and checked before it can pass 2^32
            if (sum * (uint64_t)cp->match >= (uint64_t)kChainScoreLimit)
                return refuse(SA_ERR_UNSUPPORTED, err, fn + pair + " has match * sum(length) >= 2^30 (reached at anchor " + std::to_string(a - anchor_off[k]) + ")");
        }
        plan.max_anchors = std::max(plan.max_anchors, anchor_off[k + 1] - anchor_off[k]);
    }
    plan.order.resize((size_t)np);
    std::iota(plan.order.begin(), plan.order.end(), 0u);
    std::stable_sort(plan.order.begin(), plan.order.end(),
                     [&](uint32_t a, uint32_t b) { return plan.off[a + 1] - plan.off[a] > plan.off[b + 1] - plan.off[b]; });
    return SA_OK;
}

ChainHead chain_host_pair(const ChainPlan &plan, uint64_t first, uint64_t count, int32_t *pred, int32_t *cut)
{
    const sa_chain_params &cp = plan.cp;
    const int32_t *ex = plan.ex.data() + first, *ey = plan.ey.data() + first, *len = plan.len.data() + first;
    std::vector<int64_t> f(count);
    std::vector<uint32_t> seeds(count);
    ChainHead head = {0, 0, 0, 0};
    for (uint64_t i = 0; i < count; ++i)
    {
        const int64_t L = len[i], x = ex[i] - L, y = ey[i] - L;
        int64_t best = (int64_t)cp.match * L;
        int32_t from = -1, o_best = 0;
        const uint64_t reach = std::min<uint64_t>(i, (uint64_t)cp.lookback);
        for (uint64_t d = 1; d <= reach; ++d)  // nearest first: a later equal value does not replace it
        {
            const uint64_t j = i - d;
            const int64_t o = std::max<int64_t>(0, std::max<int64_t>(ex[j] - x, ey[j] - y));
            if (o >= L) continue;
            const int64_t dx = x + o - ex[j], dy = y + o - ey[j], dd = dx > dy ? dx - dy : dy - dx;
            if (dx > cp.max_gap || dy > cp.max_gap || dd > cp.max_diag) continue;
            const int64_t cost = (dd ? cp.gap_open + (dd - 1) * cp.gap_extend : 0) + (int64_t)cp.skip * std::min(dx, dy);
            const int64_t v = f[j] + (int64_t)cp.match * (L - o) - cost;
            if (v > best) best = v, from = (int32_t)j, o_best = (int32_t)o;
        }
        f[i] = best;
        pred[i] = from;
        cut[i] = o_best;
        seeds[i] = from < 0 ? 1 : seeds[from] + 1;
        if (i == 0 || best > head.score) head = ChainHead{(int32_t)best, (uint32_t)i, seeds[i], 0};
    }
    return head;
}

void chain_walk_pair(const ChainPlan &plan, uint64_t first, uint64_t count, const ChainHead &head, const int32_t *pred, const int32_t *cut,
                     sa_seed *seeds)
{
    uint64_t i = head.last;
    for (uint32_t s = head.num_seeds; s-- > 0;)
    {
        if (i >= count) break;
        const int64_t L = plan.len[first + i], o = cut[i];
        seeds[s] = sa_seed{(uint64_t)(plan.ex[first + i] - L + o), (uint64_t)(plan.ey[first + i] - L + o), (uint64_t)(L - o)};
        i = pred[i] < 0 ? count : (uint64_t)pred[i];
    }
}

void chain_host(const ChainPlan &plan, sa_chain_result *results, std::vector<sa_seed> *seeds, std::vector<uint64_t> *seeds_off)
{
    const int64_t np = plan.num_pairs;
    seeds->clear();
    seeds_off->assign((size_t)np + 1, 0);
    std::vector<int32_t> pred(plan.max_anchors), cut(plan.max_anchors);
    for (int64_t k = 0; k < np; ++k)
    {
        const uint64_t first = plan.off[k], count = plan.off[k + 1] - first;
        const ChainHead head = chain_host_pair(plan, first, count, pred.data(), cut.data());
        results[k] = sa_chain_result{head.score, SA_OK, seeds->size(), head.num_seeds, head.last};
        seeds->resize(seeds->size() + head.num_seeds);
        chain_walk_pair(plan, first, count, head, pred.data(), cut.data(), seeds->data() + results[k].seeds_off);
        (*seeds_off)[k + 1] = seeds->size();
    }
}

}  // namespace sa
