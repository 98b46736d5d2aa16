// The score-only planner (sa_score_plan.h): validation, work order, rows per lane, launch and
// workspace of a scorer. Host only, no HIP.
#include "sa_score_plan.h"

#include <algorithm>
#include <cstdlib>
#include <numeric>

namespace sa {

const ScoreKnobs &score_knobs()
{
    static const ScoreKnobs k = [] {
        ScoreKnobs v;
        if (const char *e = std::getenv("SA_SCORE_ROWS_PER_LANE")) v.rows_per_lane = std::atoi(e);
        if (const char *e = std::getenv("SA_SCORE_WAVES")) v.waves_per_simd = std::atoi(e);
        if (const char *e = std::getenv("SA_MAX_CUS")) v.max_cus = std::atoi(e);
        return v;
    }();
    return k;
}

// the instance of each R with the most registers (local, alphabets up to 4): 53, 71, 101 and 165
// VGPRs of the SIMD's 512; the extension instances, planned as local ones, take 49, 67, 95 and 129, and
// so do the seeds instances, register for register (linear and affine)
int score_waves_per_simd(int R) { return R >= 8 ? 3 : R >= 4 ? 4 : R >= 2 ? 7 : 8; }

// the affine instances: 61, 84, 118 and 158 VGPRs (local, alphabets up to 4); extension: 59, 79, 114, 154
int score_affine_waves_per_simd(int R) { return R >= 8 ? 3 : R >= 4 ? 4 : R >= 2 ? 5 : 8; }

// the banded extension instances (kVarExtendBand, kVarSeedsBand): 69, 91, 125 and 166 VGPRs (alphabets up to 4;
// 63, 79, 110 and 160 above): one wave per SIMD fewer than the affine class at R = 1
int score_ext_band_waves_per_simd(int R) { return R >= 8 ? 3 : R >= 4 ? 4 : R >= 2 ? 5 : 7; }

namespace {

int bitlen(uint64_t v)
{
    int b = 0;
    while (v) { ++b; v >>= 1; }
    return b;
}

}  // namespace

// sa_hip.h: an in-band permitted start componentwise <= an in-band permitted end. A start on row 0
// lies above every end, so the one of the smallest column serves for all of them (the origin, or under
// TB the band's first cell of row 0), likewise the start of the smallest row on column 0; an end on
// row m lies below every start, so the rightmost serves ((m, n), or under TE the band's last cell of
// row m), likewise the lowest end on column n.
extern "C" int sa_band_reachable(int32_t mode, uint64_t text_len, uint64_t pattern_len, sa_band band)
{
    if (mode == SA_LOCAL) return 1;
    int fl;
    if (mode == SA_GLOBAL) fl = 0;
    else if (mode == SA_FIT) fl = SA_FREE_TEXT_BEGIN | SA_FREE_TEXT_END;
    else if (mode >= SA_ENDS_FREE && mode <= SA_OVERLAP) fl = mode & 15;
    else return -1;
    if (band.lo > band.hi) return 0;
    const int64_t n = (int64_t)std::min<uint64_t>(text_len, (uint64_t)1 << 40), m = (int64_t)std::min<uint64_t>(pattern_len, (uint64_t)1 << 40);
    const int64_t lo = band.lo, hi = band.hi;
    auto in = [&](int64_t i, int64_t j) { return lo <= j - i && j - i <= hi; };
    int64_t st[2][2], en[2][2];
    int ns = 0, ne = 0;
    if (in(0, 0)) st[ns][0] = 0, st[ns][1] = 0, ++ns;
    else
    {
        if ((fl & SA_FREE_TEXT_BEGIN) && lo > 0 && lo <= n) st[ns][0] = 0, st[ns][1] = lo, ++ns;
        if ((fl & SA_FREE_PATTERN_BEGIN) && hi < 0 && -hi <= m) st[ns][0] = -hi, st[ns][1] = 0, ++ns;
    }
    if (in(m, n)) en[ne][0] = m, en[ne][1] = n, ++ne;
    else
    {
        // row m: columns m + lo .. m + hi inside 0 .. n; column n: rows n - hi .. n - lo inside 0 .. m
        if ((fl & SA_FREE_TEXT_END) && m + lo <= n && m + hi >= 0) en[ne][0] = m, en[ne][1] = std::min(n, m + hi), ++ne;
        if ((fl & SA_FREE_PATTERN_END) && n - hi <= m && n - lo >= 0) en[ne][0] = std::min(m, n - lo), en[ne][1] = n, ++ne;
    }
    for (int a = 0; a < ns; ++a)
        for (int b = 0; b < ne; ++b)
            if (st[a][0] <= en[b][0] && st[a][1] <= en[b][1]) return 1;
    return 0;
}

int make_score_plan(const sa_params *P, const WaveSpec &spec, const sa_pair *pairs, int64_t np, int num_cu, const ScoreKnobs &kn,
                    ScorePlan *out, std::string *err)
{
    auto fail = [&](int code, const char *msg) { *err = msg; return code; };
    if (!P || !out || np < 0 || (np > 0 && !pairs) || !P->score_matrix) return fail(SA_ERR_INVALID, "scorer: null argument");
    const int A = P->alphabet_size;
    if (A < 1 || A > 32) return fail(SA_ERR_INVALID, "alphabet_size must be 1..32");
    const bool ends = P->mode >= SA_ENDS_FREE && P->mode <= SA_OVERLAP;
    if (P->mode != SA_GLOBAL && P->mode != SA_LOCAL && P->mode != SA_FIT && !ends)
        return fail(SA_ERR_INVALID, "mode must be SA_GLOBAL, SA_LOCAL, SA_FIT or SA_ENDS_FREE with its flags");
    if (np > INT32_MAX) return fail(SA_ERR_UNSUPPORTED, "more than 2^31-1 pairs");
    bool affine = spec.affine;
    const sa_band *const bands = spec.bands;
    if (spec.banded)
    {
        if (!affine) return fail(SA_ERR_INVALID, "a band takes gap_open and gap_extend");
        if (spec.band < 0) return fail(SA_ERR_INVALID, "band must be >= 0");
        if (P->mode == SA_FIT) return fail(SA_ERR_UNSUPPORTED, "SA_FIT takes no band");
        if (ends) return fail(SA_ERR_UNSUPPORTED, "SA_ENDS_FREE takes no band");
    }
    if (spec.band_at && (!affine || spec.banded)) return fail(SA_ERR_INVALID, "per-pair bands take gap_open and gap_extend and no half-width");
    if (spec.band_at && !bands && np > 0) return fail(SA_ERR_INVALID, "scorer: null argument");
    if (spec.seeded) return fail(SA_ERR_INVALID, "a seeded call is planned by its work items (make_seeds_score_plan)");
    if (spec.extend)
    {
        if (!affine) return fail(SA_ERR_INVALID, "extension alignment takes gap_open and gap_extend");
        if (P->mode != SA_GLOBAL) return fail(SA_ERR_INVALID, "extension alignment takes mode SA_GLOBAL: its borders are global's");
        if (spec.xdrop < SA_NO_XDROP || spec.xdrop >= (1 << 30)) return fail(SA_ERR_INVALID, "xdrop must be SA_NO_XDROP or 0 .. 2^30 - 1");
        if (spec.banded || spec.band_at) return fail(SA_ERR_UNSUPPORTED, "extension alignment inside a band (band or bands with xdrop) is not built");
        if (spec.ext_band && spec.width < 0) return fail(SA_ERR_INVALID, "width must be >= 0");
    }
    else if (spec.ext_band) return fail(SA_ERR_INVALID, "a width takes an extension (xdrop)");
    // gap open == gap extend is the linear recurrence of that penalty: the linear instances, step costs and
    // boundary row, with the penalty in the place of P->gap_penalty
    int64_t g = P->gap_penalty;
    if (spec.extend && !spec.ext_band && !spec.traced && spec.gap_open == spec.gap_extend)  // a banded instance is affine
    {
        g = spec.gap_open;
        affine = false;
    }
    const bool banded = spec.banded || spec.band_at || spec.ext_band;
    int R = P->rows_per_lane;
    if (kn.rows_per_lane) R = kn.rows_per_lane;
    if (R == 16 || R == 32) R = 8;  // a params struct shared with a plan: the scorer's tallest strip
    if (R != 0 && R != 1 && R != 2 && R != 4 && R != 8) return fail(SA_ERR_INVALID, "rows_per_lane must be 0, 1, 2, 4, 8, 16 or 32");

    // ---- the limits of the plans, unchanged; an affine gap counts as the larger of
    // |open| and |extend|, and as negative if either is ----
    if (affine)
    {
        g = std::max(std::llabs((long long)spec.gap_open), std::llabs((long long)spec.gap_extend));
        if (spec.gap_open < 0 || spec.gap_extend < 0) g = -g;
    }
    int64_t smax = INT32_MIN, sabs = 0;
    for (int e = 0; e < A * A; ++e)
    {
        smax = std::max<int64_t>(smax, P->score_matrix[e]);
        sabs = std::max<int64_t>(sabs, std::llabs((long long)P->score_matrix[e]));
    }
    uint64_t lmax = 0, hmax_local = 0;
    ScorePlan &pl = *out;
    pl = ScorePlan();
    for (int64_t p = 0; p < np; ++p)
    {
        const uint64_t n = pairs[p].text_len, m = pairs[p].pattern_len;
        if (n >= (1u << 24) - 1 || m >= (1u << 24) - 1) return fail(SA_ERR_UNSUPPORTED, "sequence longer than 2^24-2 letters");
        lmax = std::max(lmax, std::max(n, m));
        const uint64_t span = n + m;
        const uint64_t bound = ((uint64_t)sabs + (uint64_t)std::llabs(g)) * span + (uint64_t)std::llabs(g) * span;
        if (bound >= (1ull << 30)) return fail(SA_ERR_UNSUPPORTED, "scores may exceed the int32 range");
        if (banded && bound >= kBandScoreLimit) return fail(SA_ERR_UNSUPPORTED, "scores may reach the band's sentinel");
        const uint64_t h = g >= 0 ? (uint64_t)std::max<int64_t>(smax, 0) * std::min(n, m)
                                  : ((uint64_t)sabs + (uint64_t)(-g)) * span;
        hmax_local = std::max(hmax_local, h);
        pl.max_text = std::max(pl.max_text, n);
        pl.input_bytes += n + m;
    }
    // ---- the band-at scorer: every pair's band is a band and admits an alignment; the kernels take the
    // clipped bands and rely on both ----
    if (spec.band_at)
    {
        pl.bands.resize((size_t)np);
        for (int64_t p = 0; p < np; ++p)
        {
            const std::string who = "pair " + std::to_string(p) + ": band [" + std::to_string(bands[p].lo) + ", " + std::to_string(bands[p].hi) + "]";
            if (bands[p].lo > bands[p].hi)
            {
                *err = who + " has lo > hi";
                return SA_ERR_INVALID;
            }
            if (sa_band_reachable(P->mode, pairs[p].text_len, pairs[p].pattern_len, bands[p]) != 1)
            {
                *err = who + " admits no alignment of " + std::to_string(pairs[p].text_len) + " text and " +
                       std::to_string(pairs[p].pattern_len) + " pattern letters in mode " + std::to_string(P->mode) + " (sa_band_reachable)";
                return SA_ERR_INVALID;
            }
            pl.bands[p] = band_clip((int64_t)pairs[p].text_len, (int64_t)pairs[p].pattern_len, bands[p].lo, bands[p].hi);
        }
    }
    // a pair's band and the window of one of its strips: band_window_at is band_window on the bands of band_of
    auto pair_band = [&](int64_t p) {
        if (spec.ext_band) return band_ext((int64_t)pairs[p].text_len, (int64_t)pairs[p].pattern_len, spec.width);
        return spec.band_at ? pl.bands[p] : band_of((int64_t)pairs[p].text_len, (int64_t)pairs[p].pattern_len, spec.band);
    };
    pl.key_rowbits = std::max(1, bitlen(lmax + 1));
    if ((P->mode == SA_LOCAL || spec.extend) && (bitlen(hmax_local) > 26 || bitlen(hmax_local) > 64 - 2 * pl.key_rowbits))
        return fail(SA_ERR_UNSUPPORTED, "local scores may exceed the best-cell key range");

    pl.mode = P->mode;
    pl.A = A;
    pl.gap = affine ? spec.gap_open : (int)g;
    pl.spec = spec;
    pl.spec.affine = affine;
    pl.spec.gap_extend = affine ? spec.gap_extend : 0;
    pl.spec.bands = nullptr;  // the caller's; the plan keeps the clipped copy
    pl.spec.seeds = nullptr;
    pl.num_pairs = np;
    pl.num_cu = kn.max_cus > 0 ? std::min(num_cu, kn.max_cus) : num_cu;

    // ---- work order: most cells first, ties by index (waves draw pairs in this order, so the long
    // pairs start first and the short ones fill the tail) ----
    pl.order.resize((size_t)np);
    std::iota(pl.order.begin(), pl.order.end(), 0);
    std::vector<uint64_t> cells((size_t)np);
    for (int64_t p = 0; p < np; ++p)
    {
        const uint64_t n = pairs[p].text_len, m = pairs[p].pattern_len;
        cells[p] = banded ? band_cells(n, m, pair_band(p)) : n * m;
        if (banded) pl.band_cells += cells[p];
    }
    std::stable_sort(pl.order.begin(), pl.order.end(), [&](int32_t a, int32_t b) { return cells[a] > cells[b]; });

    // ---- rows per lane: a strip of 64R rows over n columns takes n + 63 steps of
    // kScoreStepBase + R * kScoreStepRow* instructions; the cheapest total wins, ties to the
    // smaller R (fewer registers, more resident waves); the affine kernel has its own counts. A banded
    // strip takes the steps of its window, jmax - jmin + 64 (n + 63 when the band admits every cell): a
    // tall strip under a narrow band mostly steps through out-of-band cells, so R falls with the band. A fit
    // step is a global step plus the best of row m: kScoreFitStepBest + (R - 1) * kScoreFitStepSelect,
    // the same in both kernels. An ends-free mode runs the fit program when the text's end is free and
    // the global one otherwise: the other free ends cost nothing per step ----
    static const int kR[4] = {1, 2, 4, 8};
    const bool fit = P->mode == SA_FIT || (ends && (P->mode & SA_FREE_TEXT_END));
    const int step_base = (affine ? kScoreAffineStepBase : kScoreStepBase) + (fit ? kScoreFitStepBest - kScoreFitStepSelect : 0);
    const int step_row = (P->mode == SA_LOCAL || spec.extend ? (affine ? kScoreAffineStepRowLocal : kScoreStepRowLocal)
                                              : (affine ? kScoreAffineStepRowGlobal : kScoreStepRowGlobal)) +
                         (fit ? kScoreFitStepSelect : 0);
    int best = 0;
    for (int k = 0; k < 4; ++k)
    {
        const uint64_t rows = 64ull * kR[k], per_step = (uint64_t)(step_base + kR[k] * step_row);
        uint64_t c = 0;
        for (int64_t p = 0; p < np; ++p)
        {
            const uint64_t n = pairs[p].text_len, m = pairs[p].pattern_len;
            if (n == 0 || m == 0) continue;
            const uint64_t strips = (m + rows - 1) / rows;
            if (!banded)
            {
                c += (n + 63) * strips * per_step;
                continue;
            }
            const Band bd = pair_band(p);
            for (uint64_t s = 0; s < strips; ++s)
            {
                const BandWindow bw = band_window_at((int64_t)n, (int64_t)m, (int64_t)rows, (int64_t)s, bd);
                if (bw.b1 > bw.b0) c += (uint64_t)(bw.jmax - bw.jmin + 64) * per_step;  // an empty strip runs no step
            }
        }
        pl.cost[k] = c;
        if (c < pl.cost[best]) best = k;
    }
    pl.R = R ? R : kR[best];
    for (int64_t p = 0; p < np; ++p)
    {
        const uint64_t rows = 64ull * pl.R, n = pairs[p].text_len, m = pairs[p].pattern_len, strips = (m + rows - 1) / rows;
        if (!banded || n == 0) pl.padded_cells += n * strips * rows;
        else
        {
            const Band bd = pair_band(p);
            for (uint64_t s = 0; s < strips; ++s)
            {
                const BandWindow bw = band_window_at((int64_t)n, (int64_t)m, (int64_t)rows, (int64_t)s, bd);
                pl.padded_cells += (uint64_t)(bw.jmax - bw.jmin + 1) * rows;
            }
        }
    }

    // ---- launch and workspace ----
    pl.waves_per_simd = kn.waves_per_simd > 0 ? std::min(kn.waves_per_simd, 8)
                        : spec.ext_band ? score_ext_band_waves_per_simd(pl.R)
                        : affine        ? score_affine_waves_per_simd(pl.R)
                                        : score_waves_per_simd(pl.R);
    pl.grid = (int)std::min<int64_t>(np, (int64_t)pl.num_cu * 4 * pl.waves_per_simd);
    pl.row_stride = (pl.max_text + 63) / 64 * 64 + 64;
    const uint64_t per_pair = 24 /* descriptor */ + (spec.band_at ? 8 : 0) /* band */ + 4 /* order */ + sizeof(sa_score_result);
    pl.device_bytes = pl.input_bytes + (uint64_t)np * per_pair + (uint64_t)pl.grid * pl.row_stride * (affine ? 8 : 4) +
                      32 * 32 * 4 /* score table */ + 256 /* counter and flags */;
    return SA_OK;
}

int make_seeds_score_plan(const sa_params *P, const WaveSpec &spec, const sa_pair *pairs, const sa_seed *seeds, int64_t np, int num_cu,
                          const ScoreKnobs &kn, ScorePlan *out, SeedItems *items, std::string *err)
{
    if (!items || !spec.extend)
    {
        *err = "seeds scorer: null argument";
        return SA_ERR_INVALID;
    }
    WaveSpec ext = spec;  // the extension each item runs; make_score_plan takes no seeded spec
    ext.seeded = false;
    ext.seeds = nullptr;
    // the mode, the xdrop and the limits, on the whole pairs: the sum of the three scores of a pair stays
    // under the bound of its (n, m), and so does every key
    ScorePlan whole;
    if (int rc = make_score_plan(P, ext, pairs, np, num_cu, kn, &whole, err)) return rc;
    if (np > 0 && !seeds)
    {
        *err = "seeds is null";
        return SA_ERR_INVALID;
    }
    items->items.clear();
    items->pairs.resize((size_t)np);
    for (int64_t p = 0; p < np; ++p)
    {
        const uint64_t n = pairs[p].text_len, m = pairs[p].pattern_len;
        const uint64_t ts = seeds[p].text_pos, ps = seeds[p].pattern_pos, L = seeds[p].length;
        // n, m < 2^24: compared so that no sum wraps
        if (ts > n || L > n - ts || ps > m || L > m - ps)
        {
            *err = "pair " + std::to_string(p) + ": seed {" + std::to_string(ts) + ", " + std::to_string(ps) + ", " + std::to_string(L) +
                   "} does not lie inside " + std::to_string(n) + " text and " + std::to_string(m) + " pattern letters";
            return SA_ERR_INVALID;
        }
        SeedPair &sp = items->pairs[p];
        sp = SeedPair{pairs[p].text_offset + ts, pairs[p].pattern_offset + ps, ts, ps, L, -1, -1};
        if (ts > 0 && ps > 0)
        {
            sp.left = (int32_t)items->items.size();
            items->items.push_back(SeedItem{sp.text_seed - 1, sp.pattern_seed - 1, (uint32_t)ts, (uint32_t)ps, -1, (int32_t)p});
        }
        const uint64_t rn = n - ts - L, rm = m - ps - L;
        if (rn > 0 && rm > 0)
        {
            sp.right = (int32_t)items->items.size();
            items->items.push_back(SeedItem{sp.text_seed + L, sp.pattern_seed + L, (uint32_t)rn, (uint32_t)rm, 1, (int32_t)p});
        }
    }
    // the items as extension pairs: cost, R, order by cells, grid and boundary rows
    std::vector<sa_pair> ip(items->items.size());
    for (size_t k = 0; k < ip.size(); ++k) ip[k] = sa_pair{0, items->items[k].n, 0, items->items[k].m};
    if (int rc = make_score_plan(P, ext, ip.data(), (int64_t)ip.size(), num_cu, kn, out, err)) return rc;
    out->spec.seeded = true;
    out->device_bytes += whole.input_bytes - out->input_bytes + (uint64_t)ip.size() * (sizeof(SeedItem) - 24) +
                         (uint64_t)np * (sizeof(SeedPair) + sizeof(sa_seed_result));
    out->input_bytes = whole.input_bytes;
    return SA_OK;
}

int make_chains_score_plan(const sa_params *P, const WaveSpec &spec, const sa_pair *pairs, int64_t np, int num_cu, const ScoreKnobs &kn,
                           ChainsScorePlan *out, std::string *err)
{
    if (!out || !spec.extend)
    {
        *err = "chains scorer: null argument";
        return SA_ERR_INVALID;
    }
    *out = ChainsScorePlan();
    if (spec.ext_band || spec.banded || spec.band_at)
    {
        *err = "chained seeds inside a band (band, bands or width with chains) are not built";
        return SA_ERR_UNSUPPORTED;
    }
    WaveSpec ext = spec;  // the extension each end item runs; make_score_plan takes no seeded spec
    ext.seeded = ext.chained = false;
    ext.seeds = nullptr;
    ext.chain_off = nullptr;
    // the mode, the xdrop and the limits, on the whole pairs: the sum of a pair's pieces stays under the bound of
    // its (n, m), and so does every key
    ScorePlan whole;
    if (int rc = make_score_plan(P, ext, pairs, np, num_cu, kn, &whole, err)) return rc;
    const sa_seed *const seeds = spec.seeds;
    const uint64_t *const off = spec.chain_off;
    if (np > 0 && (!seeds || !off))
    {
        *err = !seeds ? "seeds is null" : "chain_off is null";
        return SA_ERR_INVALID;
    }
    if (np > 0 && off[0] != 0)
    {
        *err = "pair 0: chain_off[0] is " + std::to_string(off[0]) + ", not 0";
        return SA_ERR_INVALID;
    }
    ChainItems &ci = out->items;
    ci.pairs.resize((size_t)np);
    const int64_t go = spec.gap_open, ge = spec.gap_extend;
    for (int64_t p = 0; p < np; ++p)
    {
        const std::string who = "pair " + std::to_string(p);
        if (off[p + 1] < off[p])
        {
            *err = who + ": chain_off decreases from " + std::to_string(off[p]) + " to " + std::to_string(off[p + 1]);
            return SA_ERR_INVALID;
        }
        if (off[p + 1] == off[p])
        {
            *err = who + " has no seed: a chain holds at least one";
            return SA_ERR_INVALID;
        }
        if (off[p + 1] > (uint64_t)INT32_MAX)
        {
            *err = "more than 2^31-1 seeds";
            return SA_ERR_UNSUPPORTED;
        }
        const uint64_t n = pairs[p].text_len, m = pairs[p].pattern_len, c = off[p + 1] - off[p];
        ChainPair &cp = ci.pairs[p];
        cp = ChainPair();
        cp.text_base = pairs[p].text_offset;
        cp.pattern_base = pairs[p].pattern_offset;
        cp.seed_begin = (int32_t)off[p];
        cp.seed_end = (int32_t)off[p + 1];
        cp.gap_begin = (int32_t)ci.gaps.size();
        cp.left = cp.right = -1;
        int64_t closed = 0;
        uint64_t te = 0, pe = 0;  // the end of the seed before
        for (uint64_t i = 0; i < c; ++i)
        {
            const sa_seed &sd = seeds[off[p] + i];
            const uint64_t ts = sd.text_pos, ps = sd.pattern_pos, L = sd.length;
            const std::string what = who + ", seed " + std::to_string(i) + " {" + std::to_string(ts) + ", " + std::to_string(ps) + ", " + std::to_string(L) + "}";
            // n, m < 2^24: compared so that no sum wraps
            if (ts > n || L > n - ts || ps > m || L > m - ps)
            {
                *err = what + " does not lie inside " + std::to_string(n) + " text and " + std::to_string(m) + " pattern letters";
                return SA_ERR_INVALID;
            }
            if (i > 0 && (ts < te || ps < pe))
            {
                *err = what + " begins before the end (" + std::to_string(te) + ", " + std::to_string(pe) + ") of the seed before it: a chain is colinear and its seeds do not overlap";
                return SA_ERR_INVALID;
            }
            if (i == 0)
            {
                cp.ts = ts;
                cp.ps = ps;
                if (ts > 0 && ps > 0)
                {
                    cp.left = (int32_t)ci.ends.size();
                    ci.ends.push_back(SeedItem{pairs[p].text_offset + ts - 1, pairs[p].pattern_offset + ps - 1, (uint32_t)ts, (uint32_t)ps, -1, (int32_t)p});
                }
            }
            else
            {
                const uint64_t gn = ts - te, gm = ps - pe;
                if (gn > 0 && gm > 0)
                {
                    ci.seeds.back().gap = (int32_t)ci.gaps.size();
                    ci.gaps.push_back(SeedItem{pairs[p].text_offset + te, pairs[p].pattern_offset + pe, (uint32_t)gn, (uint32_t)gm, 1, (int32_t)p});
                }
                else if (gn + gm > 0)
                {
                    closed -= go + ((int64_t)(gn + gm) - 1) * ge;  // inside int32 under the whole pair's limit
                    cp.closed_cols += (uint32_t)(gn + gm);
                }
            }
            ci.seeds.push_back(ChainSeed{pairs[p].text_offset + ts, pairs[p].pattern_offset + ps, L, -1, 0});
            te = ts + L;
            pe = ps + L;
        }
        cp.te = te;
        cp.pe = pe;
        cp.gap_end = (int32_t)ci.gaps.size();
        cp.closed_score = (int32_t)closed;
        if (n - te > 0 && m - pe > 0)
        {
            cp.right = (int32_t)ci.ends.size();
            ci.ends.push_back(SeedItem{pairs[p].text_offset + te, pairs[p].pattern_offset + pe, (uint32_t)(n - te), (uint32_t)(m - pe), 1, (int32_t)p});
        }
    }
    // the end items as extension pairs, the gap items as global pairs: each launch has its own cost, R, order by
    // cells, grid and boundary rows
    auto as_pairs = [](const std::vector<SeedItem> &items) {
        std::vector<sa_pair> ip(items.size());
        for (size_t k = 0; k < ip.size(); ++k) ip[k] = sa_pair{0, items[k].n, 0, items[k].m};
        return ip;
    };
    const std::vector<sa_pair> ep = as_pairs(ci.ends), gp = as_pairs(ci.gaps);
    if (int rc = make_score_plan(P, ext, ep.data(), (int64_t)ep.size(), num_cu, kn, &out->ends, err)) return rc;
    out->ends.spec.seeded = out->ends.spec.chained = true;
    // gap open == gap extend is the linear recurrence of that penalty: the linear items instances
    sa_params gparams = *P;
    WaveSpec gspec = WaveSpec::gaps(spec.gap_open, spec.gap_extend);
    gspec.traced = spec.traced;
    if (!spec.traced && spec.gap_open == spec.gap_extend)
    {
        gparams.gap_penalty = spec.gap_open;
        gspec = WaveSpec();
    }
    if (int rc = make_score_plan(&gparams, gspec, gp.data(), (int64_t)gp.size(), num_cu, kn, &out->gaps, err)) return rc;
    out->gaps.spec.seeded = true;
    out->device_bytes = whole.input_bytes + (out->ends.device_bytes - out->ends.input_bytes) + (out->gaps.device_bytes - out->gaps.input_bytes) +
                        (uint64_t)(ep.size() + gp.size()) * (sizeof(SeedItem) - 24) + (uint64_t)ci.seeds.size() * sizeof(ChainSeed) +
                        (uint64_t)np * (sizeof(ChainPair) + sizeof(sa_seed_result));
    out->ends.input_bytes = whole.input_bytes;
    return SA_OK;
}

}  // namespace sa
