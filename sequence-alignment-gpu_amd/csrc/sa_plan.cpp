// The host planner (sa_plan.h): one function per decision, in the order the decisions depend on each
// other: limits, R, score kind, strip layout, pair packing, bands, chain_solo, traceback groups,
// launch geometry. Host-only C++14, no HIP.
#include "sa_plan.h"

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>

namespace sa {

const Knobs &knobs()
{
    static const Knobs k = [] {
        Knobs v;
        auto get = [](const char *name) -> const char * { return std::getenv(name); };
        v.debug_sync = get("SA_DEBUG_SYNC") != nullptr;
        if (const char *e = get("SA_ROWS_PER_LANE")) v.rows_per_lane = std::atoi(e);
        if (const char *e = get("SA_WAVES_PER_GROUP")) v.waves_per_group = std::atoi(e);
        v.no_pair16 = get("SA_NO_PAIR16") != nullptr;
        if (const char *e = get("SA_BAND")) v.band = std::atoi(e) != 0 ? 1 : 0;
        if (const char *e = get("SA_BAND_R")) v.band_r = std::atoi(e) == 3 ? 3 : 2;
        if (const char *e = get("SA_HANDOFF_TIMEOUT_S")) v.handoff_timeout_s = std::atof(e);
        if (const char *e = get("SA_IO_SLEEP")) v.io_sleep = std::max(0, std::atoi(e));
        if (const char *e = get("SA_CHAIN_LDS_KB")) v.chain_lds_kb = std::max(0, std::atoi(e));
        v.timeline = get("SA_TIMELINE");
        v.tb_timing = get("SA_TB_TIMING");
        v.tb_table_timing = get("SA_TB_TABLE_TIMING");
        v.tb_generic = get("SA_TB_GENERIC") != nullptr;
        if (const char *e = get("SA_TB_STAGER")) v.tb_stager = std::atoi(e) != 0;
        if (const char *e = get("SA_TB_TABLES")) v.tb_tables = std::atoi(e) != 0;
        v.tb_strict = get("SA_TB_STRICT") != nullptr;
        if (const char *e = get("SA_TB_ROUNDS")) v.tb_rounds = std::max(0, std::atoi(e));
        if (const char *e = get("SA_MAX_CUS")) v.max_cus = std::max(0, std::atoi(e));
        if (const char *e = get("SA_CHAIN_PER_CU")) v.chain_per_cu = std::min(2, std::max(0, std::atoi(e)));
        if (const char *e = get("SA_BAND_ROWS")) v.band_rows = std::max(0LL, std::atoll(e));
        if (const char *e = get("SA_PAIR_CHAIN_R")) v.pair_chain_r = std::atoi(e) == 4 ? 4 : 8;
        if (const char *e = get("SA_TB_CAP")) v.tb_cap = std::max(0, std::atoi(e));
        if (const char *e = get("SA_TB_WIDE")) v.tb_wide = std::atoi(e) != 0;
        if (const char *e = get("SA_STAGE_KERNEL")) v.stage_kernel = std::atoi(e) != 0;
        if (const char *e = get("SA_ALIGN")) v.align = std::min(2, std::max(0, std::atoi(e)));
        return v;
    }();
    return k;
}

namespace {

// band fill with persistent workers up to this many rows (DNA-sized alphabets / larger ones); past
// them the one-wave fill with one workgroup per CU is ahead (profiles/r05/ab_chain_per_cu_v0.log, ab_chain_solo_v1.log)
constexpr int64_t kBandPersistRows = 90112, kBandPersistRowsWide = 65536;

int bitlen(uint64_t v)
{
    int b = 0;
    while (v) { ++b; v >>= 1; }
    return b;
}

int64_t longest_pattern(const Plan &pl)
{
    int64_t mmax = 0;
    for (const PairDesc &d : pl.pairs) mmax = std::max<int64_t>(mmax, (int64_t)d.pattern_len);
    return mmax;
}

// ---- limits ----
// What the score matrix and the pair shapes bound: the largest |S| and the largest local H.
struct Limits {
    int64_t smax = INT32_MIN, sabs = 0;
    uint64_t hmax_local = 0;
    int key_rowbits = 1;
};

// Numeric limits of the engine: every intermediate fits in int32, local keys fit.
int check_limits(const sa_params *P, const sa_pair *pairs, int64_t np, Limits *L, std::string *err)
{
    const int A = P->alphabet_size;
    // any int gap penalty, as the reference's CLI (std::stoi, utilities.cpp:188-199) and its fill
    // (alignSequenceCPU.cpp:175-176, 259-260) take it; the range bound below rejects what int32 cannot hold
    const int64_t g = P->gap_penalty;
    for (int e = 0; e < A * A; ++e)
    {
        L->smax = std::max<int64_t>(L->smax, P->score_matrix[e]);
        L->sabs = std::max<int64_t>(L->sabs, std::llabs((long long)P->score_matrix[e]));
    }
    uint64_t lmax = 0;
    for (int64_t p = 0; p < np; ++p)
    {
        const uint64_t n = pairs[p].text_len, m = pairs[p].pattern_len;
        if (n >= (1u << 24) - 1 || m >= (1u << 24) - 1)
        {
            *err = "sequence longer than 2^24-2 letters";
            return SA_ERR_UNSUPPORTED;
        }
        lmax = std::max(lmax, std::max(n, m));
        const uint64_t span = n + m;
        const uint64_t bound = ((uint64_t)L->sabs + (uint64_t)std::llabs(g)) * span + (uint64_t)std::llabs(g) * span;
        if (bound >= (1ull << 30))
        {
            *err = "scores may exceed the int32 range";
            return SA_ERR_UNSUPPORTED;
        }
        const uint64_t h = g >= 0 ? (uint64_t)std::max<int64_t>(L->smax, 0) * std::min(n, m)
                                  : ((uint64_t)L->sabs + (uint64_t)(-g)) * span;
        L->hmax_local = std::max(L->hmax_local, h);
    }
    // local best-cell keys: H | ~row | ~col in 64 bits, row / column fields sized for the longest
    // sequence; the in-kernel block key (H << key_bits) + step must stay inside int32
    L->key_rowbits = std::max(1, bitlen(lmax + 1));
    if (P->mode == SA_LOCAL && (bitlen(L->hmax_local) > 26 || bitlen(L->hmax_local) > 64 - 2 * L->key_rowbits))
    {
        *err = "local scores may exceed the best-cell key range";
        return SA_ERR_UNSUPPORTED;
    }
    return SA_OK;
}

// ---- R ----
// Whether the pairs can run pair-packed (fill_pair_kernel / fill_pair_chain_kernel), whatever R:
// global, an even number of pairs of one shape, a DNA-sized alphabet, every S + 2g in [0, 255] and
// every shifted-domain value within u16 (65534 at most: chains mark unpublished LDS entries with
// 0xffffffff, see sa_fill.hip)
bool pair_packable(const sa_params *P, const sa_pair *pairs, int64_t np, const Knobs &kn)
{
    const int A = P->alphabet_size;
    const int64_t g = P->gap_penalty;
    if (P->mode != SA_GLOBAL || np < 2 || np % 2 != 0 || A > 4 || g <= 0 || kn.no_pair16) return false;
    int64_t smaxp = 0;
    for (int e = 0; e < A * A; ++e)
    {
        const int64_t v = P->score_matrix[e] + 2 * g;
        if (v < 0 || v > 255) return false;
        smaxp = std::max(smaxp, v);
    }
    for (int64_t p = 0; p < np; ++p)
        if (pairs[p].text_len != pairs[0].text_len || pairs[p].pattern_len != pairs[0].pattern_len)
            return false;
    const uint64_t n = pairs[0].text_len, m = pairs[0].pattern_len;
    return n > 0 && m > 0 && (uint64_t)smaxp * std::min(n, m) <= 65534;
}

// The pair-chain question: whether pair-packed pairs of S strips each over texts of n letters run
// as fill_pair_chain_kernel (one workgroup per couple, one wave per strip, its LDS rows within a
// CU's). `lds` = false asks for the wave count alone: that is what choose_R knows to ask today, the
// KNOWN GAP of ADVICE.md (it lowers R for chains the LDS condition then refuses; pinned by
// tests/test_plan.py, row "advice_gap").
bool pair_chain_fits(int64_t S, uint64_t n, bool lds)
{
    return S <= kPairChainMax && (!lds || (size_t)(S - 1) * pair_row_entries((int)n) * 4 <= 160 * 1024);
}

int choose_R(const sa_params *P, const sa_pair *pairs, int64_t np, int num_cu, bool packable, const Knobs &kn)
{
    int R = P->rows_per_lane;
    if (kn.rows_per_lane) R = kn.rows_per_lane;
    if (R == 1 || R == 2 || R == 4 || R == 8 || R == 16 || R == 32) return R;
    // few long pairs: the shortest strips keep the wavefront deepest (one row per lane)
    if (np < 256) return 1;
    uint64_t mmax = 0;
    for (int64_t p = 0; p < np; ++p) mmax = std::max<uint64_t>(mmax, pairs[p].pattern_len);
    // many independent pairs: one strip per pair where possible (no hand-offs at all); local
    // mode keeps 3 registers per row (H, G, best key) and stops at 16 rows per lane, where
    // its working set still fits the register file
    const int rmax = P->mode == SA_LOCAL ? 16 : 32;
    int r = 1;
    while (r < rmax && (uint64_t)kWave * r < mmax) r <<= 1;
    if (packable)
    {
        // size the plan to the GPU: a couple of pairs is one wave per strip, and a batch with
        // fewer waves than SIMDs (a shard of the batch on one of N GPUs) leaves SIMDs idle, its
        // time set by one wave's n + 64 steps of R rows. Strips of 8 rows per lane chained in LDS
        // (fill_pair_chain_kernel) split each couple over up to kPairChainMax waves. Measured on
        // config 5's shards (profiles/r06/shard_sweep_v1.log): 1024 pairs 0.86 ms at R = 8 against
        // 1.22 at 16 and 1.24 at 32; 512 pairs 0.52 / 0.73 / 1.19; 2048 pairs (one wave per SIMD
        // at R = 32) 1.44 at 32 against 1.50 at 8 and 1.82 at 16: chains of two R = 16 strips never
        // pay, so the choice is one strip per pair or R = 8 chains.
        const int64_t simds = 4 * (int64_t)std::max(1, num_cu);
        const int rc = kn.pair_chain_r > 0 ? kn.pair_chain_r : 8;
        const int64_t stripsC = (int64_t)((mmax + kWave * rc - 1) / (kWave * rc));
        if ((np / 2) * (int64_t)((mmax + kWave * r - 1) / (kWave * r)) < simds && r > rc &&
            pair_chain_fits(stripsC, pairs[0].text_len, false))
            r = rc;
    }
    return r;
}

// ---- score kind ----
int choose_score_kind(const sa_params *P, int R, int64_t sabs)
{
    const int A = P->alphabet_size;
    const int64_t g = P->gap_penalty;
    // the tables hold S + 2g (global, shifted domain) or S + g (local), see run_body
    const int64_t off2 = P->mode == SA_GLOBAL ? 2 * g : g;
    bool fits8 = true;
    for (int e = 0; e < A * A; ++e)
    {
        const int64_t v = P->score_matrix[e] + off2;
        if (v < -128 || v > 127) fits8 = false;
    }
    // kArr8's hand-scheduled bodies keep the direction differences in bytes (sa_fill_steps.inc): every
    // |M - D|, |left - up| is at most 2 (|S| + 2|g|) (global, shifted domain: every boundary is 0 and
    // adjacent cells differ by at most max(S + 2g, 0)) or 2 (|S| + |g|) + |g| (local, g >= 0), below
    // 4 (max|S| + |g|). Local with g < 0 has no such bound: H(i, 1) grows like -g * i next to the
    // column-0 zeros, so M - D at column 1 (and row 1) leaves the byte range.
    const bool byte_diffs = 4 * (sabs + std::llabs(g)) <= 127 && !(P->mode == SA_LOCAL && g < 0);
    if (R == 1) return fits8 && byte_diffs ? kArr8 : kArr;
    return (A <= 4 && fits8) ? kProf : kTable;
}

// ---- strip layout ----
// The pairs' descriptors and one strip per 64 R rows, each strip handing its bottom row to the next
// through granules; the sizes the buffer table needs. (Reads pl.mode, A, R, U, sk.)
void layout_strips(const sa_pair *pairs, int64_t np, Plan &pl)
{
    const int A = pl.A, R = pl.R, U = pl.U, RB = kWave * R;
    // (a possible pair-packed plan, decided next, needs two column profiles per column)
    const bool maybePair = pl.mode == SA_GLOBAL && R >= 4 && A <= 4;
    pl.pairs.resize(np);
    for (int64_t p = 0; p < np; ++p)
    {
        PairDesc &d = pl.pairs[p];
        d.text_off = pairs[p].text_offset;
        d.text_len = pairs[p].text_len;
        d.pattern_off = pairs[p].pattern_offset;
        d.pattern_len = pairs[p].pattern_len;
        d.code_off = pl.code_bytes;
        // kArr8: code_len bytes per copy (4A copies); kArr: A arrays of code_len dwords; else one
        d.code_len = (kPad + d.text_len + 4 * kPad + 3) / 4 * 4;
        pl.code_bytes += pl.sk == kArr8 || pl.sk == kArr ? (uint64_t)A * d.code_len : (maybePair ? 2 : 1) * d.code_len;
        d.out_off = pl.out_bytes;
        pl.out_bytes += d.text_len + d.pattern_len + 16;
        d.rec_off = pl.rec_words;
        pl.rec_words += std::max(d.text_len, d.pattern_len) + 64;
        d.first_strip = (int32_t)pl.strips.size();
        const uint64_t n = d.text_len, m = d.pattern_len;
        const int ns = (n == 0 || m == 0) ? 0 : (int)((m + RB - 1) / RB);
        d.num_strips = ns;
        pl.chain = pl.chain || ns > 1;
        // n + 63 steps reach column n in lane 63; one more step moves its bottom-row value into the
        // publishing register (sa_fill.hip run_body); two bodies per loop trip
        const int nsteps = (int)(((n + kWave) + 2 * U - 1) / (2 * U) * (2 * U));
        for (int b = 0; b < ns; ++b)
        {
            StripDesc s;
            s.pair = (int32_t)p;
            s.row0 = 1 + b * RB;
            s.flags = (b > 0 ? kHasPrev : 0) | (b + 1 < ns ? kHasNext : 0);
            s.nsteps = nsteps;
            s.mask_off = pl.mask_entries;
            pl.mask_entries += (uint64_t)nsteps * R;
            s.bnd_in = b > 0 ? pl.strips.back().bnd_out : 0;
            s.bnd_out = pl.granules;
            if (b + 1 < ns) pl.granules += n + 8;
            pl.strips.push_back(s);
        }
    }
}

// Waves per workgroup (strips per group). Chains of strips (pairs taller than one strip) hand
// their rows off through LDS inside a group; single-strip pairs gain nothing from grouping.
int choose_W(const Knobs &kn)
{
    const int w = kn.waves_per_group;
    return w >= 1 && w <= kMaxWaves ? w : 4;
}

// ---- pair packing ----
// pair-packed fill: global, pairs of one shape, DNA-sized alphabet, every S + 2g in [0, 255]
// and every value within u16 (see process_pair). Lone strips: fill_pair_kernel; chains of up
// to kPairChainMax strips per pair (every pair the same count): fill_pair_chain_kernel
bool choose_pair_packing(const Plan &pl, bool packable)
{
    if (pl.R < 4 || !packable) return false;
    return !pl.chain || pair_chain_fits(pl.pairs[0].num_strips, pl.pairs[0].text_len, true);
}

// ---- bands ----
// The band fill (sa_fill.hip process_band): R = 1 chains with int8 text profiles (global, or local
// with g >= 0, which kArr8 implies), and the band groups plus the strip groups fit one workgroup per
// CU (or run as persistent workers, fill_launch). A band is BR rows per lane (64 BR rows), the strips
// below run in groups of SW, a multiple of BR, so that a group boundary inside a pair falls on a band
// boundary: every pair's first strip a multiple of BR.
//   BR = 2: 128-row bands, strip groups of W (W even);
//   BR = 3: 192-row bands, strip groups of three: every band feeds exactly one strip group (no
//           granule is written for nothing) and the chain has a third fewer hand-offs at 8 VALU per
//           band step instead of 6 (process_band3). DNA-sized alphabets reading
//           the four byte copies only (the kernels that exist); the default for plans whose groups
//           are all resident (32768^2: global +6.8 %, local +6.3 %, 8192^2 global +7.6 % in same-box
//           A/Bs, profiles/r07), with persistent workers behind SA_BAND_R=3 (not measured).
struct BandPlan {
    std::vector<StripDesc> bands, strips;  // the band descriptors; the strips with their final flags, bnd_in, bnd_out
    uint64_t granules = 0;
};

// The band plan of pl's strips for bands of BR rows per lane over strip groups of SW, or false when
// that height does not apply.
bool plan_bands(const Plan &pl, int BR, int SW, bool residentOnly, const Knobs &kn, BandPlan *out)
{
    bool band = kn.band != 0 && pl.R == 1 && pl.sk == kArr8 && pl.chain;
    int64_t nb = 0;
    for (const PairDesc &d : pl.pairs)
    {
        band = band && (d.num_strips == 0 || d.first_strip % BR == 0);
        nb += std::max(0, (d.num_strips + BR - 1) / BR - 1);
    }
    const int64_t stripGroups = ((int64_t)pl.strips.size() + SW - 1) / SW;
    const int64_t bandGroups = (nb + pl.W - 1) / pl.W;
    // every group in flight at once, or (persistent band and strip workgroups, FillArgs::band_wgs)
    // chains up to kBandPersistRows rows: past them the fill is throughput-bound and the bands' work
    // on top of the strips' costs more than their shorter ramp saves
    const bool resident = stripGroups + bandGroups <= pl.num_cu;
    const int64_t persistRows = kn.band_rows > 0 ? kn.band_rows : (pl.A <= 4 ? kBandPersistRows : kBandPersistRowsWide);
    band = band && nb > 0 &&
           (resident || (!residentOnly && (longest_pattern(pl) <= persistRows || kn.band == 1) && pl.num_cu >= 4));
    if (!band) return false;
    // bands b = 0 .. B-2 of each pair (B = ceil(strips / BR); the last band's bottom row feeds
    // nothing); every band publishes its bottom row to granules. The strips keep their planes;
    // a strip at a group start takes its feed from the granules of the band above, the others
    // from the strip above through the group's rings, and a group's last strip publishes nothing.
    out->strips = pl.strips;
    for (const PairDesc &d : pl.pairs)
    {
        const uint64_t n = d.text_len;
        const int B = (d.num_strips + BR - 1) / BR;
        const int64_t fb = (int64_t)out->bands.size();
        for (int b = 0; b + 1 < B; ++b)
        {
            StripDesc bd = pl.strips[d.first_strip + BR * b];
            bd.row0 = 1 + b * BR * kWave;
            bd.flags = (b > 0 ? kHasPrev : 0) | kHasNext;
            bd.mask_off = 0;
            bd.bnd_in = b > 0 ? out->bands.back().bnd_out : 0;
            bd.bnd_out = out->granules;
            out->granules += n + 8;
            out->bands.push_back(bd);
        }
        for (int k = 0; k < d.num_strips; ++k)
        {
            StripDesc &sd = out->strips[d.first_strip + k];
            const int i = d.first_strip + k;
            if (k + 1 < d.num_strips && (i + 1) % SW == 0) sd.flags &= ~kHasNext;
            sd.bnd_out = 0;
            sd.bnd_in = (k > 0 && i % SW == 0) ? out->bands[fb + k / BR - 1].bnd_out : 0;
        }
    }
    return true;
}

// Chains of protein-sized alphabets read copy 0 of their text profiles (the kArr8A launch selector,
// sa_fill.h): SA_ALIGN above 0 for alphabets larger than 4, above 1 for the others.
bool reads_copy0(const Plan &pl, const Knobs &kn) { return kn.align > (pl.A > 4 ? 0 : 1); }

// Three-row bands where they apply (kArr8A plans have no three-row kernels), then two-row bands,
// then the one-wave fill.
void choose_bands(Plan &pl, const Knobs &kn)
{
    BandPlan bp;
    const bool three = pl.A <= 4 && !reads_copy0(pl, kn) && pl.W >= 2 && kn.band_r != 2;
    if (three && plan_bands(pl, 3, 3, kn.band_r != 3, kn, &bp))
    {
        pl.band_r = 3;
        pl.strip_w = 3;
    }
    else if (pl.W % 2 == 0 && plan_bands(pl, 2, pl.W, false, kn, &bp))
    {
        pl.band_r = 2;
        pl.strip_w = pl.W;
    }
    else return;
    pl.band = true;
    pl.bands = std::move(bp.bands);
    pl.strips = std::move(bp.strips);
    pl.granules = bp.granules;
}

// ---- chain_solo ----
// one-wave chain fill: a second workgroup on a CU puts two compute waves on a SIMD, which
// raises the step time 25 -> 41 ns and the hand-off lag 2.5 -> 4.6 us (tools/timeline.py,
// 120000^2); the strip chains of a few long pairs are latency-bound (a strip starts one lag
// after the one above), so they get one workgroup per CU; many chained pairs keep two
bool choose_chain_solo(const Plan &pl, const Knobs &kn)
{
    if (!pl.chain || pl.band) return false;
    if (kn.chain_per_cu) return kn.chain_per_cu == 1;
    int64_t chained = 0;
    for (const PairDesc &d : pl.pairs) chained += d.num_strips > 1;
    return chained < pl.num_cu;
}

// ---- tables ----
void build_tables(const sa_params *P, Plan &pl)
{
    const int A = pl.A;
    const int64_t off2 = pl.mode == SA_GLOBAL ? 2 * (int64_t)pl.gap : pl.gap;  // (choose_score_kind)
    pl.h_prof.assign(4, 0);
    pl.h_table.resize(A * A);
    for (int e = 0; e < A * A; ++e) pl.h_table[e] = (int32_t)(P->score_matrix[e] + off2);
    if (pl.sk == kProf || pl.sk == kPair)
        for (int cp = 0; cp < A; ++cp)
        {
            uint32_t w = 0;
            for (int ct = 0; ct < A; ++ct) w |= (uint32_t)(pl.h_table[cp * A + ct] & 0xff) << (8 * ct);
            pl.h_prof[cp] = (int32_t)w;
        }
}

// ---- table traceback groups (sa_walk.h) ----
void plan_traceback(Plan &pl, const Knobs &kn)
{
    const int64_t np = (int64_t)pl.pairs.size();
    if (pl.R == 1 && kn.tb_tables)
    {
        pl.tb_pg.assign(np + 1, 0);
        for (int64_t p = 0; p < np; ++p)
        {
            const PairDesc &d = pl.pairs[p];
            pl.tb_pg[p] = (int32_t)pl.tb_groups.size();
            if (d.num_strips < kTbMinStrips || d.text_len == 0) continue;
            // strip tables only for the strips of pairs with groups (slot tbl0 + s - s_lo)
            for (int s = 0; s < d.num_strips; s += kTbG)
                pl.tb_groups.push_back({(int32_t)p, d.first_strip + s, d.first_strip + std::min(d.num_strips, s + kTbG) - 1,
                                        (int32_t)pl.tb_slots + s});
            pl.tb_slots += d.num_strips;
        }
        pl.tb_pg[np] = (int32_t)pl.tb_groups.size();
        if (pl.tb_groups.empty()) pl.tb_pg.clear();
    }
    for (const PairDesc &d : pl.pairs)
        pl.max_recs = std::max<int64_t>(pl.max_recs, (int64_t)(pl.R == 1 ? d.pattern_len : d.text_len));
}

// ---- launch geometry ----
FillLaunch fill_launch(const Plan &pl, const Knobs &kn)
{
    FillLaunch a;
    const int ns = (int)pl.strips.size(), cus = std::max(1, pl.num_cu);
    a.sk = pl.sk;
    if (ns == 0) return a;
    // (the pair-packed kernel always runs kPairWaves waves per workgroup)
    const int W = pl.sk == kPair ? kPairWaves : pl.W;
    a.W = W;
    a.num_groups = (ns + W - 1) / W;
    // chains: two workgroups of W compute waves + an I/O wave per CU; lone strips: W compute
    // waves per workgroup and up to 16 waves per CU (the batch kernel stays under 128 VGPRs)
    const int perCU = pl.chain ? std::max(1, 8 / W) : std::max(1, 16 / W);
    a.grid = std::min(a.num_groups, cus * perCU);
    if (pl.sk == kPair)
    {
        // one wave per two strips
        const int units = ns / 2;
        a.num_groups = (units + W - 1) / W;
        a.grid = std::min(a.num_groups, cus * std::max(1, 8 / W));
    }
    if (pl.sk == kPair && pl.chain)
    {
        // pair-packed chains: one workgroup per couple of pairs, one wave per strip of the couple
        a.W = pl.pairs[0].num_strips;
        a.num_groups = ns / 2 / pl.pairs[0].num_strips;
        a.pair_text_len = (int32_t)pl.pairs[0].text_len;
        a.grid = a.num_groups;
    }
    else if (pl.chain_solo)
    {
        // (choose_chain_solo) an LDS request above half a CU's keeps a second workgroup off the CU
        a.chain_lds = 96 * 1024;
        a.grid = std::min(a.num_groups, cus);
    }
    if (pl.band)
    {
        // (three-row bands: strip groups of three, the band groups keep W)
        a.strip_w = pl.strip_w;
        a.num_groups = (ns + pl.strip_w - 1) / pl.strip_w;
        // band groups on the first workgroups, strip groups on the rest, one workgroup per CU (the
        // LDS request is above half a CU's) and every group in flight at once (plan_bands checked
        // that they fit): a strip group waits only for bands, which never wait for strips
        a.num_bands = (int32_t)pl.bands.size();
        a.num_band_groups = (a.num_bands + W - 1) / W;
        a.band_wgs = a.num_band_groups;
        a.chain_lds = 96 * 1024;
        a.grid = a.num_band_groups + a.num_groups;
        if (a.grid > pl.num_cu)
        {
            // more groups than CUs: persistent workers, each taking groups from its queue in chain
            // order until it is empty (a group waits only for groups dequeued before it, so every
            // worker count makes progress); the split that a model of the band and strip chains
            //  puts ahead for 65536^2 .. 120000^2 is about 0.31 of the CUs to bands
            a.band_wgs = std::max(1, std::min(a.num_band_groups, (int)(0.31 * pl.num_cu + 0.5)));
            a.grid = a.band_wgs + std::max(1, std::min(a.num_groups, pl.num_cu - a.band_wgs));
        }
        a.band3 = pl.band_r == 3;
    }
    if (pl.sk == kArr8 && pl.chain && reads_copy0(pl, kn)) a.sk = kArr8A;
    return a;
}

}  // namespace

int make_plan(const sa_params *P, const sa_pair *pairs, int64_t np, int num_cu, const Knobs &kn, Plan *out,
              std::string *err)
{
    auto fail = [&](int code, const char *msg) {
        *err = msg;
        return code;
    };
    if (!P || !out || np < 0 || (np > 0 && !pairs) || !P->score_matrix)
        return fail(SA_ERR_INVALID, "sa_plan_create: null argument");
    const int A = P->alphabet_size;
    if (A < 1 || A > 32) return fail(SA_ERR_INVALID, "alphabet_size must be 1..32");
    if (P->mode == SA_FIT) return fail(SA_ERR_UNSUPPORTED, kFitUnsupported);
    if (P->mode >= SA_ENDS_FREE && P->mode <= SA_OVERLAP) return fail(SA_ERR_UNSUPPORTED, kEndsUnsupported);
    if (P->mode != SA_GLOBAL && P->mode != SA_LOCAL) return fail(SA_ERR_INVALID, "mode must be SA_GLOBAL or SA_LOCAL");
    Limits lim;
    if (int rc = check_limits(P, pairs, np, &lim, err)) return rc;

    Plan &pl = *out;
    pl = Plan();
    pl.mode = P->mode;
    pl.A = A;
    pl.gap = (int)P->gap_penalty;
    pl.num_cu = kn.max_cus > 0 ? std::min(num_cu, kn.max_cus) : num_cu;
    pl.key_bits = std::min(12, std::max(4, 30 - bitlen(lim.hmax_local)));
    pl.key_rowbits = lim.key_rowbits;
    if (P->alphabet) std::memcpy(pl.alphabet, P->alphabet, std::min<size_t>(A + 1, 33));
    else for (int c = 0; c <= A; ++c) pl.alphabet[c] = c == A ? '-' : (char)('A' + c);

    const bool packable = pair_packable(P, pairs, np, kn);
    pl.R = choose_R(P, pairs, np, pl.num_cu, packable, kn);
    pl.U = chunk_geom(pl.R).U;
    pl.sk = choose_score_kind(P, pl.R, lim.sabs);
    layout_strips(pairs, np, pl);
    if (pl.strips.size() >= (1u << 31)) return fail(SA_ERR_UNSUPPORTED, "too many strips");
    pl.W = choose_W(kn);
    if (choose_pair_packing(pl, packable))
    {
        pl.sk = kPair;
        pl.granules = 0;  // (the chains hand their rows off in LDS: no granules)
    }
    choose_bands(pl, kn);
    pl.chain_solo = choose_chain_solo(pl, kn);
    build_tables(P, pl);
    plan_traceback(pl, kn);
    pl.launch = fill_launch(pl, kn);
    return SA_OK;
}

}  // namespace sa
