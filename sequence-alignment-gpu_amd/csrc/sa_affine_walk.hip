// Alignments under affine gap penalties (sa_hip.h: sa_align_pairs_affine; sa_search_affine in
// sa_score.hip): the traced instances of wave_kernel (sa_score_wave.h, kWaveTrace: four direction bits
// per cell; affine, R = 8), launched through the table of sa_wave_launch.h, walk_affine_kernel, the
// traceback over the three Gotoh states, and the host side that runs both chunk by chunk of the work
// order. What is run is decided in sa_trace_plan.cpp (host only, no HIP). DESIGN.md §3.5 has the nibble,
// the walk and its tie rules.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "sa_affine.h"
#include "sa_cigar.h"
#include "sa_hip.h"
#include "sa_host.h"
#include "sa_score_wave.h"
#include "sa_trace_plan.h"
#include "sa_wave_launch.h"

namespace sa {

struct WalkArgs {
    const int8_t *text, *pattern;
    const ScorePair *pairs;
    const int32_t *order;             // the chunk's part of the work order: workgroup w walks pair order[w]
    const sa_score_result *scores;    // the fill's score and end cell of every pair
    const uint32_t *dirs;             // the chunk's direction arena
    const uint64_t *dir_off;          // per pair, in words
    const uint64_t *slot_off;         // per pair: its text_len + pattern_len bytes in each string arena
    char *out_text, *out_pattern;     // both null: results only, no letters are loaded or written
    const char *alphabet;             // A letters and the gap letter
    sa_result *results;
    int32_t A, mode;                  // mode: one of sa_mode, or SA_ENDS_FREE with its flags
    int32_t band;                     // the half-width of a banded fill, or -1; after a banded extension's fill, its width
    const Band *bands;                // after a band-at fill: every pair's band, clipped; else null
};

// One wave per pair; the walk of DESIGN.md §3.5: oracle_align's loop (oracle/sa_oracle.c) with a
// state in {H, E, F}. The position, the state and the counters are wave-uniform. The direction word
// of cell (i, j) lies at step j - 1 + lane of lane ((i - 1) % 512) / 8 of strip (i - 1) / 512, and a
// move stays in that lane column or goes to the lane before it, to the same or an earlier step. So
// the wave fetches 64 consecutive steps of the current lane column in one load (lane k: step t - k)
// and reads them with v_readlane until the path leaves the column or the window: about
// m / 8 + (m + n) / 64 dependent loads per alignment. The letters are not loaded on the path either:
// lane (len % 64) notes the cell and the direction of each emission, and every 64 emissions the wave
// loads the letters and writes 64 bytes per side, backwards from the end of the pair's slot.
// The loop makes at most n + m moves whatever the direction words hold; a walk that has not ended by
// then reports SA_ERR_HIP.
// SA_FIT starts at (m, end_text) as a local walk starts at its best cell, moves as a global one
// (column 0 forces TOP) and ends at row 0, where nothing forces LEFT: start_text is the column it
// arrives in, the 0-based index of the window's first text letter, and start_pattern is 0.
// SA_ENDS_FREE starts at the fill's result cell and ends at (i, j) when i == 0 && (TB || j == 0) or
// j == 0 && (PB || i == 0); until then column 0 forces TOP and row 0 forces LEFT. start_text and
// start_pattern are j and i of that cell. Global (no free begin) and fit (TB) end by the same rule. A
// walk from (i, j) makes at most i + j moves, so the bound of n + m holds from any start cell.
// After a banded fill (band >= 0) the words of strip s are those of its window's steps, 64 b0(s) ..
// 64 b1(s) - 1, and the strips follow one another (trace_band_strip_words): the walk keeps the strip it
// is in, that strip's first word and first step, counts up to the start cell's strip once and steps
// back one strip at a time from there, as its rows only fall. A move to an out-of-band cell ends the
// walk with SA_ERR_HIP. It cannot happen: H of an in-band cell takes E (F) only when that is a real
// score, which needs a real H or E to the left (H or F above), that is, an in-band cell there; the
// sentinel-derived values lose every maximum under the planner's limit (sa_score_wave.h, BAND).
// BANDED is a template flag so that the unbanded walk pays for none of this: 0 no band, 1 the band of
// the half-width, 2 a band-at fill. There the pair's band is read from `bands`, every mode walks (the
// start cell and the stop rule of fit and ends-free as in the unbanded walk), and a strip without an
// in-band cell holds no words (trace_band_at_strip_words is 0), so counting up to the start cell's strip
// and stepping back pass over it; the walk reads words of in-band interior cells only, whose strips
// have a window. The argument above holds for any band: on a border the walk only moves where the stop
// rule has not ended it, that is, along a border that costs, and the planner admits a pair whose
// in-band cells of such a border reach back to an in-band origin. 3 is 2 after a banded extension's fill
// (sa_align_pairs_extend_band): the band is band_ext(n, m, width), computed as the fill computed it, and holds
// the origin, where the walk ends.
template <int BANDED>
__global__ __launch_bounds__(64) void walk_affine_kernel(WalkArgs a)
{
    const int lane = threadIdx.x;
    const int pi = uniform(a.order[blockIdx.x]);
    const ScorePair pd = a.pairs[pi];
    const int n = uniform((int)pd.n), m = uniform((int)pd.m);
    const sa_score_result sr = a.scores[pi];
    const int8_t *const text = a.text + pd.text_off;
    const int8_t *const pattern = a.pattern + pd.pattern_off;
    const uint64_t slot = uniform64(a.slot_off[pi]);
    char *const ot_end = a.out_text + slot + (uint64_t)n + (uint64_t)m;  // one past the slot's last byte
    char *const op_end = a.out_pattern + slot + (uint64_t)n + (uint64_t)m;
    const uint32_t *const dirs = a.dirs + uniform64(a.dir_off[pi]);
    const uint32_t strip_words = (uint32_t)((n + 126) / 64) * (64u * 64u);
    const bool local = a.mode == SA_LOCAL, fit = a.mode == SA_FIT, ends = BANDED != 1 && (a.mode & SA_ENDS_FREE) != 0;
    const bool tbegin = fit || (ends && (a.mode & SA_FREE_TEXT_BEGIN)), pbegin = ends && (a.mode & SA_FREE_PATTERN_BEGIN);
    const int A = a.A;
    constexpr bool banded = BANDED != 0, bat = BANDED >= 2;
    Band bd;
    if constexpr (BANDED == 3) bd = band_ext(n, m, a.band);
    else if constexpr (bat)
    {
        bd = a.bands[pi];
        bd = Band{uniform(bd.lo), uniform(bd.hi)};
    }
    else bd = band_of(n, m, banded ? a.band : 0);
    int bstrip = -1, bstep0 = 0;  // banded: the strip whose base is held, and its window's first step
    int bsteps = INT32_MAX;       // and the number of its steps: no word is read outside the window
    uint64_t bbase = 0;           // its first word

    int i = local || ends ? min(uniform((int)sr.end_pattern), m) : m;
    int j = local || fit || ends ? min(uniform((int)sr.end_text), n) : n;
    int ti = j - 1, pj = i - 1;  // the reference's text and pattern indices
    int state = kDirDiag;        // H; kDirLeft: inside a run of E, kDirTop: of F
    int len = 0;
    bool ended = false;
    int cur = -1, t0 = 0;        // the window: lane column (i - 1) / 8 and its newest step
    uint32_t win = 0;
    int ri = 0, rj = 0, rd = 0;  // lane len % 64: the cell and the direction of emission len

    // emissions base .. base + count - 1, one per lane, to bytes end - 1 - (base + lane)
    const bool strings = a.out_text != nullptr;
    auto flush = [&](int base, int count) {
        if (strings && lane < count)
        {
            const bool tt = rd == kDirDiag || rd == kDirLeft, tp = rd == kDirDiag || rd == kDirTop;
            const int ct = tt ? min(max((int)text[rj - 1], 0), A - 1) : A;
            const int cp = tp ? min(max((int)pattern[ri - 1], 0), A - 1) : A;
            ot_end[-1 - (int64_t)(base + lane)] = a.alphabet[ct];
            op_end[-1 - (int64_t)(base + lane)] = a.alphabet[cp];
        }
    };

    const int max_moves = n + m;
    for (int it = 0;; ++it)
    {
        bool stop;
        if constexpr (BANDED == 1) stop = local ? (i == 0 || j == 0) : fit ? i == 0 : (i == 0 && j == 0);  // the planner admits no free ends
        else stop = local ? (i == 0 || j == 0) : (i == 0 && (tbegin || j == 0)) || (j == 0 && (pbegin || i == 0));
        if (stop)
        {
            ended = true;
            break;
        }
        if (it >= max_moves) break;
        int d, next = kDirDiag;
        if (j == 0) d = kDirTop;        // global: column 0 forces TOP,
        else if (i == 0) d = kDirLeft;  // row 0 forces LEFT, whatever the state
        else
        {
            const int col = (i - 1) >> 3, l = col & 63;
            const int t = j - 1 + l;
            if (col != cur || t0 - t >= 64)
            {
                const int strip = col >> 6;
                if (banded && strip != bstrip)
                {
                    auto words = [&](int st) { return bat ? trace_band_at_strip_words(n, m, st, bd) : trace_band_strip_words(n, m, st, bd); };
                    if (bstrip < 0)
                        for (bstrip = 0; bstrip < strip; ++bstrip) bbase += words(bstrip);
                    for (; bstrip > strip; --bstrip) bbase -= words(bstrip - 1);
                    const BandWindow bw = bat ? band_window_at(n, m, (int64_t)kTraceStripRows, strip, bd)
                                              : band_window(n, m, (int64_t)kTraceStripRows, strip, bd);
                    bstep0 = 64 * bw.b0;
                    bsteps = 64 * (bw.b1 - bw.b0);
                }
                const int step = t - lane - bstep0;
                const uint64_t sbase = banded ? bbase : (uint64_t)strip * strip_words;
                win = step >= 0 && (!banded || step < bsteps) ? dirs[sbase + ((uint32_t)step * 64u + (uint32_t)l)] : 0u;
                cur = col;
                t0 = t;
            }
            const uint32_t word = (uint32_t)__builtin_amdgcn_readlane((int)win, t0 - t);
            const int nib = (int)(word >> (4 * ((i - 1) & 7))) & 15;
            d = state == kDirDiag ? (nib & 3) : state;
            if (d == kDirStop)  // only a local H cell holds it
            {
                ended = local;
                break;
            }
            if (d == kDirLeft) next = nib & kDirEExt ? kDirLeft : kDirDiag;
            if (d == kDirTop) next = nib & kDirFExt ? kDirTop : kDirDiag;
        }
        if (lane == (len & 63))
        {
            ri = i;
            rj = j;
            rd = d;
        }
        ++len;
        const int tt = d == kDirDiag || d == kDirLeft, tp = d == kDirDiag || d == kDirTop;
        j -= tt;
        i -= tp;
        state = next;
        if ((len & 63) == 0) flush(len - 64, 64);
        if (banded && (uint32_t)(j - i - bd.lo) > (uint32_t)(bd.hi - bd.lo)) break;  // out of band: not ended
        if (local && (i == 0 || j == 0))  // the reference leaves before the decrement
        {
            ended = true;
            break;
        }
        ti = ti - tt > 0 ? ti - tt : 0;
        pj = pj - tp > 0 ? pj - tp : 0;
    }
    flush(len & ~63, len & 63);
    if (fit || ends)  // no quirks: the cell the walk ended in (fit: in row 0)
    {
        ti = j;
        pj = ends ? i : 0;
    }
    if (lane == 0)
    {
        sa_result r;
        r.score = sr.score;
        r.status = ended ? SA_OK : SA_ERR_HIP;
        r.num_alignment_bytes = (uint64_t)len;
        r.start_text = (uint64_t)(int64_t)ti;
        r.start_pattern = (uint64_t)(int64_t)pj;
        a.results[pi] = r;
    }
}

struct SeedWalkArgs {
    const int8_t *text, *pattern;
    const SeedItem *items;
    const SeedPair *pairs;
    const int32_t *order;             // the chunk's part of the pair order: workgroup w walks pair order[w]
    const sa_score_result *scores;    // the fill's score and end cell of every item
    const sa_seed_result *seed_out;   // the combine's result of every pair
    const uint32_t *dirs;             // the chunk's direction arena
    const uint64_t *dir_off;          // per item, in words
    const uint64_t *slot_off;         // num_pairs + 1 entries: pair p's slot is bytes slot_off[p] .. slot_off[p + 1] - 1
    char *out_text, *out_pattern;     // both null: results only
    const char *alphabet;
    sa_result *results;
    uint64_t *tail_len;               // per pair: the bytes of the right half's piece, at the end of the slot
    int32_t A;
    int32_t width;                    // after a banded fill (walk_seeds_kernel<true>): the width of every half's band
};

// The walk of one work item, walk_affine_kernel<0>'s for an extension: from the fill's result cell to the
// origin, row 0 forcing LEFT and column 0 TOP, the direction words read through the same 64-step window.
// Letter j of the item's text is tbase[dir * (j - 1)], as the fill read it. LEFT false writes emission k to
// out[-1 - k], backwards from the end of the pair's slot, as every other walk does. LEFT true writes it to
// out[k]: the left half's matrix is that of the reversed prefixes, so its walk from the end cell to the
// origin meets the columns of the final alignment in forward order. Returns the number of emissions;
// *ended is false for a walk that did not reach the origin within n + m moves. BANDED (after a seeds fill inside
// a width) adds walk_affine_kernel<3>'s bookkeeping for the item's band, band_ext of its own shape: the strip
// whose words are held, its first word and its window's first step, and the end of a walk that leaves the band.
template <bool LEFT, bool BANDED>
__device__ __forceinline__ int seed_walk_item(const SeedWalkArgs &a, int item, char *out_t, char *out_p, bool *ended)
{
    const int lane = threadIdx.x;
    const SeedItem sd = a.items[item];
    const int n = uniform((int)sd.n), m = uniform((int)sd.m), dir = uniform(sd.dir);
    const sa_score_result sr = a.scores[item];
    const int8_t *const text = a.text + sd.text_off;
    const int8_t *const pattern = a.pattern + sd.pattern_off;
    const uint32_t *const dirs = a.dirs + uniform64(a.dir_off[item]);
    const uint32_t strip_words = (uint32_t)((n + 126) / 64) * (64u * 64u);
    const int A = a.A;
    int i = min(uniform((int)sr.end_pattern), m), j = min(uniform((int)sr.end_text), n);
    int state = kDirDiag, len = 0;
    int cur = -1, t0 = 0;
    uint32_t win = 0;
    int ri = 0, rj = 0, rd = 0;
    const Band bd = band_ext(n, m, BANDED ? a.width : 0);
    int bstrip = -1, bstep0 = 0, bsteps = INT32_MAX;
    uint64_t bbase = 0;
    const bool strings = out_t != nullptr;
    auto flush = [&](int base, int count) {
        if (strings && lane < count)
        {
            const bool tt = rd == kDirDiag || rd == kDirLeft, tp = rd == kDirDiag || rd == kDirTop;
            const int ct = tt ? min(max((int)text[(rj - 1) * dir], 0), A - 1) : A;
            const int cp = tp ? min(max((int)pattern[(ri - 1) * dir], 0), A - 1) : A;
            const int64_t at = LEFT ? (int64_t)(base + lane) : -1 - (int64_t)(base + lane);
            out_t[at] = a.alphabet[ct];
            out_p[at] = a.alphabet[cp];
        }
    };
    *ended = false;
    const int max_moves = n + m;
    for (int it = 0;; ++it)
    {
        if (i == 0 && j == 0)
        {
            *ended = true;
            break;
        }
        if (it >= max_moves) break;
        int d, next = kDirDiag;
        if (j == 0) d = kDirTop;
        else if (i == 0) d = kDirLeft;
        else
        {
            const int col = (i - 1) >> 3, l = col & 63;
            const int t = j - 1 + l;
            if (col != cur || t0 - t >= 64)
            {
                const int strip = col >> 6;
                if (BANDED && strip != bstrip)
                {
                    if (bstrip < 0)
                        for (bstrip = 0; bstrip < strip; ++bstrip) bbase += trace_band_at_strip_words(n, m, bstrip, bd);
                    for (; bstrip > strip; --bstrip) bbase -= trace_band_at_strip_words(n, m, bstrip - 1, bd);
                    const BandWindow bw = band_window_at(n, m, (int64_t)kTraceStripRows, strip, bd);
                    bstep0 = 64 * bw.b0;
                    bsteps = 64 * (bw.b1 - bw.b0);
                }
                const int step = t - lane - bstep0;
                const uint64_t sbase = BANDED ? bbase : (uint64_t)strip * strip_words;
                win = step >= 0 && (!BANDED || step < bsteps) ? dirs[sbase + ((uint32_t)step * 64u + (uint32_t)l)] : 0u;
                cur = col;
                t0 = t;
            }
            const uint32_t word = (uint32_t)__builtin_amdgcn_readlane((int)win, t0 - t);
            const int nib = (int)(word >> (4 * ((i - 1) & 7))) & 15;
            d = state == kDirDiag ? (nib & 3) : state;
            if (d == kDirStop) break;  // no extension cell holds it
            if (d == kDirLeft) next = nib & kDirEExt ? kDirLeft : kDirDiag;
            if (d == kDirTop) next = nib & kDirFExt ? kDirTop : kDirDiag;
        }
        if (lane == (len & 63))
        {
            ri = i;
            rj = j;
            rd = d;
        }
        ++len;
        j -= d == kDirDiag || d == kDirLeft;
        i -= d == kDirDiag || d == kDirTop;
        state = next;
        if ((len & 63) == 0) flush(len - 64, 64);
        if (BANDED && (uint32_t)(j - i - bd.lo) > (uint32_t)(bd.hi - bd.lo)) break;  // out of band: not ended
    }
    flush(len & ~63, len & 63);
    return len;
}

// One wave per pair: the left item's walk written forwards from the start of the pair's slot, the seed's
// letters after it, and the right item's walk written backwards from the slot's end. The three lengths
// sum to at most n + m - L, so the slot of n + m bytes holds the head piece and the tail piece apart; the
// host joins them (tail_len). The result's score and starts are the combine's.
template <bool BANDED>
__global__ __launch_bounds__(64) void walk_seeds_kernel(SeedWalkArgs a)
{
    const int lane = threadIdx.x;
    const int pi = uniform(a.order[blockIdx.x]);
    const SeedPair sp = a.pairs[pi];
    const uint64_t slot = uniform64(a.slot_off[pi]), slot_end = uniform64(a.slot_off[pi + 1]);
    const bool strings = a.out_text != nullptr;
    const int left = uniform(sp.left), right = uniform(sp.right);
    const uint64_t L = uniform64(sp.len);
    bool ok = true;
    int len_l = 0, len_r = 0;
    if (left >= 0)
    {
        bool ended;
        len_l = seed_walk_item<true, BANDED>(a, left, strings ? a.out_text + slot : nullptr, strings ? a.out_pattern + slot : nullptr, &ended);
        ok = ok && ended;
    }
    if (strings)
    {
        const int8_t *const ts = a.text + uniform64(sp.text_seed);
        const int8_t *const ps = a.pattern + uniform64(sp.pattern_seed);
        char *const ot = a.out_text + slot + (uint64_t)len_l, *const op = a.out_pattern + slot + (uint64_t)len_l;
        for (uint64_t q = (uint64_t)lane; q < L; q += kWave)
        {
            ot[q] = a.alphabet[min(max((int)ts[q], 0), a.A - 1)];
            op[q] = a.alphabet[min(max((int)ps[q], 0), a.A - 1)];
        }
    }
    if (right >= 0)
    {
        bool ended;
        len_r = seed_walk_item<false, BANDED>(a, right, strings ? a.out_text + slot_end : nullptr, strings ? a.out_pattern + slot_end : nullptr, &ended);
        ok = ok && ended;
    }
    if (lane == 0)
    {
        const sa_seed_result so = a.seed_out[pi];
        sa_result r;
        r.score = so.score;
        r.status = ok ? SA_OK : SA_ERR_HIP;
        r.num_alignment_bytes = (uint64_t)len_l + L + (uint64_t)len_r;
        r.start_text = so.begin_text;
        r.start_pattern = so.begin_pattern;
        a.results[pi] = r;
        a.tail_len[pi] = (uint64_t)len_r;
    }
}

// Chained seeds (sa_hip.h sa_align_pairs_chains). Every item of a chunk is walked at once, one wave per item:
// workgroups 0 .. num_ends - 1 walk the end items, the rest the gap items, all through seed_walk_item. A gap
// item's walk is the global walk: its fill wrote the end cell (m, n), and from there row 0 forces LEFT and column 0
// TOP down to the origin. A pair's slot of n + m bytes is cut into sub-slots: the piece that covers the text from
// ta to tb and the pattern from pa to pb has bytes slot + ta + pa .. slot + tb + pb - 1, at least as many as it can
// have columns, apart from and in the order of every other piece's. The left end writes forwards from the start
// of its sub-slot (the slot's), every other walk backwards from the end of its own; *_len takes the piece's
// length, -1 for a walk that did not end.
struct ChainWalkArgs {
    SeedWalkArgs w;                   // what seed_walk_item takes, with the end items, their scores and their dir_off
    const SeedItem *gap_items;        // the same three of the gap items
    const sa_score_result *gap_scores;
    const uint64_t *gap_dir_off;
    const ChainPair *pairs;
    const int32_t *end_order, *gap_order;  // the chunk's parts of the two work orders
    const uint64_t *slot_off;         // num_pairs + 1 entries
    int32_t *end_len, *gap_len;       // per end item, per gap item
    int32_t num_ends;                 // of the chunk
};

__global__ __launch_bounds__(64) void walk_chain_items_kernel(ChainWalkArgs a)
{
    const int lane = threadIdx.x;
    const int b = (int)blockIdx.x;
    const bool is_end = b < a.num_ends;  // wave-uniform
    SeedWalkArgs wa = a.w;
    wa.items = is_end ? a.w.items : a.gap_items;
    wa.scores = is_end ? a.w.scores : a.gap_scores;
    wa.dir_off = is_end ? a.w.dir_off : a.gap_dir_off;
    const int item = uniform(is_end ? a.end_order[b] : a.gap_order[b - a.num_ends]);
    const SeedItem sd = wa.items[item];
    const int pi = uniform(sd.pair);
    const ChainPair cp = a.pairs[pi];
    const bool strings = wa.out_text != nullptr;
    const bool left = uniform(sd.dir) < 0;
    // the first byte of a left end's sub-slot, one past the last byte of any other piece's
    uint64_t at = uniform64(a.slot_off[pi]);
    if (!left) at += (uniform64(sd.text_off) - uniform64(cp.text_base)) + (uniform64(sd.pattern_off) - uniform64(cp.pattern_base)) + sd.n + sd.m;
    char *const ot = strings ? wa.out_text + at : nullptr, *const op = strings ? wa.out_pattern + at : nullptr;
    bool ended;
    const int len = left ? seed_walk_item<true, false>(wa, item, ot, op, &ended) : seed_walk_item<false, false>(wa, item, ot, op, &ended);
    if (lane == 0) (is_end ? a.end_len : a.gap_len)[item] = ended ? len : -1;
}

struct ChainJoinArgs {
    const int8_t *text, *pattern;
    const ChainPair *pairs;
    const ChainSeed *seeds;
    const int32_t *order;             // the chunk's part of the pair order
    const sa_seed_result *seed_out;   // the combine's result of every pair
    const int32_t *end_len, *gap_len; // the walks' piece lengths
    const uint64_t *slot_off;         // num_pairs + 1 entries
    char *out_text, *out_pattern;     // both null: results only
    const char *alphabet;
    sa_result *results;
    uint64_t *tail_len;               // per pair: 0, the joined string starts at the start of the slot
    int32_t A;
};

// One wave per pair, after the walks. The pair's pieces in the order of the strings are the left end, then seed
// and gap in turn, then the right end: 2 c + 1 of them for c seeds. 64 pieces at a time, lane l takes piece
// base + l: its length (an end's or a gap item's from its walk, a seed's L, an empty-side gap's k), where its
// bytes lie (a walked piece: in its sub-slot; a seed or an empty-side gap run: nowhere yet, they are made from the
// input letters here) and, by a prefix sum over the wave, where they go. The pieces are then placed one after
// another, each by all lanes in 64-byte steps, ascending. A piece's destination is at or left of its source and
// ends at or left of the next piece's source (the sub-slots are in order and as long as their pieces), so a step
// reads only bytes that no step before it wrote, and a step's 64 loads are complete before its stores.
__global__ __launch_bounds__(64) void chain_join_kernel(ChainJoinArgs a)
{
    const int lane = threadIdx.x;
    const int pi = uniform(a.order[blockIdx.x]);
    const ChainPair cp = a.pairs[pi];
    const uint64_t slot = uniform64(a.slot_off[pi]), slot_end = uniform64(a.slot_off[pi + 1]);
    const uint64_t tbase = uniform64(cp.text_base), pbase = uniform64(cp.pattern_base);
    const int sbegin = uniform(cp.seed_begin), c = uniform(cp.seed_end) - sbegin;
    const int left = uniform(cp.left), right = uniform(cp.right);
    const int npieces = 2 * c + 1;
    const bool strings = a.out_text != nullptr;
    const int A = a.A;
    enum { kMove = 0, kSeed = 1, kTextRun = 2, kPatternRun = 3 };
    auto bcast64 = [](uint64_t v, int l) {
        return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l) | ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l) << 32);
    };
    uint64_t total = 0;
    bool ok = true;
    for (int base = 0; base < npieces; base += kWave)
    {
        const int j = base + lane;
        int len = 0, kind = kMove;
        uint64_t src = 0, toff = 0, poff = 0;  // kMove: the piece's first byte; else the arena offsets of its letters
        if (j == 0)
        {
            len = left >= 0 ? a.end_len[left] : 0;
            src = slot;
        }
        else if (j == npieces - 1)
        {
            len = right >= 0 ? a.end_len[right] : 0;
            src = slot_end - (uint64_t)max(len, 0);
        }
        else if (j < npieces)
        {
            const int i = (j - 1) >> 1;
            const ChainSeed sd = a.seeds[sbegin + i];
            if (j & 1)
            {
                kind = kSeed;
                len = (int)sd.len;
                toff = sd.text_off;
                poff = sd.pattern_off;
            }
            else
            {
                const ChainSeed nx = a.seeds[sbegin + i + 1];
                if (sd.gap >= 0)
                {
                    len = a.gap_len[sd.gap];
                    src = slot + (nx.text_off - tbase) + (nx.pattern_off - pbase) - (uint64_t)max(len, 0);
                }
                else
                {
                    // an empty side: one run of the other side's letters against gap letters
                    toff = sd.text_off + sd.len;
                    poff = sd.pattern_off + sd.len;
                    const uint64_t gn = nx.text_off - toff, gm = nx.pattern_off - poff;
                    kind = gn ? kTextRun : kPatternRun;
                    len = (int)(gn + gm);
                }
            }
        }
        ok = ok && len >= 0;
        len = max(len, 0);
        const int incl = wave_prefix_sum(len);
        const uint64_t dst = slot + total + (uint64_t)(incl - len);
        const int count = min(kWave, npieces - base);
        for (int q = 0; strings && q < count; ++q)
        {
            const int qlen = __builtin_amdgcn_readlane(len, q), qkind = __builtin_amdgcn_readlane(kind, q);
            if (qlen == 0) continue;
            const uint64_t qdst = bcast64(dst, q);
            if (qkind == kMove)
            {
                const uint64_t qsrc = bcast64(src, q);
                if (qsrc == qdst) continue;
                for (int off = lane; off - lane < qlen; off += kWave)
                {
                    char ct = 0, cq = 0;
                    if (off < qlen)
                    {
                        ct = a.out_text[qsrc + off];
                        cq = a.out_pattern[qsrc + off];
                    }
                    if (off < qlen)
                    {
                        a.out_text[qdst + off] = ct;
                        a.out_pattern[qdst + off] = cq;
                    }
                }
            }
            else
            {
                const int8_t *const ts = a.text + bcast64(toff, q);
                const int8_t *const ps = a.pattern + bcast64(poff, q);
                for (int off = lane; off < qlen; off += kWave)
                {
                    const int ct = qkind == kPatternRun ? A : min(max((int)ts[off], 0), A - 1);
                    const int cq = qkind == kTextRun ? A : min(max((int)ps[off], 0), A - 1);
                    a.out_text[qdst + off] = a.alphabet[ct];
                    a.out_pattern[qdst + off] = a.alphabet[cq];
                }
            }
        }
        total += (uint64_t)__builtin_amdgcn_readlane(incl, kWave - 1);
    }
    const bool all_ok = ballot(!ok) == 0;
    if (lane == 0)
    {
        const sa_seed_result so = a.seed_out[pi];
        sa_result r;
        r.score = so.score;
        r.status = all_ok ? SA_OK : SA_ERR_HIP;
        r.num_alignment_bytes = total;
        r.start_text = so.begin_text;
        r.start_pattern = so.begin_pattern;
        a.results[pi] = r;
        a.tail_len[pi] = 0;
    }
}

}  // namespace sa

// ==================================================================================================
// host side
// ==================================================================================================
using namespace sa;

namespace {

struct AffineStats {
    double fill_ms = 0, walk_ms = 0;
    uint64_t arena_bytes = 0;
    int32_t chunks = 0;
};
thread_local AffineStats g_stats;

// every device buffer and event of one call, released on every return path
struct Workspace {
    std::vector<void *> bufs;
    std::vector<hipEvent_t> events;
    ~Workspace()
    {
        for (void *b : bufs) (void)hipFree(b);
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
    }
    template <typename T>
    int alloc(T **p, size_t bytes)
    {
        if (int rc = dmalloc(p, bytes)) return rc;
        bufs.push_back(*p);
        return SA_OK;
    }
    // a buffer of the size of `h`, holding it
    template <typename T>
    int upload(T **p, const std::vector<T> &h)
    {
        if (int rc = alloc(p, h.size() * sizeof(T))) return rc;
        if (!h.empty()) HIP_TRY(hipMemcpy(*p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
        return SA_OK;
    }
};

// What an aligner is called with, and its words for the messages
struct TracedCall {
    const char *who, *walk, *moves;  // "<who>: null argument", "<walk> of pair 3 did not end within <moves>"
    const sa_params *P;
    const sa_pair *pairs;
    int64_t np;
    int device;
    const void *d_text, *d_pattern;
    sa_result *results;
    char *const *aligned_text, *const *aligned_pattern;
    CigarSink *cigar = nullptr;  // set: the strings stay on the device and are encoded there (aligned_* null)
};

// The device side of one traced run. The driver owns what every aligner has; the aligner's setup adds its
// descriptors through `ws` and says what a chunk launches.
struct TracedRun {
    Workspace ws;
    hipStream_t st = nullptr;
    int A = 0;
    int32_t *d_table, *d_rows;
    uint32_t *d_ctrl, *d_dirs;
    char *d_ot = nullptr, *d_op = nullptr, *d_alpha;  // the string arenas are null for a call without strings
    sa_result *d_results;
    // from the setup: chunk c's order slices and traced fill (between the chunk's first two events), then its walk
    // kernel(s) (before the third); and where the walk leaves each pair's tail length, null when every string is
    // all tail
    std::function<int(int64_t)> fill, walk;
    const uint64_t *d_tail = nullptr;
};

// The traced run both aligners are: the checks, `plan` (which fills `pl`), the statistics, the common buffers,
// `setup`, then chunk after chunk a traced fill and a walk that reuses the arena, timed by three events, and the
// results and strings brought back. A pair's string is a head piece at the start of its slot and a tail piece at
// the slot's end. With a CIGAR sink the arenas are allocated and written as for a call with strings, neither is
// copied to the host, and once no check below has failed the encoder (sa_cigar.hip) reads them where they lie, on
// the same stream: pl.string_bytes covers the whole call, so every chunk's pairs are still there.
template <typename PLAN, typename SETUP>
int traced_run(const TracedCall &c, const TracePlan &pl, PLAN plan, SETUP setup)
{
    const std::string who = c.who;
    const int64_t np = c.np;
    if (!c.P || np < 0 || (np > 0 && (!c.pairs || !c.results)) || ((c.aligned_text == nullptr) != (c.aligned_pattern == nullptr)))
        return fail(SA_ERR_INVALID, who + ": null argument");
    DeviceGuard dg(c.device);
    if (!dg.ok) return fail(SA_ERR_HIP, "hipSetDevice failed");
    std::string err;
    if (int rc = plan(&err)) return fail(rc, err);
    if (!c.P->alphabet) return fail(SA_ERR_INVALID, who + ": params->alphabet is null");
    if (c.cigar && c.aligned_text) return fail(SA_ERR_INVALID, who + ": a call takes strings or a CIGAR sink, not both");
    g_stats = AffineStats();
    g_stats.arena_bytes = pl.arena_bytes;
    g_stats.chunks = (int32_t)pl.num_chunks();
    if (np == 0) return c.cigar ? cigar_encode(nullptr, nullptr, nullptr, 0, nullptr, nullptr, {}, 0, c.cigar) : SA_OK;
    if ((!c.d_text || !c.d_pattern) && pl.score.input_bytes) return fail(SA_ERR_INVALID, who + ": null arena");

    TracedRun r;
    r.A = pl.score.A;
    const bool strings = c.aligned_text != nullptr || c.cigar;
    int rc;
    if ((rc = r.ws.alloc(&r.d_table, 32 * 32 * 4)) || (rc = r.ws.alloc(&r.d_rows, (size_t)pl.score.grid * pl.score.row_stride * 8)) ||
        (rc = r.ws.alloc(&r.d_ctrl, 256)) || (rc = r.ws.alloc(&r.d_dirs, pl.arena_bytes)) || (rc = r.ws.alloc(&r.d_alpha, 64)) ||
        (rc = r.ws.alloc(&r.d_results, (size_t)np * sizeof(sa_result))))
        return rc;
    if (strings && ((rc = r.ws.alloc(&r.d_ot, pl.string_bytes)) || (rc = r.ws.alloc(&r.d_op, pl.string_bytes)))) return rc;
    HIP_TRY(hipMemcpy(r.d_table, c.P->score_matrix, (size_t)r.A * r.A * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(r.d_alpha, c.P->alphabet, (size_t)r.A + 1, hipMemcpyHostToDevice));
    if ((rc = setup(r))) return rc;

    hipStream_t st = r.st;
    const int64_t nchunks = pl.num_chunks();
    std::vector<hipEvent_t> &ev = r.ws.events;
    ev.reserve((size_t)nchunks * 3);
    for (int64_t e = 0; e < nchunks * 3; ++e)
    {
        hipEvent_t one;
        HIP_TRY(hipEventCreate(&one));
        ev.push_back(one);
    }
    HIP_TRY(hipMemsetAsync(r.d_ctrl, 0, 256, st));
    uint32_t ctrl[4] = {0, 0, 0, 0};  // [2] and [3]: the work counter and the bad-input flag of a chains call's gap fill
    std::vector<uint64_t> tail((size_t)np, UINT64_MAX);
    // everything enqueued on the stream, up to its synchronise; a failure on the way must not leave
    // copies into `results`, `ctrl` and `tail` pending when this function returns
    auto enqueue = [&]() -> int {
        for (int64_t k = 0; k < nchunks; ++k)
        {
            if (k) HIP_TRY(hipMemsetAsync(r.d_ctrl, 0, 4, st));  // the work counter; the bad-input flag stays
            HIP_TRY(hipEventRecord(ev[3 * k], st));
            if (int rc = r.fill(k)) return rc;
            HIP_TRY(hipEventRecord(ev[3 * k + 1], st));
            if (int rc = r.walk(k)) return rc;
            HIP_TRY(hipEventRecord(ev[3 * k + 2], st));
        }
        HIP_TRY(hipMemcpyAsync(ctrl, r.d_ctrl, sizeof(ctrl), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(c.results, r.d_results, (size_t)np * sizeof(sa_result), hipMemcpyDeviceToHost, st));
        if (r.d_tail) HIP_TRY(hipMemcpyAsync(tail.data(), r.d_tail, (size_t)np * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return SA_OK;
    };
    if ((rc = enqueue()))
    {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    for (int64_t k = 0; k < nchunks; ++k)
    {
        float f = 0, w = 0;
        HIP_TRY(hipEventElapsedTime(&f, ev[3 * k], ev[3 * k + 1]));
        HIP_TRY(hipEventElapsedTime(&w, ev[3 * k + 1], ev[3 * k + 2]));
        g_stats.fill_ms += f;
        g_stats.walk_ms += w;
    }
    if (ctrl[1] || ctrl[3]) return fail(SA_ERR_INVALID, "a text or pattern byte is outside the alphabet (0..A-1)");
    for (int64_t p = 0; p < np; ++p)
        if (c.results[p].status != SA_OK)
            return fail(SA_ERR_HIP, std::string(c.walk) + " of pair " + std::to_string(p) + " did not end within " + c.moves);
    if (c.cigar)
    {
        std::vector<CigarSlot> slots((size_t)np);
        for (int64_t p = 0; p < np; ++p) slots[p] = CigarSlot{pl.slot_off[p], c.pairs[p].text_len + c.pairs[p].pattern_len};
        return cigar_encode(st, r.d_ot, r.d_op, pl.string_bytes, r.d_results, r.d_tail, slots, c.P->alphabet[r.A], c.cigar);
    }
    if (strings && pl.string_bytes)
    {
        std::vector<char> ht(pl.string_bytes), hp(pl.string_bytes);
        HIP_TRY(hipMemcpy(ht.data(), r.d_ot, pl.string_bytes, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(hp.data(), r.d_op, pl.string_bytes, hipMemcpyDeviceToHost));
        for (int64_t p = 0; p < np; ++p)
        {
            // the head piece (a seeded pair's left half and seed) forwards from the start of the slot; the tail
            // piece (its right half; of any other pair, the whole string) written backwards from the slot's end
            const uint64_t cap = c.pairs[p].text_len + c.pairs[p].pattern_len;
            const uint64_t L = std::min<uint64_t>(c.results[p].num_alignment_bytes, cap), tl = std::min<uint64_t>(tail[p], L), hl = L - tl;
            if (hl)
            {
                std::memcpy(c.aligned_text[p], ht.data() + pl.slot_off[p], hl);
                std::memcpy(c.aligned_pattern[p], hp.data() + pl.slot_off[p], hl);
            }
            if (tl)
            {
                std::memcpy(c.aligned_text[p] + hl, ht.data() + pl.slot_off[p] + cap - tl, tl);
                std::memcpy(c.aligned_pattern[p] + hl, hp.data() + pl.slot_off[p] + cap - tl, tl);
            }
        }
    }
    return SA_OK;
}

}  // namespace

int sa::align_affine_device(const sa_params *P, const WaveSpec &spec, const sa_pair *pairs, int64_t np, int device, const void *d_text,
                            const void *d_pattern, sa_result *results, char *const *aligned_text, char *const *aligned_pattern,
                            CigarSink *cigar)
{
    if (spec.chained) return align_chains_device(P, spec, pairs, np, device, d_text, d_pattern, results, aligned_text, aligned_pattern, cigar);
    if (spec.seeded) return align_seeds_device(P, spec, pairs, np, device, d_text, d_pattern, results, aligned_text, aligned_pattern, cigar);
    TracePlan pl;
    TracedWaveArgs fa = {};
    WalkArgs wa;
    WaveChoice choice = {};
    int32_t *d_order;
    auto plan = [&](std::string *err) -> int {
        if (spec.band_at && !spec.bands && np > 0)
        {
            *err = "sa_align_pairs_band_at: bands is null";
            return SA_ERR_INVALID;
        }
        return make_trace_plan(P, spec, pairs, np, device_cus(device), score_knobs(), trace_arena_budget(), &pl, err);
    };
    auto setup = [&](TracedRun &r) -> int {
        std::vector<ScorePair> hpairs((size_t)np);
        std::vector<uint64_t> dir_words((size_t)np);
        for (int64_t p = 0; p < np; ++p)
        {
            hpairs[p] = ScorePair{pairs[p].text_offset, pairs[p].pattern_offset, (uint32_t)pairs[p].text_len, (uint32_t)pairs[p].pattern_len};
            dir_words[p] = pl.dir_off[p] / 4;
        }
        ScorePair *d_pairs;
        sa_score_result *d_scores;
        uint64_t *d_dir_off, *d_slot_off;
        Band *d_bands = nullptr;
        int rc;
        if (spec.band_at && (rc = r.ws.upload(&d_bands, pl.score.bands))) return rc;
        if ((rc = r.ws.upload(&d_pairs, hpairs)) || (rc = r.ws.upload(&d_order, pl.score.order)) ||
            (rc = r.ws.alloc(&d_scores, (size_t)np * sizeof(sa_score_result))) || (rc = r.ws.upload(&d_dir_off, dir_words)) ||
            (rc = r.ws.upload(&d_slot_off, pl.slot_off)))
            return rc;
        fa.sa = score_args(pl.score, d_text, d_pattern, d_pairs, d_order, 0, r.d_table, r.d_rows, d_scores, r.d_ctrl);
        fa.tr.dirs = r.d_dirs;
        fa.tr.dir_off = d_dir_off;
        fa.bands = d_bands;
        choice = wave_choice(pl.score.spec, pl.score.mode);
        wa.text = fa.sa.s.text;
        wa.pattern = fa.sa.s.pattern;
        wa.pairs = d_pairs;
        wa.scores = d_scores;
        wa.dirs = r.d_dirs;
        wa.dir_off = d_dir_off;
        wa.slot_off = d_slot_off;
        wa.out_text = r.d_ot;
        wa.out_pattern = r.d_op;
        wa.alphabet = r.d_alpha;
        wa.results = r.d_results;
        wa.A = r.A;
        // an extension walks as SA_ENDS_FREE with no flag: from the fill's result cell to the origin
        wa.mode = spec.extend ? SA_ENDS_FREE : pl.score.mode;
        wa.band = spec.banded ? spec.band : spec.ext_band ? spec.width : -1;
        wa.bands = d_bands;
        // the chunks differ in their part of the work order
        r.fill = [&](int64_t c) -> int {
            ScoreArgs &s = fa.sa.s;
            s.order = d_order + pl.chunk_begin[c];
            s.np = (int32_t)(pl.chunk_begin[c + 1] - pl.chunk_begin[c]);
            wa.order = s.order;
            if (!launch_wave<true>(choice, kTraceRows, r.A <= 4, (int)std::min<int64_t>(s.np, pl.score.grid), r.st, fa))
                return fail(SA_ERR_UNSUPPORTED, "affine aligner: the call's variant has no kernel instance");
            HIP_TRY(hipGetLastError());
            return SA_OK;
        };
        r.walk = [&](int64_t) -> int {
            const dim3 grid((unsigned)fa.sa.s.np);
            if (spec.ext_band) hipLaunchKernelGGL(walk_affine_kernel<3>, grid, dim3(64), 0, r.st, wa);
            else if (wa.bands) hipLaunchKernelGGL(walk_affine_kernel<2>, grid, dim3(64), 0, r.st, wa);
            else if (wa.band >= 0) hipLaunchKernelGGL(walk_affine_kernel<1>, grid, dim3(64), 0, r.st, wa);
            else hipLaunchKernelGGL(walk_affine_kernel<0>, grid, dim3(64), 0, r.st, wa);
            HIP_TRY(hipGetLastError());
            return SA_OK;
        };
        return SA_OK;
    };
    return traced_run({"affine aligner", "affine walk", "text_len + pattern_len moves", P, pairs, np, device, d_text, d_pattern, results,
                       aligned_text, aligned_pattern, cigar},
                      pl, plan, setup);
}

// every sa_align_pairs_*: the host pairs packed into two arenas, then the device path
int sa::align_host_pairs(const sa_params *P, const WaveSpec &spec, const sa_host_pair *pairs, int64_t np, int device, sa_result *results,
                         char *const *aligned_text, char *const *aligned_pattern, CigarSink *cigar)
{
    const char *const fn = spec.chained ? "sa_align_pairs_chains" : spec.seeded ? "sa_align_pairs_seeds" : "sa_align_pairs_affine";
    if (!P || np < 0 || (np > 0 && (!pairs || !results)) || ((aligned_text == nullptr) != (aligned_pattern == nullptr)))
        return fail(SA_ERR_INVALID, std::string(fn) + ": null argument");
    HostArenas in;
    if (int rc = upload_host_pairs(fn, pairs, np, device, &in)) return rc;
    return align_affine_device(P, spec, in.pairs.data(), np, device, in.text.p, in.pattern.p, results, aligned_text, aligned_pattern, cigar);
}

extern "C" {

int sa_align_pairs_affine(const sa_params *P, int32_t gap_open, int32_t gap_extend, const sa_host_pair *pairs, int64_t np,
                          int device, sa_result *results, char *const *aligned_text, char *const *aligned_pattern)
{
    return align_host_pairs(P, WaveSpec::gaps(gap_open, gap_extend), pairs, np, device, results, aligned_text, aligned_pattern);
}

int sa_align_pairs_banded(const sa_params *P, int32_t gap_open, int32_t gap_extend, int32_t band, const sa_host_pair *pairs,
                          int64_t np, int device, sa_result *results, char *const *aligned_text, char *const *aligned_pattern)
{
    return align_host_pairs(P, WaveSpec::gaps(gap_open, gap_extend).in_band(band), pairs, np, device, results, aligned_text,
                            aligned_pattern);
}

int sa_align_pairs_band_at(const sa_params *P, int32_t gap_open, int32_t gap_extend, const sa_band *bands, const sa_host_pair *pairs,
                           int64_t np, int device, sa_result *results, char *const *aligned_text, char *const *aligned_pattern)
{
    return align_host_pairs(P, WaveSpec::gaps(gap_open, gap_extend).in_bands(bands), pairs, np, device, results,
                            aligned_text, aligned_pattern);
}

int sa_align_pairs_extend(const sa_params *P, int32_t gap_open, int32_t gap_extend, int32_t xdrop, const sa_host_pair *pairs,
                          int64_t np, int device, sa_result *results, char *const *aligned_text, char *const *aligned_pattern)
{
    return align_host_pairs(P, WaveSpec::gaps(gap_open, gap_extend).extending(xdrop), pairs, np, device, results,
                            aligned_text, aligned_pattern);
}

int sa_align_pairs_seeds(const sa_params *P, int32_t gap_open, int32_t gap_extend, int32_t xdrop, const sa_seed *seeds,
                         const sa_host_pair *pairs, int64_t np, int device, sa_result *results, char *const *aligned_text,
                         char *const *aligned_pattern)
{
    return align_host_pairs(P, WaveSpec::gaps(gap_open, gap_extend).extending(xdrop).from_seeds(seeds), pairs, np, device,
                            results, aligned_text, aligned_pattern);
}

int sa_align_pairs_extend_band(const sa_params *P, int32_t gap_open, int32_t gap_extend, int32_t xdrop, int32_t width,
                               const sa_host_pair *pairs, int64_t np, int device, sa_result *results, char *const *aligned_text,
                               char *const *aligned_pattern)
{
    return align_host_pairs(P, WaveSpec::gaps(gap_open, gap_extend).extending(xdrop).within(width), pairs, np, device, results,
                            aligned_text, aligned_pattern);
}

int sa_align_pairs_seeds_band(const sa_params *P, int32_t gap_open, int32_t gap_extend, int32_t xdrop, int32_t width, const sa_seed *seeds,
                              const sa_host_pair *pairs, int64_t np, int device, sa_result *results, char *const *aligned_text,
                              char *const *aligned_pattern)
{
    return align_host_pairs(P, WaveSpec::gaps(gap_open, gap_extend).extending(xdrop).within(width).from_seeds(seeds), pairs, np, device,
                            results, aligned_text, aligned_pattern);
}

int sa_align_pairs_chains(const sa_params *P, int32_t gap_open, int32_t gap_extend, int32_t xdrop, const sa_seed *seeds, const uint64_t *chain_off,
                          const sa_host_pair *pairs, int64_t np, int device, sa_result *results, char *const *aligned_text,
                          char *const *aligned_pattern)
{
    return align_host_pairs(P, WaveSpec::gaps(gap_open, gap_extend).extending(xdrop).from_chains(seeds, chain_off), pairs, np, device,
                            results, aligned_text, aligned_pattern);
}

int sa_affine_last_stats(double *fill_ms, double *walk_ms, uint64_t *arena_bytes, int32_t *num_chunks)
{
    if (fill_ms) *fill_ms = g_stats.fill_ms;
    if (walk_ms) *walk_ms = g_stats.walk_ms;
    if (arena_bytes) *arena_bytes = g_stats.arena_bytes;
    if (num_chunks) *num_chunks = g_stats.chunks;
    return SA_OK;
}

}  // extern "C"

int sa::align_seeds_device(const sa_params *P, const WaveSpec &spec, const sa_pair *pairs, int64_t np, int device, const void *d_text,
                           const void *d_pattern, sa_result *results, char *const *aligned_text, char *const *aligned_pattern,
                           CigarSink *cigar)
{
    SeedTracePlan pl;
    TracedWaveArgs fa = {};
    SeedsCombineArgs ca;
    SeedWalkArgs wa;
    WaveChoice choice = {};
    int32_t *d_order, *d_pair_order;
    auto plan = [&](std::string *err) {
        return make_seeds_trace_plan(P, spec, pairs, spec.seeds, np, device_cus(device), score_knobs(), trace_arena_budget(), &pl, err);
    };
    auto setup = [&](TracedRun &r) -> int {
        const size_t ni = pl.seeds.items.size();
        std::vector<uint64_t> dir_words(ni), slots(pl.slot_off);
        for (size_t k = 0; k < ni; ++k) dir_words[k] = pl.dir_off[k] / 4;
        slots.push_back(pl.string_bytes);
        SeedItem *d_items;
        SeedPair *d_seed_pairs;
        sa_score_result *d_scores;
        sa_seed_result *d_seed_out;
        uint64_t *d_dir_off, *d_slot_off, *d_tail;
        int rc;
        if ((rc = r.ws.upload(&d_items, pl.seeds.items)) || (rc = r.ws.upload(&d_seed_pairs, pl.seeds.pairs)) ||
            (rc = r.ws.upload(&d_order, pl.score.order)) || (rc = r.ws.upload(&d_pair_order, pl.pair_order)) ||
            (rc = r.ws.alloc(&d_scores, ni * sizeof(sa_score_result))) || (rc = r.ws.alloc(&d_seed_out, (size_t)np * sizeof(sa_seed_result))) ||
            (rc = r.ws.upload(&d_dir_off, dir_words)) || (rc = r.ws.upload(&d_slot_off, slots)) || (rc = r.ws.alloc(&d_tail, (size_t)np * 8)))
            return rc;
        r.d_tail = d_tail;
        fa.sa = score_args(pl.score, d_text, d_pattern, nullptr, d_order, 0, r.d_table, r.d_rows, d_scores, r.d_ctrl);
        fa.tr.dirs = r.d_dirs;
        fa.tr.dir_off = d_dir_off;
        fa.items = d_items;
        choice = wave_choice(pl.score.spec, pl.score.mode);
        ca.text = fa.sa.s.text;
        ca.pattern = fa.sa.s.pattern;
        ca.pairs = d_seed_pairs;
        ca.table = r.d_table;
        ca.item_out = d_scores;
        ca.out = d_seed_out;
        ca.ctrl = r.d_ctrl;
        ca.A = r.A;
        wa.text = fa.sa.s.text;
        wa.pattern = fa.sa.s.pattern;
        wa.items = d_items;
        wa.pairs = d_seed_pairs;
        wa.scores = d_scores;
        wa.seed_out = d_seed_out;
        wa.dirs = r.d_dirs;
        wa.dir_off = d_dir_off;
        wa.slot_off = d_slot_off;
        wa.out_text = r.d_ot;
        wa.out_pattern = r.d_op;
        wa.alphabet = r.d_alpha;
        wa.results = r.d_results;
        wa.tail_len = d_tail;
        wa.A = r.A;
        wa.width = spec.ext_band ? spec.width : -1;
        // the chunk's items in one traced fill (none: no launch), then the combine and the walk of the chunk's pairs
        r.fill = [&](int64_t c) -> int {
            ScoreArgs &s = fa.sa.s;
            s.order = d_order + pl.chunk_begin[c];
            s.np = (int32_t)(pl.chunk_begin[c + 1] - pl.chunk_begin[c]);
            wa.order = ca.order = d_pair_order + pl.pair_chunk_begin[c];
            if (s.np == 0) return SA_OK;
            if (!launch_wave<true>(choice, kTraceRows, r.A <= 4, (int)std::min<int64_t>(s.np, pl.score.grid), r.st, fa))
                return fail(SA_ERR_UNSUPPORTED, "seeds aligner: the call's variant has no kernel instance");
            HIP_TRY(hipGetLastError());
            return SA_OK;
        };
        r.walk = [&](int64_t c) -> int {
            const int64_t pcount = pl.pair_chunk_begin[c + 1] - pl.pair_chunk_begin[c];
            launch_seeds_combine(ca, pcount, r.st);
            HIP_TRY(hipGetLastError());
            if (spec.ext_band) hipLaunchKernelGGL(walk_seeds_kernel<true>, dim3((unsigned)pcount), dim3(64), 0, r.st, wa);
            else hipLaunchKernelGGL(walk_seeds_kernel<false>, dim3((unsigned)pcount), dim3(64), 0, r.st, wa);
            HIP_TRY(hipGetLastError());
            return SA_OK;
        };
        return SA_OK;
    };
    return traced_run({"seeds aligner", "seeded walk", "its halves' moves", P, pairs, np, device, d_text, d_pattern, results, aligned_text,
                       aligned_pattern, cigar},
                      pl, plan, setup);
}

int sa::align_chains_device(const sa_params *P, const WaveSpec &spec, const sa_pair *pairs, int64_t np, int device, const void *d_text,
                            const void *d_pattern, sa_result *results, char *const *aligned_text, char *const *aligned_pattern,
                            CigarSink *cigar)
{
    ChainTracePlan pl;
    TracedWaveArgs fe = {}, fg = {};  // the fill of the end items and of the gap items
    ChainsCombineArgs ca;
    ChainWalkArgs wa = {};
    ChainJoinArgs ja;
    WaveChoice echoice = {}, gchoice = {};
    int32_t *d_eorder, *d_gorder, *d_pair_order;
    auto plan = [&](std::string *err) {
        return make_chains_trace_plan(P, spec, pairs, np, device_cus(device), score_knobs(), trace_arena_budget(), &pl, err);
    };
    auto setup = [&](TracedRun &r) -> int {
        const size_t ne = pl.items.ends.size(), ng = pl.items.gaps.size();
        std::vector<uint64_t> edir(ne), gdir(ng), slots(pl.slot_off);
        for (size_t k = 0; k < ne; ++k) edir[k] = pl.dir_off[k] / 4;
        for (size_t k = 0; k < ng; ++k) gdir[k] = pl.gap_dir_off[k] / 4;
        slots.push_back(pl.string_bytes);
        SeedItem *d_ends, *d_gaps;
        ChainPair *d_pairs;
        ChainSeed *d_seeds;
        sa_score_result *d_escores, *d_gscores;
        sa_seed_result *d_seed_out;
        uint64_t *d_edir, *d_gdir, *d_slot_off, *d_tail;
        int32_t *d_grows, *d_elen, *d_glen;
        int rc;
        if ((rc = r.ws.upload(&d_ends, pl.items.ends)) || (rc = r.ws.upload(&d_gaps, pl.items.gaps)) || (rc = r.ws.upload(&d_pairs, pl.items.pairs)) ||
            (rc = r.ws.upload(&d_seeds, pl.items.seeds)) || (rc = r.ws.upload(&d_eorder, pl.score.order)) || (rc = r.ws.upload(&d_gorder, pl.gaps.order)) ||
            (rc = r.ws.upload(&d_pair_order, pl.pair_order)) || (rc = r.ws.alloc(&d_escores, ne * sizeof(sa_score_result))) ||
            (rc = r.ws.alloc(&d_gscores, ng * sizeof(sa_score_result))) || (rc = r.ws.alloc(&d_seed_out, (size_t)np * sizeof(sa_seed_result))) ||
            (rc = r.ws.upload(&d_edir, edir)) || (rc = r.ws.upload(&d_gdir, gdir)) || (rc = r.ws.upload(&d_slot_off, slots)) ||
            (rc = r.ws.alloc(&d_tail, (size_t)np * 8)) || (rc = r.ws.alloc(&d_grows, (size_t)pl.gaps.grid * pl.gaps.row_stride * 8)) ||
            (rc = r.ws.alloc(&d_elen, ne * 4)) || (rc = r.ws.alloc(&d_glen, ng * 4)))
            return rc;
        r.d_tail = d_tail;
        fe.sa = score_args(pl.score, d_text, d_pattern, nullptr, d_eorder, 0, r.d_table, r.d_rows, d_escores, r.d_ctrl);
        fe.tr.dirs = r.d_dirs;
        fe.tr.dir_off = d_edir;
        fe.items = d_ends;
        echoice = wave_choice(pl.score.spec, pl.score.mode);
        fg.sa = score_args(pl.gaps, d_text, d_pattern, nullptr, d_gorder, 0, r.d_table, d_grows, d_gscores, r.d_ctrl + 2);
        fg.tr.dirs = r.d_dirs;
        fg.tr.dir_off = d_gdir;
        fg.items = d_gaps;
        gchoice = wave_choice(pl.gaps.spec, pl.gaps.mode);
        ca.text = fe.sa.s.text;
        ca.pattern = fe.sa.s.pattern;
        ca.pairs = d_pairs;
        ca.seeds = d_seeds;
        ca.table = r.d_table;
        ca.end_out = d_escores;
        ca.gap_out = d_gscores;
        ca.out = d_seed_out;
        ca.ctrl = r.d_ctrl;
        ca.A = r.A;
        wa.w.text = fe.sa.s.text;
        wa.w.pattern = fe.sa.s.pattern;
        wa.w.dirs = r.d_dirs;
        wa.w.out_text = r.d_ot;
        wa.w.out_pattern = r.d_op;
        wa.w.alphabet = r.d_alpha;
        wa.w.A = r.A;
        wa.w.width = -1;
        wa.w.items = d_ends;
        wa.w.scores = d_escores;
        wa.w.dir_off = d_edir;
        wa.gap_items = d_gaps;
        wa.gap_scores = d_gscores;
        wa.gap_dir_off = d_gdir;
        wa.pairs = d_pairs;
        wa.slot_off = d_slot_off;
        wa.end_len = d_elen;
        wa.gap_len = d_glen;
        ja.text = fe.sa.s.text;
        ja.pattern = fe.sa.s.pattern;
        ja.pairs = d_pairs;
        ja.seeds = d_seeds;
        ja.seed_out = d_seed_out;
        ja.end_len = d_elen;
        ja.gap_len = d_glen;
        ja.slot_off = d_slot_off;
        ja.out_text = r.d_ot;
        ja.out_pattern = r.d_op;
        ja.alphabet = r.d_alpha;
        ja.results = r.d_results;
        ja.tail_len = d_tail;
        ja.A = r.A;
        // the chunk's gap items and end items in a traced fill each (none: no launch), then the combine of the chunk's
        // pairs, the walk of all its items and the join of its pairs
        r.fill = [&](int64_t c) -> int {
            ScoreArgs &e = fe.sa.s, &g = fg.sa.s;
            e.order = wa.end_order = d_eorder + pl.chunk_begin[c];
            e.np = wa.num_ends = (int32_t)(pl.chunk_begin[c + 1] - pl.chunk_begin[c]);
            g.order = wa.gap_order = d_gorder + pl.gap_chunk_begin[c];
            g.np = (int32_t)(pl.gap_chunk_begin[c + 1] - pl.gap_chunk_begin[c]);
            ja.order = ca.order = d_pair_order + pl.pair_chunk_begin[c];
            if (g.np)
            {
                HIP_TRY(hipMemsetAsync(r.d_ctrl + 2, 0, 4, r.st));  // the gap fill's work counter; its bad-input flag stays
                if (!launch_wave<true>(gchoice, kTraceRows, r.A <= 4, (int)std::min<int64_t>(g.np, pl.gaps.grid), r.st, fg))
                    return fail(SA_ERR_UNSUPPORTED, "chains aligner: the gap items' variant has no kernel instance");
                HIP_TRY(hipGetLastError());
            }
            if (e.np)
            {
                if (!launch_wave<true>(echoice, kTraceRows, r.A <= 4, (int)std::min<int64_t>(e.np, pl.score.grid), r.st, fe))
                    return fail(SA_ERR_UNSUPPORTED, "chains aligner: the end items' variant has no kernel instance");
                HIP_TRY(hipGetLastError());
            }
            return SA_OK;
        };
        r.walk = [&](int64_t c) -> int {
            const int64_t pcount = pl.pair_chunk_begin[c + 1] - pl.pair_chunk_begin[c];
            const int64_t icount = (int64_t)fe.sa.s.np + fg.sa.s.np;
            launch_chains_combine(ca, pcount, r.st);
            HIP_TRY(hipGetLastError());
            if (icount)
            {
                hipLaunchKernelGGL(walk_chain_items_kernel, dim3((unsigned)icount), dim3(64), 0, r.st, wa);
                HIP_TRY(hipGetLastError());
            }
            hipLaunchKernelGGL(chain_join_kernel, dim3((unsigned)pcount), dim3(64), 0, r.st, ja);
            HIP_TRY(hipGetLastError());
            return SA_OK;
        };
        return SA_OK;
    };
    return traced_run({"chains aligner", "chained walk", "its pieces' moves", P, pairs, np, device, d_text, d_pattern, results, aligned_text,
                       aligned_pattern, cigar},
                      pl, plan, setup);
}
