// Score-only path (sa_hip.h: sa_score_batch*, sa_scorer_*, sa_search*): the score of every pair and
// the cell it is read from, without direction planes, strip descriptors, records or a traceback.
// The kernels are the untraced instances of wave_kernel<R, MODE, SMALL, F>, the one wave program of
// sa_score_wave.h, launched through the table of sa_wave_launch.h; here are the combine kernel of the
// seeds scorer, that of the chains scorer and the host side. What a scorer runs is decided in sa_score_plan.cpp (host-only, no HIP).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#include "sa_affine.h"
#include "sa_hip.h"
#include "sa_host.h"
#include "sa_score_plan.h"
#include "sa_score_wave.h"
#include "sa_wave_launch.h"

namespace sa {

// One wave per pair, after the items' fill: the seed's substitution scores, summed by the lanes in a strided
// loop and over the wave by a prefix sum, the bad-letter flag for the seed's letters, and the pair's
// sa_seed_result from its halves' results (an empty half: 0 at (0, 0)).
__global__ __launch_bounds__(64) void seeds_combine_kernel(SeedsCombineArgs a)
{
    const int lane = threadIdx.x;
    const int p = a.order ? uniform(a.order[blockIdx.x]) : (int)blockIdx.x;
    const SeedPair sp = a.pairs[p];
    const int8_t *const text = a.text + sp.text_seed;
    const int8_t *const pattern = a.pattern + sp.pattern_seed;
    const int A = a.A;
    int sum = 0;
    bool bad = false;
    for (uint64_t q = (uint64_t)lane; q < sp.len; q += kWave)
    {
        const int ct = text[q], cp = pattern[q];
        bad = bad || ct < 0 || ct >= A || cp < 0 || cp >= A;
        sum += a.table[min(max(cp, 0), A - 1) * A + min(max(ct, 0), A - 1)];
    }
    sum = __builtin_amdgcn_readlane(wave_prefix_sum(sum), kWave - 1);
    if (bad) __hip_atomic_store(&a.ctrl[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lane == 0)
    {
        sa_score_result l = {0, SA_OK, 0, 0}, r = {0, SA_OK, 0, 0};
        if (sp.left >= 0) l = a.item_out[sp.left];
        if (sp.right >= 0) r = a.item_out[sp.right];
        sa_seed_result o;
        o.score = l.score + sum + r.score;
        o.status = SA_OK;
        o.begin_text = sp.ts - l.end_text;
        o.begin_pattern = sp.ps - l.end_pattern;
        o.end_text = sp.ts + sp.len + r.end_text;
        o.end_pattern = sp.ps + sp.len + r.end_pattern;
        a.out[p] = o;
    }
}

void launch_seeds_combine(const SeedsCombineArgs &a, int64_t np, void *stream)
{
    hipLaunchKernelGGL(seeds_combine_kernel, dim3((unsigned)np), dim3(64), 0, (hipStream_t)stream, a);
}

// One wave per pair, after the fills of the end items and of the gap items (sa_hip.h sa_score_batch_chains). The
// pair's seeds lie one after another in `seeds`: 64 at a time, a lane sums the columns of its own seed when that
// is shorter than a wave, and the seeds of 64 letters or more are then summed one by one by all lanes in a
// strided loop (a ballot names them), so neither a long chain nor a long seed is serial. The gap items' scores
// are a strided sum as well; one prefix sum over the wave adds both, and lane 0 adds the closed-form gaps and the
// two end items (an empty end: 0 at (0, 0)).
__global__ __launch_bounds__(64) void chains_combine_kernel(ChainsCombineArgs a)
{
    const int lane = threadIdx.x;
    const int p = a.order ? uniform(a.order[blockIdx.x]) : (int)blockIdx.x;
    const ChainPair cp = a.pairs[p];
    const int A = a.A;
    const int sbegin = uniform(cp.seed_begin), send = uniform(cp.seed_end), gbegin = uniform(cp.gap_begin), gend = uniform(cp.gap_end);
    int sum = 0;
    bool bad = false;
    auto column = [&](const ChainSeed &sd, uint64_t q) {
        const int ct = a.text[sd.text_off + q], cq = a.pattern[sd.pattern_off + q];
        bad = bad || ct < 0 || ct >= A || cq < 0 || cq >= A;
        sum += a.table[min(max(cq, 0), A - 1) * A + min(max(ct, 0), A - 1)];
    };
    for (int base = sbegin; base < send; base += kWave)
    {
        ChainSeed mine = {0, 0, 0, -1, 0};
        if (base + lane < send) mine = a.seeds[base + lane];
        const bool wide = mine.len >= (uint64_t)kWave;
        if (!wide)
            for (uint64_t q = 0; q < mine.len; ++q) column(mine, q);
        for (uint64_t w = ballot(wide); w; w &= w - 1)
        {
            const ChainSeed sd = a.seeds[base + __builtin_ctzll(w)];  // wave-uniform
            const uint64_t len = uniform64(sd.len);
            for (uint64_t q = (uint64_t)lane; q < len; q += kWave) column(sd, q);
        }
    }
    for (int k = gbegin + lane; k < gend; k += kWave) sum += a.gap_out[k].score;
    sum = __builtin_amdgcn_readlane(wave_prefix_sum(sum), kWave - 1);
    if (bad) __hip_atomic_store(&a.ctrl[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lane == 0)
    {
        sa_score_result l = {0, SA_OK, 0, 0}, r = {0, SA_OK, 0, 0};
        if (cp.left >= 0) l = a.end_out[cp.left];
        if (cp.right >= 0) r = a.end_out[cp.right];
        sa_seed_result o;
        o.score = l.score + sum + cp.closed_score + r.score;
        o.status = SA_OK;
        o.begin_text = cp.ts - l.end_text;
        o.begin_pattern = cp.ps - l.end_pattern;
        o.end_text = cp.te + r.end_text;
        o.end_pattern = cp.pe + r.end_pattern;
        a.out[p] = o;
    }
}

void launch_chains_combine(const ChainsCombineArgs &a, int64_t np, void *stream)
{
    hipLaunchKernelGGL(chains_combine_kernel, dim3((unsigned)np), dim3(64), 0, (hipStream_t)stream, a);
}

}  // namespace sa

// ==================================================================================================
// host side
// ==================================================================================================
using namespace sa;

struct sa_scorer : ScorePlan {
    int device = 0;
    ScorePair *d_pairs = nullptr;
    int32_t *d_order = nullptr, *d_table = nullptr, *d_rows = nullptr;
    Band *d_bands = nullptr;  // band-at scorer (spec.band_at): ScorePlan::bands
    sa_score_result *d_out = nullptr;
    uint32_t *d_ctrl = nullptr;
    bool ran = false;
    // seeds scorer (spec.seeded): the plan (num_pairs, order, d_out) is the work items'; seed_pairs counts the caller's pairs
    int64_t seed_pairs = 0;
    SeedItem *d_items = nullptr;
    SeedPair *d_seed_pairs = nullptr;
    sa_seed_result *d_seed_out = nullptr;
    // chains scorer (spec.chained, with spec.seeded): the plan and the buffers above are the end items'; the gap
    // items have a plan, a work order, boundary rows and results of their own, and their launch counts its work
    // and flags its bad letters in d_ctrl[2] and d_ctrl[3]
    ScorePlan gaps;
    int32_t *d_gap_order = nullptr, *d_gap_rows = nullptr;
    SeedItem *d_gap_items = nullptr;
    sa_score_result *d_gap_out = nullptr;
    ChainPair *d_chain_pairs = nullptr;
    ChainSeed *d_chain_seeds = nullptr;
};

namespace {

void free_scorer(sa_scorer *s)
{
    if (!s) return;
    DeviceGuard dg(s->device);
    void *bufs[] = {s->d_pairs, s->d_order, s->d_table, s->d_rows, s->d_out, s->d_ctrl, s->d_bands, s->d_items, s->d_seed_pairs, s->d_seed_out,
                    s->d_gap_order, s->d_gap_rows, s->d_gap_items, s->d_gap_out, s->d_chain_pairs, s->d_chain_seeds};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    delete s;
}

}  // namespace

// every sa_scorer_create*: `spec` is the variant the function stands for. A seeded spec plans the work items
// (num_pairs, order and d_out are then theirs) and keeps the pairs' seeds and results beside them; a chained
// spec plans the end items so and the gap items beside them
static int create_scorer(const sa_params *P, const WaveSpec &spec, const sa_pair *pairs, int64_t np, int device, sa_scorer **out)
{
    if (!out)
        return fail(SA_ERR_INVALID, spec.chained  ? "sa_scorer_create_chains: null argument"
                                    : spec.seeded ? "sa_scorer_create_seeds: null argument"
                                                  : "sa_scorer_create: null argument");
    *out = nullptr;
    if (spec.band_at && !spec.bands && np > 0) return fail(SA_ERR_INVALID, "sa_scorer_create_band_at: bands is null");
    DeviceGuard dg(device);
    if (!dg.ok) return fail(SA_ERR_HIP, "hipSetDevice failed");
    std::unique_ptr<sa_scorer, void (*)(sa_scorer *)> s(new sa_scorer(), free_scorer);
    s->device = device;
    std::string err;
    SeedItems si;
    ChainsScorePlan cp;
    if (spec.chained)
    {
        if (int rc = make_chains_score_plan(P, spec, pairs, np, device_cus(device), score_knobs(), &cp, &err)) return fail(rc, err);
        static_cast<ScorePlan &>(*s) = cp.ends;
        s->gaps = cp.gaps;
        s->device_bytes = cp.device_bytes;
    }
    else if (int rc = spec.seeded ? make_seeds_score_plan(P, spec, pairs, spec.seeds, np, device_cus(device), score_knobs(), s.get(), &si, &err)
                             : make_score_plan(P, spec, pairs, np, device_cus(device), score_knobs(), s.get(), &err))
        return fail(rc, err);
    if (spec.seeded) s->seed_pairs = np;
    const size_t nw = (size_t)s->num_pairs;  // what the waves draw: pairs, or items
    int rc;
    if ((rc = dmalloc(&s->d_order, nw * 4))) return rc;
    if ((rc = dmalloc(&s->d_table, 32 * 32 * 4))) return rc;
    if ((rc = dmalloc(&s->d_rows, (size_t)s->grid * s->row_stride * (s->spec.affine ? 8 : 4)))) return rc;
    if ((rc = dmalloc(&s->d_out, nw * sizeof(sa_score_result)))) return rc;
    if ((rc = dmalloc(&s->d_ctrl, 256))) return rc;
    if (nw) HIP_TRY(hipMemcpy(s->d_order, s->order.data(), nw * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->d_table, P->score_matrix, (size_t)s->A * s->A * 4, hipMemcpyHostToDevice));
    // the descriptors: the items with the pairs' seeds and results, or the pairs with their bands
    auto upload = [](auto **d, const auto &h) -> int {
        if (int rc = dmalloc(d, h.size() * sizeof(h[0]))) return rc;
        if (h.size()) HIP_TRY(hipMemcpy(*d, h.data(), h.size() * sizeof(h[0]), hipMemcpyHostToDevice));
        return SA_OK;
    };
    if (spec.chained)
    {
        if ((rc = upload(&s->d_items, cp.items.ends)) || (rc = upload(&s->d_gap_items, cp.items.gaps)) ||
            (rc = upload(&s->d_gap_order, s->gaps.order)) || (rc = upload(&s->d_chain_pairs, cp.items.pairs)) ||
            (rc = upload(&s->d_chain_seeds, cp.items.seeds)))
            return rc;
        if ((rc = dmalloc(&s->d_gap_rows, (size_t)s->gaps.grid * s->gaps.row_stride * (s->gaps.spec.affine ? 8 : 4))) ||
            (rc = dmalloc(&s->d_gap_out, (size_t)s->gaps.num_pairs * sizeof(sa_score_result))) ||
            (rc = dmalloc(&s->d_seed_out, (size_t)np * sizeof(sa_seed_result))))
            return rc;
    }
    else if (spec.seeded)
    {
        if ((rc = upload(&s->d_items, si.items)) || (rc = upload(&s->d_seed_pairs, si.pairs))) return rc;
        if ((rc = dmalloc(&s->d_seed_out, (size_t)np * sizeof(sa_seed_result)))) return rc;
    }
    else
    {
        std::vector<ScorePair> h((size_t)np);
        for (int64_t p = 0; p < np; ++p)
            h[p] = ScorePair{pairs[p].text_offset, pairs[p].pattern_offset, (uint32_t)pairs[p].text_len, (uint32_t)pairs[p].pattern_len};
        if ((rc = upload(&s->d_pairs, h))) return rc;
        if (spec.band_at && (rc = upload(&s->d_bands, s->bands))) return rc;
    }
    *out = s.release();
    return SA_OK;
}

// every sa_score_batch*: upload, create, run, and the fetch of its result type; a seeded spec is sa_score_batch_seeds
template <typename RESULT>
static int score_batch(const sa_params *P, const WaveSpec &spec, const sa_host_pair *pairs, int64_t np, int device, RESULT *out,
                       int (*fetch)(sa_scorer *, RESULT *, void *) = sa_scorer_fetch)
{
    const char *const fn = spec.chained ? "sa_score_batch_chains" : spec.seeded ? "sa_score_batch_seeds" : "sa_score_batch";
    if (!P || np < 0 || (np > 0 && (!pairs || !out))) return fail(SA_ERR_INVALID, std::string(fn) + ": null argument");
    HostArenas in;
    if (int rc = upload_host_pairs(fn, pairs, np, device, &in)) return rc;
    sa_scorer *raw = nullptr;
    if (int rc = create_scorer(P, spec, in.pairs.data(), np, device, &raw)) return rc;
    std::unique_ptr<sa_scorer, void (*)(sa_scorer *)> s(raw, free_scorer);
    if (int rc = sa_scorer_run(s.get(), in.text.p, in.pattern.p, nullptr)) return rc;
    return fetch(s.get(), out, nullptr);
}

extern "C" {

int sa_scorer_create(const sa_params *P, const sa_pair *pairs, int64_t np, int device, sa_scorer **out)
{
    return create_scorer(P, WaveSpec(), pairs, np, device, out);
}

int sa_scorer_create_affine(const sa_params *P, int32_t gap_open, int32_t gap_extend, const sa_pair *pairs, int64_t np,
                            int device, sa_scorer **out)
{
    return create_scorer(P, WaveSpec::gaps(gap_open, gap_extend), pairs, np, device, out);
}

int sa_scorer_create_banded(const sa_params *P, int32_t gap_open, int32_t gap_extend, int32_t band, const sa_pair *pairs,
                            int64_t np, int device, sa_scorer **out)
{
    return create_scorer(P, WaveSpec::gaps(gap_open, gap_extend).in_band(band), pairs, np, device, out);
}

int sa_scorer_create_band_at(const sa_params *P, int32_t gap_open, int32_t gap_extend, const sa_band *bands, const sa_pair *pairs,
                             int64_t np, int device, sa_scorer **out)
{
    return create_scorer(P, WaveSpec::gaps(gap_open, gap_extend).in_bands(bands), pairs, np, device, out);
}

int sa_scorer_create_extend(const sa_params *P, int32_t gap_open, int32_t gap_extend, int32_t xdrop, const sa_pair *pairs,
                            int64_t np, int device, sa_scorer **out)
{
    return create_scorer(P, WaveSpec::gaps(gap_open, gap_extend).extending(xdrop), pairs, np, device, out);
}

int sa_scorer_create_seeds(const sa_params *P, int32_t gap_open, int32_t gap_extend, int32_t xdrop, const sa_seed *seeds,
                           const sa_pair *pairs, int64_t np, int device, sa_scorer **out)
{
    return create_scorer(P, WaveSpec::gaps(gap_open, gap_extend).extending(xdrop).from_seeds(seeds), pairs, np, device, out);
}

int sa_score_batch_seeds(const sa_params *P, int32_t gap_open, int32_t gap_extend, int32_t xdrop, const sa_seed *seeds,
                         const sa_host_pair *pairs, int64_t np, int device, sa_seed_result *out)
{
    return score_batch(P, WaveSpec::gaps(gap_open, gap_extend).extending(xdrop).from_seeds(seeds), pairs, np, device, out, sa_scorer_fetch_seeds);
}

int sa_scorer_create_chains(const sa_params *P, int32_t gap_open, int32_t gap_extend, int32_t xdrop, const sa_seed *seeds, const uint64_t *chain_off,
                            const sa_pair *pairs, int64_t np, int device, sa_scorer **out)
{
    return create_scorer(P, WaveSpec::gaps(gap_open, gap_extend).extending(xdrop).from_chains(seeds, chain_off), pairs, np, device, out);
}

int sa_score_batch_chains(const sa_params *P, int32_t gap_open, int32_t gap_extend, int32_t xdrop, const sa_seed *seeds, const uint64_t *chain_off,
                          const sa_host_pair *pairs, int64_t np, int device, sa_seed_result *out)
{
    return score_batch(P, WaveSpec::gaps(gap_open, gap_extend).extending(xdrop).from_chains(seeds, chain_off), pairs, np, device, out,
                       sa_scorer_fetch_seeds);
}

int sa_scorer_create_extend_band(const sa_params *P, int32_t gap_open, int32_t gap_extend, int32_t xdrop, int32_t width,
                                 const sa_pair *pairs, int64_t np, int device, sa_scorer **out)
{
    return create_scorer(P, WaveSpec::gaps(gap_open, gap_extend).extending(xdrop).within(width), pairs, np, device, out);
}

int sa_scorer_create_seeds_band(const sa_params *P, int32_t gap_open, int32_t gap_extend, int32_t xdrop, int32_t width,
                                const sa_seed *seeds, const sa_pair *pairs, int64_t np, int device, sa_scorer **out)
{
    return create_scorer(P, WaveSpec::gaps(gap_open, gap_extend).extending(xdrop).within(width).from_seeds(seeds), pairs, np, device, out);
}

int sa_score_batch_seeds_band(const sa_params *P, int32_t gap_open, int32_t gap_extend, int32_t xdrop, int32_t width,
                              const sa_seed *seeds, const sa_host_pair *pairs, int64_t np, int device, sa_seed_result *out)
{
    return score_batch(P, WaveSpec::gaps(gap_open, gap_extend).extending(xdrop).within(width).from_seeds(seeds), pairs, np, device, out,
                       sa_scorer_fetch_seeds);
}

int sa_scorer_destroy(sa_scorer *s)
{
    free_scorer(s);
    return SA_OK;
}

int sa_scorer_run(sa_scorer *s, const void *d_text, const void *d_pattern, void *stream)
{
    if (!s || ((!d_text || !d_pattern) && s->input_bytes)) return fail(SA_ERR_INVALID, "sa_scorer_run: null argument");
    DeviceGuard dg(s->device);
    if (!dg.ok) return fail(SA_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    // the run's first enqueued operation: the work counter and the bad-input flag at zero
    HIP_TRY(hipMemsetAsync(s->d_ctrl, 0, 256, st));
    s->ran = true;
    // a seeds scorer: the plan is the work items', filled in one launch (both halves of every pair balance
    // over the waves), then the combine of the pairs
    if ((s->spec.seeded ? s->seed_pairs : s->num_pairs) == 0) return SA_OK;
    if (s->num_pairs)
    {
        WaveArgs a = {};
        a.sa = score_args(*s, d_text, d_pattern, s->d_pairs, s->d_order, s->num_pairs, s->d_table, s->d_rows, s->d_out, s->d_ctrl);
        if (s->spec.seeded) a.items = s->d_items;
        else a.bands = s->d_bands;
        if (!launch_wave<false>(wave_choice(s->spec, s->mode), s->R, s->A <= 4, s->grid, st, a))
            return fail(SA_ERR_UNSUPPORTED, "sa_scorer_run: the scorer's variant has no kernel instance");
        HIP_TRY(hipGetLastError());
    }
    if (s->spec.chained)
    {
        // the gap items, the global program in a launch of its own plan (R and grid from the gaps' shapes), then the
        // combine of the pairs
        if (s->gaps.num_pairs)
        {
            WaveArgs a = {};
            a.sa = score_args(s->gaps, d_text, d_pattern, nullptr, s->d_gap_order, s->gaps.num_pairs, s->d_table, s->d_gap_rows, s->d_gap_out,
                              s->d_ctrl + 2);
            a.items = s->d_gap_items;
            if (!launch_wave<false>(wave_choice(s->gaps.spec, s->gaps.mode), s->gaps.R, s->A <= 4, s->gaps.grid, st, a))
                return fail(SA_ERR_UNSUPPORTED, "sa_scorer_run: the chains scorer's gap items have no kernel instance");
            HIP_TRY(hipGetLastError());
        }
        ChainsCombineArgs c;
        c.text = (const int8_t *)d_text;
        c.pattern = (const int8_t *)d_pattern;
        c.pairs = s->d_chain_pairs;
        c.seeds = s->d_chain_seeds;
        c.order = nullptr;
        c.table = s->d_table;
        c.end_out = s->d_out;
        c.gap_out = s->d_gap_out;
        c.out = s->d_seed_out;
        c.ctrl = s->d_ctrl;
        c.A = s->A;
        launch_chains_combine(c, s->seed_pairs, st);
        HIP_TRY(hipGetLastError());
    }
    else if (s->spec.seeded)
    {
        SeedsCombineArgs c;
        c.text = (const int8_t *)d_text;
        c.pattern = (const int8_t *)d_pattern;
        c.pairs = s->d_seed_pairs;
        c.order = nullptr;
        c.table = s->d_table;
        c.item_out = s->d_out;
        c.out = s->d_seed_out;
        c.ctrl = s->d_ctrl;
        c.A = s->A;
        launch_seeds_combine(c, s->seed_pairs, st);
        HIP_TRY(hipGetLastError());
    }
    return SA_OK;
}

int sa_scorer_fetch_seeds(sa_scorer *s, sa_seed_result *out, void *stream)
{
    if (!s || !s->spec.seeded) return fail(SA_ERR_INVALID, "sa_scorer_fetch_seeds: not a seeds scorer");
    if (!out && s->seed_pairs) return fail(SA_ERR_INVALID, "sa_scorer_fetch_seeds: null argument");
    if (!s->ran) return fail(SA_ERR_INVALID, "sa_scorer_fetch_seeds: the scorer has not been run");
    DeviceGuard dg(s->device);
    if (!dg.ok) return fail(SA_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    uint32_t ctrl[4] = {0, 0, 0, 0};  // [3]: the bad-input flag of a chains scorer's gap launch
    HIP_TRY(hipMemcpyAsync(ctrl, s->d_ctrl, sizeof(ctrl), hipMemcpyDeviceToHost, st));
    if (s->seed_pairs)
        HIP_TRY(hipMemcpyAsync(out, s->d_seed_out, (size_t)s->seed_pairs * sizeof(sa_seed_result), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (ctrl[1] || ctrl[3]) return fail(SA_ERR_INVALID, "a text or pattern byte is outside the alphabet (0..A-1)");
    return SA_OK;
}

int sa_scorer_fetch(sa_scorer *s, sa_score_result *out, void *stream)
{
    if (s && s->spec.seeded)
    {
        // a seeds scorer: the score with the absolute end cell
        if (!out && s->seed_pairs) return fail(SA_ERR_INVALID, "sa_scorer_fetch: null argument");
        std::vector<sa_seed_result> sr((size_t)s->seed_pairs);
        if (int rc = sa_scorer_fetch_seeds(s, sr.data(), stream)) return rc;
        for (int64_t p = 0; p < s->seed_pairs; ++p) out[p] = sa_score_result{sr[p].score, sr[p].status, sr[p].end_text, sr[p].end_pattern};
        return SA_OK;
    }
    if (!s || (!out && s->num_pairs)) return fail(SA_ERR_INVALID, "sa_scorer_fetch: null argument");
    if (!s->ran) return fail(SA_ERR_INVALID, "sa_scorer_fetch: the scorer has not been run");
    DeviceGuard dg(s->device);
    if (!dg.ok) return fail(SA_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    uint32_t ctrl[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(ctrl, s->d_ctrl, sizeof(ctrl), hipMemcpyDeviceToHost, st));
    if (s->num_pairs)
        HIP_TRY(hipMemcpyAsync(out, s->d_out, (size_t)s->num_pairs * sizeof(sa_score_result), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (ctrl[1]) return fail(SA_ERR_INVALID, "a text or pattern byte is outside the alphabet (0..A-1)");
    return SA_OK;
}

int sa_scorer_info(const sa_scorer *s, int64_t *num_waves, int32_t *rows_per_lane, uint64_t *device_bytes)
{
    if (!s) return fail(SA_ERR_INVALID, "sa_scorer_info: null scorer");
    // a chains scorer: the larger of its two launches' grids, and the rows per lane of the launch with more cells
    const bool by_gaps = s->spec.chained && s->gaps.padded_cells > s->padded_cells;
    if (num_waves) *num_waves = s->spec.chained ? std::max(s->grid, s->gaps.grid) : s->grid;
    if (rows_per_lane) *rows_per_lane = by_gaps ? s->gaps.R : s->R;
    if (device_bytes) *device_bytes = s->device_bytes;
    return SA_OK;
}

int sa_score_batch(const sa_params *P, const sa_host_pair *pairs, int64_t np, int device, sa_score_result *out)
{
    return score_batch(P, WaveSpec(), pairs, np, device, out);
}

int sa_score_batch_affine(const sa_params *P, int32_t gap_open, int32_t gap_extend, const sa_host_pair *pairs, int64_t np,
                          int device, sa_score_result *out)
{
    return score_batch(P, WaveSpec::gaps(gap_open, gap_extend), pairs, np, device, out);
}

int sa_score_batch_banded(const sa_params *P, int32_t gap_open, int32_t gap_extend, int32_t band, const sa_host_pair *pairs,
                          int64_t np, int device, sa_score_result *out)
{
    return score_batch(P, WaveSpec::gaps(gap_open, gap_extend).in_band(band), pairs, np, device, out);
}

int sa_score_batch_band_at(const sa_params *P, int32_t gap_open, int32_t gap_extend, const sa_band *bands,
                           const sa_host_pair *pairs, int64_t np, int device, sa_score_result *out)
{
    return score_batch(P, WaveSpec::gaps(gap_open, gap_extend).in_bands(bands), pairs, np, device, out);
}

int sa_score_batch_extend(const sa_params *P, int32_t gap_open, int32_t gap_extend, int32_t xdrop, const sa_host_pair *pairs,
                          int64_t np, int device, sa_score_result *out)
{
    return score_batch(P, WaveSpec::gaps(gap_open, gap_extend).extending(xdrop), pairs, np, device, out);
}

int sa_score_batch_extend_band(const sa_params *P, int32_t gap_open, int32_t gap_extend, int32_t xdrop, int32_t width,
                               const sa_host_pair *pairs, int64_t np, int device, sa_score_result *out)
{
    return score_batch(P, WaveSpec::gaps(gap_open, gap_extend).extending(xdrop).within(width), pairs, np, device, out);
}

}  // extern "C"

// The hits of a linear search through a plan: the texts and the query are already on the device.
static int align_hits_linear(const sa_params *P, const std::vector<sa_pair> &hp, int device, const void *d_text,
                             const void *d_query, sa_result *hit_results, char *const *aligned_text,
                             char *const *aligned_pattern)
{
    const int64_t nh = (int64_t)hp.size();
    int rc;
    sa_plan *plan = nullptr;
    if ((rc = sa_plan_create(P, hp.data(), nh, device, &plan))) return rc;
    std::unique_ptr<sa_plan, int (*)(sa_plan *)> hold(plan, sa_plan_destroy);
    if ((rc = sa_plan_fill(plan, d_text, d_query, nullptr))) return rc;
    if ((rc = sa_plan_traceback(plan, nullptr))) return rc;
    const uint64_t ob = sa_plan_output_bytes(plan);
    std::vector<char> tbuf(std::max<uint64_t>(ob, 1)), pbuf(std::max<uint64_t>(ob, 1));
    std::vector<uint64_t> offs((size_t)nh);
    const bool strings = aligned_text != nullptr;
    if ((rc = sa_plan_fetch_all(plan, hit_results, strings ? tbuf.data() : nullptr, strings ? pbuf.data() : nullptr,
                                tbuf.size(), offs.data(), nullptr)))
        return rc;
    for (int64_t h = 0; h < nh; ++h)
    {
        const uint64_t L = std::min<uint64_t>(hit_results[h].num_alignment_bytes, hp[h].text_len + hp[h].pattern_len);
        if (strings && L)
        {
            std::memcpy(aligned_text[h], tbuf.data() + offs[h], L);
            std::memcpy(aligned_pattern[h], pbuf.data() + offs[h], L);
        }
    }
    return SA_OK;
}

// sa_search and sa_search_affine: `spec` without the affine gap model is the linear search. They differ in the scorer they
// create and in the aligner of the hits.
static int search(const sa_params *P, const WaveSpec &spec, const char *query, uint64_t m, const char *const *texts,
                  const uint64_t *text_lens, int64_t nt, int k, int device, sa_score_result *scores, int64_t *hit_index,
                  sa_result *hit_results, char *const *aligned_text, char *const *aligned_pattern, int64_t *num_hits)
{
    if (!P || nt < 0 || k < 0 || (m && !query) || (nt > 0 && (!texts || !text_lens)) || !num_hits ||
        (k > 0 && (!hit_index || !hit_results)) || ((aligned_text == nullptr) != (aligned_pattern == nullptr)))
        return fail(SA_ERR_INVALID, "sa_search: bad argument");
    *num_hits = 0;
    DeviceGuard dg(device);
    if (!dg.ok) return fail(SA_ERR_HIP, "hipSetDevice failed");
    // every text against the one copy of the query
    std::vector<sa_pair> dp((size_t)nt);
    uint64_t tb = 0;
    for (int64_t i = 0; i < nt; ++i)
    {
        if (text_lens[i] && !texts[i]) return fail(SA_ERR_INVALID, "sa_search: null text");
        dp[i] = sa_pair{tb, text_lens[i], 0, m};
        tb += text_lens[i];
    }
    std::vector<sa_score_result> sc((size_t)nt);
    DevBuf<char> dt, dq;
    int rc;
    {
        sa_scorer *raw = nullptr;
        if ((rc = create_scorer(P, spec, dp.data(), nt, device, &raw))) return rc;
        std::unique_ptr<sa_scorer, void (*)(sa_scorer *)> s(raw, free_scorer);
        std::vector<char> ht(tb);
        for (int64_t i = 0; i < nt; ++i)
            if (text_lens[i]) std::memcpy(ht.data() + dp[i].text_offset, texts[i], text_lens[i]);
        if ((rc = dmalloc(&dt.p, tb)) || (rc = dmalloc(&dq.p, m))) return rc;
        if (tb) HIP_TRY(hipMemcpy(dt.p, ht.data(), tb, hipMemcpyHostToDevice));
        if (m) HIP_TRY(hipMemcpy(dq.p, query, m, hipMemcpyHostToDevice));
        if ((rc = sa_scorer_run(s.get(), dt.p, dq.p, nullptr))) return rc;
        if ((rc = sa_scorer_fetch(s.get(), sc.data(), nullptr))) return rc;
    }
    if (scores && nt) std::memcpy(scores, sc.data(), (size_t)nt * sizeof(sa_score_result));
    // the k best: score descending, ties to the lower index
    const int64_t nh = std::min<int64_t>(k, nt);
    if (nh == 0) return SA_OK;
    std::vector<int64_t> rank((size_t)nt);
    std::iota(rank.begin(), rank.end(), 0);
    std::partial_sort(rank.begin(), rank.begin() + nh, rank.end(), [&](int64_t x, int64_t y) {
        return sc[x].score != sc[y].score ? sc[x].score > sc[y].score : x < y;
    });
    // the hits: the texts and the query are already on the device
    std::vector<sa_pair> hp((size_t)nh);
    for (int64_t h = 0; h < nh; ++h) hp[h] = dp[rank[h]];
    // the plans have no fit and no ends-free modes: a linear search in one of them aligns through the
    // traced path with gap_open = gap_extend = gap_penalty, which is the linear recurrence
    const bool traced = spec.affine || P->mode == SA_FIT || (P->mode & SA_ENDS_FREE);
    const WaveSpec hs = spec.affine ? spec : WaveSpec::gaps(P->gap_penalty, P->gap_penalty);
    rc = traced ? align_affine_device(P, hs, hp.data(), nh, device, dt.p, dq.p, hit_results, aligned_text, aligned_pattern)
                : align_hits_linear(P, hp, device, dt.p, dq.p, hit_results, aligned_text, aligned_pattern);
    if (rc) return rc;
    for (int64_t h = 0; h < nh; ++h) hit_index[h] = rank[h];
    *num_hits = nh;
    return SA_OK;
}

extern "C" {

int sa_search(const sa_params *P, const char *query, uint64_t m, const char *const *texts, const uint64_t *text_lens,
              int64_t nt, int k, int device, sa_score_result *scores, int64_t *hit_index, sa_result *hit_results,
              char *const *aligned_text, char *const *aligned_pattern, int64_t *num_hits)
{
    return search(P, WaveSpec(), query, m, texts, text_lens, nt, k, device, scores, hit_index, hit_results, aligned_text,
                  aligned_pattern, num_hits);
}

int sa_search_affine(const sa_params *P, int32_t gap_open, int32_t gap_extend, const char *query, uint64_t m,
                     const char *const *texts, const uint64_t *text_lens, int64_t nt, int k, int device,
                     sa_score_result *scores, int64_t *hit_index, sa_result *hit_results, char *const *aligned_text,
                     char *const *aligned_pattern, int64_t *num_hits)
{
    return search(P, WaveSpec::gaps(gap_open, gap_extend), query, m, texts, text_lens, nt, k, device, scores, hit_index, hit_results, aligned_text,
                  aligned_pattern, num_hits);
}

}  // extern "C"
