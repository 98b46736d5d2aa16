// Score-only path (sa_hip.h: sa_score_batch, sa_scorer_*, sa_search): the score of every pair and
// the cell it is read from, without direction planes, strip descriptors, records or a traceback.
//
// score_kernel<R, LOCAL, SMALL> is persistent with one wave per workgroup. A wave draws the next
// pair of the work order (sa_score_plan.cpp: most cells first) with one atomicAdd and runs the pair's
// strips of 64 R rows one after another; no wave ever waits for another wave. Lane l owns rows
// 64R s + R l + 1 .. + R of strip s and computes, at step t, its R cells of column t - l + 1; H of the
// row above its first row and the text letter come from lane l - 1 by a DPP shift, everything else
// stays in registers. The strip's top row H[64R s][1..n] is read from the wave's own row buffer in
// 64-column bodies (one coalesced dword per lane per 64 steps, shifted to lane 0 one lane per step)
// and its bottom row is collected from lane 63 the same way and written back in place: the writes
// trail the reads by at least 63 columns. The recurrence is the reference's
// (alignSequenceCPU.cpp:175-192, :259-273) in int32; the local result is the first maximum in
// row-major order, taken as the maximum of the key (H, ~row, ~col) over rows, lanes and strips.
// DESIGN.md §3.4 has the resource usage of the instances and the rule for R.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <type_traits>
#include <vector>

#include "sa_hip.h"
#include "sa_score_args.h"
#include "sa_score_plan.h"
#include "sa_wave.h"

namespace sa {

int set_error(int code, const std::string &msg);  // sa_engine.hip: what sa_last_error() reports

template <int R, bool LOCAL, bool SMALL>
__global__ __launch_bounds__(64) void score_kernel(ScoreArgs a)
{
    __shared__ int32_t tab[SMALL ? 1 : 32 * 32];
    const int lane = threadIdx.x;
    const int A = a.A, g = a.gap;
    if (!SMALL)
    {
        for (int e = lane; e < A * A; e += kWave) tab[e] = a.table[e];
        __syncthreads();
    }
    int32_t *const rowbuf = a.rows + (uint64_t)blockIdx.x * a.row_stride;
    const int kb = a.key_rowbits;
    const uint32_t kmask = (1u << kb) - 1u;
    bool bad = false;
    for (;;)
    {
        int w = 0;
        if (lane == 0) w = (int)atomicAdd(&a.ctrl[0], 1u);
        w = uniform(w);
        if (w >= a.np) break;
        const int pi = uniform(a.order[w]);
        const ScorePair pd = a.pairs[pi];
        const int n = uniform((int)pd.n), m = uniform((int)pd.m);
        if (n == 0 || m == 0)
        {
            // H[m][n] of an empty side is a run of gaps (alignSequenceCPU.cpp:232-236, :247-248)
            if (lane == 0)
            {
                sa_score_result r;
                r.score = LOCAL ? 0 : -g * max(n, m);
                r.status = SA_OK;
                r.end_text = LOCAL ? 0 : (uint64_t)n;
                r.end_pattern = LOCAL ? 0 : (uint64_t)m;
                a.out[pi] = r;
            }
            continue;
        }
        const int8_t *const text = a.text + pd.text_off;
        const int8_t *const pattern = a.pattern + pd.pattern_off;
        const int nstrips = (m + 64 * R - 1) / (64 * R);
        const int nbodies = (n + 63 + 63) / 64;  // steps 0 .. n + 62
        int hl[R];  // H[row][column - 1] of the lane's rows; after a strip, H[row][n]
        uint64_t lanekey = 0;
        for (int s = 0; s < nstrips; ++s)
        {
            const int row1 = s * 64 * R + R * lane;  // rows row1 + 1 .. row1 + R
            int s0[R], s1[R], s2[R], s3[R];  // S[pattern letter of the row][0..3] (SMALL)
            int prow[R];               // A * pattern letter of the row (LDS table row)
            int best[R], bestt[R];
#pragma unroll
            for (int r = 0; r < R; ++r)
            {
                int c = 0;
                if (row1 + r < m)
                {
                    c = pattern[row1 + r];
                    bad = bad || c < 0 || c >= A;
                    c = min(max(c, 0), A - 1);
                }
                prow[r] = c * A;
                if constexpr (SMALL)
                {
                    s0[r] = a.table[c * A];
                    s1[r] = 1 < A ? a.table[c * A + 1] : 0;
                    s2[r] = 2 < A ? a.table[c * A + 2] : 0;
                    s3[r] = 3 < A ? a.table[c * A + 3] : 0;
                }
                hl[r] = LOCAL ? 0 : -(row1 + r + 1) * g;
                best[r] = 0;
                bestt[r] = 0;
            }
            int upprev = LOCAL ? 0 : -row1 * g;  // H[row1][column - 1]
            int tl = 0, ofeed = 0, feed = 0, tfeed = 0;
            auto step = [&](auto predc, const int t) {
                constexpr bool PRED = decltype(predc)::value;
                const int up = dpp_shr1(feed, hl[R - 1]);  // lane 0: the top row's next column
                tl = dpp_shr1(tfeed, tl);                  // lane 0: the next text letter
                feed = dpp_shl1(feed, feed);
                tfeed = dpp_shl1(tfeed, tfeed);
                // ramp-up and ramp-down bodies: a lane outside columns 1..n keeps its state
                const bool valid = !PRED || (unsigned)(t - lane) < (unsigned)n;
                const bool b0 = (tl & 1) != 0, b1 = (tl & 2) != 0;
                int d = upprev, u = up;
#pragma unroll
                for (int r = 0; r < R; ++r)
                {
                    int sv;
                    if constexpr (SMALL)
                    {
                        const int x0 = s0[r], x1 = s1[r], x2 = s2[r], x3 = s3[r];
                        sv = b1 ? (b0 ? x3 : x2) : (b0 ? x1 : x0);
                    }
                    else sv = tab[prow[r] + tl];
                    int h = max(d + sv, max(hl[r] - g, u - g));
                    if (LOCAL) h = max(h, 0);
                    d = hl[r];
                    if (PRED) h = valid ? h : hl[r];
                    if (LOCAL)
                    {
                        // a row meets its columns in ascending order: strictly greater keeps the first
                        const bool better = h > best[r];
                        best[r] = better ? h : best[r];
                        bestt[r] = better ? t : bestt[r];
                    }
                    hl[r] = h;
                    u = h;
                }
                upprev = valid ? up : upprev;
                ofeed = dpp_shl1(hl[R - 1], ofeed);  // lane 63's bottom-row value enters, the rest move down
            };
            for (int b = 0; b < nbodies; ++b)
            {
                const int c0 = 64 * b + lane;  // text index of tfeed; feed holds column c0 + 1
                tfeed = 0;
                if (c0 < n)
                {
                    const int c = text[c0];
                    bad = bad || c < 0 || c >= A;
                    tfeed = min(max(c, 0), A - 1);
                }
                if (s == 0) feed = LOCAL ? 0 : -(c0 + 1) * g;
                else feed = c0 < n ? rowbuf[c0] : 0;
                if (b == 0 || 64 * b + 64 > n)
                {
#pragma unroll 2
                    for (int k = 0; k < 64; ++k) step(std::true_type{}, 64 * b + k);
                }
                else
                {
#pragma unroll 4
                    for (int k = 0; k < 64; ++k) step(std::false_type{}, 64 * b + k);
                }
                // the 64 values lane 63 produced in this body: columns 64 b - 62 .. 64 b + 1, all read before
                if (s + 1 < nstrips)
                {
                    const int col = 64 * b - 62 + lane;
                    if (col >= 1 && col <= n) rowbuf[col - 1] = ofeed;
                }
            }
            if (LOCAL)
            {
#pragma unroll
                for (int r = 0; r < R; ++r)
                {
                    const int row = row1 + r + 1, col = bestt[r] - lane + 1;
                    const uint64_t key = ((uint64_t)(uint32_t)best[r] << (2 * kb)) |
                                         ((uint64_t)(~(uint32_t)row & kmask) << kb) | (uint64_t)(~(uint32_t)col & kmask);
                    if (row <= m && best[r] > 0 && key > lanekey) lanekey = key;
                }
            }
        }
        sa_score_result res;
        res.status = SA_OK;
        if (LOCAL)
        {
            const uint64_t key = wave_max_u64(lanekey);
            const uint32_t H = (uint32_t)(key >> (2 * kb));
            res.score = (int32_t)H;
            res.end_pattern = H ? (uint64_t)(~(uint32_t)(key >> kb) & kmask) : 0;
            res.end_text = H ? (uint64_t)(~(uint32_t)key & kmask) : 0;
        }
        else
        {
            const int last = m - 1 - (nstrips - 1) * 64 * R;  // row m inside the last strip
            const int rm = last % R;
            int v = hl[0];
#pragma unroll
            for (int r = 1; r < R; ++r) v = r == rm ? hl[r] : v;
            res.score = __builtin_amdgcn_readlane(v, last / R);
            res.end_text = (uint64_t)n;
            res.end_pattern = (uint64_t)m;
        }
        if (lane == 0) a.out[pi] = res;
    }
    if (bad) __hip_atomic_store(&a.ctrl[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace sa

// ==================================================================================================
// host side
// ==================================================================================================
using namespace sa;

namespace {

int fail_s(int code, const std::string &msg) { return sa::set_error(code, msg); }

#define HIP_TRY_S(expr)                                                                        \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return fail_s(SA_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(e_)); \
    } while (0)

struct DevGuard {
    int prev = -1;
    bool ok = false;
    explicit DevGuard(int device)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(device) == hipSuccess;
    }
    ~DevGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DevGuard(const DevGuard &) = delete;
    DevGuard &operator=(const DevGuard &) = delete;
};

template <typename T>
int dmalloc_s(T **p, size_t bytes)
{
    *p = nullptr;
    if (hipMalloc((void **)p, std::max<size_t>(bytes, 16)) != hipSuccess)
    {
        (void)hipGetLastError();
        *p = nullptr;
        return fail_s(SA_ERR_NOMEM, "device allocation of " + std::to_string(bytes) + " bytes failed");
    }
    return SA_OK;
}

template <int R>
void launch_score_r(const ScoreArgs &a, bool local, bool small, int grid, hipStream_t st)
{
    if (local)
    {
        if (small) hipLaunchKernelGGL((score_kernel<R, true, true>), dim3(grid), dim3(64), 0, st, a);
        else hipLaunchKernelGGL((score_kernel<R, true, false>), dim3(grid), dim3(64), 0, st, a);
    }
    else
    {
        if (small) hipLaunchKernelGGL((score_kernel<R, false, true>), dim3(grid), dim3(64), 0, st, a);
        else hipLaunchKernelGGL((score_kernel<R, false, false>), dim3(grid), dim3(64), 0, st, a);
    }
}

// Device buffer freed on every return path of the one-shot calls.
struct DevBuf {
    char *p = nullptr;
    ~DevBuf()
    {
        if (p) (void)hipFree(p);
    }
};

}  // namespace

struct sa_scorer : ScorePlan {
    int device = 0;
    ScorePair *d_pairs = nullptr;
    int32_t *d_order = nullptr, *d_table = nullptr, *d_rows = nullptr;
    sa_score_result *d_out = nullptr;
    uint32_t *d_ctrl = nullptr;
    bool ran = false;
};

namespace {

void free_scorer(sa_scorer *s)
{
    if (!s) return;
    DevGuard dg(s->device);
    void *bufs[] = {s->d_pairs, s->d_order, s->d_table, s->d_rows, s->d_out, s->d_ctrl};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    delete s;
}

}  // namespace

// sa_scorer_create and sa_scorer_create_affine: `gapm` null is the linear scorer
static int create_scorer(const sa_params *P, const ScoreGap *gapm, const sa_pair *pairs, int64_t np, int device, sa_scorer **out)
{
    if (!out) return fail_s(SA_ERR_INVALID, "sa_scorer_create: null argument");
    *out = nullptr;
    DevGuard dg(device);
    if (!dg.ok) return fail_s(SA_ERR_HIP, "hipSetDevice failed");
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0)
    {
        (void)hipGetLastError();
        cus = 256;
    }
    std::unique_ptr<sa_scorer, void (*)(sa_scorer *)> s(new sa_scorer(), free_scorer);
    s->device = device;
    std::string err;
    if (int rc = make_score_plan(P, pairs, np, cus, score_knobs(), s.get(), &err, gapm)) return fail_s(rc, err);
    std::vector<ScorePair> h((size_t)np);
    for (int64_t p = 0; p < np; ++p)
        h[p] = ScorePair{pairs[p].text_offset, pairs[p].pattern_offset, (uint32_t)pairs[p].text_len, (uint32_t)pairs[p].pattern_len};
    const int A = s->A;
    int rc;
    if ((rc = dmalloc_s(&s->d_pairs, h.size() * sizeof(ScorePair)))) return rc;
    if ((rc = dmalloc_s(&s->d_order, (size_t)np * 4))) return rc;
    if ((rc = dmalloc_s(&s->d_table, 32 * 32 * 4))) return rc;
    if ((rc = dmalloc_s(&s->d_rows, (size_t)s->grid * s->row_stride * (s->affine ? 8 : 4)))) return rc;
    if ((rc = dmalloc_s(&s->d_out, (size_t)np * sizeof(sa_score_result)))) return rc;
    if ((rc = dmalloc_s(&s->d_ctrl, 256))) return rc;
    if (np)
    {
        HIP_TRY_S(hipMemcpy(s->d_pairs, h.data(), h.size() * sizeof(ScorePair), hipMemcpyHostToDevice));
        HIP_TRY_S(hipMemcpy(s->d_order, s->order.data(), (size_t)np * 4, hipMemcpyHostToDevice));
    }
    HIP_TRY_S(hipMemcpy(s->d_table, P->score_matrix, (size_t)A * A * 4, hipMemcpyHostToDevice));
    *out = s.release();
    return SA_OK;
}

// sa_score_batch and sa_score_batch_affine
static int score_batch(const sa_params *P, const ScoreGap *gapm, const sa_host_pair *pairs, int64_t np, int device,
                       sa_score_result *out)
{
    if (!P || np < 0 || (np > 0 && (!pairs || !out))) return fail_s(SA_ERR_INVALID, "sa_score_batch: null argument");
    std::vector<sa_pair> dp((size_t)np);
    uint64_t tb = 0, pb = 0;
    for (int64_t p = 0; p < np; ++p)
    {
        if ((pairs[p].text_len && !pairs[p].text) || (pairs[p].pattern_len && !pairs[p].pattern))
            return fail_s(SA_ERR_INVALID, "sa_score_batch: null sequence");
        dp[p] = sa_pair{tb, pairs[p].text_len, pb, pairs[p].pattern_len};
        tb += pairs[p].text_len;
        pb += pairs[p].pattern_len;
    }
    DevGuard dg(device);
    if (!dg.ok) return fail_s(SA_ERR_HIP, "hipSetDevice failed");
    sa_scorer *raw = nullptr;
    if (int rc = create_scorer(P, gapm, dp.data(), np, device, &raw)) return rc;
    std::unique_ptr<sa_scorer, void (*)(sa_scorer *)> s(raw, free_scorer);
    std::vector<char> ht(tb), hp(pb);
    for (int64_t p = 0; p < np; ++p)
    {
        if (pairs[p].text_len) std::memcpy(ht.data() + dp[p].text_offset, pairs[p].text, pairs[p].text_len);
        if (pairs[p].pattern_len) std::memcpy(hp.data() + dp[p].pattern_offset, pairs[p].pattern, pairs[p].pattern_len);
    }
    DevBuf dt, dpat;
    int rc;
    if ((rc = dmalloc_s(&dt.p, tb)) || (rc = dmalloc_s(&dpat.p, pb))) return rc;
    if (tb) HIP_TRY_S(hipMemcpy(dt.p, ht.data(), tb, hipMemcpyHostToDevice));
    if (pb) HIP_TRY_S(hipMemcpy(dpat.p, hp.data(), pb, hipMemcpyHostToDevice));
    if ((rc = sa_scorer_run(s.get(), dt.p, dpat.p, nullptr))) return rc;
    return sa_scorer_fetch(s.get(), out, nullptr);
}

extern "C" {

int sa_scorer_create(const sa_params *P, const sa_pair *pairs, int64_t np, int device, sa_scorer **out)
{
    return create_scorer(P, nullptr, pairs, np, device, out);
}

int sa_scorer_create_affine(const sa_params *P, int32_t gap_open, int32_t gap_extend, const sa_pair *pairs, int64_t np,
                            int device, sa_scorer **out)
{
    const ScoreGap gapm = {gap_open, gap_extend};
    return create_scorer(P, &gapm, pairs, np, device, out);
}

int sa_scorer_destroy(sa_scorer *s)
{
    free_scorer(s);
    return SA_OK;
}

int sa_scorer_run(sa_scorer *s, const void *d_text, const void *d_pattern, void *stream)
{
    if (!s || ((!d_text || !d_pattern) && s->input_bytes)) return fail_s(SA_ERR_INVALID, "sa_scorer_run: null argument");
    DevGuard dg(s->device);
    if (!dg.ok) return fail_s(SA_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    // the run's first enqueued operation: the work counter and the bad-input flag at zero
    HIP_TRY_S(hipMemsetAsync(s->d_ctrl, 0, 256, st));
    s->ran = true;
    if (s->num_pairs == 0) return SA_OK;
    ScoreArgs a;
    a.text = (const int8_t *)d_text;
    a.pattern = (const int8_t *)d_pattern;
    a.pairs = s->d_pairs;
    a.order = s->d_order;
    a.table = s->d_table;
    a.rows = s->d_rows;
    a.out = s->d_out;
    a.ctrl = s->d_ctrl;
    a.np = (int32_t)s->num_pairs;
    a.A = s->A;
    a.gap = s->gap;
    a.key_rowbits = s->key_rowbits;
    a.row_stride = s->row_stride;
    const bool local = s->mode == SA_LOCAL, small = s->A <= 4;
    if (s->affine)
    {
        launch_score_affine(a, s->gap_extend, s->R, local, small, s->grid, st);
        HIP_TRY_S(hipGetLastError());
        return SA_OK;
    }
    switch (s->R)
    {
    case 1: launch_score_r<1>(a, local, small, s->grid, st); break;
    case 2: launch_score_r<2>(a, local, small, s->grid, st); break;
    case 4: launch_score_r<4>(a, local, small, s->grid, st); break;
    default: launch_score_r<8>(a, local, small, s->grid, st); break;
    }
    HIP_TRY_S(hipGetLastError());
    return SA_OK;
}

int sa_scorer_fetch(sa_scorer *s, sa_score_result *out, void *stream)
{
    if (!s || (!out && s->num_pairs)) return fail_s(SA_ERR_INVALID, "sa_scorer_fetch: null argument");
    if (!s->ran) return fail_s(SA_ERR_INVALID, "sa_scorer_fetch: the scorer has not been run");
    DevGuard dg(s->device);
    if (!dg.ok) return fail_s(SA_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    uint32_t ctrl[2] = {0, 0};
    HIP_TRY_S(hipMemcpyAsync(ctrl, s->d_ctrl, sizeof(ctrl), hipMemcpyDeviceToHost, st));
    if (s->num_pairs)
        HIP_TRY_S(hipMemcpyAsync(out, s->d_out, (size_t)s->num_pairs * sizeof(sa_score_result), hipMemcpyDeviceToHost, st));
    HIP_TRY_S(hipStreamSynchronize(st));
    if (ctrl[1]) return fail_s(SA_ERR_INVALID, "a text or pattern byte is outside the alphabet (0..A-1)");
    return SA_OK;
}

int sa_scorer_info(const sa_scorer *s, int64_t *num_waves, int32_t *rows_per_lane, uint64_t *device_bytes)
{
    if (!s) return fail_s(SA_ERR_INVALID, "sa_scorer_info: null scorer");
    if (num_waves) *num_waves = s->grid;
    if (rows_per_lane) *rows_per_lane = s->R;
    if (device_bytes) *device_bytes = s->device_bytes;
    return SA_OK;
}

int sa_score_batch(const sa_params *P, const sa_host_pair *pairs, int64_t np, int device, sa_score_result *out)
{
    return score_batch(P, nullptr, pairs, np, device, out);
}

int sa_score_batch_affine(const sa_params *P, int32_t gap_open, int32_t gap_extend, const sa_host_pair *pairs, int64_t np,
                          int device, sa_score_result *out)
{
    const ScoreGap gapm = {gap_open, gap_extend};
    return score_batch(P, &gapm, pairs, np, device, out);
}

int sa_search(const sa_params *P, const char *query, uint64_t m, const char *const *texts, const uint64_t *text_lens,
              int64_t nt, int k, int device, sa_score_result *scores, int64_t *hit_index, sa_result *hit_results,
              char *const *aligned_text, char *const *aligned_pattern, int64_t *num_hits)
{
    if (!P || nt < 0 || k < 0 || (m && !query) || (nt > 0 && (!texts || !text_lens)) || !num_hits ||
        (k > 0 && (!hit_index || !hit_results)) || ((aligned_text == nullptr) != (aligned_pattern == nullptr)))
        return fail_s(SA_ERR_INVALID, "sa_search: bad argument");
    *num_hits = 0;
    DevGuard dg(device);
    if (!dg.ok) return fail_s(SA_ERR_HIP, "hipSetDevice failed");
    // every text against the one copy of the query
    std::vector<sa_pair> dp((size_t)nt);
    uint64_t tb = 0;
    for (int64_t i = 0; i < nt; ++i)
    {
        if (text_lens[i] && !texts[i]) return fail_s(SA_ERR_INVALID, "sa_search: null text");
        dp[i] = sa_pair{tb, text_lens[i], 0, m};
        tb += text_lens[i];
    }
    std::vector<sa_score_result> sc((size_t)nt);
    DevBuf dt, dq;
    int rc;
    {
        sa_scorer *raw = nullptr;
        if ((rc = sa_scorer_create(P, dp.data(), nt, device, &raw))) return rc;
        std::unique_ptr<sa_scorer, void (*)(sa_scorer *)> s(raw, free_scorer);
        std::vector<char> ht(tb);
        for (int64_t i = 0; i < nt; ++i)
            if (text_lens[i]) std::memcpy(ht.data() + dp[i].text_offset, texts[i], text_lens[i]);
        if ((rc = dmalloc_s(&dt.p, tb)) || (rc = dmalloc_s(&dq.p, m))) return rc;
        if (tb) HIP_TRY_S(hipMemcpy(dt.p, ht.data(), tb, hipMemcpyHostToDevice));
        if (m) HIP_TRY_S(hipMemcpy(dq.p, query, m, hipMemcpyHostToDevice));
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
    // the hits through a plan: the texts are already on the device
    std::vector<sa_pair> hp((size_t)nh);
    for (int64_t h = 0; h < nh; ++h) hp[h] = dp[rank[h]];
    sa_plan *plan = nullptr;
    if ((rc = sa_plan_create(P, hp.data(), nh, device, &plan))) return rc;
    std::unique_ptr<sa_plan, int (*)(sa_plan *)> hold(plan, sa_plan_destroy);
    if ((rc = sa_plan_fill(plan, dt.p, dq.p, nullptr))) return rc;
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
        hit_index[h] = rank[h];
        const uint64_t L = std::min<uint64_t>(hit_results[h].num_alignment_bytes, hp[h].text_len + m);
        if (strings && L)
        {
            std::memcpy(aligned_text[h], tbuf.data() + offs[h], L);
            std::memcpy(aligned_pattern[h], pbuf.data() + offs[h], L);
        }
    }
    *num_hits = nh;
    return SA_OK;
}

}  // extern "C"
