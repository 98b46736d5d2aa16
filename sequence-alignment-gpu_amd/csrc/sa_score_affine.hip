// Score-only path with affine gap penalties (sa_hip.h: sa_score_batch_affine, sa_scorer_create_affine):
// Gotoh's three-state recurrence, a gap of k cells costing gap_open + (k - 1) gap_extend.
//
//   E[i][j] = max(E[i][j-1] - ge, H[i][j-1] - go)      gap run along the row
//   F[i][j] = max(F[i-1][j] - ge, H[i-1][j] - go)      gap run along the column
//   H[i][j] = max(H[i-1][j-1] + S[p[i-1]][t[j-1]], E[i][j], F[i][j])      local: max(0, .)
//
// score_affine_kernel<R, LOCAL, SMALL> has score_kernel's shape (sa_score.hip): persistent, one wave
// per workgroup, pairs drawn from the work order with one atomicAdd, lane l owning R rows of a 64 R
// row strip at column t - l + 1 of step t, the strips of a pair one after another in the same wave, no
// wave ever waiting for another. Per row a lane keeps H[row][column - 1] and E[row][column - 1]; F
// runs down the lane's R rows inside a step, and the lane above hands down H and F of its bottom row
// (two DPP shifts where the linear kernel has one). The wave's boundary row holds (H, F) of the
// strip's bottom row, two ints per column, read and written as one 8-byte access per lane per
// 64-step body under the linear kernel's in-place rule: the writes trail the reads by at least 63
// columns. The borders need no minus infinity: E[i][0] := H[i][0] - go + ge and
// F[0][j] := H[0][j] - go + ge make the first step of a run yield H - go from both branches.
// The local result is the first maximum in row-major order, as in score_kernel. DESIGN.md §3.4 has
// the resource usage of the instances and the step costs the planner uses.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "sa_hip.h"
#include "sa_score_args.h"
#include "sa_wave.h"

namespace sa {

struct ScoreAffineArgs {
    ScoreArgs s;
    int32_t gap_extend;
};

template <int R, bool LOCAL, bool SMALL>
__global__ __launch_bounds__(64) void score_affine_kernel(ScoreAffineArgs aa)
{
    __shared__ int32_t tab[SMALL ? 1 : 32 * 32];
    const ScoreArgs &a = aa.s;
    const int lane = threadIdx.x;
    const int A = a.A, go = a.gap, ge = aa.gap_extend;
    if (!SMALL)
    {
        for (int e = lane; e < A * A; e += kWave) tab[e] = a.table[e];
        __syncthreads();
    }
    int2 *const rowbuf = (int2 *)a.rows + (uint64_t)blockIdx.x * a.row_stride;
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
            // H[m][n] of an empty side is one gap run of max(n, m) cells
            if (lane == 0)
            {
                const int k = max(n, m);
                sa_score_result r;
                r.score = LOCAL || k == 0 ? 0 : -(go + (k - 1) * ge);
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
            int el[R];                 // E[row][column - 1]
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
                hl[r] = LOCAL ? 0 : -(go + (row1 + r) * ge);  // H[row][0], row = row1 + r + 1
                el[r] = hl[r] - go + ge;                       // stands for E[row][0] = -infinity
                best[r] = 0;
                bestt[r] = 0;
            }
            int upprev = LOCAL || row1 == 0 ? 0 : -(go + (row1 - 1) * ge);  // H[row1][column - 1]
            int fb = 0;                                       // F[row1 + R][column] of the lane's last step
            int tl = 0, tfeed = 0, feedh = 0, feedf = 0, ofeedh = 0, ofeedf = 0;
            auto step = [&](auto predc, const int t) {
                constexpr bool PRED = decltype(predc)::value;
                const int uph = dpp_shr1(feedh, hl[R - 1]);  // lane 0: the top row's next column, H
                const int upf = dpp_shr1(feedf, fb);         // and F
                tl = dpp_shr1(tfeed, tl);                    // lane 0: the next text letter
                feedh = dpp_shl1(feedh, feedh);
                feedf = dpp_shl1(feedf, feedf);
                tfeed = dpp_shl1(tfeed, tfeed);
                // ramp-up and ramp-down bodies: a lane outside columns 1..n keeps its state
                const bool valid = !PRED || (unsigned)(t - lane) < (unsigned)n;
                const bool b0 = (tl & 1) != 0, b1 = (tl & 2) != 0;
                int d = upprev, uh = uph, uf = upf;
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
                    int e = max(el[r] - ge, hl[r] - go);
                    int f = max(uf - ge, uh - go);
                    int h = max(d + sv, max(e, f));
                    if (LOCAL) h = max(h, 0);
                    d = hl[r];
                    if (PRED)
                    {
                        h = valid ? h : hl[r];
                        e = valid ? e : el[r];
                    }
                    if (LOCAL)
                    {
                        // a row meets its columns in ascending order: strictly greater keeps the first
                        const bool better = h > best[r];
                        best[r] = better ? h : best[r];
                        bestt[r] = better ? t : bestt[r];
                    }
                    hl[r] = h;
                    el[r] = e;
                    uh = h;
                    uf = f;
                }
                upprev = valid ? uph : upprev;
                fb = valid ? uf : fb;
                // lane 63's bottom-row (H, F) enters, the rest move down
                ofeedh = dpp_shl1(hl[R - 1], ofeedh);
                ofeedf = dpp_shl1(fb, ofeedf);
            };
            for (int b = 0; b < nbodies; ++b)
            {
                const int c0 = 64 * b + lane;  // text index of tfeed; the feed holds column c0 + 1
                tfeed = 0;
                if (c0 < n)
                {
                    const int c = text[c0];
                    bad = bad || c < 0 || c >= A;
                    tfeed = min(max(c, 0), A - 1);
                }
                if (s == 0)
                {
                    feedh = LOCAL ? 0 : -(go + c0 * ge);  // H[0][c0 + 1]
                    feedf = feedh - go + ge;              // stands for F[0][c0 + 1] = -infinity
                }
                else
                {
                    const int2 v = c0 < n ? rowbuf[c0] : make_int2(0, 0);
                    feedh = v.x;
                    feedf = v.y;
                }
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
                // the 64 pairs lane 63 produced in this body: columns 64 b - 62 .. 64 b + 1, all read before
                if (s + 1 < nstrips)
                {
                    const int col = 64 * b - 62 + lane;
                    if (col >= 1 && col <= n) rowbuf[col - 1] = make_int2(ofeedh, ofeedf);
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

namespace {

template <int R>
void launch_affine_r(const ScoreAffineArgs &a, bool local, bool small, int grid, hipStream_t st)
{
    if (local)
    {
        if (small) hipLaunchKernelGGL((score_affine_kernel<R, true, true>), dim3(grid), dim3(64), 0, st, a);
        else hipLaunchKernelGGL((score_affine_kernel<R, true, false>), dim3(grid), dim3(64), 0, st, a);
    }
    else
    {
        if (small) hipLaunchKernelGGL((score_affine_kernel<R, false, true>), dim3(grid), dim3(64), 0, st, a);
        else hipLaunchKernelGGL((score_affine_kernel<R, false, false>), dim3(grid), dim3(64), 0, st, a);
    }
}

}  // namespace

void launch_score_affine(const ScoreArgs &a, int gap_extend, int R, bool local, bool small, int grid, hipStream_t st)
{
    ScoreAffineArgs aa;
    aa.s = a;
    aa.gap_extend = gap_extend;
    switch (R)
    {
    case 1: launch_affine_r<1>(aa, local, small, grid, st); break;
    case 2: launch_affine_r<2>(aa, local, small, grid, st); break;
    case 4: launch_affine_r<4>(aa, local, small, grid, st); break;
    default: launch_affine_r<8>(aa, local, small, grid, st); break;
    }
}

}  // namespace sa
