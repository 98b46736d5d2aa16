// Chaining (sa_hip.h sa_chain_anchors): chain_dp_kernel, the recurrence of sa_hip.h one wave per pair, and
// chain_walk_kernel, which follows the predecessors back into a seed array of exactly the counted size; the host
// side that runs them and the C ABI. The definition itself, the validation and the host function's body are plain
// C++ in sa_chain_plan.cpp. DESIGN.md §3.6 has the reasoning.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "sa_chain_plan.h"
#include "sa_hip.h"
#include "sa_host.h"
#include "sa_wave.h"

namespace sa {

constexpr int kChainRing = 1024;             // the largest lookback: anchor i lives in slot i & 1023
constexpr int kChainSaturate = 1 << 30;      // a cost that reaches it can never be chosen (f < 2^30)
constexpr int kChainNone = INT32_MIN;        // the candidate of a lane without an admissible predecessor

struct ChainRun {
    const int32_t *ex, *ey, *len;   // the call's anchors, structure of arrays
    const uint64_t *off;            // num_pairs + 1
    const uint32_t *order;          // pairs, most anchors first
    unsigned int *counter;          // the work draw
    int32_t *pred, *cut;            // per anchor: index of the predecessor within the pair (-1: none) and the o of its transition
    ChainHead *heads;               // per pair
    const uint64_t *seeds_off;      // walk: num_pairs + 1
    sa_seed *seeds;                 // walk
    uint32_t num_pairs;
    sa_chain_params cp;
};

__device__ __forceinline__ int wave_max(int x) { return __builtin_amdgcn_readlane(wave_prefix_max(x), kWave - 1); }

// One wave64 per workgroup; a wave draws pairs from the counter until none is left. A pair's anchors are taken 64
// at a time into registers (lane l anchor base + l, one coalesced load each of ex, ey and L) and then handled in
// index order: anchor i's three values come out of those registers by readlane, so they are wave-uniform, and in
// round r lane l evaluates predecessor j = i - 1 - l - 64 r from the ring. A lane keeps the best of its rounds
// (strictly greater only: its j falls from round to round, so the largest j stays); after the last round one wave
// maximum finds the value and a second one, over the lanes that hold it, the largest j. ex, ey, f and the chain
// length of the last 1024 anchors are an LDS ring (16 KiB, 12 of them the window the transition reads), written by
// lane 0 once f(i) is known, so the serial loop never waits on global memory for what the wave just produced; the
// workgroup is one wave, so the barrier between that store and the next anchor's loads is a wait on LDS alone.
// pred and o of the 64 anchors collect in the lane of each anchor and go out as one coalesced store a block. The
// running best (f, index, length) is wave-uniform. A round whose every predecessor ends left of x_i - max_gap ends
// the anchor: the order makes that true of every earlier round too.
__global__ __launch_bounds__(64) void chain_dp_kernel(ChainRun a)
{
    __shared__ int32_t ring_ex[kChainRing], ring_ey[kChainRing], ring_f[kChainRing], ring_n[kChainRing];
    const int lane = threadIdx.x;
    const sa_chain_params cp = a.cp;
    const int64_t far_gap = cp.max_gap;
    for (;;)
    {
        // Every lane takes part in the draw, lane 0 adding 1 and the others 0, so that no branch on the lane stands
        // between the end of a pair and the readfirstlane below: behind `if (lane == 0)` the compiler threads the
        // other lanes from the end of the body straight to a readfirstlane that then reads lane 1's zero, for ever.
        unsigned int drawn = atomicAdd(a.counter, lane == 0 ? 1u : 0u);
        drawn = (unsigned int)uniform((int)drawn);
        if (drawn >= a.num_pairs) return;
        const uint32_t pair = (uint32_t)uniform((int)a.order[drawn]);
        const uint64_t first = uniform64(a.off[pair]), count = uniform64(a.off[pair + 1]) - first;
        int32_t best_f = 0;
        uint32_t best_i = 0, best_n = 0;
        __syncthreads();  // the ring of the pair before is read no more
        for (uint64_t base = 0; base < count; base += kWave)
        {
            const int block = count - base < (uint64_t)kWave ? (int)(count - base) : kWave;
            const bool mine = lane < block;
            const int32_t my_ex = mine ? a.ex[first + base + lane] : 0, my_ey = mine ? a.ey[first + base + lane] : 0;
            const int32_t my_len = mine ? a.len[first + base + lane] : 1;
            int32_t my_pred = -1, my_cut = 0;
            for (int ii = 0; ii < block; ++ii)
            {
                const uint64_t i = base + (uint64_t)ii;
                const int32_t exi = __builtin_amdgcn_readlane(my_ex, ii), eyi = __builtin_amdgcn_readlane(my_ey, ii);
                const int32_t Li = __builtin_amdgcn_readlane(my_len, ii);
                const int32_t xi = exi - Li, yi = eyi - Li;
                const uint32_t reach = i < (uint64_t)cp.lookback ? (uint32_t)i : (uint32_t)cp.lookback;
                int32_t cand = kChainNone, cand_j = -1, cand_o = 0, cand_n = 0;
                for (uint32_t d0 = 0; d0 < reach; d0 += kWave)
                {
                    const uint32_t d = d0 + 1 + (uint32_t)lane;  // i - j
                    const bool valid = d <= reach;
                    const uint32_t j = (uint32_t)i - d, slot = j & (kChainRing - 1);
                    // every lane reads its slot, which is inside the ring whatever j is; an idle lane's stale values become 0
                    const int32_t slot_ex = ring_ex[slot], slot_ey = ring_ey[slot], slot_f = ring_f[slot], nj = ring_n[slot];
                    const int32_t exj = valid ? slot_ex : 0, eyj = valid ? slot_ey : 0, fj = valid ? slot_f : 0;
                    const int32_t o = max(0, max(exj - xi, eyj - yi));
                    bool ok = valid && o < Li;
                    const uint32_t dx = (uint32_t)xi + (uint32_t)o - (uint32_t)exj, dy = (uint32_t)yi + (uint32_t)o - (uint32_t)eyj;
                    const uint32_t dd = dx > dy ? dx - dy : dy - dx, lo = dx < dy ? dx : dy;
                    ok = ok && dx <= (uint32_t)cp.max_gap && dy <= (uint32_t)cp.max_gap && dd <= (uint32_t)cp.max_diag;
                    uint64_t cost = dd ? (uint64_t)(uint32_t)cp.gap_open + (uint64_t)(dd - 1) * (uint32_t)cp.gap_extend : 0;
                    cost += (uint64_t)lo * (uint32_t)cp.skip;
                    const int32_t paid = cost < (uint64_t)kChainSaturate ? (int32_t)cost : kChainSaturate;
                    const int32_t kept = ok ? Li - o : 0;
                    const int32_t v = ok ? fj + cp.match * kept - paid : kChainNone;  // both terms below 2^30, paid at most 2^30
                    if (v > cand) cand = v, cand_j = (int32_t)j, cand_o = o, cand_n = nj;
                    if (all_lanes(!valid || (int64_t)exj < (int64_t)xi - far_gap)) break;
                }
                const int32_t anew = cp.match * Li;
                const int32_t top = wave_max(cand);
                int32_t f = anew, from = -1, o_taken = 0;
                uint32_t n = 1;
                if (top > anew)
                {
                    from = wave_max(cand == top ? cand_j : -1);
                    const int holder = __builtin_ctzll(ballot(cand == top && cand_j == from));
                    o_taken = __builtin_amdgcn_readlane(cand_o, holder);
                    n = (uint32_t)__builtin_amdgcn_readlane(cand_n, holder) + 1;
                    f = top;
                }
                if (lane == ii) my_pred = from, my_cut = o_taken;
                if (i == 0 || f > best_f) best_f = f, best_i = (uint32_t)i, best_n = n;
                if (lane == 0)
                {
                    const uint32_t slot = (uint32_t)i & (kChainRing - 1);
                    ring_ex[slot] = exi, ring_ey[slot] = eyi, ring_f[slot] = f, ring_n[slot] = (int32_t)n;
                }
                __syncthreads();
            }
            if (mine) a.pred[first + base + lane] = my_pred, a.cut[first + base + lane] = my_cut;
        }
        if (lane == 0) a.heads[pair] = ChainHead{best_f, best_i, best_n, 0};
    }
}

// One lane per pair. The walk takes exactly the counted number of steps from the chain's last anchor, last seed
// first, and every store is guarded by that count, which is also the size of the pair's part of the seed array (the
// host laid the offsets out from the same heads): a predecessor that were wrong could neither run on nor write
// outside. An index outside the pair ends the walk.
__global__ __launch_bounds__(64) void chain_walk_kernel(ChainRun a)
{
    const uint64_t pair = (uint64_t)blockIdx.x * kWave + threadIdx.x;
    if (pair >= a.num_pairs) return;
    const uint64_t first = a.off[pair], count = a.off[pair + 1] - first;
    const uint64_t out = a.seeds_off[pair], room = a.seeds_off[pair + 1] - out;
    const ChainHead head = a.heads[pair];
    const uint64_t steps = head.num_seeds < room ? head.num_seeds : room;
    uint64_t i = head.last;
    for (uint64_t s = steps; s-- > 0;)
    {
        if (i >= count) break;
        const int32_t L = a.len[first + i], o = a.cut[first + i], from = a.pred[first + i];
        a.seeds[out + s] = sa_seed{(uint64_t)(a.ex[first + i] - L + o), (uint64_t)(a.ey[first + i] - L + o), (uint64_t)(L - o)};
        i = from < 0 ? count : (uint64_t)from;
    }
}

}  // namespace sa

using namespace sa;

namespace {

struct ChainStats {
    double dp_ms = 0, walk_ms = 0;
    uint64_t device_bytes = 0;
};
thread_local ChainStats g_chain_stats;

struct ChainEvents {
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    ~ChainEvents()
    {
        for (hipEvent_t one : e)
            if (one) (void)hipEventDestroy(one);
    }
};

size_t round16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

// The device run of a validated call: results, seeds and offsets as chain_host leaves them
int chain_device(const ChainPlan &plan, int device, sa_chain_result *results, std::vector<sa_seed> *seeds, std::vector<uint64_t> *seeds_off)
{
    const size_t np = (size_t)plan.num_pairs, total = plan.ex.size();
    seeds->clear();
    seeds_off->assign(np + 1, 0);
    if (np == 0) return SA_OK;
    DeviceGuard dg(device);
    if (!dg.ok) return fail(SA_ERR_HIP, "hipSetDevice failed");
    // one buffer: the 8-byte arrays first (anchor offsets, seed offsets, heads), then the 4-byte ones
    const size_t b_off = round16((np + 1) * 8), b_heads = round16(np * sizeof(ChainHead)), b_anchor = round16(total * 4), b_order = round16(np * 4);
    const size_t bytes = 2 * b_off + b_heads + 5 * b_anchor + b_order + 16;
    DevBuf<char> buf;
    DevBuf<sa_seed> d_seeds;
    ChainEvents ev;
    int rc;
    if ((rc = dmalloc(&buf.p, bytes))) return rc;
    char *at = buf.p;
    auto take = [&](size_t n) { char *p = at; at += n; return p; };
    uint64_t *const d_off = (uint64_t *)take(b_off), *const d_seeds_off = (uint64_t *)take(b_off);
    ChainHead *const d_heads = (ChainHead *)take(b_heads);
    int32_t *const d_ex = (int32_t *)take(b_anchor), *const d_ey = (int32_t *)take(b_anchor), *const d_len = (int32_t *)take(b_anchor);
    int32_t *const d_pred = (int32_t *)take(b_anchor), *const d_cut = (int32_t *)take(b_anchor);
    uint32_t *const d_order = (uint32_t *)take(b_order);
    unsigned int *const d_counter = (unsigned int *)take(16);
    hipStream_t st = nullptr;
    for (hipEvent_t &one : ev.e) HIP_TRY(hipEventCreate(&one));
    HIP_TRY(hipMemcpyAsync(d_off, plan.off.data(), (np + 1) * 8, hipMemcpyHostToDevice, st));
    if (total)
    {
        HIP_TRY(hipMemcpyAsync(d_ex, plan.ex.data(), total * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_ey, plan.ey.data(), total * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_len, plan.len.data(), total * 4, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(d_order, plan.order.data(), np * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_counter, 0, 16, st));
    ChainRun a = {d_ex, d_ey, d_len, d_off, d_order, d_counter, d_pred, d_cut, d_heads, d_seeds_off, nullptr, (uint32_t)np, plan.cp};
    // 16 KiB of LDS a wave: ten workgroups fit a compute unit's 160 KiB; eight leave the draw something to balance
    const size_t waves = std::min<size_t>(np, (size_t)device_cus(device) * 8);
    HIP_TRY(hipEventRecord(ev.e[0], st));
    hipLaunchKernelGGL(chain_dp_kernel, dim3((unsigned)waves), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.e[1], st));
    std::vector<ChainHead> heads(np);
    HIP_TRY(hipMemcpyAsync(heads.data(), d_heads, np * sizeof(ChainHead), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    uint64_t sum = 0;
    for (size_t k = 0; k < np; ++k)
    {
        results[k] = sa_chain_result{heads[k].score, SA_OK, sum, heads[k].num_seeds, heads[k].last};
        sum += heads[k].num_seeds;
        (*seeds_off)[k + 1] = sum;
    }
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    g_chain_stats.dp_ms = ms;
    g_chain_stats.device_bytes = bytes;
    if (sum == 0) return SA_OK;
    seeds->resize(sum);
    if ((rc = dmalloc(&d_seeds.p, sum * sizeof(sa_seed)))) return rc;
    g_chain_stats.device_bytes += sum * sizeof(sa_seed);
    HIP_TRY(hipMemcpyAsync(d_seeds_off, seeds_off->data(), (np + 1) * 8, hipMemcpyHostToDevice, st));
    a.seeds = d_seeds.p;
    HIP_TRY(hipEventRecord(ev.e[2], st));
    hipLaunchKernelGGL(chain_walk_kernel, dim3((unsigned)((np + kWave - 1) / kWave)), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.e[3], st));
    HIP_TRY(hipMemcpyAsync(seeds->data(), d_seeds.p, sum * sizeof(sa_seed), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipEventElapsedTime(&ms, ev.e[2], ev.e[3]));
    g_chain_stats.walk_ms = ms;
    return SA_OK;
}

}  // namespace

struct sa_chain_set {
    std::vector<sa_seed> seeds;
    std::vector<uint64_t> off;
};

namespace {

int chain_call(const char *fn, bool on_device, const sa_chain_params *cp, const sa_seed *anchors, const uint64_t *anchor_off, int64_t np,
               int device, sa_chain_result *results, sa_chain_set **out)
{
    if (out) *out = nullptr;
    if (on_device) g_chain_stats = ChainStats();
    if (!results) return fail(SA_ERR_INVALID, std::string(fn) + ": results is null");
    if (!out) return fail(SA_ERR_INVALID, std::string(fn) + ": out is null");
    ChainPlan plan;
    std::string err;
    if (int rc = chain_plan(fn, cp, anchors, anchor_off, np, &plan, &err)) return fail(rc, err);
    sa_chain_set *set = new sa_chain_set;
    if (on_device)
    {
        if (int rc = chain_device(plan, device, results, &set->seeds, &set->off))
        {
            delete set;
            return rc;
        }
    }
    else chain_host(plan, results, &set->seeds, &set->off);
    *out = set;
    return SA_OK;
}

}  // namespace

extern "C" {

int sa_chain_anchors(const sa_chain_params *cp, const sa_seed *anchors, const uint64_t *anchor_off, int64_t np, int device,
                     sa_chain_result *results, sa_chain_set **out)
{
    return chain_call("sa_chain_anchors", true, cp, anchors, anchor_off, np, device, results, out);
}

int sa_chain_anchors_host(const sa_chain_params *cp, const sa_seed *anchors, const uint64_t *anchor_off, int64_t np,
                          sa_chain_result *results, sa_chain_set **out)
{
    return chain_call("sa_chain_anchors_host", false, cp, anchors, anchor_off, np, 0, results, out);
}

const sa_seed *sa_chain_set_seeds(const sa_chain_set *set) { return set && !set->seeds.empty() ? set->seeds.data() : nullptr; }

const uint64_t *sa_chain_set_off(const sa_chain_set *set) { return set ? set->off.data() : nullptr; }

int sa_chain_set_destroy(sa_chain_set *set)
{
    delete set;
    return SA_OK;
}

int sa_chain_last_stats(double *dp_ms, double *walk_ms, uint64_t *device_bytes)
{
    if (dp_ms) *dp_ms = g_chain_stats.dp_ms;
    if (walk_ms) *walk_ms = g_chain_stats.walk_ms;
    if (device_bytes) *device_bytes = g_chain_stats.device_bytes;
    return SA_OK;
}

}  // extern "C"
