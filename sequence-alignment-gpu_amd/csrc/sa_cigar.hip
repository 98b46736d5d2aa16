// CIGAR output (sa_hip.h sa_align_pairs_cigar): cigar_encode_kernel, which turns the aligned strings a traced run
// left in its device arenas into BAM-packed run-length ops, the host side that runs it twice (count, then write
// into a buffer of the counted size), the entry point that names a variant by an sa_align_spec, and the host-only
// functions on strings and ops. The strings never reach the host: DESIGN.md §3.5 has the reasoning.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "sa_affine.h"
#include "sa_cigar.h"
#include "sa_hip.h"
#include "sa_host.h"
#include "sa_score_plan.h"
#include "sa_wave.h"

namespace sa {

// What pass 1 leaves per pair and pass 2 reads num_ops of
struct CigarCounts {
    uint32_t num_ops, matches, mismatches, text_gap_letters, pattern_gap_letters, gap_opens;
};

struct CigarArgs {
    const char *text, *pattern;   // the call's two string arenas
    const sa_result *results;     // num_alignment_bytes of every pair
    const uint64_t *tail;         // per pair, the length of the piece at the slot's end; null: the whole string
    const CigarSlot *slots;
    CigarCounts *counts;
    const uint64_t *ops_off;      // pass 2: the pair's first op
    uint32_t *ops;                // pass 2
    int32_t eqx;
    char gap;
};

constexpr int kCigarNone = 15;  // the code before column 0 and of a lane past the last column: equal to no op's

// One wave per pair, grid = pairs. The pair's L columns are the hl bytes at the start of its slot followed by the
// tl bytes at the slot's end (traced_run's host loop has the same two lengths), taken 64 at a time, lane l column
// base + l. Wave-uniform across the steps: the open run (its code and length so far), the number of ops closed,
// the five counts. In a step one ballot marks the lanes whose code differs from the column before them, lane 0
// comparing with the open run's code: the run starts. A lane whose right neighbour starts a run ends one; it finds
// its run's start as the highest start bit at or below itself, or, without one, in the open run, and its op index
// as the ops closed before the step plus the run ends below it. The run that reaches the step's last column stays
// open; a start at lane 0 closes the one carried in, and the last one is closed after the loop. So a run merges
// across the head/tail junction and across any number of steps. No LDS, no atomics, no other workgroup's data;
// WRITE false counts only (pass 1), WRITE true stores the ops and no counts (pass 2).
template <bool WRITE>
__global__ __launch_bounds__(64) void cigar_encode_kernel(CigarArgs a)
{
    const int lane = threadIdx.x;
    const uint64_t pi = blockIdx.x;
    const CigarSlot sl = a.slots[pi];
    const uint64_t slot = uniform64(sl.off), cap = uniform64(sl.cap);
    const uint64_t bytes = uniform64(a.results[pi].num_alignment_bytes), L = bytes < cap ? bytes : cap;
    const uint64_t tail = a.tail ? uniform64(a.tail[pi]) : L, tl = tail < L ? tail : L, hl = L - tl;
    const uint64_t tail_at = slot + cap - tl;
    uint32_t *const ops = WRITE ? a.ops + uniform64(a.ops_off[pi]) : nullptr;
    const uint32_t limit = WRITE ? (uint32_t)uniform((int)a.counts[pi].num_ops) : 0;  // no store beyond the counted ops
    const bool eqx = a.eqx != 0;
    const char gap = a.gap;
    const uint64_t below = (1ull << lane) - 1;
    uint32_t open_code = kCigarNone, open_len = 0, nops = 0;
    uint32_t matches = 0, mismatches = 0, tgaps = 0, pgaps = 0, opens = 0;
    auto put = [&](uint32_t idx, uint32_t len, uint32_t code) {
        if (WRITE && idx < limit) ops[idx] = len << 4 | code;
    };
    for (uint64_t base = 0; base < L; base += kWave)
    {
        const uint64_t col = base + (uint64_t)lane;
        const int count = L - base < (uint64_t)kWave ? (int)(L - base) : kWave;
        const bool valid = lane < count;
        int cls = kCigarNone;
        if (valid)
        {
            const uint64_t at = col < hl ? slot + col : tail_at + (col - hl);
            const char ct = a.text[at], cp = a.pattern[at];
            cls = ct == gap ? SA_CIGAR_OP_I : cp == gap ? SA_CIGAR_OP_D : ct == cp ? SA_CIGAR_OP_EQ : SA_CIGAR_OP_X;
        }
        const int code = valid && !eqx && cls >= SA_CIGAR_OP_EQ ? SA_CIGAR_OP_M : cls;
        const int prev = dpp_shr1((int)open_code, code);
        const uint64_t starts = ballot(valid && code != prev);
        const uint64_t ends = starts >> 1;
        if (open_len != 0 && (starts & 1))
        {
            if (lane == 0) put(nops, open_len, open_code);
            ++nops;
        }
        if ((ends >> lane) & 1)
        {
            const uint64_t mine = starts & (below | (1ull << lane));
            const uint32_t len = mine ? (uint32_t)(lane - (63 - __builtin_clzll(mine)) + 1) : open_len + (uint32_t)lane + 1;
            put(nops + (uint32_t)__builtin_popcountll(ends & below), len, (uint32_t)code);
        }
        nops += (uint32_t)__builtin_popcountll(ends);
        open_len = starts ? (uint32_t)(count - (63 - __builtin_clzll(starts))) : open_len + (uint32_t)count;
        open_code = (uint32_t)__builtin_amdgcn_readlane(code, count - 1);
        if (!WRITE)
        {
            const uint64_t ins = ballot(cls == SA_CIGAR_OP_I), del = ballot(cls == SA_CIGAR_OP_D);
            matches += (uint32_t)__builtin_popcountll(ballot(cls == SA_CIGAR_OP_EQ));
            mismatches += (uint32_t)__builtin_popcountll(ballot(cls == SA_CIGAR_OP_X));
            tgaps += (uint32_t)__builtin_popcountll(ins);
            pgaps += (uint32_t)__builtin_popcountll(del);
            opens += (uint32_t)__builtin_popcountll(starts & (ins | del));
        }
    }
    if (open_len != 0)
    {
        if (lane == 0) put(nops, open_len, open_code);
        ++nops;
    }
    if (!WRITE && lane == 0) a.counts[pi] = CigarCounts{nops, matches, mismatches, tgaps, pgaps, opens};
}

}  // namespace sa

using namespace sa;

namespace {

struct CigarStats {
    double encode_ms = 0;
    uint64_t ops_bytes = 0, string_bytes = 0;
};
thread_local CigarStats g_cigar_stats;

// the four events of one encoder run, destroyed on every return path
struct EncodeEvents {
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    ~EncodeEvents()
    {
        for (hipEvent_t one : e)
            if (one) (void)hipEventDestroy(one);
    }
};

bool flags_ok(int32_t flags) { return flags == SA_CIGAR_M || flags == SA_CIGAR_EQX; }

// the definition of sa_hip.h, column by column: the ops that fit `cap` into `ops`, their number and the counts
uint64_t encode_strings(const char *at, const char *ap, uint64_t len, char gap, bool eqx, uint32_t *ops, uint64_t cap, sa_cigar_result *c)
{
    uint64_t nops = 0;
    uint32_t open_code = kCigarNone, open_len = 0;
    auto close = [&]() {
        if (open_len == 0) return;
        if (nops < cap) ops[nops] = open_len << 4 | open_code;
        ++nops;
    };
    for (uint64_t k = 0; k < len; ++k)
    {
        const bool ins = at[k] == gap, del = !ins && ap[k] == gap, eq = !ins && !del && at[k] == ap[k];
        const uint32_t code = ins ? SA_CIGAR_OP_I : del ? SA_CIGAR_OP_D : !eqx ? SA_CIGAR_OP_M : eq ? SA_CIGAR_OP_EQ : SA_CIGAR_OP_X;
        if (code != open_code)
        {
            close();
            open_code = code;
            open_len = 0;
            c->gap_opens += ins || del;
        }
        ++open_len;
        c->text_gap_letters += ins;
        c->pattern_gap_letters += del;
        c->matches += eq;
        c->mismatches += !ins && !del && !eq;
    }
    close();
    return nops;
}

}  // namespace

struct sa_cigars {
    std::vector<uint32_t> ops;
};

void sa::cigar_reset_stats() { g_cigar_stats = CigarStats(); }

int sa::cigar_encode(void *stream, const char *d_text, const char *d_pattern, uint64_t string_bytes, const sa_result *d_results,
                     const uint64_t *d_tail, const std::vector<CigarSlot> &slots, char gap_letter, CigarSink *sink)
{
    hipStream_t st = (hipStream_t)stream;
    const size_t np = slots.size();
    g_cigar_stats = CigarStats();
    g_cigar_stats.string_bytes = 2 * string_bytes;
    sink->ops.clear();
    if (np == 0) return SA_OK;
    // one buffer for the three per-pair arrays (slots, then the ops' offsets, then the counts: all of 8-byte items)
    DevBuf<char> d_pairs;
    DevBuf<uint32_t> d_ops;
    EncodeEvents ev;
    int rc;
    if ((rc = dmalloc(&d_pairs.p, np * (sizeof(CigarSlot) + 8 + sizeof(CigarCounts))))) return rc;
    CigarSlot *const d_slots = (CigarSlot *)d_pairs.p;
    uint64_t *const d_off = (uint64_t *)(d_slots + np);
    CigarCounts *const d_counts = (CigarCounts *)(d_off + np);
    for (hipEvent_t &one : ev.e) HIP_TRY(hipEventCreate(&one));
    HIP_TRY(hipMemcpyAsync(d_slots, slots.data(), np * sizeof(CigarSlot), hipMemcpyHostToDevice, st));
    CigarArgs a = {d_text, d_pattern, d_results, d_tail, d_slots, d_counts, nullptr, nullptr, sink->flags == SA_CIGAR_EQX, gap_letter};
    std::vector<CigarCounts> counts(np);
    HIP_TRY(hipEventRecord(ev.e[0], st));
    hipLaunchKernelGGL(cigar_encode_kernel<false>, dim3((unsigned)np), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.e[1], st));
    HIP_TRY(hipMemcpyAsync(counts.data(), d_counts, np * sizeof(CigarCounts), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<uint64_t> off(np);
    uint64_t total = 0;
    for (size_t p = 0; p < np; ++p)
    {
        sa_cigar_result &r = sink->results[p];
        off[p] = r.ops_off = total;
        r.num_ops = counts[p].num_ops;
        r.matches = counts[p].matches;
        r.mismatches = counts[p].mismatches;
        r.text_gap_letters = counts[p].text_gap_letters;
        r.pattern_gap_letters = counts[p].pattern_gap_letters;
        r.gap_opens = counts[p].gap_opens;
        total += counts[p].num_ops;
    }
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    g_cigar_stats.encode_ms = ms;
    if (total == 0) return SA_OK;
    sink->ops.resize(total);
    if ((rc = dmalloc(&d_ops.p, total * 4))) return rc;
    HIP_TRY(hipMemcpyAsync(d_off, off.data(), np * 8, hipMemcpyHostToDevice, st));
    a.ops_off = d_off;
    a.ops = d_ops.p;
    HIP_TRY(hipEventRecord(ev.e[2], st));
    hipLaunchKernelGGL(cigar_encode_kernel<true>, dim3((unsigned)np), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.e[3], st));
    HIP_TRY(hipMemcpyAsync(sink->ops.data(), d_ops.p, total * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipEventElapsedTime(&ms, ev.e[2], ev.e[3]));
    g_cigar_stats.encode_ms += ms;
    g_cigar_stats.ops_bytes = total * 4;
    return SA_OK;
}

extern "C" {

int sa_align_pairs_cigar(const sa_params *P, const sa_align_spec *spec, int32_t flags, const sa_host_pair *pairs, int64_t np, int device,
                         sa_cigar_result *results, sa_cigars **out)
{
    const std::string fn = "sa_align_pairs_cigar: ";
    if (out) *out = nullptr;
    cigar_reset_stats();
    if (!spec) return fail(SA_ERR_INVALID, fn + "spec is null");
    if (!P || np < 0 || (np > 0 && (!pairs || !results))) return fail(SA_ERR_INVALID, fn + "null argument");
    if (np > 0 && !out) return fail(SA_ERR_INVALID, fn + "out is null");
    if (!flags_ok(flags)) return fail(SA_ERR_INVALID, fn + "flags holds unknown bits (SA_CIGAR_M or SA_CIGAR_EQX)");
    const bool band = spec->band != -1, width = spec->width != -1, extend = spec->extend != 0;
    if (band && spec->bands) return fail(SA_ERR_INVALID, fn + "spec->band and spec->bands exclude each other");
    if ((band || spec->bands) && extend)
        return fail(SA_ERR_INVALID, fn + "spec->extend takes neither spec->band nor spec->bands: extension alignment inside a band is spec->width");
    if (width && !extend) return fail(SA_ERR_INVALID, fn + "spec->width requires spec->extend");
    if (spec->seeds && !extend) return fail(SA_ERR_INVALID, fn + "spec->seeds requires spec->extend");
    if (spec->chain_off && !spec->seeds) return fail(SA_ERR_INVALID, fn + "spec->chain_off requires spec->seeds");
    if (spec->chain_off && width) return fail(SA_ERR_INVALID, fn + "spec->chain_off and spec->width exclude each other");
    for (int64_t p = 0; p < np; ++p)
        if (pairs[p].text_len + pairs[p].pattern_len >= (1ull << 28))
            return fail(SA_ERR_UNSUPPORTED, fn + "pair " + std::to_string(p) + " has text_len + pattern_len >= 2^28: a run must fit 28 bits");

    WaveSpec ws = WaveSpec::gaps(spec->gap_open, spec->gap_extend);
    if (band) ws = ws.in_band(spec->band);
    if (spec->bands) ws = ws.in_bands(spec->bands);
    if (extend) ws = ws.extending(spec->xdrop);
    if (width) ws = ws.within(spec->width);
    if (spec->chain_off) ws = ws.from_chains(spec->seeds, spec->chain_off);
    else if (spec->seeds) ws = ws.from_seeds(spec->seeds);

    std::vector<sa_result> res((size_t)np);
    for (int64_t p = 0; p < np; ++p) results[p] = sa_cigar_result{};
    CigarSink sink;
    sink.flags = flags;
    sink.results = results;
    if (int rc = align_host_pairs(P, ws, pairs, np, device, res.data(), nullptr, nullptr, &sink)) return rc;
    for (int64_t p = 0; p < np; ++p)
    {
        results[p].score = res[p].score;
        results[p].status = res[p].status;
        results[p].num_alignment_bytes = res[p].num_alignment_bytes;
        results[p].start_text = res[p].start_text;
        results[p].start_pattern = res[p].start_pattern;
    }
    if (out)
    {
        sa_cigars *c = new sa_cigars;
        c->ops = std::move(sink.ops);
        *out = c;
    }
    return SA_OK;
}

const uint32_t *sa_cigars_ops(const sa_cigars *c) { return c && !c->ops.empty() ? c->ops.data() : nullptr; }

uint64_t sa_cigars_num_ops(const sa_cigars *c) { return c ? c->ops.size() : 0; }

int sa_cigars_destroy(sa_cigars *c)
{
    delete c;
    return SA_OK;
}

int sa_cigar_from_strings(const char *at, const char *ap, uint64_t len, char gap_letter, int32_t flags, uint32_t *ops, uint64_t cap,
                          sa_cigar_result *counts)
{
    const std::string fn = "sa_cigar_from_strings: ";
    if (len > 0 && (!at || !ap)) return fail(SA_ERR_INVALID, fn + "null string");
    if (cap > 0 && !ops) return fail(SA_ERR_INVALID, fn + "ops is null");
    if (!flags_ok(flags)) return fail(SA_ERR_INVALID, fn + "flags holds unknown bits (SA_CIGAR_M or SA_CIGAR_EQX)");
    if (len >= (1ull << 28)) return fail(SA_ERR_UNSUPPORTED, fn + "len >= 2^28: a run must fit 28 bits");
    sa_cigar_result c = {};
    c.num_alignment_bytes = len;
    const uint64_t nops = encode_strings(at, ap, len, gap_letter, flags == SA_CIGAR_EQX, ops, cap, &c);
    c.num_ops = (uint32_t)nops;
    if (counts) *counts = c;
    if (nops > cap) return fail(SA_ERR_INVALID, fn + "cap is " + std::to_string(cap) + ", the strings have " + std::to_string(nops) + " ops");
    return SA_OK;
}

int sa_cigar_format(const uint32_t *ops, uint64_t num_ops, char *buf, uint64_t cap)
{
    const std::string fn = "sa_cigar_format: ";
    if (!buf || cap == 0 || (num_ops > 0 && !ops)) return fail(SA_ERR_INVALID, fn + "null argument");
    // straight into buf while it fits (its last byte is kept for the NUL); `need` counts on past cap, for the message
    static const char letters[16] = {'M', 'I', 'D', 0, 0, 0, 0, '=', 'X', 0, 0, 0, 0, 0, 0, 0};
    uint64_t need = 0;
    for (uint64_t k = 0; k < num_ops; ++k)
    {
        const char letter = letters[ops[k] & 15];
        if (!letter) return fail(SA_ERR_INVALID, fn + "op " + std::to_string(k) + " has code " + std::to_string(ops[k] & 15) + ", none of M, I, D, = and X");
        char digits[10];
        int nd = 0;
        for (uint32_t v = ops[k] >> 4; nd == 0 || v; v /= 10) digits[nd++] = (char)('0' + v % 10);
        if (need + nd + 1 < cap)
        {
            char *q = buf + need;
            while (nd) *q++ = digits[--nd], ++need;
            *q = letter;
            ++need;
        }
        else need += nd + 1;
    }
    if (need + 1 > cap)
    {
        buf[0] = 0;
        return fail(SA_ERR_INVALID, fn + "cap is " + std::to_string(cap) + ", the text needs " + std::to_string(need + 1) + " bytes");
    }
    buf[need] = 0;
    return SA_OK;
}

int sa_cigar_last_stats(double *encode_ms, uint64_t *ops_bytes, uint64_t *string_bytes_not_copied)
{
    if (encode_ms) *encode_ms = g_cigar_stats.encode_ms;
    if (ops_bytes) *ops_bytes = g_cigar_stats.ops_bytes;
    if (string_bytes_not_copied) *string_bytes_not_copied = g_cigar_stats.string_bytes;
    return SA_OK;
}

}  // extern "C"
