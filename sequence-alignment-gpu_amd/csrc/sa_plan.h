// The host planner: everything the engine decides before its first HIP call, as one pure function
// of (params, pair shapes, CU count, knobs). No HIP here: sa_plan.cpp builds into libsa_hip.so and,
// with the plain host compiler, into bin/sa_plan_check (csrc/host/plan_check.cpp), which
// tests/test_plan.py runs without a GPU. sa_engine.hip validates, plans, allocates and uploads, and
// launches what the plan says. DESIGN.md "Planner" has the decision order.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "sa_hip.h"
#include "sa_layout.h"

namespace sa {

// What sa_plan_create, sa_align_pair and sa_align_batch answer to mode SA_FIT (SA_ERR_UNSUPPORTED):
// the plans have no fit mode, the score-only and traced wave paths do.
constexpr const char *kFitUnsupported =
    "SA_FIT is not implemented in the plans: use sa_score_batch, sa_scorer_create, sa_score_batch_affine, "
    "sa_scorer_create_affine, sa_align_pairs_affine, sa_search or sa_search_affine";

// And to SA_ENDS_FREE with any flags: the same functions take it.
constexpr const char *kEndsUnsupported =
    "SA_ENDS_FREE is not implemented in the plans: use sa_score_batch, sa_scorer_create, sa_score_batch_affine, "
    "sa_scorer_create_affine, sa_align_pairs_affine, sa_search or sa_search_affine";

// Environment knobs, read once per process (the first time the engine needs one) and never again:
// every field is a tuning or debugging switch; the defaults are the measured best settings.
struct Knobs {
    bool debug_sync = false;        // SA_DEBUG_SYNC: synchronise and check after every launch
    int rows_per_lane = 0;          // SA_ROWS_PER_LANE: force R (1..32)
    int waves_per_group = 0;        // SA_WAVES_PER_GROUP: force W (1..4)
    bool no_pair16 = false;         // SA_NO_PAIR16: disable the pair-packed batch fill
    int band = -1;                  // SA_BAND: 1 / 0 force the band fill (128-row score strips
                                    // feeding the 64-row strips, sa_fill.hip process_band) on / off
                                    // (1 also past kBandPersistRows*); default: on wherever it applies
                                    // (plan_bands)
    int band_r = 0;                 // SA_BAND_R: 2 / 3 force the bands' rows per lane (128-row bands and
                                    // strip groups of W, or 192-row bands and strip groups of three)
                                    // wherever that height applies; default: choose_bands
    double handoff_timeout_s = 20;  // SA_HANDOFF_TIMEOUT_S: in-kernel hand-off give-up time
    int io_sleep = 4;               // SA_IO_SLEEP: I/O wave idle poll period (s_sleep units)
    int chain_lds_kb = 0;           // SA_CHAIN_LDS_KB: dynamic LDS per chain workgroup
    const char *timeline = nullptr; // SA_TIMELINE=<file>: per-strip fill timestamps
    const char *tb_timing = nullptr;// SA_TB_TIMING=<file>: per-pair traceback timestamps
    const char *tb_table_timing = nullptr;  // SA_TB_TABLE_TIMING=<file>: per-strip table kernel stamps
    bool tb_generic = false;        // SA_TB_GENERIC: row walk without the unrolled strip code
    bool tb_stager = true;          // SA_TB_STAGER=0: the row walker stages every strip itself
    bool tb_tables = true;          // SA_TB_TABLES=0: no table traceback (every pair walks sequentially)
    int tb_rounds = 0;              // SA_TB_ROUNDS: rounds of tables (default: sa_plan_traceback)
    bool tb_strict = false;         // SA_TB_STRICT: no sequential walk after the table traceback
                                    // (tests: a pair it left keeps a stale head and fails its check)
    int max_cus = 0;                // SA_MAX_CUS: plan as if the device had at most this many CUs (tests)
    int chain_per_cu = 0;           // SA_CHAIN_PER_CU: 1 / 2 chain workgroups per CU (default: choose_chain_solo)
    int64_t band_rows = 0;          // SA_BAND_ROWS: band fill up to this many rows past resident
                                    // capacity (default kBandPersistRows*)
    int pair_chain_r = 0;           // SA_PAIR_CHAIN_R: rows per lane of small batches' pair-packed chains (4 / 8)
    int tb_cap = 0;                 // SA_TB_CAP: column-walk waves at most (0: one per pair)
    bool tb_wide = true;            // SA_TB_WIDE=0: strip tables always 512 threads per strip
    bool stage_kernel = true;       // SA_STAGE_KERNEL=0: one-shot calls stage through DMA copies
    int align = 1;                  // SA_ALIGN=0: chains of alphabets larger than 4 read the four
                                    // byte copies of their text profiles (kArr8) instead of copy 0
                                    // shifted in registers (kArr8A); 2: every alphabet (experiments)
};
const Knobs &knobs();

// The fill launch of a plan: what sa_plan_fill copies into FillArgs and hands to the launcher.
struct FillLaunch {
    int W = 1;               // waves per workgroup the launcher gets (pair chains: strips per pair)
    int sk = 0;              // score-kind selector: the plan's kind, or kArr8A (reads copy 0)
    bool band3 = false;      // launch_fill_band3 instead of launch_fill
    int num_groups = 0, num_bands = 0, num_band_groups = 0, band_wgs = 0, strip_w = 0;
    int grid = 0;
    int chain_lds = 0;       // floor of the dynamic LDS request (SA_CHAIN_LDS_KB may ask for more)
    int pair_text_len = 0;
};

// Everything decided before the first HIP call (no device pointers).
struct Plan {
    int mode = 0, A = 0, gap = 0, R = 0, U = 0, W = 1, key_bits = 12, key_rowbits = 21;
    int sk = 0;          // ScoreKind of the fill
    bool chain = false;  // some pair has more than one strip
    bool chain_solo = false;  // one chain workgroup per CU (one compute wave per SIMD), see choose_chain_solo
    // band fill (R = 1 int8-profile chains): 128-row score strips ahead of the 64-row strips
    bool band = false;
    int band_r = 2;      // rows per lane of the bands (3: 192-row bands, strip groups of three)
    int strip_w = 1;     // strips per strip group of the band fill (W, or 3 under three-row bands)
    int num_cu = 0;      // the device's CUs, SA_MAX_CUS at most
    std::vector<PairDesc> pairs;
    std::vector<StripDesc> strips, bands;
    char alphabet[33] = {0};
    // table traceback (sa_walk.h TbArgs; R = 1 plans with a pair of kTbMinStrips strips or more)
    std::vector<TbGroup> tb_groups;
    std::vector<int32_t> tb_pg;  // [np + 1] first group of each pair
    int64_t tb_slots = 0;        // strip tables (the strips of pairs with groups)
    int64_t max_recs = 1;        // records per pair at most (row walk: pattern rows, column walk: text columns)
    std::vector<int32_t> h_prof, h_table;  // host copies the (asynchronous) uploads read from
    // what the buffer table is sized from: text-code dwords, direction slots, granules, output bytes
    // per string, record words
    uint64_t code_bytes = 0, mask_entries = 0, granules = 0, out_bytes = 0, rec_words = 0;
    FillLaunch launch;
};

// Plans `np` pairs for a device of `num_cu` compute units under knob set `kn`. Returns SA_OK, or
// the SA_ERR_* code with its message in *err (*out is then unspecified).
int make_plan(const sa_params *P, const sa_pair *pairs, int64_t np, int num_cu, const Knobs &kn, Plan *out,
              std::string *err);

// The plan's sa_fill_kind (sa_hip.h).
inline int fill_kind(const Plan &pl)
{
    if (pl.sk == kPair) return pl.chain ? SA_FILL_PAIR_CHAIN : SA_FILL_PAIR;
    return pl.band ? (pl.band_r == 3 ? SA_FILL_BAND3 : SA_FILL_BAND) : SA_FILL_STRIPS;
}

}  // namespace sa
