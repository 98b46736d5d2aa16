// The launch table of the wave program (sa_score_wave.h): the one place that turns a call's run-time
// choice (its WaveSpec and mode, R, the alphabet size) into an instance of wave_kernel. sa_score.hip
// launches through it untraced and sa_affine_walk.hip traced, so each object holds its half of the
// instances. Host only but for the kernel it names.
#pragma once
#include <hip/hip_runtime.h>

#include <tuple>
#include <type_traits>

#include "sa_hip.h"
#include "sa_score_plan.h"
#include "sa_score_wave.h"

namespace sa {

// The base arguments of a launch from its plan and its device buffers; `order` and `np` are the launch's
// part of the work order. `pairs` is null where the wave draws work items.
inline ScoreAffineArgs score_args(const ScorePlan &pl, const void *d_text, const void *d_pattern, const ScorePair *pairs, const int32_t *order,
                                  int64_t np, const int32_t *table, int32_t *rows, sa_score_result *out, uint32_t *ctrl)
{
    ScoreAffineArgs aa;
    ScoreArgs &a = aa.s;
    a.text = (const int8_t *)d_text;
    a.pattern = (const int8_t *)d_pattern;
    a.pairs = pairs;
    a.order = order;
    a.table = table;
    a.rows = rows;
    a.out = out;
    a.ctrl = ctrl;
    a.np = (int32_t)np;
    a.A = pl.A;
    a.gap = pl.gap;
    a.key_rowbits = pl.key_rowbits;
    a.row_stride = pl.row_stride;
    aa.gap_extend = pl.spec.gap_extend;
    return aa;
}

// What a call launches: the variant's flags (without kWaveTrace), the program, and the int the variant
// reads from its arguments (the half-width, the SA_FREE_* flags or the xdrop), and the width of a banded
// extension, whose int is its xdrop.
struct WaveChoice {
    unsigned flags;
    int program;
    int32_t value;
    int32_t width;
};

// The single mode -> program mapping.
//  - Extension (and seeds) is the global program; inside a width it is the affine band-at instance of it.
//  - Work items without an extension (the gap pieces of chained seeds) are the global program, linear or affine.
//  - Per-pair bands: SA_LOCAL is the local program; every other mode runs as the ends-free mode it equals,
//    SA_GLOBAL with no flag and SA_FIT with the text's two.
//  - Ends-free is the fit program when the text's end is free and the global program otherwise.
//  - Anything else is the program of its mode; the half-width band adds its flag.
// The planner has refused what has no instance (a linear band, SA_FIT or free ends under a half-width, a band
// under an extension), so a spec that got past it names a row of the table below.
constexpr WaveChoice wave_choice(const WaveSpec &sp, int mode)
{
    const unsigned aff = sp.affine ? kWaveAffine : 0u;
    if (sp.extend && sp.ext_band) return WaveChoice{kVarExtendBand | (sp.seeded ? kWaveSeed : 0u), SA_GLOBAL, sp.xdrop, sp.width};
    if (sp.extend) return WaveChoice{aff | kWaveExtend | (sp.seeded ? kWaveSeed : 0u), SA_GLOBAL, sp.xdrop, 0};
    if (sp.seeded) return WaveChoice{aff | kWaveSeed, SA_GLOBAL, 0, 0};
    if (sp.band_at && mode == SA_LOCAL) return WaveChoice{kVarBandAtLocal, SA_LOCAL, 0, 0};
    const int ends = sp.band_at && mode == SA_GLOBAL ? 0
                     : sp.band_at && mode == SA_FIT  ? SA_FREE_TEXT_BEGIN | SA_FREE_TEXT_END
                                                     : mode & 15;
    if (sp.band_at) return WaveChoice{kVarBandAt, ends & SA_FREE_TEXT_END ? SA_FIT : SA_GLOBAL, ends, 0};
    if (mode & SA_ENDS_FREE) return WaveChoice{aff | kWaveEnds, ends & SA_FREE_TEXT_END ? SA_FIT : SA_GLOBAL, ends, 0};
    if (sp.banded) return WaveChoice{kVarBand, mode, sp.band, 0};
    return WaveChoice{aff, mode, 0, 0};
}

namespace wave_choice_check {
constexpr WaveSpec spec(bool affine, bool banded = false, bool band_at = false, bool extend = false, bool seeded = false, bool ext_band = false)
{
    WaveSpec s;
    s.affine = affine;
    s.banded = banded;
    s.band = banded ? 7 : 0;
    s.band_at = band_at;
    s.extend = extend;
    s.xdrop = extend ? 9 : SA_NO_XDROP;
    s.seeded = seeded;
    s.ext_band = ext_band;
    s.width = ext_band ? 5 : 0;
    return s;
}
constexpr bool is(WaveChoice c, unsigned flags, int program, int value, int width = 0)
{
    return c.flags == flags && c.program == program && c.value == value && c.width == width;
}
static_assert(is(wave_choice(spec(false), SA_FIT), kVarLinear, SA_FIT, 0), "a plain mode is its own program");
static_assert(is(wave_choice(spec(true), SA_LOCAL), kVarAffine, SA_LOCAL, 0), "a plain mode is its own program");
static_assert(is(wave_choice(spec(true, true), SA_LOCAL), kVarBand, SA_LOCAL, 7), "the half-width band keeps the mode");
static_assert(is(wave_choice(spec(false), SA_ENDS_FREE | SA_FREE_PATTERN_END), kVarEnds, SA_GLOBAL, SA_FREE_PATTERN_END),
              "ends-free with the text's end bound: the global program");
static_assert(is(wave_choice(spec(true), SA_OVERLAP), kVarAffineEnds, SA_FIT, 15), "ends-free with the text's end free: the fit program");
static_assert(is(wave_choice(spec(true, false, true), SA_GLOBAL), kVarBandAt, SA_GLOBAL, 0), "band-at global: ends-free, no flag");
static_assert(is(wave_choice(spec(true, false, true), SA_FIT), kVarBandAt, SA_FIT, SA_FREE_TEXT_BEGIN | SA_FREE_TEXT_END),
              "band-at fit: ends-free with the text's two flags");
static_assert(is(wave_choice(spec(true, false, true), SA_ENDS_FREE | SA_FREE_PATTERN_BEGIN), kVarBandAt, SA_GLOBAL, SA_FREE_PATTERN_BEGIN),
              "band-at ends-free: its own flags");
static_assert(is(wave_choice(spec(true, false, true), SA_LOCAL), kVarBandAtLocal, SA_LOCAL, 0), "band-at local: no free ends");
static_assert(is(wave_choice(spec(false, false, false, true), SA_GLOBAL), kVarExtend, SA_GLOBAL, 9), "extension: the global program");
static_assert(is(wave_choice(spec(true, false, false, true, true), SA_GLOBAL), kVarAffineSeeds, SA_GLOBAL, 9), "seeds: extension of a work item");
static_assert(is(wave_choice(spec(true, false, false, true, false, true), SA_GLOBAL), kVarExtendBand, SA_GLOBAL, 9, 5),
              "extension inside a width: the affine band-at instance of the global program");
static_assert(is(wave_choice(spec(true, false, false, true, true, true), SA_GLOBAL), kVarSeedsBand, SA_GLOBAL, 9, 5),
              "seeds inside a width: the same of a work item");
static_assert(is(wave_choice(spec(true, false, false, false, true), SA_GLOBAL), kVarAffineItems, SA_GLOBAL, 0), "a chain's gap pieces: the global program of a work item");
static_assert(is(wave_choice(spec(false, false, false, false, true), SA_GLOBAL), kVarItems, SA_GLOBAL, 0), "the same, linear");
}  // namespace wave_choice_check

// One row of the table: a variant and the programs it has instances of.
template <unsigned F, int... PROGRAMS>
struct WaveRow {
};

// The instance set, a variant per row. Untraced, every row exists at R = 1, 2, 4, 8 and both alphabet sizes;
// traced, the affine rows exist at R = 8.
//                      variant           programs                      reads
using WaveTable = std::tuple<
    WaveRow<kVarLinear,       SA_GLOBAL, SA_LOCAL, SA_FIT>,  // -
    WaveRow<kVarAffine,       SA_GLOBAL, SA_LOCAL, SA_FIT>,  // -
    WaveRow<kVarBand,         SA_GLOBAL, SA_LOCAL>,          // band
    WaveRow<kVarEnds,         SA_GLOBAL, SA_FIT>,            // ends
    WaveRow<kVarAffineEnds,   SA_GLOBAL, SA_FIT>,            // ends
    WaveRow<kVarBandAtLocal,  SA_LOCAL>,                     // bands
    WaveRow<kVarBandAt,       SA_GLOBAL, SA_FIT>,            // ends, bands
    WaveRow<kVarExtend,       SA_GLOBAL>,                    // xdrop
    WaveRow<kVarAffineExtend, SA_GLOBAL>,                    // xdrop
    WaveRow<kVarSeeds,        SA_GLOBAL>,                    // xdrop, items
    WaveRow<kVarAffineSeeds,  SA_GLOBAL>,                    // xdrop, items
    WaveRow<kVarExtendBand,   SA_GLOBAL>,                    // xdrop, width
    WaveRow<kVarSeedsBand,    SA_GLOBAL>,                    // xdrop, width, items
    WaveRow<kVarItems,        SA_GLOBAL>,                    // items
    WaveRow<kVarAffineItems,  SA_GLOBAL>>;                   // items

template <bool TRACE>
using WaveArgsT = ArgsOf<TRACE ? kWaveTrace : 0u>;

namespace detail {

template <bool TRACE, unsigned F, int PROGRAM>
bool launch_wave_program(const WaveChoice &c, int R, bool small, int grid, hipStream_t st, const WaveArgsT<TRACE> &a)
{
    if (c.flags != F || c.program != PROGRAM) return false;
    auto with_r = [&](auto rc) {
        constexpr int RR = decltype(rc)::value;
        constexpr unsigned FF = F | (TRACE ? kWaveTrace : 0u);
        if (small) hipLaunchKernelGGL((wave_kernel<RR, PROGRAM, true, FF>), dim3(grid), dim3(64), 0, st, a);
        else hipLaunchKernelGGL((wave_kernel<RR, PROGRAM, false, FF>), dim3(grid), dim3(64), 0, st, a);
    };
    if constexpr (TRACE) with_r(std::integral_constant<int, 8>{});
    else
        switch (R)
        {
        case 1: with_r(std::integral_constant<int, 1>{}); break;
        case 2: with_r(std::integral_constant<int, 2>{}); break;
        case 4: with_r(std::integral_constant<int, 4>{}); break;
        default: with_r(std::integral_constant<int, 8>{}); break;
        }
    return true;
}

template <bool TRACE, unsigned F, int... PROGRAMS>
bool launch_wave_row(WaveRow<F, PROGRAMS...>, const WaveChoice &c, int R, bool small, int grid, hipStream_t st, const WaveArgsT<TRACE> &a)
{
    if constexpr (TRACE && !(F & kWaveAffine)) return false;  // no traced linear instance
    else return (launch_wave_program<TRACE, F, PROGRAMS>(c, R, small, grid, st, a) || ...);
}

template <bool TRACE, typename... ROWS>
bool launch_wave_table(std::tuple<ROWS...> *, const WaveChoice &c, int R, bool small, int grid, hipStream_t st, const WaveArgsT<TRACE> &a)
{
    return (launch_wave_row<TRACE>(ROWS{}, c, R, small, grid, st, a) || ...);
}

}  // namespace detail

// Launches the instance of `c` on `grid` one-wave workgroups; `a` holds everything but the variant's int,
// which is c.value, and the width, which is c.width. R is 1, 2, 4 or 8 (traced: 8 whatever it says), small is A <= 4. False: the table has
// no such instance and nothing was launched, which is an error of the caller's planner.
template <bool TRACE>
bool launch_wave(const WaveChoice &c, int R, bool small, int grid, hipStream_t st, WaveArgsT<TRACE> a)
{
    a.band = c.value;
    a.width = c.width;
    return detail::launch_wave_table<TRACE>((WaveTable *)nullptr, c, R, small, grid, st, a);
}

}  // namespace sa
