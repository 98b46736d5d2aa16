/* sa_hip.h — C ABI of the MI355X (gfx950) alignment engine: the drop-in boundary for the
 * reference's GPU path.
 *
 * The reference exposes exactly one GPU entry point,
 *     uint64_t SequenceAlignment::alignSequenceGPU(const Request&, Response*);
 *         (robertszafa/sequence-alignment-gpu: SequenceAlignment.hpp:127, implemented in
 *          alignSequenceGPU.cu:463-653)
 * with C++ linkage and C++ structs. This header is the plain-C layer underneath our C++14
 * re-implementation of that function (sequence-alignment-gpu_amd/csrc/host/align_gpu.cpp):
 * plain pointers and sizes, no torch / HIP types in the signatures, so any FFI (ctypes, cgo,
 * JNI, N-API) can bind it. INTEGRATION.md shows the bindings.
 *
 * Semantics are those of the reference's CPU path (alignSequenceCPU.cpp:10-333), bit-exact:
 * score, aligned text, aligned pattern, start indices — including the local-alignment
 * start-index quirk and the "first maximum in row-major order" rule.
 *
 * Error behaviour mirrors the reference boundary: every entry point returns SA_OK (0) on
 * success and a non-zero code otherwise (the reference returns 1 on failure,
 * alignSequenceGPU.cu:543-545, :590-593); sa_last_error() gives the message.
 */
#ifndef SA_HIP_H
#define SA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SA_ABI_VERSION 1

/* Request::alignmentType (SequenceAlignment.hpp:78; GLOBAL/LOCAL/SEMI_GLOBAL of programArgs :17).
 *
 * SA_FIT (semi-global, "fit"): the whole pattern p (m letters) inside the text t (n letters), the
 * text free at both ends. The reference declares SEMI_GLOBAL and never implements it, so there is
 * nothing to be bit-exact with; this is the definition. The recurrences are those of the other
 * modes (linear, or Gotoh's under sa_score_batch_affine below).
 *   borders: H[0][j] = 0 for every j; H[i][0] as in global mode, -i gap_penalty or
 *            -(gap_open + (i - 1) gap_extend); F[0][j] follows from H[0][j] = 0
 *   result:  score = max over j in 1..n of H[m][j]; end_pattern = m; end_text = the smallest such j
 *            (column 0 is left out: it is never strictly better than column 1)
 *   walk:    from (m, end_text) in state H with the tie rules of the other modes, until row 0; row 0
 *            forces no LEFT moves, column 0 with i > 0 forces TOP
 *   strings: start_text = the column the walk reached row 0 in = the 0-based index of the window's
 *            first text letter, start_pattern = 0; aligned_text without its gap letters is
 *            t[start_text : end_text], aligned_pattern without them is p
 *   empty:   m == 0 scores 0 at (0, 0) with an empty alignment; n == 0 < m scores -m gap_penalty or
 *            -(gap_open + (m - 1) gap_extend) at (m, 0): the pattern against m gap letters
 * SA_FIT is taken by sa_score_batch, sa_scorer_create, sa_score_batch_affine,
 * sa_scorer_create_affine, sa_align_pairs_affine, sa_search and sa_search_affine; sa_search aligns
 * its fit hits as sa_align_pairs_affine does with gap_open = gap_extend = gap_penalty (the linear
 * recurrence); the band-at functions take it with a band per pair. sa_plan_create, sa_align_pair and
 * sa_align_batch answer SA_ERR_UNSUPPORTED.
 *
 * SA_ENDS_FREE (ends-free alignment): global alignment in which each of the four sequence ends may
 * cost nothing. mode = SA_ENDS_FREE | any of the four flags below, 16..31; 3..15 and values from 32
 * on are SA_ERR_INVALID. TB, TE, PB, PE stand for the flags. SA_OVERLAP (all four) is the overlap
 * (dovetail) alignment of assembly and read merging; TB | PE asks whether the end of the text
 * overlaps the start of the pattern; PB | PE is the text contained in the pattern. The recurrence is
 * the linear one, or Gotoh's as sa_score_batch_affine states it; gap(k) is k gap_penalty, or
 * gap_open + (k - 1) gap_extend.
 *   borders:    H[0][0] = 0; H[0][j] = TB ? 0 : -gap(j); H[i][0] = PB ? 0 : -gap(i); E[i][0] and
 *               F[0][j] are minus infinity
 *   candidates: (m, n) always; (m, j), 0 <= j <= n, if TE; (i, n), 0 <= i <= m, if PE
 *   result:     the maximum of H over the candidates; sa_score_result.end_pattern and end_text are
 *               its cell. Ties: an interior candidate (i >= 1 and j >= 1) beats a border candidate;
 *               among interior candidates the first in row-major order wins, so a last-column cell
 *               (i < m, n) comes before every cell of row m, and within row m the leftmost wins; among
 *               border candidates the first in row-major order wins
 *   empty:      with n == 0 or m == 0 every candidate is a border cell and the rules above apply to
 *               the border values (penalties may be negative: gap(k) need not grow with k)
 *   walk:       from the result cell in state H with the tie rules of the other modes (DESIGN.md
 *               3.5); it ends at (i, j) when i == 0 && (TB || j == 0) or j == 0 && (PB || i == 0);
 *               otherwise column 0 forces TOP and row 0 forces LEFT
 *   strings:    start_text = j and start_pattern = i of the cell the walk ended in, without quirks;
 *               aligned_text without its gap letters is t[start_text : end_text], aligned_pattern
 *               without them is p[start_pattern : end_pattern]
 * Identities: SA_ENDS_FREE | TB | TE gives every output of SA_FIT. SA_ENDS_FREE alone gives every
 * output of SA_GLOBAL, but for a pair with both sides empty, where global keeps the reference's
 * (uint64)-1 starts and ends-free reports 0. Swapping text and pattern (the score matrix
 * transposed) while swapping TB with PB and TE with PE gives the same score.
 * The modes are taken by sa_score_batch, sa_scorer_create, sa_score_batch_affine,
 * sa_scorer_create_affine, sa_align_pairs_affine, sa_search and sa_search_affine; sa_search aligns
 * its hits as sa_align_pairs_affine does with gap_open = gap_extend = gap_penalty; the band-at functions
 * take them with a band per pair. The banded functions on a half-width (a band with free ends needs a
 * diagonal of its own), sa_plan_create, sa_align_pair and sa_align_batch answer SA_ERR_UNSUPPORTED. */
enum sa_mode { SA_GLOBAL = 0, SA_LOCAL = 1, SA_FIT = 2, SA_ENDS_FREE = 16 };
enum sa_free_end {
    SA_FREE_TEXT_BEGIN = 1,    /* TB: H[0][j] = 0                             */
    SA_FREE_TEXT_END = 2,      /* TE: the result may lie anywhere in row m    */
    SA_FREE_PATTERN_BEGIN = 4, /* PB: H[i][0] = 0                             */
    SA_FREE_PATTERN_END = 8,   /* PE: the result may lie anywhere in column n */
    SA_OVERLAP = SA_ENDS_FREE | 15
};

enum sa_status {
    SA_OK = 0,
    SA_ERR_INVALID = 1,     /* bad argument (sizes, alphabet, score range)                  */
    SA_ERR_NOMEM = 2,       /* device allocation failed (reference: MEM_ERROR, :543)       */
    SA_ERR_HIP = 3,         /* a HIP runtime call failed                                    */
    SA_ERR_UNSUPPORTED = 4, /* input outside the engine's documented limits                 */
    SA_ERR_TIMEOUT = 5      /* an in-kernel hand-off did not complete (engine aborted)      */
};

/* Scoring scheme of a Request (SequenceAlignment.hpp:71-99). */
typedef struct sa_params {
    int32_t mode;                 /* SA_GLOBAL (Needleman-Wunsch), SA_LOCAL (Smith-Waterman), or
                                     SA_FIT or SA_ENDS_FREE | flags (score-only and affine
                                     functions only, see sa_mode)                                */
    int32_t alphabet_size;        /* Request::alphabetSize, 1..32 (4 DNA, 23 protein)           */
    int32_t gap_penalty;          /* Request::gapPenalty (linear gap, subtracted per gap cell)  */
    int32_t rows_per_lane;        /* 0 = automatic; else 1,2,4,8,16,32 (tuning knob)            */
    const int32_t *score_matrix;  /* host, alphabet_size^2 ints, row-major [pattern][text]
                                     (Request::scoreMatrix, indexed as alignSequenceCPU.cpp:172) */
    const char *alphabet;         /* host, alphabet_size letters followed by the gap letter
                                     (Request::alphabet; DNA_ALPHABET / PROTEIN_ALPHABET :56-58) */
} sa_params;

/* One (text, pattern) pair inside device-resident arenas of alphabet indices. */
typedef struct sa_pair {
    uint64_t text_offset;     /* byte offset of the text in the text arena        */
    uint64_t text_len;        /* Request::textNumBytes    (columns of the DP)     */
    uint64_t pattern_offset;  /* byte offset of the pattern in the pattern arena  */
    uint64_t pattern_len;     /* Request::patternNumBytes (rows of the DP)        */
} sa_pair;

/* Per-pair outcome: the scalar fields of Response (SequenceAlignment.hpp:101-120). */
typedef struct sa_result {
    int32_t score;                 /* Response::score                                     */
    int32_t status;                /* SA_OK or an error code for this pair               */
    uint64_t num_alignment_bytes;  /* Response::numAlignmentBytes                         */
    uint64_t start_text;           /* Response::startInAlignedText    (may be (uint64)-1) */
    uint64_t start_pattern;        /* Response::startInAlignedPattern (may be (uint64)-1) */
} sa_result;

typedef struct sa_plan sa_plan;

/* ---- one-shot, host pointers (what alignSequenceGPU needs) ------------------------------ */

/* Align one pair held in host memory (alphabet indices). Synchronous. aligned_text and
 * aligned_pattern receive num_alignment_bytes letters in forward order; cap must be at least
 * text_len + pattern_len. If fill_us is non-NULL it receives the device time of the DP fill in
 * microseconds (the quantity the reference returns under -DBENCHMARK, alignSequenceGPU.cu:613-626). */
int sa_align_pair(const sa_params *params, const char *text, uint64_t text_len,
                  const char *pattern, uint64_t pattern_len, int device, sa_result *out,
                  char *aligned_text, char *aligned_pattern, uint64_t cap, double *fill_us);

/* sa_align_pair keeps, per device, a stream, two events and a grow-only device arena across calls
 * (calls on one device are serialised). This releases them for `device` (-1: every device); they
 * are also released at process exit. */
int sa_release_workspace(int device);

/* ---- many pairs from host memory, sharded over GPUs ------------------------------------ */

/* One pair in host memory (alphabet indices), as a Request holds it (SequenceAlignment.hpp:71-99). */
typedef struct sa_host_pair {
    const char *text;
    uint64_t text_len;
    const char *pattern;
    uint64_t pattern_len;
} sa_host_pair;

/* Align num_pairs independent pairs with one scoring scheme over devices 0..num_gpus-1 of this
 * process (one host thread and one plan per device; the per-pair results are gathered to device 0
 * with RCCL, loaded on first use, communicators kept for the process). Synchronous. results: num_pairs entries. aligned_text / aligned_pattern: NULL (scores only) or
 * num_pairs host buffers, buffer i of at least text_len + pattern_len bytes, receiving pair i's
 * num_alignment_bytes letters in forward order. The pair -> device deal is sa_batch_deal's. If
 * num_gpus exceeds the device count, devices are shared round-robin (no RCCL then).
 * Calls are serialised process-wide (one batch at a time, whatever the devices). Each shard keeps its
 * stream, device arenas, RCCL buffers and plan across calls; a call whose shards have the same pair
 * shapes and scoring parameters as the previous one reuses the plans. */
int sa_align_batch(const sa_params *params, const sa_host_pair *pairs, int64_t num_pairs, int num_gpus,
                   sa_result *results, char *const *aligned_text, char *const *aligned_pattern);

/* The deal sa_align_batch uses (host only, no device calls): shard_of[i] in 0..num_shards-1 for
 * work cells[i] = text_len * pattern_len. Equal work: round-robin (i mod num_shards); otherwise
 * longest-processing-time (largest first to the least-loaded shard, ties to the lower shard). */
int sa_batch_deal(const uint64_t *cells, int64_t num_pairs, int num_shards, int32_t *shard_of);

/* Debug record of the calling thread's last sa_align_batch: shards used, whether the results came
 * through the RCCL gather (1) or straight from each shard (0, shards sharing a device), each shard's
 * wall time from upload to the end of its traceback (shard_ms: up to cap entries) and the gather's
 * wall time (0 without RCCL). */
int sa_batch_last_stats(int32_t *num_shards, int32_t *used_rccl, double *shard_ms, int32_t cap, double *gather_ms);

/* ---- plans: many pairs, device-resident inputs, explicit stream ------------------------- */

/* Build a plan (strip layout, workspace) for num_pairs pairs on `device`. Allocates all device
 * workspace once; the plan can be filled/traced back any number of times. */
int sa_plan_create(const sa_params *params, const sa_pair *pairs, int64_t num_pairs, int device,
                   sa_plan **out);
int sa_plan_destroy(sa_plan *plan);

/* Enqueue the DP fill of every pair on `stream` (a hipStream_t; NULL = the HIP null stream, which is
 * also what torch.cuda's default stream handle 0 denotes).
 * d_text / d_pattern are device arenas of alphabet indices addressed by sa_pair offsets. */
int sa_plan_fill(sa_plan *plan, const void *d_text, const void *d_pattern, void *stream);

/* Enqueue the traceback of every pair (after sa_plan_fill on the same stream). */
int sa_plan_traceback(sa_plan *plan, void *stream);

/* Synchronise `stream` and copy the per-pair results to host (num_pairs entries). Returns
 * SA_ERR_TIMEOUT if the fill aborted. */
int sa_plan_fetch_results(sa_plan *plan, sa_result *out, void *stream);

/* Synchronise `stream` and copy pair `index`'s aligned strings (forward order) to host. */
int sa_plan_fetch_alignment(sa_plan *plan, int64_t index, char *aligned_text, char *aligned_pattern,
                            uint64_t cap, void *stream);

/* Bytes of each of the plan's two aligned-string arenas (text and pattern side). */
uint64_t sa_plan_output_bytes(const sa_plan *plan);

/* Synchronise `stream` and copy every pair's result and both aligned-string arenas to host in one
 * pass (what a batch caller needs: one copy each instead of one per pair). text_buf / pattern_buf
 * hold buf_bytes >= sa_plan_output_bytes(plan) bytes; pair i's aligned text / pattern are the
 * results[i].num_alignment_bytes letters at text_buf + offsets[i] / pattern_buf + offsets[i]
 * (offsets: num_pairs entries). results, text_buf and pattern_buf may each be NULL (not copied).
 * Returns SA_ERR_TIMEOUT if the fill aborted. */
int sa_plan_fetch_all(sa_plan *plan, sa_result *results, char *text_buf, char *pattern_buf, uint64_t buf_bytes,
                      uint64_t *offsets, void *stream);

/* Introspection for benches and tests. */
int sa_plan_info(const sa_plan *plan, int64_t *num_strips, int32_t *rows_per_lane,
                 uint64_t *device_bytes, uint64_t *mask_bytes);
/* Which fill kernel sa_plan_fill launches for the plan (benches and tests). */
enum {
    SA_FILL_STRIPS = 0,      /* one wave per strip (fill_kernel; chains hand rows off in LDS / granules) */
    SA_FILL_BAND = 1,        /* band fill: 128-row score strips feeding the 64-row strips (R = 1) */
    SA_FILL_PAIR = 2,        /* pair-packed lone strips: two pairs per wave (fill_pair_kernel) */
    SA_FILL_PAIR_CHAIN = 3,  /* pair-packed chains: a couple of pairs per workgroup, a wave per strip */
    SA_FILL_BAND3 = 4        /* band fill with 192-row bands (three rows per lane) feeding strip groups of three */
};
int sa_plan_fill_kind(const sa_plan *plan);
/* Verification: synchronise `stream` and decode pair `index`'s direction bit-planes into the
 * reference's (pattern_len+1) x (text_len+1) byte DIRECTION matrix (LEFT=0, DIAG=1, TOP=2, STOP=3;
 * row 0 / column 0 as the reference fill sets them, alignSequenceCPU.cpp:145-164, :232-248), so the
 * fill can be compared byte-for-byte with the reference's M. Local plans with one row per lane
 * (rows_per_lane 1) hold no STOP bit in their planes (the raw decisions): STOP is put back wherever
 * the cell's score is 0 (alignSequenceCPU.cpp:188-190), recomputed here on the host from the last
 * fill's inputs, so every plan returns the reference's M. M_out must hold (m+1)*(n+1) bytes. */
int sa_plan_fetch_directions(sa_plan *plan, int64_t index, uint8_t *M_out, void *stream);

/* Device pointer to the per-pair sa_result array written by sa_plan_traceback. */
const void *sa_plan_device_results(const sa_plan *plan);

/* Copies the per-pair sa_result array (num_pairs * sizeof(sa_result) bytes) to device memory d_dst
 * on `stream` (asynchronous, device to device: the batch path's results go to the RCCL gather without
 * a host round trip). The abort / bad-input flags are not checked here (sa_plan_fetch_results does). */
int sa_plan_copy_results(const sa_plan *plan, void *d_dst, void *stream);

/* ---- score only: many pairs without direction planes or traceback ----------------------- */

/* The score of a pair and the cell it is read from. No direction planes, no traceback: a scorer's
 * device memory is the inputs, the results and one boundary row per resident wave, whatever the
 * number of cells. The limits of the plans apply unchanged. */
typedef struct sa_score_result {
    int32_t score;         /* Response::score of the reference for this pair            */
    int32_t status;        /* SA_OK or this pair's error                                */
    uint64_t end_text;     /* column j of the scored cell (global: text_len)            */
    uint64_t end_pattern;  /* row i of the scored cell (global: pattern_len); local: the
                              first maximum in row-major order, (0,0) when the score is 0;
                              fit: (pattern_len, leftmost best column of that row);
                              ends-free: the result cell (see sa_mode)                    */
} sa_score_result;
typedef struct sa_scorer sa_scorer;

/* Score num_pairs pairs held in host memory on `device`. Synchronous. out: num_pairs entries. */
int sa_score_batch(const sa_params *params, const sa_host_pair *pairs, int64_t num_pairs, int device,
                   sa_score_result *out);

/* A scorer for num_pairs pairs addressed in device-resident arenas (as sa_plan_create). It may be
 * run any number of times. params->rows_per_lane: 0 = automatic, else 1, 2, 4, 8 (16 and 32 are
 * taken as 8). */
int sa_scorer_create(const sa_params *params, const sa_pair *pairs, int64_t num_pairs, int device, sa_scorer **out);
/* Enqueue the scoring of every pair on `stream` (NULL = the HIP null stream). */
int sa_scorer_run(sa_scorer *scorer, const void *d_text, const void *d_pattern, void *stream);
/* Synchronise `stream` and copy the per-pair results to host (num_pairs entries). Returns
 * SA_ERR_INVALID if an input byte was outside the alphabet. */
int sa_scorer_fetch(sa_scorer *scorer, sa_score_result *out, void *stream);
/* Waves launched, rows per lane and device bytes (inputs, results, row buffers, constants). */
int sa_scorer_info(const sa_scorer *scorer, int64_t *num_waves, int32_t *rows_per_lane, uint64_t *device_bytes);
int sa_scorer_destroy(sa_scorer *scorer);

/* Affine gap penalties (Gotoh) for the score-only path: a gap of k cells costs
 * gap_open + (k - 1) * gap_extend, both subtracted as gap_penalty is; params->gap_penalty is ignored.
 *   E[i][j] = max(E[i][j-1] - gap_extend, H[i][j-1] - gap_open)
 *   F[i][j] = max(F[i-1][j] - gap_extend, H[i-1][j] - gap_open)
 *   H[i][j] = max(H[i-1][j-1] + S[p[i-1]][t[j-1]], E[i][j], F[i][j]), local: max(0, .)
 * with H[0][j] = -(gap_open + (j - 1) gap_extend) (local: 0), likewise H[i][0], H[0][0] = 0. With
 * gap_open == gap_extend == g this is the linear recurrence of gap penalty g. Results as above; an
 * empty side scores -(gap_open + (max(m, n) - 1) gap_extend) in global mode (0 when both are empty).
 * Any int penalties; the limits of the plans apply with |gap_penalty| read as
 * max(|gap_open|, |gap_extend|) (SA_ERR_UNSUPPORTED). The scorer works with sa_scorer_run, _fetch,
 * _info and _destroy; pairs may share one pattern (pattern_offset 0 for all): a query against a
 * database. */
int sa_score_batch_affine(const sa_params *params, int32_t gap_open, int32_t gap_extend,
                          const sa_host_pair *pairs, int64_t num_pairs, int device, sa_score_result *out);
int sa_scorer_create_affine(const sa_params *params, int32_t gap_open, int32_t gap_extend,
                            const sa_pair *pairs, int64_t num_pairs, int device, sa_scorer **out);

/* Linear gap penalty (params->gap_penalty); sa_search_affine below is the same search under gap open /
 * gap extend, scores and alignments alike.
 * Score `query` (the pattern) against num_texts texts and align the k best: ranked by score
 * descending, ties to the lower index; *num_hits = min(k, num_texts). scores (num_texts entries) may
 * be NULL. hit_index / hit_results: k entries. aligned_text / aligned_pattern: both NULL, or k host
 * buffers each of at least (its hit's text_len + query_len) bytes; buffers sized for the longest text
 * always do. The hits are aligned through a plan on the same device: their results and strings are
 * what sa_align_pair returns for the pair. k = 0 gives scores only. Synchronous.
 * In mode SA_FIT the plans cannot align: the hits go through sa_align_pairs_affine's path with
 * gap_open = gap_extend = gap_penalty, which is the linear recurrence (see sa_mode). */
int sa_search(const sa_params *params, const char *query, uint64_t query_len, const char *const *texts,
              const uint64_t *text_lens, int64_t num_texts, int k, int device, sa_score_result *scores,
              int64_t *hit_index, sa_result *hit_results, char *const *aligned_text,
              char *const *aligned_pattern, int64_t *num_hits);

/* ---- alignments under affine gap penalties ------------------------------------------------ */

/* Align num_pairs host pairs on `device` under gap_open / gap_extend (recurrence of sa_score_batch_affine;
 * tie rules and walk: DESIGN.md 3.5). results, aligned_text, aligned_pattern as sa_align_batch takes them
 * (strings NULL/NULL: results only). With gap_open == gap_extend == g every output equals sa_align_pair's
 * for gap_penalty g. Synchronous. The fill keeps four direction bits per cell of the pairs it has in
 * flight: the pairs are processed in chunks whose directions fit 2 GiB (SA_TRACE_ARENA_BYTES), and a
 * single pair above that is SA_ERR_UNSUPPORTED. */
int sa_align_pairs_affine(const sa_params *params, int32_t gap_open, int32_t gap_extend,
                          const sa_host_pair *pairs, int64_t num_pairs, int device, sa_result *results,
                          char *const *aligned_text, char *const *aligned_pattern);

/* sa_search under gap_open / gap_extend: scores from the affine scorer, the k best aligned by the path
 * above on the same device (texts and query uploaded once). Arguments and ranking as sa_search. */
int sa_search_affine(const sa_params *params, int32_t gap_open, int32_t gap_extend, const char *query,
                     uint64_t query_len, const char *const *texts, const uint64_t *text_lens, int64_t num_texts,
                     int k, int device, sa_score_result *scores, int64_t *hit_index, sa_result *hit_results,
                     char *const *aligned_text, char *const *aligned_pattern, int64_t *num_hits);

/* ---- banded alignment: scores and alignments inside a diagonal band -------------------------- */

/* For a pair with n text letters, m pattern letters and band half-width w >= 0 let d = n - m,
 * lo = min(0, d) - w and hi = max(0, d) + w. Cell (i, j), 0 <= i <= m, 0 <= j <= n, border cells
 * included, is in band iff lo <= j - i <= hi. (0, 0) and (m, n) are always in band, and every row has
 * an in-band cell in columns 1..n.
 * The recurrence is Gotoh's as sa_score_batch_affine states it, with one addition: H, E and F of every
 * out-of-band cell are minus infinity. Nothing else changes: the borders of in-band border cells, the
 * tie rules, the local clamp, the local result (the first maximum in row-major order,
 * now over in-band cells; 0 at (0, 0) without a positive one) and the empty-side results.
 * gap_open == gap_extend == g is the linear recurrence of gap penalty g: a caller with a linear gap
 * passes its gap_penalty twice. The band is exact, cell by cell: no result depends on rows_per_lane,
 * on the grid or on how the engine rounds its work. With w >= max(n, m) every cell is in band and
 * every output equals that of the unbanded function (sa_score_batch_affine, sa_scorer_create_affine,
 * sa_align_pairs_affine).
 * One half-width serves all pairs of a call. Modes: SA_GLOBAL and SA_LOCAL; SA_FIT with a band is
 * SA_ERR_UNSUPPORTED (a fit band needs a diagonal of its own), and so is SA_ENDS_FREE with any flags:
 * the band-at functions below take both, with a band of the caller's per pair.
 * band < 0 is SA_ERR_INVALID. The score
 * limit is half that of the unbanded functions: (max|S| + G)(n + m) + G (n + m) must stay below 2^29,
 * G = max(|gap_open|, |gap_extend|) (SA_ERR_UNSUPPORTED). The search functions take no
 * band: texts of unrelated lengths share no diagonal.
 * The scorer is an ordinary sa_scorer (run, fetch, info, destroy). sa_align_pairs_banded keeps
 * direction bits for the band only, about (2 w + |d| + 575) * 256 bytes per 512 rows (DESIGN.md 8
 * has the exact sum): the chunks are cut by these bytes and a pair is refused only when its band
 * exceeds SA_TRACE_ARENA_BYTES.
 * sa_affine_last_stats reports the call. */
int sa_score_batch_banded(const sa_params *params, int32_t gap_open, int32_t gap_extend, int32_t band,
                          const sa_host_pair *pairs, int64_t num_pairs, int device, sa_score_result *out);
int sa_scorer_create_banded(const sa_params *params, int32_t gap_open, int32_t gap_extend, int32_t band,
                            const sa_pair *pairs, int64_t num_pairs, int device, sa_scorer **out);
int sa_align_pairs_banded(const sa_params *params, int32_t gap_open, int32_t gap_extend, int32_t band,
                          const sa_host_pair *pairs, int64_t num_pairs, int device, sa_result *results,
                          char *const *aligned_text, char *const *aligned_pattern);

/* ---- banded alignment on a diagonal of the caller's: one band per pair, every mode ----------- */

/* bands[k] is the band of pair k: cell (i, j), 0 <= i <= m, 0 <= j <= n, border cells included, is in
 * band iff lo <= j - i <= hi. The caller who knows where the pattern lies in the text (read mapping
 * after a seed hit, read merging, seed extension) says so: a fit of a read that starts near text
 * letter c takes {c - w, c + w}. Nothing is derived from the lengths.
 * Modes: SA_GLOBAL, SA_LOCAL, SA_FIT and SA_ENDS_FREE | flags, all 16 sets. The recurrence is Gotoh's
 * as sa_score_batch_affine states it (a linear caller passes its penalty twice), and H, E and F of
 * every out-of-band cell are minus infinity, border cells included.
 *   borders:      "free" is TB for row 0, PB for column 0, and either under SA_LOCAL. H[0][0] = 0 iff
 *                 the origin is in band; a free border cell is 0 iff it is in band; a non-free border
 *                 cell (0, j) or (i, 0) is -gap(j) or -gap(i) iff it and the origin are in band (a
 *                 border gap run starts at a real origin); every other border cell is minus infinity
 *   result:       the rules of the mode over real (not minus infinity), in-band cells. Global: (m, n).
 *                 Local: the first maximum in row-major order over in-band cells, or 0 at (0, 0)
 *                 without a positive one. Fit and ends-free: the candidates and the tie order of
 *                 SA_ENDS_FREE above, over the in-band candidates only
 *   walk:         as the mode has it, the stop rule of ends-free included; it never leaves the band
 *   empty:        with n == 0 or m == 0 every candidate is a border cell and the rules above apply
 *   reachability: a pair is reachable iff some candidate is real, which holds iff an in-band permitted
 *                 start is componentwise <= an in-band permitted end. Starts: the origin; under TB the
 *                 cells (0, j); under PB the cells (i, 0). Ends: (m, n); under TE row m; under PE column
 *                 n. A local pair is always reachable. sa_band_reachable is the closed form (host only,
 *                 no device call): 1 reachable, 0 not, -1 for a bad mode
 * Refusals: the three device functions refuse the whole call with SA_ERR_INVALID when a pair is
 * unreachable and name the first such pair's index in sa_last_error(): callers filter with
 * sa_band_reachable first. lo > hi is SA_ERR_INVALID, and so is bands == NULL with num_pairs > 0. Any
 * other int32 lo and hi are accepted; values beyond [-m, n] act as if clipped to it. The score limit is
 * that of the banded functions above (SA_ERR_UNSUPPORTED).
 * Identities: bands[k] = {min(0, d) - w, max(0, d) + w}, d = n - m, in global or local mode gives every
 * output of the banded function above at half-width w; bands[k] = {-m, n} gives every output of the
 * unbanded affine function in every mode; SA_ENDS_FREE | TB | TE equals SA_FIT.
 * The scorer is an ordinary sa_scorer. sa_align_pairs_band_at keeps direction bits for the band's
 * strips only, as sa_align_pairs_banded does, so a pair whose full directions exceed
 * SA_TRACE_ARENA_BYTES aligns when its band fits. sa_affine_last_stats reports the call. The search
 * functions take no band. */
typedef struct sa_band { int32_t lo, hi; } sa_band;
int sa_score_batch_band_at(const sa_params *params, int32_t gap_open, int32_t gap_extend, const sa_band *bands,
                           const sa_host_pair *pairs, int64_t num_pairs, int device, sa_score_result *out);
int sa_scorer_create_band_at(const sa_params *params, int32_t gap_open, int32_t gap_extend, const sa_band *bands,
                             const sa_pair *pairs, int64_t num_pairs, int device, sa_scorer **out);
int sa_align_pairs_band_at(const sa_params *params, int32_t gap_open, int32_t gap_extend, const sa_band *bands,
                           const sa_host_pair *pairs, int64_t num_pairs, int device, sa_result *results,
                           char *const *aligned_text, char *const *aligned_pattern);
int sa_band_reachable(int32_t mode, uint64_t text_len, uint64_t pattern_len, sa_band band);

/* ---- extension alignment: anchored start, best cell anywhere, row X-drop ---------------------- */

/* The alignment starts at the origin (the end of a seed), ends at whichever cell scores best, and the
 * fill stops once a row's best has dropped more than xdrop below the best seen: the primitive of
 * seed-and-extend mapping. H, E and F are Gotoh's matrices as sa_score_batch_affine states them, with
 * global borders and no clamp: H[0][0] = 0, H[0][j] = -gap(j), H[i][0] = -gap(i),
 * gap(k) = gap_open + (k - 1) gap_extend. For n >= 1 and m >= 1:
 *   row maxima:   r(i) = max over 1 <= j <= n of H[i][j], i = 1..m
 *   running best: B(0) = 0 (the origin, the empty extension), B(i) = max(B(i - 1), r(i))
 *   stop row i*:  with xdrop = X >= 0 the smallest i in 1..m with B(i - 1) - r(i) > X; with
 *                 xdrop = SA_NO_XDROP, or when no row qualifies, i* = m + 1
 *   result:       over the interior cells (i, j), 1 <= i < i*, 1 <= j <= n: if their maximum is > 0 it is
 *                 the score and end_pattern, end_text its first cell in row-major order; otherwise the
 *                 score is 0 at (0, 0) with an empty alignment (the rule local has). Border cells are
 *                 never candidates
 *   walk:         from the result cell in state H, with the tie rules of DESIGN.md 3.5, to the origin;
 *                 row 0 forces LEFT and column 0 forces TOP
 *   strings:      start_text = start_pattern = 0 without quirks, for the empty alignment too.
 *                 aligned_text without its gap letters is text[0 : end_text], aligned_pattern without
 *                 them pattern[0 : end_pattern]; sa_result carries no end cell, it follows from the
 *                 strings (the scorers report it)
 *   empty:        n == 0 or m == 0 scores 0 at (0, 0) with an empty alignment
 * The drop is defined on rows of the full, unpruned matrix: every cell of the rows < i* has its plain
 * value, so no output depends on rows_per_lane, on the grid or on how much work the engine skips.
 * Skipping rows >= i* is an optimisation; they count for nothing even if the score recovers there.
 * Identities: (I1) the score and both strings equal those of sa_align_pairs_affine in SA_GLOBAL mode on
 * text[:end_text], pattern[:end_pattern]. (I2) The score is non-decreasing in X, and X = 2^30 - 1 gives
 * every output of SA_NO_XDROP (under the score limit no difference B - r reaches 2^30). (I3) Under
 * non-negative penalties the SA_NO_XDROP score is >= max(0, the score of SA_ENDS_FREE | TE | PE).
 * (I4) gap_open == gap_extend == g is the linear recurrence of gap penalty g, and the scorers then run
 * the linear kernels. Extending to the left of a seed is the same call on both sequences reversed: the
 * seeds functions below do both sides in one call and reverse nothing.
 * params->mode must be SA_GLOBAL (the borders are global's), else SA_ERR_INVALID; xdrop < -1 or
 * xdrop >= 2^30 is SA_ERR_INVALID. One xdrop serves all pairs of a call. The limits are those of the
 * unbanded affine functions and of local mode's best-cell key (SA_ERR_UNSUPPORTED). There is no band.
 * The scorer is an ordinary sa_scorer. sa_align_pairs_extend plans a pair with the direction bytes of a
 * global pair and chunks as sa_align_pairs_affine does; sa_affine_last_stats reports the call. */
#define SA_NO_XDROP (-1)
int sa_score_batch_extend(const sa_params *params, int32_t gap_open, int32_t gap_extend, int32_t xdrop,
                          const sa_host_pair *pairs, int64_t num_pairs, int device, sa_score_result *out);
int sa_scorer_create_extend(const sa_params *params, int32_t gap_open, int32_t gap_extend, int32_t xdrop,
                            const sa_pair *pairs, int64_t num_pairs, int device, sa_scorer **out);
int sa_align_pairs_extend(const sa_params *params, int32_t gap_open, int32_t gap_extend, int32_t xdrop,
                          const sa_host_pair *pairs, int64_t num_pairs, int device, sa_result *results,
                          char *const *aligned_text, char *const *aligned_pattern);

/* ---- seed extension: both ways from a seed, the left side read in place ----------------------- */

/* seeds[k] belongs to pair k, text t of n letters and pattern p of m letters, and says that
 * t[text_pos : text_pos + length] lies against p[pattern_pos : pattern_pos + length] without a gap; ts,
 * ps and L below. L = 0 is a bare anchor point. The seed's letters need not match: they are scored as
 * they are.
 *   right half: extension alignment of t[ts + L :] against p[ps + L :], exactly what sa_score_batch_extend
 *               defines under gap_open, gap_extend and xdrop
 *   left half:  extension alignment of reverse(t[: ts]) against reverse(p[: ps]), the same definition; the
 *               rows of its X-drop are rows of that reversed matrix. Nothing is reversed or copied: the
 *               kernels read the two prefixes backwards where they lie
 *   seed score: the sum over q < L of S[p[ps + q]][t[ts + q]]
 *   result:     score = left.score + seed + right.score; begin_text = ts - left.end_text,
 *               begin_pattern = ps - left.end_pattern, end_text = ts + L + right.end_text,
 *               end_pattern = ps + L + right.end_pattern: the alignment covers t[begin_text : end_text] and
 *               p[begin_pattern : end_pattern]
 *   strings:    reverse(left.aligned) + the seed's L letters + right.aligned, on both sides. In sa_result
 *               start_text = begin_text, start_pattern = begin_pattern and num_alignment_bytes is the sum of
 *               the three lengths, without quirks; an empty result (L = 0, both halves empty) has
 *               start = (ts, ps)
 *   empty half: ts == 0, ps == 0 or a seed that reaches an end: the half scores 0 with an empty alignment,
 *               extension's own rule
 * Identities: (S1) every output equals this composition of the extension functions on host-sliced and
 * host-reversed copies. (S2) The seed {0, 0, 0} gives every output of the _extend function, with
 * begin = (0, 0). (S3) Mirror: the pair reverse(t), reverse(p) with the seed {n - ts - L, m - ps - L, L} has
 * the same score, begin' = (n - end_text, m - end_pattern), end' = (n - begin_text, m - begin_pattern) and
 * both strings reversed; its left half is this pair's right half, so the identity is exact, ties
 * included. (S4) gap_open == gap_extend runs the linear kernels, as (I4) of extension.
 * Refusals: params->mode other than SA_GLOBAL or a bad xdrop as the extension functions have them;
 * seeds == NULL with num_pairs > 0, ts + L > n or ps + L > m: SA_ERR_INVALID, the first such pair's index
 * in sa_last_error(); a byte outside the alphabet that a kernel reads, the seed's letters included:
 * SA_ERR_INVALID. The score limit and the best-cell key limit are the extension functions', applied to the
 * whole pair's (n, m), which covers the sum. There is no band.
 * A seeds scorer works with sa_scorer_run, _info and _destroy, any number of times on new arena contents;
 * sa_scorer_fetch on it gives the score with end_text and end_pattern, both absolute, and
 * sa_scorer_fetch_seeds on any other scorer is SA_ERR_INVALID. Its device memory is the extension scorer's
 * plus the work items (a pair's non-empty halves) and their results. sa_align_pairs_seeds keeps direction
 * bytes for the two rectangles ps x ts and (m - ps - L) x (n - ts - L), each as a global pair of that shape,
 * never for n x m: a seeded pair whose full directions exceed SA_TRACE_ARENA_BYTES aligns, and a pair is
 * SA_ERR_UNSUPPORTED only when its two halves together exceed it (they share a chunk).
 * sa_affine_last_stats reports the call. */
typedef struct sa_seed { uint64_t text_pos, pattern_pos, length; } sa_seed;
typedef struct sa_seed_result {
    int32_t score, status;
    uint64_t begin_text, begin_pattern, end_text, end_pattern;
} sa_seed_result;
int sa_score_batch_seeds(const sa_params *params, int32_t gap_open, int32_t gap_extend, int32_t xdrop, const sa_seed *seeds,
                         const sa_host_pair *pairs, int64_t num_pairs, int device, sa_seed_result *out);
int sa_scorer_create_seeds(const sa_params *params, int32_t gap_open, int32_t gap_extend, int32_t xdrop, const sa_seed *seeds,
                           const sa_pair *pairs, int64_t num_pairs, int device, sa_scorer **out);
int sa_scorer_fetch_seeds(sa_scorer *scorer, sa_seed_result *out, void *stream);
int sa_align_pairs_seeds(const sa_params *params, int32_t gap_open, int32_t gap_extend, int32_t xdrop, const sa_seed *seeds,
                         const sa_host_pair *pairs, int64_t num_pairs, int device, sa_result *results,
                         char *const *aligned_text, char *const *aligned_pattern);

/* ---- banded extension: extension and seeds within a width of the anchor's diagonal ------------ */

/* width = w >= 0, one per call. Cell (i, j) of an extension matrix is in band iff |j - i| <= w: the band
 * lies about the diagonal of the extension's anchor, the origin. For a seeded pair this holds for each half
 * in its own coordinates, the left half being the reversed-prefix matrix, so the same w serves both halves
 * and nothing is mirrored. Everything is the extension definition above, on the banded matrix:
 *   cells:      Gotoh's recurrence with global borders and no clamp; H, E and F of every out-of-band cell
 *               are minus infinity, border cells included: H[0][j] = -gap(j) for j <= w, H[i][0] = -gap(i)
 *               for i <= w. The origin is always in band
 *   row maxima: r(i) is the maximum of H[i][j] over the in-band j in 1..n, minus infinity when the row has
 *               none, which is the case for i > n + w
 *   stop row:   B and i* as defined; a minus-infinity row drops under every X >= 0, and under SA_NO_XDROP
 *               nothing drops
 *   result:     the first maximum in row-major order over the in-band interior cells of rows < i*, if it
 *               is > 0; otherwise 0 at (0, 0)
 *   walk:       from that cell to the origin; it never leaves the band
 *   empty:      as extension has it
 * r, B and i* are defined on the banded matrix: no output depends on rows_per_lane, the grid or how much
 * work is skipped.
 * Identities: (W1) w >= max(n, m) gives every output of the unbanded _extend / _seeds function at every
 * xdrop. (W2) The score and both strings equal sa_align_pairs_band_at in SA_GLOBAL mode with band {-w, w}
 * on text[:end_text], pattern[:end_pattern]; the end cell is in band, so that pair is reachable. (W3) Under
 * SA_NO_XDROP the score is non-decreasing in w and never above the unbanded score. (W4)
 * gap_open == gap_extend == g gives the outputs of the linear recurrence of g; the instance that runs is
 * affine, as for the band-at scorer. (W5) Seeds S1, S2 and S3 hold with the same width on both sides, S3
 * exactly, ties included, because the band is symmetric.
 * Refusals: width < 0 is SA_ERR_INVALID; any width above max(n, m) acts as if clipped to it. The mode and
 * xdrop rules are extension's (the seeds functions': theirs). The limits are extension's best-cell key range
 * plus the banded score limit (SA_ERR_UNSUPPORTED, "scores may reach the band's sentinel"). band / bands
 * (the functions above) stay separate: there is no _banded or _band_at extension.
 * The aligners keep direction bytes for the band's windows only, as sa_align_pairs_band_at does for a band
 * of the caller's: a pair (a seeded pair: its two halves) whose full rectangle exceeds
 * SA_TRACE_ARENA_BYTES aligns when its band fits. sa_scorer_fetch_seeds serves a banded seeds scorer
 * unchanged, and sa_affine_last_stats reports the aligner calls. */
int sa_score_batch_extend_band(const sa_params *params, int32_t gap_open, int32_t gap_extend, int32_t xdrop, int32_t width,
                               const sa_host_pair *pairs, int64_t num_pairs, int device, sa_score_result *out);
int sa_scorer_create_extend_band(const sa_params *params, int32_t gap_open, int32_t gap_extend, int32_t xdrop, int32_t width,
                                 const sa_pair *pairs, int64_t num_pairs, int device, sa_scorer **out);
int sa_align_pairs_extend_band(const sa_params *params, int32_t gap_open, int32_t gap_extend, int32_t xdrop, int32_t width,
                               const sa_host_pair *pairs, int64_t num_pairs, int device, sa_result *results,
                               char *const *aligned_text, char *const *aligned_pattern);
int sa_score_batch_seeds_band(const sa_params *params, int32_t gap_open, int32_t gap_extend, int32_t xdrop, int32_t width,
                              const sa_seed *seeds, const sa_host_pair *pairs, int64_t num_pairs, int device, sa_seed_result *out);
int sa_scorer_create_seeds_band(const sa_params *params, int32_t gap_open, int32_t gap_extend, int32_t xdrop, int32_t width,
                                const sa_seed *seeds, const sa_pair *pairs, int64_t num_pairs, int device, sa_scorer **out);
int sa_align_pairs_seeds_band(const sa_params *params, int32_t gap_open, int32_t gap_extend, int32_t xdrop, int32_t width,
                              const sa_seed *seeds, const sa_host_pair *pairs, int64_t num_pairs, int device, sa_result *results,
                              char *const *aligned_text, char *const *aligned_pattern);

/* ---- chained seeds: gap fills between the seeds of a chain, extensions at its two ends ----------- */

/* Pair k, text t of n letters and pattern p of m letters, owns the seeds seeds[chain_off[k] .. chain_off[k + 1])
 * of one flat sa_seed array; chain_off has num_pairs + 1 entries, chain_off[0] == 0, and is non-decreasing. A
 * pair's seeds {ts_i, ps_i, L_i}, i = 0 .. c - 1, c >= 1, are colinear and do not overlap:
 * ts_i + L_i <= ts_(i+1), ps_i + L_i <= ps_(i+1), ts_(c-1) + L_(c-1) <= n and ps_(c-1) + L_(c-1) <= m. L_i = 0 is
 * allowed, and a seed's letters need not match: they are scored as they are. The chain says where the path is,
 * so only the rectangle two consecutive seeds enclose is filled between them, and only the two ends extend.
 *   left end:  the seeds functions' left half for seed 0: extension of reverse(t[: ts_0]) against
 *              reverse(p[: ps_0]) under gap_open, gap_extend and xdrop
 *   right end: the seeds functions' right half for seed c - 1
 *   gap i:     i = 0 .. c - 2, the SA_GLOBAL alignment, as sa_align_pairs_affine defines it (score, walk and
 *              tie rules), of t[ts_i + L_i : ts_(i+1)] against p[ps_i + L_i : ps_(i+1)]. Both sides empty:
 *              score 0, no columns. One side empty, k letters on the other: one gap run, score
 *              -(gap_open + (k - 1) gap_extend), k columns. xdrop does not apply to gaps
 *   seed i:    the sum over q < L_i of S[p[ps_i + q]][t[ts_i + q]], L_i columns
 *   result:    an sa_seed_result. score is the sum of all pieces; begin_text = ts_0 - left.end_text,
 *              begin_pattern = ps_0 - left.end_pattern; end_text = ts_(c-1) + L_(c-1) + right.end_text,
 *              end_pattern = ps_(c-1) + L_(c-1) + right.end_pattern
 *   strings:   reverse(left.aligned) + seed_0 + gap_0 + seed_1 + ... + seed_(c-1) + right.aligned, on both
 *              sides. In sa_result start_text = begin_text, start_pattern = begin_pattern and
 *              num_alignment_bytes is the sum of the piece lengths
 * Identities: (C1) every output equals this composition, built from sa_align_pairs_extend on host-sliced and
 * host-reversed ends and sa_align_pairs_affine in SA_GLOBAL mode on host-sliced gaps. (C2) A chain of one seed
 * gives every output of the seeds function. (C3) Cutting a seed {ts, ps, L} into {ts, ps, a} and
 * {ts + a, ps + a, L - a} changes no output: the gap between them is empty. (C4) Mirror: reversing both
 * sequences and the chain (seed i becomes {n - ts_i - L_i, m - ps_i - L_i, L_i}, the order reversed) gives the
 * same score, begin' = (n - end_text, m - end_pattern) and end' = (n - begin_text, m - begin_pattern), exactly,
 * under 0 <= gap_extend <= gap_open (otherwise a gap run along a rectangle's border costs its closed form while
 * one inside it may open anew cell by cell, and the reversed rectangle may score differently).
 * The ends mirror exactly, ties included, as (S3) has it. A gap's string is that of the global aligner on the
 * reversed rectangle, and the global walk's tie rules are not symmetric (between a diagonal and a gap of equal
 * score it prefers the gap, between E and F it prefers E, and it meets them from the far corner), so among
 * equally good gap alignments the mirrored call may pick another one: the identity holds for scores and
 * intervals, and for the strings only in that every gap's string is the global aligner's on its reversed
 * rectangle. (C5) gap_open == gap_extend runs the linear kernels for every piece and gives the linear
 * recurrence's outputs.
 * Refusals: SA_ERR_INVALID, sa_last_error() naming the pair and (where one is at fault) the seed's index in
 * its chain, for seeds or chain_off NULL with num_pairs > 0, chain_off[0] != 0, chain_off decreasing, a pair
 * with no seed, a seed out of range, and a seed out of order or overlapping the one before it. The mode and
 * xdrop rules are the seeds functions'. A byte outside the alphabet that any piece reads is SA_ERR_INVALID:
 * seed letters and gap letters always, the letters of an end only where its X-drop let the fill reach them.
 * The score limit and the best-cell key limit are checked on the whole pair's (n, m), as for seeds. There is
 * no band: the functions take no width, and sa_search*, the plans, sa_align_pair, sa_align_batch, the
 * multi-GPU path and the CLI take no chains.
 * A chains scorer runs two fills on the caller's stream, one of the gap pieces and one of the ends, each with
 * the rows per lane and the grid that suit its own items (gaps are many and small, ends few and larger), then
 * one combine. It works with sa_scorer_run, _info, _fetch, _fetch_seeds and _destroy as a seeds scorer does;
 * sa_scorer_info reports the larger grid and the rows per lane of the launch with more cells. Its device
 * memory is that of the two launches plus the work items, the seeds and a record per pair.
 * sa_align_pairs_chains keeps direction bytes for the pieces only, each gap rectangle and each end as a global
 * pair of its shape, never for n x m, and keeps a pair's pieces in one chunk: a read whose full directions exceed
 * SA_TRACE_ARENA_BYTES many times over aligns, and a pair is SA_ERR_UNSUPPORTED only when its pieces together
 * exceed it. Every piece is walked at once, a wave each, into a part of the pair's n + m string bytes of its own,
 * and one wave per pair then joins the pieces with the seeds' letters in place. sa_affine_last_stats reports the
 * call: the two fills as the fill, the combine, the walks and the join as the walk. */
int sa_score_batch_chains(const sa_params *params, int32_t gap_open, int32_t gap_extend, int32_t xdrop, const sa_seed *seeds,
                          const uint64_t *chain_off, const sa_host_pair *pairs, int64_t num_pairs, int device, sa_seed_result *out);
int sa_scorer_create_chains(const sa_params *params, int32_t gap_open, int32_t gap_extend, int32_t xdrop, const sa_seed *seeds,
                            const uint64_t *chain_off, const sa_pair *pairs, int64_t num_pairs, int device, sa_scorer **out);
int sa_align_pairs_chains(const sa_params *params, int32_t gap_open, int32_t gap_extend, int32_t xdrop, const sa_seed *seeds,
                          const uint64_t *chain_off, const sa_host_pair *pairs, int64_t num_pairs, int device, sa_result *results,
                          char *const *aligned_text, char *const *aligned_pattern);

/* ---- chaining: one colinear chain per pair from a seeder's unfiltered anchors ------------------- */

/* Pair k owns the anchors anchors[anchor_off[k] .. anchor_off[k + 1]) of one flat sa_seed array; anchor_off has
 * num_pairs + 1 entries, anchor_off[0] == 0, and is non-decreasing. A pair may have no anchors. An anchor
 * {x, y, L} is {text_pos, pattern_pos, length} with L >= 1; its ends are ex = x + L and ey = y + L. Its letters
 * are not looked at: the functions take no sequences, so repeats, overlaps and off-diagonal hits are welcome.
 *   order:      a pair's anchors come in canonical order, non-decreasing (ex, ey, L) lexicographically; equal
 *               keys are identical anchors and are allowed. The order is checked in one pass and a call out of
 *               order is refused: nothing here sorts
 *   transition: for j < i within one pair, o = max(0, ex_j - x_i, ey_j - y_i) letters are cut from the front
 *               of i; dx = x_i + o - ex_j, dy = y_i + o - ey_j, dd = |dx - dy|. j -> i is admissible iff
 *               o < L_i, dx <= max_gap, dy <= max_gap, dd <= max_diag and i - j <= lookback, and then
 *               value(j -> i) = match (L_i - o) - (dd ? gap_open + (dd - 1) gap_extend : 0) - skip min(dx, dy)
 *   recurrence: f(i) = max(match L_i, max over admissible j of f(j) + value(j -> i)); pred(i) is the j that
 *               attains it. A predecessor is taken only when it is strictly better than starting anew at i,
 *               and among equal predecessors the largest j wins
 *   result:     the chain ends at the anchor with the largest f, ties to the lowest index (last_anchor), and is
 *               followed back through pred. Its seeds in forward order are {x_i + o_i, y_i + o_i, L_i - o_i},
 *               the first with o = 0; score = f(end). A pair without anchors has score 0, no seeds and
 *               last_anchor 0. status is SA_OK
 * All arithmetic is that of exact integers. f < 2^30 is enforced below, so a cost that reaches 2^30 can never be
 * chosen, and an implementation may saturate there (the device kernel does, the host function does not).
 * Identities: (K1) the output of every pair with anchors is a chain as sa_score_batch_chains defines one:
 * colinear, no overlap, every L >= 1; each seed is the tail of one input anchor on that anchor's diagonal and
 * shares its end. (K2) sa_chain_anchors equals sa_chain_anchors_host in every field and every seed. (K3) With
 * lookback >= the pair's anchor count the score is the maximum over all index-increasing subsequences with
 * admissible consecutive transitions. (K4) Anchors that already form a valid chain come back unchanged, with
 * score match sum(L), under gap_open = gap_extend = skip = 0, no limits and lookback >= 1. (K5) A pair's result
 * does not depend on the other pairs of the call (seeds_off apart), and adding (cx, cy) to every anchor of a
 * pair adds the same constant to its seeds and changes nothing else.
 * sa_chain_anchors runs chain_dp_kernel (one wave per pair, drawn from a counter, most anchors first; the last
 * `lookback` anchors in an LDS ring; 64 predecessors per round) and, once the host has turned the chain lengths
 * into offsets, chain_walk_kernel, which writes every pair's seeds into an array of exactly the counted size
 * that one copy brings back. sa_chain_anchors_host is the definition on the host and makes no device call.
 * *out owns the seeds and their offsets until sa_chain_set_destroy; on failure it stays NULL.
 * sa_chain_set_seeds and sa_chain_set_off are exactly the `seeds` and `chain_off` arguments of
 * sa_score_batch_chains, sa_scorer_create_chains and sa_align_pairs_chains and of sa_align_spec. Those functions
 * refuse a pair without a seed, so a caller first drops the pairs whose num_seeds == 0 (and their entries of
 * chain_off); they also want every seed inside its pair's sequences, which a seeder's anchors are.
 * Refusals, all before any device call, sa_last_error() naming the pair and the anchor (its index within the
 * pair) where one is at fault. SA_ERR_INVALID: params, results or out NULL; a parameter outside the ranges
 * below; num_pairs < 0; anchors or anchor_off NULL with num_pairs > 0; anchor_off[0] != 0 or anchor_off
 * decreasing; L == 0; a pair out of canonical order. SA_ERR_UNSUPPORTED: x + L or y + L at or above 2^31 - 1;
 * a pair with match sum(L) >= 2^30; num_pairs >= 2^31.
 * Not built: finding the anchors on the device, sorting them, secondary chains, and a handle that keeps the
 * anchors on the device between calls. */
#define SA_CHAIN_NO_LIMIT INT32_MAX
typedef struct sa_chain_params {
    int32_t match;                  /* 1 .. 1024 */
    int32_t gap_open, gap_extend;   /* 0 .. 2^20: a diagonal change of dd costs gap_open + (dd - 1) gap_extend */
    int32_t skip;                   /* 0 .. 2^20, per letter of min(dx, dy) */
    int32_t max_gap, max_diag;      /* >= 0, or SA_CHAIN_NO_LIMIT */
    int32_t lookback;               /* 1 .. 1024 */
} sa_chain_params;
typedef struct sa_chain_result {
    int32_t score, status;
    uint64_t seeds_off;             /* first seed of this pair's chain = chain_off[k] */
    uint32_t num_seeds;
    uint32_t last_anchor;           /* index, within the pair, of the anchor the chain ends in; 0 without anchors */
} sa_chain_result;
typedef struct sa_chain_set sa_chain_set;   /* owns the call's host seed array and its chain_off */

int sa_chain_anchors(const sa_chain_params *params, const sa_seed *anchors, const uint64_t *anchor_off,
                     int64_t num_pairs, int device, sa_chain_result *results, sa_chain_set **out);
int sa_chain_anchors_host(const sa_chain_params *params, const sa_seed *anchors, const uint64_t *anchor_off,
                          int64_t num_pairs, sa_chain_result *results, sa_chain_set **out);   /* no device call */
const sa_seed *sa_chain_set_seeds(const sa_chain_set *set);     /* NULL when there are none */
const uint64_t *sa_chain_set_off(const sa_chain_set *set);      /* num_pairs + 1 entries */
int sa_chain_set_destroy(sa_chain_set *set);
/* For benches and tests only: the calling thread's last sa_chain_anchors. Device time of chain_dp_kernel and of
 * chain_walk_kernel in milliseconds and the bytes of device memory the call held. Each pointer may be NULL. */
int sa_chain_last_stats(double *dp_ms, double *walk_ms, uint64_t *device_bytes);

/* ---- CIGAR output: run-length alignments from every sa_align_pairs_* variant -------------------- */

/* Take a pair's aligned strings at and ap exactly as the sa_align_pairs_* function of the same variant returns
 * them: L = num_alignment_bytes columns, the gap letter is alphabet[alphabet_size]. Column c is
 *   I  if at[c] is the gap letter: the pattern (the query) has a letter the text lacks
 *   D  if ap[c] is the gap letter
 *   otherwise, under SA_CIGAR_EQX: = if at[c] == ap[c] as characters, else X
 *   otherwise, under SA_CIGAR_M (flags = 0): M
 * The CIGAR is the run-length encoding of that column sequence in forward order, each op one BAM-packed
 * uint32: len << 4 | code, with M = 0, I = 1, D = 2, = = 7, X = 8.
 * Identity: (G1) the ops and the counts are this function of the strings and nothing else, so every tie rule and
 * quirk of every mode carries over. sa_cigar_from_strings below is that function on the host.
 * sa_align_pairs_cigar runs the variant that `spec` names (sa_align_spec: the arguments of the sa_align_pairs_*
 * function it stands for) through that function's own planner, fill and walks, leaves the strings on the device,
 * and encodes them there: cigar_encode_kernel, one wave per pair, once to count each pair's ops and once to write
 * them into an array of exactly the counted size, which one copy brings to the host. results[k] holds pair k's
 * sa_result fields verbatim, where its ops lie in the call's op array (ops_off is the exclusive sum of num_ops in
 * pair order) and the counts: matches and mismatches are counted from the letters, under SA_CIGAR_M too;
 * text_gap_letters are the columns of I, pattern_gap_letters those of D, and gap_opens the runs of I plus the runs
 * of D; the four column counts add up to num_alignment_bytes. *out owns the op array until sa_cigars_destroy; on
 * failure it stays NULL.
 * Refusals: SA_ERR_INVALID before any device call, the message naming the fields, for spec == NULL, out == NULL
 * with num_pairs > 0, flags other than SA_CIGAR_M or SA_CIGAR_EQX, band with bands, a band of either kind with
 * extend, width without extend, seeds without extend, chain_off without seeds and chain_off with width.
 * SA_ERR_UNSUPPORTED for a pair with text_len + pattern_len >= 2^28: a run must fit 28 bits. Everything else is
 * refused as the named variant refuses it, in that variant's words.
 * sa_cigar_from_strings serves the callers of the plans and of sa_align_pair, which have no device CIGAR: ops
 * (cap entries) may be NULL with cap 0, counts may be NULL; a cap below the number of ops is SA_ERR_INVALID with
 * counts->num_ops still set to the number needed. It fills the counts and num_alignment_bytes = len; score,
 * status, the starts and ops_off are 0. sa_cigar_format writes the ops as text ("12=1X3I", NUL-terminated) and
 * returns SA_ERR_INVALID when cap bytes do not hold it or an op's code is none of the five. */
enum sa_cigar_flags { SA_CIGAR_M = 0, SA_CIGAR_EQX = 1 };
enum sa_cigar_op { SA_CIGAR_OP_M = 0, SA_CIGAR_OP_I = 1, SA_CIGAR_OP_D = 2, SA_CIGAR_OP_EQ = 7, SA_CIGAR_OP_X = 8 };

typedef struct sa_align_spec {      /* which sa_align_pairs_* function this call stands for */
    int32_t gap_open, gap_extend;
    int32_t band;                   /* >= 0: _banded; -1 none */
    int32_t xdrop;                  /* with extend != 0: SA_NO_XDROP or 0 .. 2^30 - 1 */
    int32_t width;                  /* >= 0: _extend_band / _seeds_band; -1 none */
    int32_t extend;                 /* 0 / 1: extension alignment (required by seeds and chain_off) */
    const sa_band *bands;           /* non-NULL: _band_at */
    const sa_seed *seeds;           /* non-NULL: _seeds, or with chain_off _chains */
    const uint64_t *chain_off;
} sa_align_spec;

typedef struct sa_cigar_result {
    int32_t score, status;
    uint64_t num_alignment_bytes, start_text, start_pattern;   /* sa_result's, verbatim */
    uint64_t ops_off;               /* first op of this pair in the call's op array */
    uint32_t num_ops;
    uint32_t matches, mismatches;   /* under SA_CIGAR_M too: counted from the letters */
    uint32_t text_gap_letters;      /* columns of I */
    uint32_t pattern_gap_letters;   /* columns of D */
    uint32_t gap_opens;             /* runs of I plus runs of D */
} sa_cigar_result;

typedef struct sa_cigars sa_cigars; /* owns the call's host op array */

int sa_align_pairs_cigar(const sa_params *params, const sa_align_spec *spec, int32_t flags, const sa_host_pair *pairs,
                         int64_t num_pairs, int device, sa_cigar_result *results, sa_cigars **out);
const uint32_t *sa_cigars_ops(const sa_cigars *cigars);   /* NULL when there are 0 ops */
uint64_t sa_cigars_num_ops(const sa_cigars *cigars);
int sa_cigars_destroy(sa_cigars *cigars);

/* host only, no device call */
int sa_cigar_from_strings(const char *at, const char *ap, uint64_t len, char gap_letter, int32_t flags, uint32_t *ops,
                          uint64_t cap, sa_cigar_result *counts);
int sa_cigar_format(const uint32_t *ops, uint64_t num_ops, char *buf, uint64_t cap);
/* For benches and tests only, as sa_affine_last_stats below (which reports the fill and the walks of the call as
 * for the string call): the calling thread's last sa_align_pairs_cigar. Device time of the two encoder passes in
 * milliseconds, the bytes of ops copied to the host, and the bytes of the two string arenas that were not. */
int sa_cigar_last_stats(double *encode_ms, uint64_t *ops_bytes, uint64_t *string_bytes_not_copied);

/* For benches and tests only, not a stable part of the ABI (it may change or go without a new
 * SA_ABI_VERSION). Debug record of the calling thread's last sa_align_pairs_affine, sa_align_pairs_banded, sa_align_pairs_band_at, sa_align_pairs_extend, sa_align_pairs_seeds,
 * sa_align_pairs_extend_band, sa_align_pairs_seeds_band, sa_align_pairs_chains, sa_align_pairs_cigar or sa_search_affine (k > 0): device
 * time of the traced fills and of the walks in milliseconds (summed over the chunks), the bytes of the
 * direction arena and the number of chunks. Each pointer may be NULL. */
int sa_affine_last_stats(double *fill_ms, double *walk_ms, uint64_t *arena_bytes, int32_t *num_chunks);

/* ---- misc ------------------------------------------------------------------------------ */
int sa_device_count(int *count);
const char *sa_last_error(void);
int sa_abi_version(void);
/* Hash of the sources the library was built from (sequence-alignment-gpu_amd/python/sa_amd/buildid.py):
 * callers compare it with the hash of the sources they ship with and refuse a stale binary. */
const char *sa_build_id(void);
/* Runs the engine's wave-level primitive self-test on `device` (DPP lane shifts, ballots);
 * returns SA_OK when the hardware behaves as the kernels assume. */
int sa_selftest(int device);

#ifdef __cplusplus
}
#endif
#endif /* SA_HIP_H */
