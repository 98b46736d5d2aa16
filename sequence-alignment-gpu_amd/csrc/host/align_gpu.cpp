// alignSequenceGPU — the drop-in replacement of the reference's GPU entry point
// (SequenceAlignment.hpp:127, alignSequenceGPU.cu:463-653), implemented in C++14 over the C ABI
// of sa_hip.h. Behaviour kept from the reference boundary:
//   * the callee allocates Response::alignedTextBytes / alignedPatternBytes with new[]
//     (alignSequenceGPU.cu:402-403) so the caller's ~Response can delete[] them;
//   * returns 0 on success, 1 on failure with the message on stdout (:543, :590);
//   * under -DBENCHMARK the caller gets alignSequenceGPUFillMicros: DP fill time in microseconds,
//     no traceback (:555-626).
// Differences: buffers are max(2*text, text+pattern) bytes (the reference's 2*text overflows when
// a direct caller passes a pattern longer than the text), previously held Response buffers are
// released instead of leaked, and the device is SA_DEVICE (default 0) instead of always 0.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "SequenceAlignment.hpp"
#include "sa_hip.h"

namespace
{
int deviceFromEnv()
{
    const char *e = std::getenv("SA_DEVICE");
    return e ? std::atoi(e) : 0;
}

// `fit`: the caller is one of the functions that take SEMI_GLOBAL (the score-only and affine ones);
// `ends`: the caller is one of the ends-free functions, the mode is SA_ENDS_FREE with these flags and
// Request::alignmentType is ignored
bool toParams(const SequenceAlignment::Request &request, sa_params *p, bool fit = false, const int *ends = nullptr)
{
    if (ends) p->mode = SA_ENDS_FREE | *ends;
    else if (request.alignmentType == SequenceAlignment::programArgs::GLOBAL) p->mode = SA_GLOBAL;
    else if (request.alignmentType == SequenceAlignment::programArgs::LOCAL) p->mode = SA_LOCAL;
    else if (fit && request.alignmentType == SequenceAlignment::programArgs::SEMI_GLOBAL) p->mode = SA_FIT;
    else return false;
    p->alphabet_size = request.alphabetSize;
    p->gap_penalty = request.gapPenalty;
    p->rows_per_lane = 0;
    p->score_matrix = request.scoreMatrix;
    p->alphabet = request.alphabet;
    return true;
}

// the flags of an ends-free function: SA_FREE_TEXT_BEGIN | ... | SA_FREE_PATTERN_END, nothing else
bool endsFlagsOk(int freeEnds, const char *name)
{
    if (freeEnds >= 0 && freeEnds <= 15) return true;
    std::cout << "error: " << name << " takes freeEnds 0..15 (SA_FREE_TEXT_BEGIN | SA_FREE_TEXT_END | SA_FREE_PATTERN_BEGIN | SA_FREE_PATTERN_END)\n";
    return false;
}

// Fresh Response buffers for a request (the callee allocates); what a Response held before is released
bool allocResponse(const SequenceAlignment::Request &rq, SequenceAlignment::Response &rs)
{
    const uint64_t cap = std::max<uint64_t>(1, std::max(2 * rq.textNumBytes, rq.textNumBytes + rq.patternNumBytes));
    delete[] rs.alignedTextBytes;
    delete[] rs.alignedPatternBytes;
    rs.alignedTextBytes = rs.alignedPatternBytes = nullptr;
    try
    {
        rs.alignedTextBytes = new char[cap];
        rs.alignedPatternBytes = new char[cap];
    }
    catch (const std::bad_alloc &)
    {
        std::cout << SequenceAlignment::MEM_ERROR;
        return false;
    }
    return true;
}

// a failed C ABI call: its message on stdout (a failed allocation as MEM_ERROR), and the 1 the caller returns
uint64_t reportFailure(int rc, bool memError = true)
{
    std::cout << (rc == SA_ERR_NOMEM && memError ? SequenceAlignment::MEM_ERROR : "error: " + std::string(sa_last_error()) + "\n");
    return 1;
}

void storeResult(const sa_result &res, SequenceAlignment::Response &rs)
{
    rs.score = res.score;
    rs.numAlignmentBytes = res.num_alignment_bytes;
    rs.startInAlignedText = res.start_text;
    rs.startInAlignedPattern = res.start_pattern;
}

uint64_t runGPU(const SequenceAlignment::Request &request, SequenceAlignment::Response *response, bool fillOnly)
{
    sa_params params;
    if (!toParams(request, &params))
    {
        std::cout << "error: only --global and --local alignments are implemented\n";
        return 1;
    }
    const uint64_t n = request.textNumBytes, m = request.patternNumBytes;
    const uint64_t cap = std::max<uint64_t>(1, std::max(2 * n, n + m));
    sa_result result;
    double fillMicros = 0.0;
    if (fillOnly)
    {
        // fill-time contract: no strings are produced, Response is left untouched
        if (sa_align_pair(&params, request.textBytes, n, request.patternBytes, m, deviceFromEnv(), &result,
                          nullptr, nullptr, cap, &fillMicros) != SA_OK)
        {
            std::cout << "error: " << sa_last_error() << "\n";
            return 1;
        }
        return std::max<uint64_t>(1, (uint64_t)(fillMicros + 0.5));
    }
    if (!allocResponse(request, *response)) return 1;  // `cap` bytes each
    const int rc = sa_align_pair(&params, request.textBytes, n, request.patternBytes, m, deviceFromEnv(), &result,
                                 response->alignedTextBytes, response->alignedPatternBytes, cap, nullptr);
    if (rc != SA_OK) return reportFailure(rc);
    storeResult(result, *response);
    return 0;
}

bool sameScheme(const sa_params &a, const sa_params &b)
{
    return a.mode == b.mode && a.alphabet_size == b.alphabet_size && a.gap_penalty == b.gap_penalty &&
           a.alphabet == b.alphabet &&
           std::memcmp(a.score_matrix, b.score_matrix, sizeof(int) * a.alphabet_size * a.alphabet_size) == 0;
}

}  // namespace

uint64_t SequenceAlignment::alignSequenceGPUBatch(const Request *requests, Response *responses, uint64_t numRequests,
                                                  int numGpus)
{
    // requests sharing one scoring scheme go to sa_align_batch together (one plan per device)
    std::vector<sa_params> params(numRequests);
    for (uint64_t i = 0; i < numRequests; ++i)
        if (!toParams(requests[i], &params[i]))
        {
            std::cout << "error: only --global and --local alignments are implemented\n";
            return 1;
        }
    std::vector<bool> done(numRequests, false);
    for (uint64_t lead = 0; lead < numRequests; ++lead)
    {
        if (done[lead]) continue;
        std::vector<uint64_t> group;
        for (uint64_t i = lead; i < numRequests; ++i)
            if (!done[i] && sameScheme(params[lead], params[i])) group.push_back(i);
        std::vector<sa_host_pair> pairs(group.size());
        std::vector<char *> at(group.size()), ap(group.size());
        std::vector<sa_result> res(group.size());
        for (size_t q = 0; q < group.size(); ++q)
        {
            const Request &rq = requests[group[q]];
            Response &rs = responses[group[q]];
            pairs[q] = sa_host_pair{rq.textBytes, rq.textNumBytes, rq.patternBytes, rq.patternNumBytes};
            if (!allocResponse(rq, rs)) return 1;
            at[q] = rs.alignedTextBytes;
            ap[q] = rs.alignedPatternBytes;
        }
        const int rc = sa_align_batch(&params[lead], pairs.data(), (int64_t)pairs.size(), std::max(1, numGpus),
                                      res.data(), at.data(), ap.data());
        if (rc != SA_OK) return reportFailure(rc);
        for (size_t q = 0; q < group.size(); ++q)
        {
            storeResult(res[q], responses[group[q]]);
            done[group[q]] = true;
        }
    }
    return 0;
}

uint64_t SequenceAlignment::alignSequenceGPU(const Request &request, Response *response)
{
    return runGPU(request, response, false);
}

uint64_t SequenceAlignment::alignSequenceGPUFillMicros(const Request &request, Response *response)
{
    return runGPU(request, response, true);
}

namespace
{
using SequenceAlignment::Request;
using SequenceAlignment::Response;

// What one of the batch functions below asks for, as a value; a null pointer is "not asked for".
struct Variant {
    const char *name;                 // the public function, for the messages
    bool affine;                      // gap open and gap extend, and Request::gapPenalty is ignored; else the linear gapPenalty
    int gapOpen, gapExtend;
    const int *band = nullptr;        // the band's half-width
    const int *ends = nullptr;        // the SA_FREE_* flags: the mode is SA_ENDS_FREE with them, Request::alignmentType is ignored
    const int *lo = nullptr, *hi = nullptr;       // the per-request bands of the ...BandAt functions
    const int *xdrop = nullptr;       // extension: the mode is SA_GLOBAL, whose borders an extension has, whatever alignmentType says
    const std::vector<sa_seed> *seeds = nullptr;  // with xdrop: the ...Seeds functions
    const int *width = nullptr;       // with xdrop: the ...ExtendBand and ...SeedsBand functions
    const std::vector<uint64_t> *chainOff = nullptr;  // with xdrop and seeds: the ...Chains functions, request k's seeds are [chainOff[k], chainOff[k + 1])
    explicit Variant(const char *n) : name(n), affine(false), gapOpen(0), gapExtend(0) {}
    Variant(const char *n, int open, int extend) : name(n), affine(true), gapOpen(open), gapExtend(extend) {}
};

// The requests of a call as the C ABI takes them. With `responses` (the aligners), each request's Response
// gets its fresh buffers as soon as the request has passed, and at / ap point at them.
struct Packed {
    std::vector<sa_params> params;  // one scheme: params[0] is the call's
    std::vector<sa_host_pair> pairs;
    std::vector<sa_band> bands;
    std::vector<char *> at, ap;
};
bool pack(const Variant &v, const Request *requests, Response *responses, uint64_t numRequests, Packed *k)
{
    k->params.resize(numRequests);
    k->pairs.resize(numRequests);
    for (uint64_t i = 0; i < numRequests; ++i)
    {
        const int none = 0;
        if (!toParams(requests[i], &k->params[i], true, v.xdrop ? &none : v.ends))
        {
            std::cout << "error: " << v.name << " takes global, local and semi-global alignments\n";
            return false;
        }
        if (v.xdrop) k->params[i].mode = SA_GLOBAL;
        if (v.affine) k->params[i].gap_penalty = 0;
        if (!sameScheme(k->params[0], k->params[i]))
        {
            std::cout << "error: " << v.name << " needs one scoring scheme for all requests\n";
            return false;
        }
        k->pairs[i] = sa_host_pair{requests[i].textBytes, requests[i].textNumBytes, requests[i].patternBytes,
                                   requests[i].patternNumBytes};
        if (!responses) continue;
        if (!allocResponse(requests[i], responses[i])) return false;
        k->at.push_back(responses[i].alignedTextBytes);
        k->ap.push_back(responses[i].alignedPatternBytes);
    }
    for (uint64_t i = 0; v.lo && i < numRequests; ++i) k->bands.push_back(sa_band{v.lo[i], v.hi[i]});
    return true;
}

// every score...GPU... function
uint64_t scoreRequests(const Variant &v, const Request *requests, uint64_t numRequests, int device, int *scores)
{
    if (numRequests == 0) return 0;
    Packed k;
    if (!pack(v, requests, nullptr, numRequests, &k)) return 1;
    const sa_params *P = &k.params[0];
    const sa_host_pair *pairs = k.pairs.data();
    const int64_t n = (int64_t)numRequests;
    std::vector<sa_score_result> res(numRequests);
    std::vector<sa_seed_result> sres(v.seeds ? numRequests : 0);
    const int rc = v.chainOff ? sa_score_batch_chains(P, v.gapOpen, v.gapExtend, *v.xdrop, v.seeds->data(), v.chainOff->data(), pairs, n, device, sres.data())
                   : v.seeds && v.width ? sa_score_batch_seeds_band(P, v.gapOpen, v.gapExtend, *v.xdrop, *v.width, v.seeds->data(), pairs, n, device, sres.data())
                   : v.width  ? sa_score_batch_extend_band(P, v.gapOpen, v.gapExtend, *v.xdrop, *v.width, pairs, n, device, res.data())
                   : v.seeds  ? sa_score_batch_seeds(P, v.gapOpen, v.gapExtend, *v.xdrop, v.seeds->data(), pairs, n, device, sres.data())
                   : v.xdrop  ? sa_score_batch_extend(P, v.gapOpen, v.gapExtend, *v.xdrop, pairs, n, device, res.data())
                   : v.lo     ? sa_score_batch_band_at(P, v.gapOpen, v.gapExtend, k.bands.data(), pairs, n, device, res.data())
                   : v.band   ? sa_score_batch_banded(P, v.gapOpen, v.gapExtend, *v.band, pairs, n, device, res.data())
                   : v.affine ? sa_score_batch_affine(P, v.gapOpen, v.gapExtend, pairs, n, device, res.data())
                              : sa_score_batch(P, pairs, n, device, res.data());
    if (rc != SA_OK) return reportFailure(rc, !v.seeds);  // scoreSequencesGPUSeeds has never said MEM_ERROR
    for (uint64_t i = 0; i < numRequests; ++i) scores[i] = v.seeds ? sres[i].score : res[i].score;
    return 0;
}

// every align...GPU... function that takes a gap model
uint64_t alignRequests(const Variant &v, const Request *requests, Response *responses, uint64_t numRequests, int device)
{
    if (numRequests == 0) return 0;
    Packed k;
    if (!pack(v, requests, responses, numRequests, &k)) return 1;
    const sa_params *P = &k.params[0];
    const sa_host_pair *pairs = k.pairs.data();
    const int64_t n = (int64_t)numRequests;
    std::vector<sa_result> res(numRequests);
    char **at = k.at.data(), **ap = k.ap.data();
    const int rc = v.chainOff ? sa_align_pairs_chains(P, v.gapOpen, v.gapExtend, *v.xdrop, v.seeds->data(), v.chainOff->data(), pairs, n, device, res.data(), at, ap)
                   : v.seeds && v.width ? sa_align_pairs_seeds_band(P, v.gapOpen, v.gapExtend, *v.xdrop, *v.width, v.seeds->data(), pairs, n, device, res.data(), at, ap)
                   : v.width ? sa_align_pairs_extend_band(P, v.gapOpen, v.gapExtend, *v.xdrop, *v.width, pairs, n, device, res.data(), at, ap)
                   : v.seeds ? sa_align_pairs_seeds(P, v.gapOpen, v.gapExtend, *v.xdrop, v.seeds->data(), pairs, n, device, res.data(), at, ap)
                   : v.xdrop ? sa_align_pairs_extend(P, v.gapOpen, v.gapExtend, *v.xdrop, pairs, n, device, res.data(), at, ap)
                   : v.lo    ? sa_align_pairs_band_at(P, v.gapOpen, v.gapExtend, k.bands.data(), pairs, n, device, res.data(), at, ap)
                   : v.band  ? sa_align_pairs_banded(P, v.gapOpen, v.gapExtend, *v.band, pairs, n, device, res.data(), at, ap)
                             : sa_align_pairs_affine(P, v.gapOpen, v.gapExtend, pairs, n, device, res.data(), at, ap);
    if (rc != SA_OK) return reportFailure(rc);
    for (uint64_t i = 0; i < numRequests; ++i) storeResult(res[i], responses[i]);
    return 0;
}

// the seeds of the ...Seeds functions: three arrays, one entry per request
bool seedsOk(const uint64_t *textPos, const uint64_t *patternPos, const uint64_t *length, uint64_t numRequests, const char *name,
             std::vector<sa_seed> *seeds)
{
    if (numRequests && (!textPos || !patternPos || !length))
    {
        std::cout << "error: " << name << " needs seedTextPos, seedPatternPos and seedLength, one entry per request\n";
        return false;
    }
    for (uint64_t i = 0; i < numRequests; ++i) seeds->push_back(sa_seed{textPos[i], patternPos[i], length[i]});
    return true;
}

// the mode argument of the band-at functions: -1 leaves the mode to Request::alignmentType
bool bandAtArgsOk(int freeEnds, const int *lo, const int *hi, uint64_t numRequests, const char *name)
{
    if (numRequests && (!lo || !hi))
    {
        std::cout << "error: " << name << " needs bandLo and bandHi, one entry per request\n";
        return false;
    }
    return freeEnds == -1 || endsFlagsOk(freeEnds, name);
}
}  // namespace

uint64_t SequenceAlignment::scoreSequencesGPU(const Request *requests, uint64_t numRequests, int device, int *scores)
{
    return scoreRequests(Variant("scoreSequencesGPU"), requests, numRequests, device, scores);
}

uint64_t SequenceAlignment::scoreSequencesGPUAffine(const Request *requests, uint64_t numRequests, int device, int gapOpen,
                                                    int gapExtend, int *scores)
{
    return scoreRequests(Variant("scoreSequencesGPUAffine", gapOpen, gapExtend), requests, numRequests, device, scores);
}

uint64_t SequenceAlignment::alignSequencesGPUAffine(const Request *requests, Response *responses, uint64_t numRequests,
                                                    int device, int gapOpen, int gapExtend)
{
    return alignRequests(Variant("alignSequencesGPUAffine", gapOpen, gapExtend), requests, responses, numRequests, device);
}

uint64_t SequenceAlignment::scoreSequencesGPUBanded(const Request *requests, uint64_t numRequests, int device, int gapOpen,
                                                    int gapExtend, int band, int *scores)
{
    Variant v("scoreSequencesGPUBanded", gapOpen, gapExtend);
    v.band = &band;
    return scoreRequests(v, requests, numRequests, device, scores);
}

uint64_t SequenceAlignment::alignSequencesGPUBanded(const Request *requests, Response *responses, uint64_t numRequests,
                                                    int device, int gapOpen, int gapExtend, int band)
{
    Variant v("alignSequencesGPUBanded", gapOpen, gapExtend);
    v.band = &band;
    return alignRequests(v, requests, responses, numRequests, device);
}

uint64_t SequenceAlignment::scoreSequencesGPUEndsFree(const Request *requests, uint64_t numRequests, int device, int gapOpen,
                                                      int gapExtend, int freeEnds, int *scores)
{
    if (!endsFlagsOk(freeEnds, "scoreSequencesGPUEndsFree")) return 1;
    Variant v("scoreSequencesGPUEndsFree", gapOpen, gapExtend);
    v.ends = &freeEnds;
    return scoreRequests(v, requests, numRequests, device, scores);
}

uint64_t SequenceAlignment::alignSequencesGPUEndsFree(const Request *requests, Response *responses, uint64_t numRequests,
                                                      int device, int gapOpen, int gapExtend, int freeEnds)
{
    if (!endsFlagsOk(freeEnds, "alignSequencesGPUEndsFree")) return 1;
    Variant v("alignSequencesGPUEndsFree", gapOpen, gapExtend);
    v.ends = &freeEnds;
    return alignRequests(v, requests, responses, numRequests, device);
}

uint64_t SequenceAlignment::scoreSequencesGPUBandAt(const Request *requests, uint64_t numRequests, int device, int gapOpen,
                                                    int gapExtend, int freeEnds, const int *bandLo, const int *bandHi, int *scores)
{
    if (!bandAtArgsOk(freeEnds, bandLo, bandHi, numRequests, "scoreSequencesGPUBandAt")) return 1;
    Variant v("scoreSequencesGPUBandAt", gapOpen, gapExtend);
    v.ends = freeEnds < 0 ? nullptr : &freeEnds;
    v.lo = bandLo;
    v.hi = bandHi;
    return scoreRequests(v, requests, numRequests, device, scores);
}

uint64_t SequenceAlignment::alignSequencesGPUBandAt(const Request *requests, Response *responses, uint64_t numRequests, int device,
                                                    int gapOpen, int gapExtend, int freeEnds, const int *bandLo, const int *bandHi)
{
    if (!bandAtArgsOk(freeEnds, bandLo, bandHi, numRequests, "alignSequencesGPUBandAt")) return 1;
    Variant v("alignSequencesGPUBandAt", gapOpen, gapExtend);
    v.ends = freeEnds < 0 ? nullptr : &freeEnds;
    v.lo = bandLo;
    v.hi = bandHi;
    return alignRequests(v, requests, responses, numRequests, device);
}

uint64_t SequenceAlignment::scoreSequencesGPUExtend(const Request *requests, uint64_t numRequests, int device, int gapOpen,
                                                    int gapExtend, int xdrop, int *scores)
{
    Variant v("scoreSequencesGPUExtend", gapOpen, gapExtend);
    v.xdrop = &xdrop;
    return scoreRequests(v, requests, numRequests, device, scores);
}

uint64_t SequenceAlignment::alignSequencesGPUExtend(const Request *requests, Response *responses, uint64_t numRequests, int device,
                                                    int gapOpen, int gapExtend, int xdrop)
{
    Variant v("alignSequencesGPUExtend", gapOpen, gapExtend);
    v.xdrop = &xdrop;
    return alignRequests(v, requests, responses, numRequests, device);
}

// the chains of the ...Chains functions: a count per request and three flat arrays over all requests' seeds
bool chainsOk(const uint64_t *count, const uint64_t *textPos, const uint64_t *patternPos, const uint64_t *length, uint64_t numRequests,
              const char *name, std::vector<sa_seed> *seeds, std::vector<uint64_t> *off)
{
    off->assign(1, 0);
    for (uint64_t i = 0; count && i < numRequests; ++i) off->push_back(off->back() + count[i]);
    if (numRequests && (!count || (off->back() && (!textPos || !patternPos || !length))))
    {
        std::cout << "error: " << name << " needs seedCount, one entry per request, and seedTextPos, seedPatternPos and seedLength, one entry per seed\n";
        return false;
    }
    for (uint64_t i = 0; i < off->back(); ++i) seeds->push_back(sa_seed{textPos[i], patternPos[i], length[i]});
    seeds->push_back(sa_seed{0, 0, 0});  // a call without a seed still passes an address: the library names the request
    return true;
}

uint64_t SequenceAlignment::scoreSequencesGPUChains(const Request *requests, uint64_t numRequests, int device, int gapOpen, int gapExtend,
                                                    int xdrop, const uint64_t *seedCount, const uint64_t *seedTextPos,
                                                    const uint64_t *seedPatternPos, const uint64_t *seedLength, int *scores)
{
    std::vector<sa_seed> seeds;
    std::vector<uint64_t> off;
    if (!chainsOk(seedCount, seedTextPos, seedPatternPos, seedLength, numRequests, "scoreSequencesGPUChains", &seeds, &off)) return 1;
    Variant v("scoreSequencesGPUChains", gapOpen, gapExtend);
    v.xdrop = &xdrop;
    v.seeds = &seeds;
    v.chainOff = &off;
    return scoreRequests(v, requests, numRequests, device, scores);
}

uint64_t SequenceAlignment::alignSequencesGPUChains(const Request *requests, Response *responses, uint64_t numRequests, int device,
                                                    int gapOpen, int gapExtend, int xdrop, const uint64_t *seedCount,
                                                    const uint64_t *seedTextPos, const uint64_t *seedPatternPos, const uint64_t *seedLength)
{
    std::vector<sa_seed> seeds;
    std::vector<uint64_t> off;
    if (!chainsOk(seedCount, seedTextPos, seedPatternPos, seedLength, numRequests, "alignSequencesGPUChains", &seeds, &off)) return 1;
    Variant v("alignSequencesGPUChains", gapOpen, gapExtend);
    v.xdrop = &xdrop;
    v.seeds = &seeds;
    v.chainOff = &off;
    return alignRequests(v, requests, responses, numRequests, device);
}

uint64_t SequenceAlignment::alignSequencesGPUCigar(const Request *requests, CigarResponse *responses, uint64_t numRequests, int device,
                                                   const sa_align_spec &spec, bool eqx, int freeEnds)
{
    if (numRequests == 0) return 0;
    if (freeEnds != -1 && !endsFlagsOk(freeEnds, "alignSequencesGPUCigar")) return 1;
    Variant v("alignSequencesGPUCigar", spec.gap_open, spec.gap_extend);
    if (spec.extend) v.xdrop = &spec.xdrop;  // an extension's mode is SA_GLOBAL, whatever alignmentType says
    if (freeEnds != -1) v.ends = &freeEnds;
    Packed k;
    if (!pack(v, requests, nullptr, numRequests, &k)) return 1;
    std::vector<sa_cigar_result> res(numRequests);
    sa_cigars *cigars = nullptr;
    const int rc = sa_align_pairs_cigar(&k.params[0], &spec, eqx ? SA_CIGAR_EQX : SA_CIGAR_M, k.pairs.data(), (int64_t)numRequests, device,
                                        res.data(), &cigars);
    if (rc != SA_OK) return reportFailure(rc);
    const uint32_t *ops = sa_cigars_ops(cigars);
    for (uint64_t i = 0; i < numRequests; ++i)
    {
        CigarResponse &rs = responses[i];
        rs.score = res[i].score;
        rs.numAlignmentBytes = res[i].num_alignment_bytes;
        rs.startInAlignedText = res[i].start_text;
        rs.startInAlignedPattern = res[i].start_pattern;
        rs.ops.clear();
        if (res[i].num_ops) rs.ops.assign(ops + res[i].ops_off, ops + res[i].ops_off + res[i].num_ops);
        rs.matches = res[i].matches;
        rs.mismatches = res[i].mismatches;
        rs.textGapLetters = res[i].text_gap_letters;
        rs.patternGapLetters = res[i].pattern_gap_letters;
        rs.gapOpens = res[i].gap_opens;
    }
    sa_cigars_destroy(cigars);
    return 0;
}

uint64_t SequenceAlignment::chainAnchorsGPU(ChainResponse *responses, uint64_t numPairs, int device, const sa_chain_params &params,
                                            const uint64_t *anchorCount, const uint64_t *anchorTextPos, const uint64_t *anchorPatternPos,
                                            const uint64_t *anchorLength)
{
    if (numPairs == 0) return 0;
    if (!responses || !anchorCount)
    {
        std::cout << "error: chainAnchorsGPU: null argument\n";
        return 1;
    }
    std::vector<uint64_t> off(numPairs + 1, 0);
    for (uint64_t k = 0; k < numPairs; ++k) off[k + 1] = off[k] + anchorCount[k];
    if (off[numPairs] > 0 && (!anchorTextPos || !anchorPatternPos || !anchorLength))
    {
        std::cout << "error: chainAnchorsGPU: null anchor array\n";
        return 1;
    }
    std::vector<sa_seed> anchors(off[numPairs] + 1);  // one more: a call without any anchor still passes an address
    for (uint64_t a = 0; a < off[numPairs]; ++a) anchors[a] = sa_seed{anchorTextPos[a], anchorPatternPos[a], anchorLength[a]};
    std::vector<sa_chain_result> res(numPairs);
    sa_chain_set *set = nullptr;
    const int rc = sa_chain_anchors(&params, anchors.data(), off.data(), (int64_t)numPairs, device, res.data(), &set);
    if (rc != SA_OK) return reportFailure(rc);
    const sa_seed *seeds = sa_chain_set_seeds(set);
    for (uint64_t k = 0; k < numPairs; ++k)
    {
        ChainResponse &rs = responses[k];
        rs.score = res[k].score;
        rs.lastAnchor = res[k].last_anchor;
        rs.seedTextPos.clear(), rs.seedPatternPos.clear(), rs.seedLength.clear();
        for (uint64_t s = res[k].seeds_off; s < res[k].seeds_off + res[k].num_seeds; ++s)
        {
            rs.seedTextPos.push_back(seeds[s].text_pos);
            rs.seedPatternPos.push_back(seeds[s].pattern_pos);
            rs.seedLength.push_back(seeds[s].length);
        }
    }
    sa_chain_set_destroy(set);
    return 0;
}

uint64_t SequenceAlignment::scoreSequencesGPUSeeds(const Request *requests, uint64_t numRequests, int device, int gapOpen, int gapExtend,
                                                   int xdrop, const uint64_t *seedTextPos, const uint64_t *seedPatternPos,
                                                   const uint64_t *seedLength, int *scores)
{
    std::vector<sa_seed> seeds;
    if (!seedsOk(seedTextPos, seedPatternPos, seedLength, numRequests, "scoreSequencesGPUSeeds", &seeds)) return 1;
    Variant v("scoreSequencesGPUSeeds", gapOpen, gapExtend);
    v.xdrop = &xdrop;
    v.seeds = &seeds;
    return scoreRequests(v, requests, numRequests, device, scores);
}

uint64_t SequenceAlignment::alignSequencesGPUSeeds(const Request *requests, Response *responses, uint64_t numRequests, int device,
                                                   int gapOpen, int gapExtend, int xdrop, const uint64_t *seedTextPos,
                                                   const uint64_t *seedPatternPos, const uint64_t *seedLength)
{
    std::vector<sa_seed> seeds;
    if (!seedsOk(seedTextPos, seedPatternPos, seedLength, numRequests, "alignSequencesGPUSeeds", &seeds)) return 1;
    Variant v("alignSequencesGPUSeeds", gapOpen, gapExtend);
    v.xdrop = &xdrop;
    v.seeds = &seeds;
    return alignRequests(v, requests, responses, numRequests, device);
}

uint64_t SequenceAlignment::scoreSequencesGPUExtendBand(const Request *requests, uint64_t numRequests, int device, int gapOpen,
                                                        int gapExtend, int xdrop, int width, int *scores)
{
    Variant v("scoreSequencesGPUExtendBand", gapOpen, gapExtend);
    v.xdrop = &xdrop;
    v.width = &width;
    return scoreRequests(v, requests, numRequests, device, scores);
}

uint64_t SequenceAlignment::alignSequencesGPUExtendBand(const Request *requests, Response *responses, uint64_t numRequests, int device,
                                                        int gapOpen, int gapExtend, int xdrop, int width)
{
    Variant v("alignSequencesGPUExtendBand", gapOpen, gapExtend);
    v.xdrop = &xdrop;
    v.width = &width;
    return alignRequests(v, requests, responses, numRequests, device);
}

uint64_t SequenceAlignment::scoreSequencesGPUSeedsBand(const Request *requests, uint64_t numRequests, int device, int gapOpen,
                                                       int gapExtend, int xdrop, int width, const uint64_t *seedTextPos,
                                                       const uint64_t *seedPatternPos, const uint64_t *seedLength, int *scores)
{
    std::vector<sa_seed> seeds;
    if (!seedsOk(seedTextPos, seedPatternPos, seedLength, numRequests, "scoreSequencesGPUSeedsBand", &seeds)) return 1;
    Variant v("scoreSequencesGPUSeedsBand", gapOpen, gapExtend);
    v.xdrop = &xdrop;
    v.width = &width;
    v.seeds = &seeds;
    return scoreRequests(v, requests, numRequests, device, scores);
}

uint64_t SequenceAlignment::alignSequencesGPUSeedsBand(const Request *requests, Response *responses, uint64_t numRequests, int device,
                                                       int gapOpen, int gapExtend, int xdrop, int width, const uint64_t *seedTextPos,
                                                       const uint64_t *seedPatternPos, const uint64_t *seedLength)
{
    std::vector<sa_seed> seeds;
    if (!seedsOk(seedTextPos, seedPatternPos, seedLength, numRequests, "alignSequencesGPUSeedsBand", &seeds)) return 1;
    Variant v("alignSequencesGPUSeedsBand", gapOpen, gapExtend);
    v.xdrop = &xdrop;
    v.width = &width;
    v.seeds = &seeds;
    return alignRequests(v, requests, responses, numRequests, device);
}
