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
    delete[] response->alignedTextBytes;
    delete[] response->alignedPatternBytes;
    response->alignedTextBytes = nullptr;
    response->alignedPatternBytes = nullptr;
    try
    {
        response->alignedTextBytes = new char[cap];
        response->alignedPatternBytes = new char[cap];
    }
    catch (const std::bad_alloc &)
    {
        std::cout << SequenceAlignment::MEM_ERROR;
        return 1;
    }
    const int rc = sa_align_pair(&params, request.textBytes, n, request.patternBytes, m, deviceFromEnv(), &result,
                                 response->alignedTextBytes, response->alignedPatternBytes, cap, nullptr);
    if (rc != SA_OK)
    {
        std::cout << (rc == SA_ERR_NOMEM ? SequenceAlignment::MEM_ERROR : "error: " + std::string(sa_last_error()) + "\n");
        return 1;
    }
    response->score = result.score;
    response->numAlignmentBytes = result.num_alignment_bytes;
    response->startInAlignedText = result.start_text;
    response->startInAlignedPattern = result.start_pattern;
    return 0;
}

bool sameScheme(const sa_params &a, const sa_params &b)
{
    return a.mode == b.mode && a.alphabet_size == b.alphabet_size && a.gap_penalty == b.gap_penalty &&
           a.alphabet == b.alphabet &&
           std::memcmp(a.score_matrix, b.score_matrix, sizeof(int) * a.alphabet_size * a.alphabet_size) == 0;
}

// Fresh Response buffers for a request of a batch call (the callee allocates, as alignSequenceGPU does)
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

void storeResult(const sa_result &res, SequenceAlignment::Response &rs)
{
    rs.score = res.score;
    rs.numAlignmentBytes = res.num_alignment_bytes;
    rs.startInAlignedText = res.start_text;
    rs.startInAlignedPattern = res.start_pattern;
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
        if (rc != SA_OK)
        {
            std::cout << (rc == SA_ERR_NOMEM ? SequenceAlignment::MEM_ERROR : "error: " + std::string(sa_last_error()) + "\n");
            return 1;
        }
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
// scoreSequencesGPU, scoreSequencesGPUAffine and scoreSequencesGPUBanded: `gap` null is the requests'
// linear gapPenalty, else {gap open, gap extend} and gapPenalty is ignored; `band` non-null is the
// band's half-width; `ends` non-null is scoreSequencesGPUEndsFree with these flags; `lo` and `hi` non-null
// are scoreSequencesGPUBandAt's per-request bands; `xdrop` non-null is scoreSequencesGPUExtend (the mode is
// SA_GLOBAL, whose borders an extension has, and Request::alignmentType is ignored); `seeds` non-null (with
// `xdrop`) is scoreSequencesGPUSeeds
uint64_t scoreRequests(const SequenceAlignment::Request *requests, uint64_t numRequests, int device, const int *gap,
                       int *scores, const char *name, const int *band = nullptr, const int *ends = nullptr,
                       const int *lo = nullptr, const int *hi = nullptr, const int *xdrop = nullptr,
                       const std::vector<sa_seed> *seeds = nullptr)
{
    if (numRequests == 0) return 0;
    std::vector<sa_params> params(numRequests);
    std::vector<sa_host_pair> pairs(numRequests);
    for (uint64_t i = 0; i < numRequests; ++i)
    {
        const int none = 0;
        if (!toParams(requests[i], &params[i], true, xdrop ? &none : ends))
        {
            std::cout << "error: " << name << " takes global, local and semi-global alignments\n";
            return 1;
        }
        if (xdrop) params[i].mode = SA_GLOBAL;
        if (gap) params[i].gap_penalty = 0;
        if (!sameScheme(params[0], params[i]))
        {
            std::cout << "error: " << name << " needs one scoring scheme for all requests\n";
            return 1;
        }
        pairs[i] = sa_host_pair{requests[i].textBytes, requests[i].textNumBytes, requests[i].patternBytes,
                                requests[i].patternNumBytes};
    }
    std::vector<sa_score_result> res(numRequests);
    std::vector<sa_band> bands;
    for (uint64_t i = 0; lo && i < numRequests; ++i) bands.push_back(sa_band{lo[i], hi[i]});
    if (seeds)
    {
        std::vector<sa_seed_result> sres(numRequests);
        if (sa_score_batch_seeds(&params[0], gap[0], gap[1], *xdrop, seeds->data(), pairs.data(), (int64_t)numRequests, device, sres.data()) != SA_OK)
        {
            std::cout << "error: " + std::string(sa_last_error()) + "\n";
            return 1;
        }
        for (uint64_t i = 0; i < numRequests; ++i) scores[i] = sres[i].score;
        return 0;
    }
    const int rc = xdrop ? sa_score_batch_extend(&params[0], gap[0], gap[1], *xdrop, pairs.data(), (int64_t)numRequests, device, res.data())
                   : lo ? sa_score_batch_band_at(&params[0], gap[0], gap[1], bands.data(), pairs.data(), (int64_t)numRequests, device, res.data())
                   : band ? sa_score_batch_banded(&params[0], gap[0], gap[1], *band, pairs.data(), (int64_t)numRequests, device, res.data())
                   : gap ? sa_score_batch_affine(&params[0], gap[0], gap[1], pairs.data(), (int64_t)numRequests, device, res.data())
                         : sa_score_batch(&params[0], pairs.data(), (int64_t)numRequests, device, res.data());
    if (rc != SA_OK)
    {
        std::cout << (rc == SA_ERR_NOMEM ? SequenceAlignment::MEM_ERROR : "error: " + std::string(sa_last_error()) + "\n");
        return 1;
    }
    for (uint64_t i = 0; i < numRequests; ++i) scores[i] = res[i].score;
    return 0;
}

// alignSequencesGPUAffine and, with `band`, alignSequencesGPUBanded; with `ends`, alignSequencesGPUEndsFree;
// with `lo` and `hi`, alignSequencesGPUBandAt; with `xdrop`, alignSequencesGPUExtend; with `seeds` too,
// alignSequencesGPUSeeds
uint64_t alignRequests(const SequenceAlignment::Request *requests, SequenceAlignment::Response *responses, uint64_t numRequests,
                       int device, int gapOpen, int gapExtend, const int *band, const std::string &name,
                       const int *ends = nullptr, const int *lo = nullptr, const int *hi = nullptr, const int *xdrop = nullptr,
                       const std::vector<sa_seed> *seeds = nullptr);

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

uint64_t SequenceAlignment::scoreSequencesGPUBandAt(const Request *requests, uint64_t numRequests, int device, int gapOpen,
                                                    int gapExtend, int freeEnds, const int *bandLo, const int *bandHi, int *scores)
{
    if (!bandAtArgsOk(freeEnds, bandLo, bandHi, numRequests, "scoreSequencesGPUBandAt")) return 1;
    const int gap[2] = {gapOpen, gapExtend};
    return scoreRequests(requests, numRequests, device, gap, scores, "scoreSequencesGPUBandAt", nullptr,
                         freeEnds < 0 ? nullptr : &freeEnds, bandLo, bandHi);
}

uint64_t SequenceAlignment::alignSequencesGPUBandAt(const Request *requests, Response *responses, uint64_t numRequests, int device,
                                                    int gapOpen, int gapExtend, int freeEnds, const int *bandLo, const int *bandHi)
{
    if (!bandAtArgsOk(freeEnds, bandLo, bandHi, numRequests, "alignSequencesGPUBandAt")) return 1;
    return alignRequests(requests, responses, numRequests, device, gapOpen, gapExtend, nullptr, "alignSequencesGPUBandAt",
                         freeEnds < 0 ? nullptr : &freeEnds, bandLo, bandHi);
}

uint64_t SequenceAlignment::scoreSequencesGPUExtend(const Request *requests, uint64_t numRequests, int device, int gapOpen,
                                                    int gapExtend, int xdrop, int *scores)
{
    const int gap[2] = {gapOpen, gapExtend};
    return scoreRequests(requests, numRequests, device, gap, scores, "scoreSequencesGPUExtend", nullptr, nullptr, nullptr, nullptr, &xdrop);
}

uint64_t SequenceAlignment::alignSequencesGPUExtend(const Request *requests, Response *responses, uint64_t numRequests, int device,
                                                    int gapOpen, int gapExtend, int xdrop)
{
    return alignRequests(requests, responses, numRequests, device, gapOpen, gapExtend, nullptr, "alignSequencesGPUExtend", nullptr, nullptr,
                         nullptr, &xdrop);
}

uint64_t SequenceAlignment::scoreSequencesGPUSeeds(const Request *requests, uint64_t numRequests, int device, int gapOpen, int gapExtend,
                                                   int xdrop, const uint64_t *seedTextPos, const uint64_t *seedPatternPos,
                                                   const uint64_t *seedLength, int *scores)
{
    std::vector<sa_seed> seeds;
    if (!seedsOk(seedTextPos, seedPatternPos, seedLength, numRequests, "scoreSequencesGPUSeeds", &seeds)) return 1;
    const int gap[2] = {gapOpen, gapExtend};
    return scoreRequests(requests, numRequests, device, gap, scores, "scoreSequencesGPUSeeds", nullptr, nullptr, nullptr, nullptr, &xdrop,
                         &seeds);
}

uint64_t SequenceAlignment::alignSequencesGPUSeeds(const Request *requests, Response *responses, uint64_t numRequests, int device,
                                                   int gapOpen, int gapExtend, int xdrop, const uint64_t *seedTextPos,
                                                   const uint64_t *seedPatternPos, const uint64_t *seedLength)
{
    std::vector<sa_seed> seeds;
    if (!seedsOk(seedTextPos, seedPatternPos, seedLength, numRequests, "alignSequencesGPUSeeds", &seeds)) return 1;
    return alignRequests(requests, responses, numRequests, device, gapOpen, gapExtend, nullptr, "alignSequencesGPUSeeds", nullptr, nullptr,
                         nullptr, &xdrop, &seeds);
}

uint64_t SequenceAlignment::scoreSequencesGPU(const Request *requests, uint64_t numRequests, int device, int *scores)
{
    return scoreRequests(requests, numRequests, device, nullptr, scores, "scoreSequencesGPU");
}

uint64_t SequenceAlignment::scoreSequencesGPUAffine(const Request *requests, uint64_t numRequests, int device, int gapOpen,
                                                    int gapExtend, int *scores)
{
    const int gap[2] = {gapOpen, gapExtend};
    return scoreRequests(requests, numRequests, device, gap, scores, "scoreSequencesGPUAffine");
}

uint64_t SequenceAlignment::scoreSequencesGPUBanded(const Request *requests, uint64_t numRequests, int device, int gapOpen,
                                                    int gapExtend, int band, int *scores)
{
    const int gap[2] = {gapOpen, gapExtend};
    return scoreRequests(requests, numRequests, device, gap, scores, "scoreSequencesGPUBanded", &band);
}

uint64_t SequenceAlignment::alignSequencesGPUAffine(const Request *requests, Response *responses, uint64_t numRequests,
                                                    int device, int gapOpen, int gapExtend)
{
    return alignRequests(requests, responses, numRequests, device, gapOpen, gapExtend, nullptr, "alignSequencesGPUAffine");
}

uint64_t SequenceAlignment::alignSequencesGPUBanded(const Request *requests, Response *responses, uint64_t numRequests,
                                                    int device, int gapOpen, int gapExtend, int band)
{
    return alignRequests(requests, responses, numRequests, device, gapOpen, gapExtend, &band, "alignSequencesGPUBanded");
}

uint64_t SequenceAlignment::scoreSequencesGPUEndsFree(const Request *requests, uint64_t numRequests, int device, int gapOpen,
                                                      int gapExtend, int freeEnds, int *scores)
{
    if (!endsFlagsOk(freeEnds, "scoreSequencesGPUEndsFree")) return 1;
    const int gap[2] = {gapOpen, gapExtend};
    return scoreRequests(requests, numRequests, device, gap, scores, "scoreSequencesGPUEndsFree", nullptr, &freeEnds);
}

uint64_t SequenceAlignment::alignSequencesGPUEndsFree(const Request *requests, Response *responses, uint64_t numRequests,
                                                      int device, int gapOpen, int gapExtend, int freeEnds)
{
    if (!endsFlagsOk(freeEnds, "alignSequencesGPUEndsFree")) return 1;
    return alignRequests(requests, responses, numRequests, device, gapOpen, gapExtend, nullptr, "alignSequencesGPUEndsFree", &freeEnds);
}

namespace
{
uint64_t alignRequests(const SequenceAlignment::Request *requests, SequenceAlignment::Response *responses, uint64_t numRequests,
                       int device, int gapOpen, int gapExtend, const int *band, const std::string &name, const int *ends,
                       const int *lo, const int *hi, const int *xdrop, const std::vector<sa_seed> *seeds)
{
    if (numRequests == 0) return 0;
    std::vector<sa_params> params(numRequests);
    std::vector<sa_host_pair> pairs(numRequests);
    std::vector<char *> at(numRequests), ap(numRequests);
    for (uint64_t i = 0; i < numRequests; ++i)
    {
        const int none = 0;
        if (!toParams(requests[i], &params[i], true, xdrop ? &none : ends))
        {
            std::cout << "error: " << name << " takes global, local and semi-global alignments\n";
            return 1;
        }
        if (xdrop) params[i].mode = SA_GLOBAL;
        params[i].gap_penalty = 0;
        if (!sameScheme(params[0], params[i]))
        {
            std::cout << "error: " << name << " needs one scoring scheme for all requests\n";
            return 1;
        }
        pairs[i] = sa_host_pair{requests[i].textBytes, requests[i].textNumBytes, requests[i].patternBytes,
                                requests[i].patternNumBytes};
        if (!allocResponse(requests[i], responses[i])) return 1;
        at[i] = responses[i].alignedTextBytes;
        ap[i] = responses[i].alignedPatternBytes;
    }
    std::vector<sa_result> res(numRequests);
    std::vector<sa_band> bands;
    for (uint64_t i = 0; lo && i < numRequests; ++i) bands.push_back(sa_band{lo[i], hi[i]});
    const int rc = seeds ? sa_align_pairs_seeds(&params[0], gapOpen, gapExtend, *xdrop, seeds->data(), pairs.data(), (int64_t)numRequests,
                                                device, res.data(), at.data(), ap.data())
                   : xdrop ? sa_align_pairs_extend(&params[0], gapOpen, gapExtend, *xdrop, pairs.data(), (int64_t)numRequests, device,
                                                 res.data(), at.data(), ap.data())
                   : lo ? sa_align_pairs_band_at(&params[0], gapOpen, gapExtend, bands.data(), pairs.data(), (int64_t)numRequests, device,
                                                 res.data(), at.data(), ap.data())
                   : band ? sa_align_pairs_banded(&params[0], gapOpen, gapExtend, *band, pairs.data(), (int64_t)numRequests, device,
                                                res.data(), at.data(), ap.data())
                        : sa_align_pairs_affine(&params[0], gapOpen, gapExtend, pairs.data(), (int64_t)numRequests, device,
                                                res.data(), at.data(), ap.data());
    if (rc != SA_OK)
    {
        std::cout << (rc == SA_ERR_NOMEM ? SequenceAlignment::MEM_ERROR : "error: " + std::string(sa_last_error()) + "\n");
        return 1;
    }
    for (uint64_t i = 0; i < numRequests; ++i) storeResult(res[i], responses[i]);
    return 0;
}
}  // namespace
