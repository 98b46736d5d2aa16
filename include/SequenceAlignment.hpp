// SequenceAlignment.hpp — the request/response API of robertszafa/sequence-alignment-gpu, re-declared
// for the MI355X build so that existing callers (the alignSequence CLI, tests, benchmarks) compile
// against it unchanged.
//
// Interface parity with the reference header (SequenceAlignment.hpp of the reference):
//   programArgs / argumentMap / USAGE / error strings          :10-50
//   alphabets, sizes, defaults                                  :52-68
//   Request / Response (same members, same order, same owners)  :71-120
//   DIRECTION                                                   :122
//   alignSequenceCPU / alignSequenceGPU / traceBackNW / traceBackSW  :125-131
// Differences: the implementation is compiled into libsequence_alignment.so instead of being
// #included into every translation unit (reference :138-140), so the free functions of
// utilities.cpp are declared here too, and the -DBENCHMARK contract of alignSequenceGPU
// (return fill time in microseconds, skip the traceback; alignSequenceGPU.cu:555-626) is
// selected per caller by the macro below instead of by recompiling the engine.
#pragma once

#include <cstdint>
#include <iostream>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

struct sa_align_spec;    // sa_hip.h: what alignSequencesGPUCigar takes
struct sa_chain_params;  // sa_hip.h: what chainAnchorsGPU takes

namespace SequenceAlignment
{
enum programArgs
{
    CPU, GPU,                     // device
    DNA, PROTEIN,                 // sequence type
    GLOBAL, LOCAL, SEMI_GLOBAL,   // algorithm (SEMI_GLOBAL is declared by the reference, never implemented there;
                                  // here scoreSequencesGPU, scoreSequencesGPUAffine and alignSequencesGPUAffine take it)
    SCORE_MATRIX,                 // next argument: score matrix file
    GAP_PENALTY,                  // next argument: gap penalty
};

const std::unordered_map<std::string, programArgs> argumentMap = {
    {"--cpu", programArgs::CPU},          {"-c", programArgs::CPU},
    {"--gpu", programArgs::GPU},          {"-g", programArgs::GPU},
    {"--dna", programArgs::DNA},          {"-d", programArgs::DNA},
    {"--protein", programArgs::PROTEIN},  {"-p", programArgs::PROTEIN},
    {"--global", programArgs::GLOBAL},    {"--local", programArgs::LOCAL},
    {"--score-matrix", programArgs::SCORE_MATRIX}, {"-s", programArgs::SCORE_MATRIX},
    {"--gap-penalty", programArgs::GAP_PENALTY},
};

// User-facing text (byte-identical to the reference: the CLI prints it).
const std::string USAGE =
    "Usage: ./alignSequence [-d|-p] [-c|-g] [--global|--local] [-s <file>] [--gap-penalty <int>] <file> <file>\n"
    "       -d, --dna             - align dna sequences (default)\n"
    "       -p, --protein         - align protein sequence\n"
    "       -c, --cpu             - use cpu device (default)\n"
    "       -g, --gpu             - use gpu device\n"
    "       --global              - use global alignment (default)\n"
    "       --local               - use local alignment\n"
    "       -s, --score-matrix    - next argument is a score matrix file\n"
    "       --gap-penalty         - next argument is a gap open penalty (default 5)\n";
const std::string SEQ_NOT_READ_ERROR = "error: text sequence or pattern sequence not read\n";
const std::string MEM_ERROR = "error: sequence is too long, not enough memory\n";
const std::string SCORE_MATRIX_NOT_READ_ERROR =
    "error: matrix scores not read. Only integer scores accepted (int)\n";
const std::string GAP_PENALTY_NOT_READ_ERROR =
    "error: gap penalty not read. Only integer scores accepted (int)\n";

const unsigned int NUM_DNA_CHARS = 4;
const unsigned int NUM_PROTEIN_CHARS = 23;
// Letter i of a sequence is stored as its index in the alphabet; the entry after the last
// letter is the gap character used in aligned output.
const char DNA_ALPHABET[] = {'A', 'T', 'C', 'G', '-'};
const char PROTEIN_ALPHABET[] = {'A', 'R', 'N', 'D', 'C', 'Q', 'E', 'G', 'H', 'I', 'L', 'K',
                                 'M', 'F', 'P', 'S', 'T', 'W', 'Y', 'V', 'B', 'Z', 'X', '-'};

const programArgs DEFAULT_DEVICE = programArgs::CPU;
const programArgs DEFAULT_SEQUENCE = programArgs::DNA;
const programArgs DEFAULT_ALIGNMENT_TYPE = programArgs::GLOBAL;
static const char *DEFAULT_ALPHABET __attribute__((unused)) = DNA_ALPHABET;
const int DEFAULT_ALPHABET_SIZE = NUM_DNA_CHARS;
const short DEFAULT_GAP_PENALTY = 5;
const std::string DEFAULT_DNA_SCORE_MATRIX_FILE = "scoreMatrices/dna/blast.txt";
const std::string DEFAULT_PROTEIN_SCORE_MATRIX_FILE = "scoreMatrices/protein/blosum50.txt";

struct Request
{
    programArgs deviceType;
    programArgs sequenceType;
    programArgs alignmentType;
    char *textBytes = nullptr;        // alphabet indices, owned (delete[])
    uint64_t textNumBytes;
    char *patternBytes = nullptr;     // alphabet indices, owned (delete[])
    uint64_t patternNumBytes;
    const char *alphabet; int alphabetSize;
    int scoreMatrix[NUM_PROTEIN_CHARS * NUM_PROTEIN_CHARS];  // row-major, stride alphabetSize
    int gapPenalty;

    ~Request()
    {
        delete[] textBytes;
        delete[] patternBytes;
        textBytes = nullptr;
        patternBytes = nullptr;
    }
};

struct Response
{
    char *alignedTextBytes = nullptr;     // letters or '-', forward order, owned (delete[])
    char *alignedPatternBytes = nullptr;
    uint64_t numAlignmentBytes;
    uint64_t startInAlignedText;          // may be (uint64_t)-1 for an empty local alignment
    uint64_t startInAlignedPattern;
    int score;

    ~Response()
    {
        delete[] alignedTextBytes;
        delete[] alignedPatternBytes;
        alignedTextBytes = nullptr;
        alignedPatternBytes = nullptr;
    }
};

enum DIRECTION { LEFT, DIAG, TOP, STOP };

/// CPU device (-c): host implementation in libsequence_alignment.so.
uint64_t alignSequenceCPU(const Request &, Response *);

/// GPU device (-g): the MI355X engine through the C ABI of sa_hip.h. Returns 0 or 1.
uint64_t alignSequenceGPU(const Request &, Response *);

/// -DBENCHMARK contract of the reference: DP fill only, returns its device time in microseconds.
uint64_t alignSequenceGPUFillMicros(const Request &, Response *);

/// Extension (the reference has no multi-GPU path): numRequests independent requests in one call,
/// sharded over devices 0..numGpus-1 (sa_align_batch: one plan per device, RCCL result gather).
/// Fills responses[i] as alignSequenceGPU would. Returns 0, or 1 with the message on stdout.
uint64_t alignSequenceGPUBatch(const Request *requests, Response *responses, uint64_t numRequests, int numGpus);

/// Extension: Response::score of numRequests requests on `device`, without alignments (sa_score_batch:
/// no direction matrix, no traceback). All requests must share one scoring scheme (alignment type,
/// alphabet, score matrix, gap penalty). scores: numRequests entries. Returns 0, or 1 with the
/// message on stdout. Request::alignmentType may also be SEMI_GLOBAL (sa_hip.h: SA_FIT, the whole
/// pattern inside the text, the text free at both ends), here and in the two functions below; every
/// other entry point and the CLI keep rejecting it.
uint64_t scoreSequencesGPU(const Request *requests, uint64_t numRequests, int device, int *scores);

/// Extension: the same under affine gap penalties (sa_score_batch_affine, Gotoh): a gap of k letters
/// costs gapOpen + (k - 1) * gapExtend and Request::gapPenalty is ignored. One scoring scheme for all
/// requests, as above. Returns 0, or 1 with the message on stdout.
uint64_t scoreSequencesGPUAffine(const Request *requests, uint64_t numRequests, int device, int gapOpen, int gapExtend,
                                 int *scores);

/// Extension: numRequests requests aligned on `device` under affine gap penalties
/// (sa_align_pairs_affine: traced Gotoh fill and a traceback over the three states). Fills
/// responses[i] as alignSequenceGPUBatch does; Request::gapPenalty is ignored. One scoring scheme for
/// all requests, as above. Returns 0, or 1 with the message on stdout.
uint64_t alignSequencesGPUAffine(const Request *requests, Response *responses, uint64_t numRequests, int device,
                                 int gapOpen, int gapExtend);

/// Extension: the two functions above inside a diagonal band of half-width `band` >= 0
/// (sa_score_batch_banded, sa_align_pairs_banded; sa_hip.h has the definition): cell (i, j) counts iff
/// min(0, n - m) - band <= j - i <= max(0, n - m) + band, n text and m pattern letters. Global and
/// local alignments only; a caller with a linear gap passes its penalty as gapOpen and gapExtend. With
/// band >= max(n, m) every value equals the unbanded function's. Returns 0, or 1 with the message on
/// stdout.
uint64_t scoreSequencesGPUBanded(const Request *requests, uint64_t numRequests, int device, int gapOpen, int gapExtend,
                                 int band, int *scores);
uint64_t alignSequencesGPUBanded(const Request *requests, Response *responses, uint64_t numRequests, int device,
                                 int gapOpen, int gapExtend, int band);

/// Extension: scores and alignments with free sequence ends (sa_hip.h: SA_ENDS_FREE; sa_score_batch_affine
/// and sa_align_pairs_affine in mode SA_ENDS_FREE | freeEnds). freeEnds is any of SA_FREE_TEXT_BEGIN (1),
/// SA_FREE_TEXT_END (2), SA_FREE_PATTERN_BEGIN (4) and SA_FREE_PATTERN_END (8) or'ed together: 15 is the
/// overlap (dovetail) alignment, 3 the fit of the pattern inside the text, 0 global alignment.
/// Request::alignmentType is ignored (programArgs is the reference's enum and has no such type), and so
/// is Request::gapPenalty: a caller with a linear gap passes its penalty as gapOpen and gapExtend. One
/// alphabet and score matrix for all requests. Response::startInAlignedText and startInAlignedPattern
/// are the 0-based indices of the first aligned letters. Returns 0, or 1 with the message on stdout.
uint64_t scoreSequencesGPUEndsFree(const Request *requests, uint64_t numRequests, int device, int gapOpen, int gapExtend,
                                   int freeEnds, int *scores);
uint64_t alignSequencesGPUEndsFree(const Request *requests, Response *responses, uint64_t numRequests, int device,
                                   int gapOpen, int gapExtend, int freeEnds);

/// Extension: scores and alignments inside a band of the caller's per request (sa_score_batch_band_at,
/// sa_align_pairs_band_at; sa_hip.h has the definition): request k counts cell (i, j) iff
/// bandLo[k] <= j - i <= bandHi[k], whatever its lengths. A read that a seed places at text letter c fits
/// inside {c - w, c + w}. freeEnds chooses the mode as the ...EndsFree functions do, with one value more:
/// 0..15 is SA_ENDS_FREE | freeEnds and Request::alignmentType is ignored (3 the fit, 15 the overlap);
/// -1 leaves the mode to Request::alignmentType, GLOBAL, LOCAL or SEMI_GLOBAL (the fit), so local
/// alignment is reached this way only. Request::gapPenalty is ignored: a caller with a linear gap passes
/// its penalty as gapOpen and gapExtend. One alphabet and score matrix for all requests. A request whose
/// band admits no alignment of the mode fails the whole call (sa_band_reachable tells beforehand), and
/// so does bandLo[k] > bandHi[k]. Responses as alignSequencesGPUEndsFree fills them (-1: as
/// alignSequencesGPUAffine does for the type). Returns 0, or 1 with the message on stdout.
uint64_t scoreSequencesGPUBandAt(const Request *requests, uint64_t numRequests, int device, int gapOpen, int gapExtend,
                                 int freeEnds, const int *bandLo, const int *bandHi, int *scores);
uint64_t alignSequencesGPUBandAt(const Request *requests, Response *responses, uint64_t numRequests, int device,
                                 int gapOpen, int gapExtend, int freeEnds, const int *bandLo, const int *bandHi);

/// Extension: extension alignment (sa_score_batch_extend, sa_align_pairs_extend; sa_hip.h has the
/// definition): the alignment starts at the first letters of both sequences (the end of a seed), ends at
/// the best-scoring cell, and rows after the first one whose best lies more than xdrop below the best seen
/// count for nothing; xdrop -1 (SA_NO_XDROP) never stops. Request::alignmentType and Request::gapPenalty are
/// ignored: a caller with a linear gap passes its penalty as gapOpen and gapExtend. One alphabet and score
/// matrix for all requests. Response::startInAlignedText and startInAlignedPattern are 0; the aligned
/// strings without their gap letters are the prefixes of text and pattern the extension covers. Returns 0,
/// or 1 with the message on stdout.
uint64_t scoreSequencesGPUExtend(const Request *requests, uint64_t numRequests, int device, int gapOpen, int gapExtend,
                                 int xdrop, int *scores);
uint64_t alignSequencesGPUExtend(const Request *requests, Response *responses, uint64_t numRequests, int device,
                                 int gapOpen, int gapExtend, int xdrop);

/// Extension: seed extension (sa_score_batch_seeds, sa_align_pairs_seeds; sa_hip.h has the definition). Request
/// k carries the seed text[seedTextPos[k] : + seedLength[k]] against pattern[seedPatternPos[k] : + seedLength[k]],
/// which lies without a gap and is scored as it is; the extension alignment of what follows the seed and the
/// one of what precedes it, both sequences read backwards in place, are joined with it in one call under one
/// xdrop (-1, SA_NO_XDROP, never stops). The score is the sum of the three; Response::startInAlignedText and
/// startInAlignedPattern are the 0-based indices of the first aligned letters, and the aligned strings are
/// the left extension, the seed's letters and the right extension in forward order. Request::alignmentType
/// and Request::gapPenalty are ignored; one alphabet and score matrix for all requests. A seed that does
/// not lie inside its request fails the whole call. Returns 0, or 1 with the message on stdout.
uint64_t scoreSequencesGPUSeeds(const Request *requests, uint64_t numRequests, int device, int gapOpen, int gapExtend,
                                int xdrop, const uint64_t *seedTextPos, const uint64_t *seedPatternPos,
                                const uint64_t *seedLength, int *scores);
uint64_t alignSequencesGPUSeeds(const Request *requests, Response *responses, uint64_t numRequests, int device,
                                int gapOpen, int gapExtend, int xdrop, const uint64_t *seedTextPos,
                                const uint64_t *seedPatternPos, const uint64_t *seedLength);

/// Extension: the four functions above inside a width of the anchor's diagonal (sa_score_batch_extend_band,
/// sa_align_pairs_extend_band, sa_score_batch_seeds_band, sa_align_pairs_seeds_band; sa_hip.h has the
/// definition): cell (i, j) of an extension matrix counts iff |j - i| <= width, for a seeded request in each
/// half's own coordinates, one width >= 0 for all requests. With width >= max(n, m) every value equals the
/// function's without a width. The aligners keep direction bytes for the band only. Everything else as the
/// functions above. Returns 0, or 1 with the message on stdout.
uint64_t scoreSequencesGPUExtendBand(const Request *requests, uint64_t numRequests, int device, int gapOpen, int gapExtend,
                                     int xdrop, int width, int *scores);
uint64_t alignSequencesGPUExtendBand(const Request *requests, Response *responses, uint64_t numRequests, int device,
                                     int gapOpen, int gapExtend, int xdrop, int width);
uint64_t scoreSequencesGPUSeedsBand(const Request *requests, uint64_t numRequests, int device, int gapOpen, int gapExtend,
                                    int xdrop, int width, const uint64_t *seedTextPos, const uint64_t *seedPatternPos,
                                    const uint64_t *seedLength, int *scores);
uint64_t alignSequencesGPUSeedsBand(const Request *requests, Response *responses, uint64_t numRequests, int device,
                                    int gapOpen, int gapExtend, int xdrop, int width, const uint64_t *seedTextPos,
                                    const uint64_t *seedPatternPos, const uint64_t *seedLength);

/// Extension: chained seeds (sa_score_batch_chains, sa_align_pairs_chains; sa_hip.h has the definition). Request k
/// carries seedCount[k] >= 1 seeds, colinear and without overlap, in the order of the sequences; the seeds of all
/// requests lie one request after another in seedTextPos, seedPatternPos and seedLength, as the ...Seeds functions
/// carry one each. Between two consecutive seeds the rectangle they enclose is aligned globally, before the first
/// and after the last seed the sequences are extended under xdrop (-1, SA_NO_XDROP, never stops), and the seeds'
/// letters are scored as they are. The score is the sum of all pieces; Response::startInAlignedText and
/// startInAlignedPattern are the 0-based indices of the first aligned letters, and the aligned strings are the
/// pieces in forward order. Request::alignmentType and Request::gapPenalty are ignored; one alphabet and score
/// matrix for all requests. A chain that is empty, out of order or outside its request fails the whole call.
/// Returns 0, or 1 with the message on stdout.
uint64_t scoreSequencesGPUChains(const Request *requests, uint64_t numRequests, int device, int gapOpen, int gapExtend,
                                 int xdrop, const uint64_t *seedCount, const uint64_t *seedTextPos,
                                 const uint64_t *seedPatternPos, const uint64_t *seedLength, int *scores);
uint64_t alignSequencesGPUChains(const Request *requests, Response *responses, uint64_t numRequests, int device,
                                 int gapOpen, int gapExtend, int xdrop, const uint64_t *seedCount,
                                 const uint64_t *seedTextPos, const uint64_t *seedPatternPos, const uint64_t *seedLength);

/// Extension: CIGAR output (sa_align_pairs_cigar; sa_hip.h has the definition). `spec` (sa_hip.h sa_align_spec) names
/// the align...GPU... function the call stands for by that function's arguments: gap_open and gap_extend alone
/// alignSequencesGPUAffine, band >= 0 ...Banded, bands ...BandAt, extend with xdrop ...Extend, width >= 0 with it
/// ...ExtendBand, seeds (one per request) ...Seeds or ...SeedsBand, seeds with chain_off (numRequests + 1 offsets
/// into them) ...Chains. The mode is Request::alignmentType's, or with freeEnds 0..15 the ends-free mode of those
/// flags, and an extension's is global. Every request is aligned exactly as that function aligns it; instead of
/// two strings a CigarResponse gets the run-length ops of the alignment, BAM-packed (length << 4 | code; with
/// `eqx` = 7 and X 8, else M 0; I 1: the pattern has a letter the text lacks; D 2), and the column counts, which
/// are counted from the letters whatever `eqx` is. The strings stay on the device and are never copied.
/// Returns 0, or 1 with the message on stdout.
struct CigarResponse
{
    int score = 0;
    uint64_t numAlignmentBytes = 0, startInAlignedText = 0, startInAlignedPattern = 0;
    std::vector<uint32_t> ops;
    uint32_t matches = 0, mismatches = 0, textGapLetters = 0, patternGapLetters = 0, gapOpens = 0;
};
uint64_t alignSequencesGPUCigar(const Request *requests, CigarResponse *responses, uint64_t numRequests, int device,
                                const ::sa_align_spec &spec, bool eqx = true, int freeEnds = -1);

/// Extension: chaining (sa_chain_anchors; sa_hip.h has the definition). Pair k carries anchorCount[k] >= 0 anchors, a
/// seeder's unfiltered exact matches {anchorTextPos, anchorPatternPos, anchorLength}, length >= 1, in canonical order
/// (non-decreasing text end, pattern end, length); the anchors of all pairs lie one pair after another in the three
/// arrays, as the ...Chains functions carry their seeds. No sequences are taken: the letters are not looked at. Each
/// pair gets the best colinear chain without overlaps under `params` (sa_hip.h sa_chain_params): its score, the index
/// of the anchor it ends in, and its seeds in forward order, which are what the ...Chains functions take as the seeds
/// of a request (a pair without anchors has no seeds; leave it out of such a call). A pair out of order fails the
/// whole call. Returns 0, or 1 with the message on stdout.
struct ChainResponse
{
    int score = 0;
    uint32_t lastAnchor = 0;
    std::vector<uint64_t> seedTextPos, seedPatternPos, seedLength;
};
uint64_t chainAnchorsGPU(ChainResponse *responses, uint64_t numPairs, int device, const ::sa_chain_params &params,
                         const uint64_t *anchorCount, const uint64_t *anchorTextPos, const uint64_t *anchorPatternPos,
                         const uint64_t *anchorLength);

/// Host tracebacks over a full (m+1)x(n+1) byte DIRECTION matrix (used by the CPU device).
void traceBackNW(const char *, const uint64_t, const uint64_t, const Request &, Response *);
void traceBackSW(const char *, const uint64_t, const uint64_t, const uint64_t, const Request &, Response *);

}  // namespace SequenceAlignment

// Callers compiled with -DBENCHMARK get the reference's benchmark behaviour.
#ifdef BENCHMARK
#define alignSequenceGPU alignSequenceGPUFillMicros
#endif

// Free functions of the reference's utilities.cpp (global namespace there too).
char indexOfLetter(const char letter, const char *alphabet, const int alphabetSize);
int getScore(char char1, char char2, const char *alphabet, const int alphabetSize, const int *scoreMatrix);
int validateAndTransform(std::string &sequence, const char *alphabet, const int alphabetSize);
int readSequenceFile(const std::string fname, SequenceAlignment::Request *request);
int parseScoreMatrixFile(const std::string &fname, const int alphabetSize, int *buffer);
int parseArguments(int argc, const char *argv[], SequenceAlignment::Request *request);
void prettyAlignmentPrint(SequenceAlignment::Response &response, std::ostream &stream);

// CPU fill kernels exposed like the reference (tests/benchmarks.cu:153-154 calls them directly).
int fillMatrixNW(char *M, const uint64_t numRows, const uint64_t numCols, const SequenceAlignment::Request &request);
std::pair<int, uint64_t> fillMatrixSW(char *M, const uint64_t numRows, const uint64_t numCols,
                                      const SequenceAlignment::Request &request);
