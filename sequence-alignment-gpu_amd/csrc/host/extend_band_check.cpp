// sa_extend_band_check — a C++14 caller of the banded extension functions (sa_hip.h sa_score_batch_extend_band):
// <count> DNA Requests of up to <n> letters a side, the pattern a mutated copy of the text for its first part
// and unrelated letters after it, through SequenceAlignment::scoreSequencesGPUExtendBand,
// alignSequencesGPUExtendBand, scoreSequencesGPUSeedsBand and alignSequencesGPUSeedsBand (gap open 11, gap
// extend 2) at the widths 5 and 64, at X-drop 20 and without a drop. The identities of sa_hip.h are checked:
//   W2  the end cell follows from the aligned strings, and alignSequencesGPUBandAt in global mode with the band
//       {-w, w} on text[:end_text], pattern[:end_pattern] gives the same score and the same two strings
//   W3  without a drop the score at width 5 is no larger than at width 64, which is no larger than
//       scoreSequencesGPUExtend's
//   W1  the width <n> gives every output of scoreSequencesGPUExtend, alignSequencesGPUExtend,
//       scoreSequencesGPUSeeds and alignSequencesGPUSeeds, the latter two under random seeds
//   S2  the seed {0, 0, 0} gives the scores of the banded extension at the same width
// The scorer's score must equal the aligner's and both starts of an extension must be 0.
//   usage: sa_extend_band_check <n> <count> [device]
// Prints the first difference, or "OK <count>" as its last line; exit status 0 iff all equal.
// With --expected: the digest of the requests, seeds and widths (check_ref.h) and nothing of either library.
#include "check_ref.h"

namespace
{
using SequenceAlignment::Request;
using SequenceAlignment::Response;

bool sameStrings(const Response &a, const Response &b)
{
    return a.score == b.score && a.numAlignmentBytes == b.numAlignmentBytes &&
           std::memcmp(a.alignedTextBytes, b.alignedTextBytes, a.numAlignmentBytes) == 0 &&
           std::memcmp(a.alignedPatternBytes, b.alignedPatternBytes, a.numAlignmentBytes) == 0;
}

int differs(uint64_t i, const char *what, int width, int xdrop)
{
    std::cout << "request " << i << " at width " << width << ", xdrop " << xdrop << ": " << what << " differs\n";
    return 1;
}
}  // namespace

int main(int argc, char **argv)
{
    const bool expectedOnly = check::takeExpected(argc, argv);
    if (argc < 3)
    {
        std::cout << "usage: sa_extend_band_check <n> <count> [device]\n";
        return 2;
    }
    const uint64_t maxLen = std::max<uint64_t>(1, std::strtoull(argv[1], nullptr, 10));
    const uint64_t count = std::strtoull(argv[2], nullptr, 10);
    const int device = argc > 3 ? std::atoi(argv[3]) : 0;
    const int gapOpen = 11, gapExtend = 2;
    std::vector<Request> reqs(count);
    std::vector<uint64_t> seedT(count), seedP(count), seedL(count), zero(count, 0);
    uint64_t seed = 86421;
    for (uint64_t i = 0; i < count; ++i)
    {
        Request &r = reqs[i];
        check::scheme(r);
        r.textNumBytes = 1 + check::next(seed) % maxLen;
        r.patternNumBytes = 1 + check::next(seed) % maxLen;
        check::randomText(r, seed);
        // the pattern: the text with substitutions and a few letters left out up to letter `related`,
        // unrelated letters from there on
        const uint64_t related = check::next(seed) % (r.patternNumBytes + 1);
        check::relatedPattern(r, seed, 0, related, true, 4);
        seedT[i] = check::next(seed) % (r.textNumBytes + 1);
        seedP[i] = check::next(seed) % (r.patternNumBytes + 1);
        seedL[i] = check::next(seed) % (std::min(r.textNumBytes - seedT[i], r.patternNumBytes - seedP[i]) + 1);
    }
    const int xdrops[2] = {20, SA_NO_XDROP};
    const int widths[2] = {5, 64};
    const int wide = (int)std::min<uint64_t>(maxLen, 1u << 30);  // W1: a width that admits every cell
    if (expectedOnly)
    {
        check::Digest sent;
        sent.requests(reqs);
        sent.numbers(seedT), sent.numbers(seedP), sent.numbers(seedL);
        for (int xdrop : xdrops) sent.number(xdrop);
        for (int width : widths) sent.number(width);
        sent.number(wide);
        return check::printExpected("sa_extend_band_check", argc, argv, sent, nullptr);
    }
    for (int xdrop : xdrops)
    {
        std::vector<int> full(count), narrower(count, 0);
        if (SequenceAlignment::scoreSequencesGPUExtend(reqs.data(), count, device, gapOpen, gapExtend, xdrop, full.data())) return 1;
        for (int width : widths)
        {
            std::vector<Response> resp(count), respPrefix(count);
            std::vector<int> scores(count), seeded(count);
            if (SequenceAlignment::scoreSequencesGPUExtendBand(reqs.data(), count, device, gapOpen, gapExtend, xdrop, width, scores.data())) return 1;
            if (SequenceAlignment::alignSequencesGPUExtendBand(reqs.data(), resp.data(), count, device, gapOpen, gapExtend, xdrop, width)) return 1;
            if (SequenceAlignment::scoreSequencesGPUSeedsBand(reqs.data(), count, device, gapOpen, gapExtend, xdrop, width, zero.data(), zero.data(),
                                                              zero.data(), seeded.data()))
                return 1;
            // W2: the prefixes the extensions cover, as global requests inside {-w, w}
            std::vector<Request> pre(count);
            std::vector<int> lo(count, -width), hi(count, width);
            for (uint64_t i = 0; i < count; ++i)
            {
                uint64_t endText, endPattern;
                check::countLetters(resp[i], reqs[i].alphabet[reqs[i].alphabetSize], endText, endPattern);
                if (endText > reqs[i].textNumBytes || endPattern > reqs[i].patternNumBytes) return differs(i, "the letters of the strings", width, xdrop);
                const int64_t off = (int64_t)endText - (int64_t)endPattern;
                if (off < -width || off > width) return differs(i, "the end cell's diagonal (out of band)", width, xdrop);
                check::slice(pre[i], reqs[i], 0, endText, 0, endPattern, false);
            }
            if (SequenceAlignment::alignSequencesGPUBandAt(pre.data(), respPrefix.data(), count, device, gapOpen, gapExtend, 0, lo.data(), hi.data()))
                return 1;
            for (uint64_t i = 0; i < count; ++i)
            {
                const Response &g = resp[i];
                if (scores[i] != g.score) return differs(i, "the scorer against the aligner", width, xdrop);
                if (seeded[i] != g.score) return differs(i, "the seed {0, 0, 0} against the extension (S2)", width, xdrop);
                if (g.score < 0) return differs(i, "the sign of the score", width, xdrop);
                if (g.startInAlignedText != 0 || g.startInAlignedPattern != 0) return differs(i, "a start", width, xdrop);
                if (!sameStrings(g, respPrefix[i])) return differs(i, "the band-at global alignment of the prefixes (W2)", width, xdrop);
                if (xdrop == SA_NO_XDROP && (g.score < narrower[i] || g.score > full[i])) return differs(i, "the order of the widths' scores (W3)", width, xdrop);
                narrower[i] = g.score;
            }
        }
        // W1
        std::vector<Response> a(count), b(count), c(count), d(count);
        std::vector<int> s1(count), s2(count), s3(count);
        if (SequenceAlignment::scoreSequencesGPUExtendBand(reqs.data(), count, device, gapOpen, gapExtend, xdrop, wide, s1.data())) return 1;
        if (SequenceAlignment::alignSequencesGPUExtend(reqs.data(), a.data(), count, device, gapOpen, gapExtend, xdrop)) return 1;
        if (SequenceAlignment::alignSequencesGPUExtendBand(reqs.data(), b.data(), count, device, gapOpen, gapExtend, xdrop, wide)) return 1;
        if (SequenceAlignment::scoreSequencesGPUSeeds(reqs.data(), count, device, gapOpen, gapExtend, xdrop, seedT.data(), seedP.data(), seedL.data(),
                                                      s2.data()))
            return 1;
        if (SequenceAlignment::scoreSequencesGPUSeedsBand(reqs.data(), count, device, gapOpen, gapExtend, xdrop, wide, seedT.data(), seedP.data(),
                                                          seedL.data(), s3.data()))
            return 1;
        if (SequenceAlignment::alignSequencesGPUSeeds(reqs.data(), c.data(), count, device, gapOpen, gapExtend, xdrop, seedT.data(), seedP.data(),
                                                      seedL.data()))
            return 1;
        if (SequenceAlignment::alignSequencesGPUSeedsBand(reqs.data(), d.data(), count, device, gapOpen, gapExtend, xdrop, wide, seedT.data(),
                                                          seedP.data(), seedL.data()))
            return 1;
        for (uint64_t i = 0; i < count; ++i)
        {
            if (s1[i] != full[i]) return differs(i, "the scorer against scoreSequencesGPUExtend (W1)", wide, xdrop);
            if (!sameStrings(a[i], b[i])) return differs(i, "the aligner against alignSequencesGPUExtend (W1)", wide, xdrop);
            if (s2[i] != s3[i]) return differs(i, "the seeds scorer against scoreSequencesGPUSeeds (W1)", wide, xdrop);
            if (!sameStrings(c[i], d[i]) || c[i].startInAlignedText != d[i].startInAlignedText ||
                c[i].startInAlignedPattern != d[i].startInAlignedPattern)
                return differs(i, "the seeds aligner against alignSequencesGPUSeeds (W1)", wide, xdrop);
            if (s3[i] != d[i].score) return differs(i, "the seeds scorer against the seeds aligner", wide, xdrop);
        }
    }
    std::cout << "OK " << count << "\n";
    return 0;
}
