// sa_extend_check — a C++14 caller of the extension-alignment functions (sa_hip.h sa_score_batch_extend):
// <count> DNA Requests of up to <n> letters a side, the pattern a mutated copy of the text for its first
// part and unrelated letters after it, through SequenceAlignment::scoreSequencesGPUExtend and
// alignSequencesGPUExtend (gap open 11, gap extend 2) at X-drop 20 and without a drop. Identity I1 of
// sa_hip.h is checked: the end cell follows from the aligned strings (their letters without the gap
// letter), and alignSequencesGPUAffine in global mode on text[:end_text], pattern[:end_pattern] must give
// the same score and the same two strings. The scorer's score must equal the aligner's, both starts must
// be 0, and the score without a drop must be no smaller than the score at X-drop 20.
//   usage: sa_extend_check <n> <count> [device]
// Prints the first difference, or "OK <count>" as its last line; exit status 0 iff all equal.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <vector>

#include "SequenceAlignment.hpp"
#include "sa_hip.h"

namespace
{
uint64_t next(uint64_t &s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return s >> 33;
}

void scheme(SequenceAlignment::Request &r)
{
    static const int blast[16] = {5, -4, -4, -4, -4, 5, -4, -4, -4, -4, 5, -4, -4, -4, -4, 5};
    r.deviceType = SequenceAlignment::programArgs::GPU;
    r.sequenceType = SequenceAlignment::programArgs::DNA;
    r.alignmentType = SequenceAlignment::programArgs::GLOBAL;
    r.alphabet = SequenceAlignment::DNA_ALPHABET;
    r.alphabetSize = SequenceAlignment::NUM_DNA_CHARS;
    r.gapPenalty = 5;  // ignored by the affine and the extend calls
    std::memcpy(r.scoreMatrix, blast, sizeof(blast));
}
}  // namespace

int main(int argc, char **argv)
{
    if (argc < 3)
    {
        std::cout << "usage: sa_extend_check <n> <count> [device]\n";
        return 2;
    }
    const uint64_t maxLen = std::max<uint64_t>(1, std::strtoull(argv[1], nullptr, 10));
    const uint64_t count = std::strtoull(argv[2], nullptr, 10);
    const int device = argc > 3 ? std::atoi(argv[3]) : 0;
    const int gapOpen = 11, gapExtend = 2;
    std::vector<SequenceAlignment::Request> reqs(count);
    uint64_t seed = 97531;
    for (uint64_t i = 0; i < count; ++i)
    {
        SequenceAlignment::Request &r = reqs[i];
        scheme(r);
        r.textNumBytes = 1 + next(seed) % maxLen;
        r.patternNumBytes = 1 + next(seed) % maxLen;
        r.textBytes = new char[r.textNumBytes];
        r.patternBytes = new char[r.patternNumBytes];
        for (uint64_t x = 0; x < r.textNumBytes; ++x) r.textBytes[x] = (char)(next(seed) % 4);
        // the pattern: the text with substitutions and a few letters left out up to letter `related`,
        // unrelated letters from there on
        const uint64_t related = next(seed) % (r.patternNumBytes + 1);
        uint64_t src = 0;
        for (uint64_t x = 0; x < r.patternNumBytes; ++x, ++src)
        {
            if (next(seed) % 64 == 0) src += next(seed) % 4;
            r.patternBytes[x] = x < related && src < r.textNumBytes && next(seed) % 8 ? r.textBytes[src] : (char)(next(seed) % 4);
        }
    }
    std::vector<int> previous(count, 0);
    const int xdrops[2] = {20, SA_NO_XDROP};
    for (int xdrop : xdrops)
    {
        std::vector<SequenceAlignment::Response> resp(count), respPrefix(count);
        std::vector<int> scores(count);
        if (SequenceAlignment::scoreSequencesGPUExtend(reqs.data(), count, device, gapOpen, gapExtend, xdrop, scores.data())) return 1;
        if (SequenceAlignment::alignSequencesGPUExtend(reqs.data(), resp.data(), count, device, gapOpen, gapExtend, xdrop)) return 1;
        // the prefixes the extensions cover, as global requests
        std::vector<SequenceAlignment::Request> pre(count);
        for (uint64_t i = 0; i < count; ++i)
        {
            const char gapLetter = reqs[i].alphabet[reqs[i].alphabetSize];
            uint64_t endText = 0, endPattern = 0;
            for (uint64_t x = 0; x < resp[i].numAlignmentBytes; ++x)
            {
                endText += resp[i].alignedTextBytes[x] != gapLetter;
                endPattern += resp[i].alignedPatternBytes[x] != gapLetter;
            }
            if (endText > reqs[i].textNumBytes || endPattern > reqs[i].patternNumBytes)
            {
                std::cout << "request " << i << " at xdrop " << xdrop << ": the strings hold more letters than the sequences\n";
                return 1;
            }
            scheme(pre[i]);
            pre[i].textNumBytes = endText;
            pre[i].patternNumBytes = endPattern;
            pre[i].textBytes = new char[std::max<uint64_t>(endText, 1)];
            pre[i].patternBytes = new char[std::max<uint64_t>(endPattern, 1)];
            std::memcpy(pre[i].textBytes, reqs[i].textBytes, endText);
            std::memcpy(pre[i].patternBytes, reqs[i].patternBytes, endPattern);
        }
        if (SequenceAlignment::alignSequencesGPUAffine(pre.data(), respPrefix.data(), count, device, gapOpen, gapExtend)) return 1;
        for (uint64_t i = 0; i < count; ++i)
        {
            const SequenceAlignment::Response &g = resp[i], &a = respPrefix[i];
            const char *field = nullptr;
            if (scores[i] != g.score) field = "scoreSequencesGPUExtend against alignSequencesGPUExtend";
            else if (g.score < 0) field = "a negative score";
            else if (g.startInAlignedText != 0 || g.startInAlignedPattern != 0) field = "a start";
            else if (g.score != a.score) field = "score against the global alignment of the prefixes";
            else if (g.numAlignmentBytes != a.numAlignmentBytes) field = "numAlignmentBytes";
            else if (std::memcmp(g.alignedTextBytes, a.alignedTextBytes, g.numAlignmentBytes) != 0) field = "alignedTextBytes";
            else if (std::memcmp(g.alignedPatternBytes, a.alignedPatternBytes, g.numAlignmentBytes) != 0) field = "alignedPatternBytes";
            else if (xdrop == SA_NO_XDROP && g.score < previous[i]) field = "the score without a drop against the score at xdrop 20";
            if (field)
            {
                std::cout << "request " << i << " (" << reqs[i].textNumBytes << "x" << reqs[i].patternNumBytes << ") at xdrop " << xdrop
                          << ": " << field << " differs: extend score " << g.score << " (scorer " << scores[i] << ") length "
                          << g.numAlignmentBytes << ", prefixes " << pre[i].textNumBytes << "x" << pre[i].patternNumBytes << " score "
                          << a.score << " length " << a.numAlignmentBytes << "\n";
                return 1;
            }
            previous[i] = g.score;
        }
    }
    std::cout << "OK " << count << "\n";
    return 0;
}
