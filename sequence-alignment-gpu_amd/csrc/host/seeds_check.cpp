// sa_seeds_check — a C++14 caller of the seed-extension functions (sa_hip.h sa_score_batch_seeds): <count>
// DNA Requests of up to <n> letters a side, each with a seed of random place and length around which the
// pattern is a mutated copy of the text and unrelated further out, through
// SequenceAlignment::scoreSequencesGPUSeeds and alignSequencesGPUSeeds (gap open 11, gap extend 2) at X-drop
// 20 and without a drop. Identity S1 of sa_hip.h is checked against the library's own extension functions:
// alignSequencesGPUExtend on the two halves, the left one reversed here on the host, must give the score
// (with the seed's substitution scores added), the two starts and, joined around the seed's letters, both
// strings. The scorer's score must equal the aligner's.
//   usage: sa_seeds_check <n> <count> [device]
// Prints the first difference, or "OK <count>" as its last line; exit status 0 iff all equal.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "SequenceAlignment.hpp"
#include "sa_hip.h"

namespace
{
const int blast[16] = {5, -4, -4, -4, -4, 5, -4, -4, -4, -4, 5, -4, -4, -4, -4, 5};

uint64_t next(uint64_t &s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return s >> 33;
}

void scheme(SequenceAlignment::Request &r)
{
    r.deviceType = SequenceAlignment::programArgs::GPU;
    r.sequenceType = SequenceAlignment::programArgs::DNA;
    r.alignmentType = SequenceAlignment::programArgs::GLOBAL;
    r.alphabet = SequenceAlignment::DNA_ALPHABET;
    r.alphabetSize = SequenceAlignment::NUM_DNA_CHARS;
    r.gapPenalty = 5;  // ignored by the extend and the seeds calls
    std::memcpy(r.scoreMatrix, blast, sizeof(blast));
}

// a request over letters [from, from + len) of `src`, forwards, or backwards from letter from + len - 1
void slice(SequenceAlignment::Request &r, const SequenceAlignment::Request &src, uint64_t tFrom, uint64_t tLen, uint64_t pFrom,
           uint64_t pLen, bool reversed)
{
    scheme(r);
    r.textNumBytes = tLen;
    r.patternNumBytes = pLen;
    r.textBytes = new char[std::max<uint64_t>(tLen, 1)];
    r.patternBytes = new char[std::max<uint64_t>(pLen, 1)];
    for (uint64_t x = 0; x < tLen; ++x) r.textBytes[x] = src.textBytes[reversed ? tFrom + tLen - 1 - x : tFrom + x];
    for (uint64_t x = 0; x < pLen; ++x) r.patternBytes[x] = src.patternBytes[reversed ? pFrom + pLen - 1 - x : pFrom + x];
}
}  // namespace

int main(int argc, char **argv)
{
    if (argc < 3)
    {
        std::cout << "usage: sa_seeds_check <n> <count> [device]\n";
        return 2;
    }
    const uint64_t maxLen = std::max<uint64_t>(1, std::strtoull(argv[1], nullptr, 10));
    const uint64_t count = std::strtoull(argv[2], nullptr, 10);
    const int device = argc > 3 ? std::atoi(argv[3]) : 0;
    const int gapOpen = 11, gapExtend = 2;
    std::vector<SequenceAlignment::Request> reqs(count), left(count), right(count);
    std::vector<uint64_t> ts(count), ps(count), len(count);
    uint64_t seed = 86420;
    for (uint64_t i = 0; i < count; ++i)
    {
        SequenceAlignment::Request &r = reqs[i];
        scheme(r);
        r.textNumBytes = 1 + next(seed) % maxLen;
        r.patternNumBytes = 1 + next(seed) % maxLen;
        ts[i] = next(seed) % (r.textNumBytes + 1);
        ps[i] = next(seed) % (r.patternNumBytes + 1);
        const uint64_t room = std::min(r.textNumBytes - ts[i], r.patternNumBytes - ps[i]);
        len[i] = i % 5 == 0 ? 0 : next(seed) % (std::min<uint64_t>(room, 40) + 1);
        r.textBytes = new char[r.textNumBytes];
        r.patternBytes = new char[r.patternNumBytes];
        for (uint64_t x = 0; x < r.textNumBytes; ++x) r.textBytes[x] = (char)(next(seed) % 4);
        // the pattern: the text on the seed's diagonal with substitutions within `related` letters of the
        // seed, unrelated letters further out
        const uint64_t related = next(seed) % (maxLen + 1);
        for (uint64_t x = 0; x < r.patternNumBytes; ++x)
        {
            const int64_t src = (int64_t)x - (int64_t)ps[i] + (int64_t)ts[i];
            const uint64_t away = x < ps[i] ? ps[i] - x : x - ps[i];
            const bool copy = away < related + len[i] && src >= 0 && src < (int64_t)r.textNumBytes && next(seed) % 8;
            r.patternBytes[x] = copy ? r.textBytes[src] : (char)(next(seed) % 4);
        }
        slice(left[i], r, 0, ts[i], 0, ps[i], true);
        slice(right[i], r, ts[i] + len[i], r.textNumBytes - ts[i] - len[i], ps[i] + len[i], r.patternNumBytes - ps[i] - len[i], false);
    }
    const int xdrops[2] = {20, SA_NO_XDROP};
    for (int xdrop : xdrops)
    {
        std::vector<SequenceAlignment::Response> resp(count), respLeft(count), respRight(count);
        std::vector<int> scores(count);
        if (SequenceAlignment::scoreSequencesGPUSeeds(reqs.data(), count, device, gapOpen, gapExtend, xdrop, ts.data(), ps.data(), len.data(),
                                                      scores.data()))
            return 1;
        if (SequenceAlignment::alignSequencesGPUSeeds(reqs.data(), resp.data(), count, device, gapOpen, gapExtend, xdrop, ts.data(), ps.data(),
                                                      len.data()))
            return 1;
        if (SequenceAlignment::alignSequencesGPUExtend(left.data(), respLeft.data(), count, device, gapOpen, gapExtend, xdrop)) return 1;
        if (SequenceAlignment::alignSequencesGPUExtend(right.data(), respRight.data(), count, device, gapOpen, gapExtend, xdrop)) return 1;
        for (uint64_t i = 0; i < count; ++i)
        {
            const SequenceAlignment::Response &g = resp[i], &l = respLeft[i], &r = respRight[i];
            const char gapLetter = reqs[i].alphabet[reqs[i].alphabetSize];
            int mid = 0;
            std::string wantText, wantPattern;
            uint64_t leftText = 0, leftPattern = 0;
            for (uint64_t x = l.numAlignmentBytes; x-- > 0;)
            {
                wantText += l.alignedTextBytes[x];
                wantPattern += l.alignedPatternBytes[x];
                leftText += l.alignedTextBytes[x] != gapLetter;
                leftPattern += l.alignedPatternBytes[x] != gapLetter;
            }
            for (uint64_t q = 0; q < len[i]; ++q)
            {
                const int ct = reqs[i].textBytes[ts[i] + q], cp = reqs[i].patternBytes[ps[i] + q];
                mid += blast[cp * 4 + ct];
                wantText += reqs[i].alphabet[ct];
                wantPattern += reqs[i].alphabet[cp];
            }
            wantText.append(r.alignedTextBytes, r.numAlignmentBytes);
            wantPattern.append(r.alignedPatternBytes, r.numAlignmentBytes);
            const char *field = nullptr;
            if (scores[i] != g.score) field = "scoreSequencesGPUSeeds against alignSequencesGPUSeeds";
            else if (g.score != l.score + mid + r.score) field = "score against the two extensions and the seed";
            else if (g.startInAlignedText != ts[i] - leftText || g.startInAlignedPattern != ps[i] - leftPattern) field = "a start";
            else if (g.numAlignmentBytes != wantText.size()) field = "numAlignmentBytes";
            else if (std::memcmp(g.alignedTextBytes, wantText.data(), wantText.size()) != 0) field = "alignedTextBytes";
            else if (std::memcmp(g.alignedPatternBytes, wantPattern.data(), wantPattern.size()) != 0) field = "alignedPatternBytes";
            if (field)
            {
                std::cout << "request " << i << " (" << reqs[i].textNumBytes << "x" << reqs[i].patternNumBytes << ", seed " << ts[i] << ":"
                          << ps[i] << ":" << len[i] << ") at xdrop " << xdrop << ": " << field << " differs: seeds score " << g.score
                          << " (scorer " << scores[i] << ") length " << g.numAlignmentBytes << ", left " << l.score << " seed " << mid
                          << " right " << r.score << " length " << wantText.size() << "\n";
                return 1;
            }
        }
    }
    std::cout << "OK " << count << "\n";
    return 0;
}
