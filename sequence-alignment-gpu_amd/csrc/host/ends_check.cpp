// sa_ends_check — a C++14 caller of scoreSequencesGPUEndsFree and alignSequencesGPUEndsFree (sa_hip.h:
// SA_ENDS_FREE, global alignment with free sequence ends): N DNA Requests of mixed sizes, request i
// under the flag set i % 16, so every call takes the requests of one flag set. Scores under the linear
// gap 5 (passed as gap open and gap extend) and under gap open 11 / gap extend 2, alignments under
// 11 / 2, each compared with the plain double loop, result pick and walk below. In half the requests
// the end of the text is a mutated copy of the start of the pattern: two reads that overlap.
//   usage: sa_ends_check <max length> <requests> [device]
// Prints the first difference, or "OK <requests>" as its last line; exit status 0 iff all equal.
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
uint64_t next(uint64_t &s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return s >> 33;
}

struct Expected
{
    int score = 0;
    uint64_t startText = 0, startPattern = 0;
    std::string text, pattern;
};

enum { LEFT = 0, DIAG = 1, TOP = 2, EEXT = 4, FEXT = 8 };

// Gotoh's recurrence row by row under the ends-free borders (row 0 is 0 under TB, column 0 under PB,
// one gap run otherwise; E and F of the borders are minus infinity, a value no score reaches), the
// result cell by the tie order of sa_hip.h, and the walk from there. go == ge is the linear recurrence.
Expected endsAlign(const SequenceAlignment::Request &r, int go, int ge, int flags)
{
    const bool TB = flags & SA_FREE_TEXT_BEGIN, TE = flags & SA_FREE_TEXT_END, PB = flags & SA_FREE_PATTERN_BEGIN,
               PE = flags & SA_FREE_PATTERN_END;
    const int64_t n = (int64_t)r.textNumBytes, m = (int64_t)r.patternNumBytes, NEG = -(1ll << 40);
    const int64_t cols = n + 1;
    std::vector<int64_t> H((size_t)((m + 1) * cols), 0), E((size_t)((m + 1) * cols), NEG), F((size_t)((m + 1) * cols), NEG);
    std::vector<uint8_t> D((size_t)((m + 1) * cols), 0);
    for (int64_t j = 1; j <= n; ++j) H[j] = TB ? 0 : -(go + (j - 1) * (int64_t)ge);
    for (int64_t i = 1; i <= m; ++i) H[i * cols] = PB ? 0 : -(go + (i - 1) * (int64_t)ge);
    for (int64_t i = 1; i <= m; ++i)
        for (int64_t j = 1; j <= n; ++j)
        {
            const int64_t c = i * cols + j;
            const int64_t eExt = E[c - 1] - ge, eOpen = H[c - 1] - go, fExt = F[c - cols] - ge, fOpen = H[c - cols] - go;
            E[c] = std::max(eExt, eOpen);
            F[c] = std::max(fExt, fOpen);
            const int64_t diag = H[c - cols - 1] + r.scoreMatrix[r.patternBytes[i - 1] * r.alphabetSize + r.textBytes[j - 1]];
            H[c] = std::max(diag, std::max(E[c], F[c]));
            uint8_t d = diag > std::max(E[c], F[c]) ? DIAG : E[c] >= F[c] ? LEFT : TOP;
            if (eExt > eOpen) d |= EEXT;
            if (fExt > fOpen) d |= FEXT;
            D[c] = d;
        }
    // the candidates in row-major order, interior and border apart; strictly greater keeps the first
    bool haveIn = false, haveBo = false;
    int64_t inV = 0, inI = 0, inJ = 0, boV = 0, boI = 0, boJ = 0;
    for (int64_t i = 0; i <= m; ++i)
        for (int64_t j = 0; j <= n; ++j)
        {
            if (!((i == m && j == n) || (TE && i == m) || (PE && j == n))) continue;
            const int64_t v = H[i * cols + j];
            if (i >= 1 && j >= 1)
            {
                if (!haveIn || v > inV) inV = v, inI = i, inJ = j;
                haveIn = true;
            }
            else
            {
                if (!haveBo || v > boV) boV = v, boI = i, boJ = j;
                haveBo = true;
            }
        }
    const bool interior = haveIn && (!haveBo || inV >= boV);
    int64_t i = interior ? inI : boI, j = interior ? inJ : boJ;
    Expected x;
    x.score = (int)H[i * cols + j];
    int state = DIAG;  // H; LEFT: inside a run of E, TOP: of F
    const char GAP = r.alphabet[r.alphabetSize];
    while (!((i == 0 && (TB || j == 0)) || (j == 0 && (PB || i == 0))))
    {
        int d, nextState = DIAG;
        if (j == 0) d = TOP;
        else if (i == 0) d = LEFT;
        else
        {
            const uint8_t nib = D[i * cols + j];
            d = state == DIAG ? (nib & 3) : state;
            if (d == LEFT) nextState = nib & EEXT ? LEFT : DIAG;
            if (d == TOP) nextState = nib & FEXT ? TOP : DIAG;
        }
        const int tt = d == DIAG || d == LEFT, tp = d == DIAG || d == TOP;
        x.text.push_back(tt ? r.alphabet[(int)r.textBytes[j - 1]] : GAP);
        x.pattern.push_back(tp ? r.alphabet[(int)r.patternBytes[i - 1]] : GAP);
        j -= tt;
        i -= tp;
        state = nextState;
    }
    std::reverse(x.text.begin(), x.text.end());
    std::reverse(x.pattern.begin(), x.pattern.end());
    x.startText = (uint64_t)j;
    x.startPattern = (uint64_t)i;
    return x;
}
}  // namespace

int main(int argc, const char *argv[])
{
    if (argc < 3)
    {
        std::cerr << "usage: sa_ends_check <max length> <requests> [device]\n";
        return 2;
    }
    const uint64_t maxLen = std::max<uint64_t>(1, std::strtoull(argv[1], nullptr, 10)), count = std::strtoull(argv[2], nullptr, 10);
    const int device = argc > 3 ? std::atoi(argv[3]) : 0;
    const int gapLinear = 5, gapOpen = 11, gapExtend = 2;
    static const int blast[16] = {5, -4, -4, -4, -4, 5, -4, -4, -4, -4, 5, -4, -4, -4, -4, 5};
    std::vector<SequenceAlignment::Request> reqs(count);
    uint64_t seed = 24680;
    for (uint64_t i = 0; i < count; ++i)
    {
        SequenceAlignment::Request &r = reqs[i];
        r.deviceType = SequenceAlignment::programArgs::GPU;
        r.sequenceType = SequenceAlignment::programArgs::DNA;
        r.alignmentType = SequenceAlignment::programArgs::LOCAL;  // ignored by the ends-free functions
        r.alphabet = SequenceAlignment::DNA_ALPHABET;
        r.alphabetSize = SequenceAlignment::NUM_DNA_CHARS;
        r.gapPenalty = gapLinear;  // ignored too: the gap is an argument of the call
        std::memcpy(r.scoreMatrix, blast, sizeof(blast));
        r.patternNumBytes = 1 + next(seed) % maxLen;
        r.textNumBytes = 1 + next(seed) % maxLen;
        r.textBytes = new char[r.textNumBytes];
        r.patternBytes = new char[r.patternNumBytes];
        for (uint64_t x = 0; x < r.textNumBytes; ++x) r.textBytes[x] = (char)(next(seed) % 4);
        for (uint64_t x = 0; x < r.patternNumBytes; ++x) r.patternBytes[x] = (char)(next(seed) % 4);
        // two overlapping reads: the last `over` letters of the text are the first letters of the
        // pattern with substitutions and, now and then, a letter left out
        if (((i / 16) & 1) == 0)
        {
            const uint64_t over = 1 + next(seed) % std::min(r.textNumBytes, r.patternNumBytes);
            uint64_t src = 0;
            for (uint64_t x = r.textNumBytes - over; x < r.textNumBytes && src < r.patternNumBytes; ++x, ++src)
            {
                if (next(seed) % 48 == 0) ++src;
                if (src < r.patternNumBytes && next(seed) % 10) r.textBytes[x] = r.patternBytes[src];
            }
        }
    }
    for (int flags = 0; flags < 16; ++flags)
    {
        std::vector<uint64_t> ids;
        for (uint64_t i = (uint64_t)flags; i < count; i += 16) ids.push_back(i);
        if (ids.empty()) continue;
        std::vector<SequenceAlignment::Request> sub(ids.size());
        for (size_t q = 0; q < ids.size(); ++q) sub[q] = reqs[ids[q]];
        std::vector<SequenceAlignment::Response> resp(ids.size());
        std::vector<int> linear(ids.size()), affine(ids.size());
        bool failed = SequenceAlignment::scoreSequencesGPUEndsFree(sub.data(), sub.size(), device, gapLinear, gapLinear, flags, linear.data()) ||
                      SequenceAlignment::scoreSequencesGPUEndsFree(sub.data(), sub.size(), device, gapOpen, gapExtend, flags, affine.data()) ||
                      SequenceAlignment::alignSequencesGPUEndsFree(sub.data(), resp.data(), sub.size(), device, gapOpen, gapExtend, flags);
        for (size_t q = 0; q < ids.size() && !failed; ++q)
        {
            const SequenceAlignment::Request &rq = sub[q];
            const Expected lin = endsAlign(rq, gapLinear, gapLinear, flags), x = endsAlign(rq, gapOpen, gapExtend, flags);
            const SequenceAlignment::Response &g = resp[q];
            const char *field = nullptr;
            if (linear[q] != lin.score) field = "scoreSequencesGPUEndsFree (linear)";
            else if (affine[q] != x.score) field = "scoreSequencesGPUEndsFree";
            else if (g.score != x.score) field = "score";
            else if (g.numAlignmentBytes != x.text.size()) field = "numAlignmentBytes";
            else if (g.startInAlignedText != x.startText) field = "startInAlignedText";
            else if (g.startInAlignedPattern != x.startPattern) field = "startInAlignedPattern";
            else if (std::memcmp(g.alignedTextBytes, x.text.data(), x.text.size()) != 0) field = "alignedTextBytes";
            else if (std::memcmp(g.alignedPatternBytes, x.pattern.data(), x.pattern.size()) != 0) field = "alignedPatternBytes";
            if (field)
            {
                std::cout << "request " << ids[q] << " (" << rq.textNumBytes << "x" << rq.patternNumBytes << ", flags " << flags
                          << "): " << field << " differs: gpu scores " << linear[q] << " / " << affine[q] << " / " << g.score
                          << " length " << g.numAlignmentBytes << " start " << (int64_t)g.startInAlignedText << "/"
                          << (int64_t)g.startInAlignedPattern << ", cpu scores " << lin.score << " / " << x.score << " length "
                          << x.text.size() << " start " << (int64_t)x.startText << "/" << (int64_t)x.startPattern << "\n";
                failed = true;
            }
        }
        // the copies in `sub` share the originals' sequences: they must not release them
        for (SequenceAlignment::Request &rq : sub) rq.textBytes = rq.patternBytes = nullptr;
        if (failed) return 1;
    }
    std::cout << "OK " << count << "\n";
    return 0;
}
