// sa_fit_check — a C++14 caller of the three functions that take SEMI_GLOBAL (sa_hip.h: SA_FIT, the
// whole pattern inside the text, the text free at both ends): N DNA Requests of mixed sizes through
// scoreSequencesGPU (linear gap 5), scoreSequencesGPUAffine and alignSequencesGPUAffine (gap open 11,
// gap extend 2), each compared with the plain double loop and walk below. Texts are a few times
// longer than the patterns; half the patterns are a mutated piece of their text.
//   usage: sa_fit_check <max pattern length> <requests> [device]
// Prints the first difference, or "OK <requests>" as its last line; exit status 0 iff all equal.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "SequenceAlignment.hpp"

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
    uint64_t startText = 0;
    std::string text, pattern;
};

enum { LEFT = 0, DIAG = 1, TOP = 2, EEXT = 4, FEXT = 8 };

// Gotoh's recurrence row by row under the fit borders (row 0 is 0, column 0 is one gap run; E and F
// of the borders are minus infinity, a value no score reaches), the leftmost maximum of row m over
// columns 1..n, and the walk from there to row 0. go == ge is the linear recurrence.
Expected fitAlign(const SequenceAlignment::Request &r, int go, int ge)
{
    const int64_t n = (int64_t)r.textNumBytes, m = (int64_t)r.patternNumBytes, NEG = -(1ll << 40);
    const int64_t cols = n + 1;
    std::vector<int64_t> H((size_t)((m + 1) * cols), 0), E((size_t)((m + 1) * cols), NEG), F((size_t)((m + 1) * cols), NEG);
    std::vector<uint8_t> D((size_t)((m + 1) * cols), 0);
    for (int64_t i = 1; i <= m; ++i) H[i * cols] = -(go + (i - 1) * (int64_t)ge);
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
    Expected x;
    int64_t i = m, j = n ? 1 : 0;
    for (int64_t c = 2; c <= n; ++c)
        if (H[m * cols + c] > H[m * cols + j]) j = c;
    if (m == 0) j = 0;
    x.score = (int)H[m * cols + j];
    int state = DIAG;  // H; LEFT: inside a run of E, TOP: of F
    const char GAP = r.alphabet[r.alphabetSize];
    while (i > 0)
    {
        int d, nextState = DIAG;
        if (j == 0) d = TOP;
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
    return x;
}
}  // namespace

int main(int argc, const char *argv[])
{
    if (argc < 3)
    {
        std::cerr << "usage: sa_fit_check <max pattern length> <requests> [device]\n";
        return 2;
    }
    const uint64_t maxLen = std::max<uint64_t>(1, std::strtoull(argv[1], nullptr, 10)), count = std::strtoull(argv[2], nullptr, 10);
    const int device = argc > 3 ? std::atoi(argv[3]) : 0;
    const int gapLinear = 5, gapOpen = 11, gapExtend = 2;
    static const int blast[16] = {5, -4, -4, -4, -4, 5, -4, -4, -4, -4, 5, -4, -4, -4, -4, 5};
    std::vector<SequenceAlignment::Request> reqs(count);
    std::vector<SequenceAlignment::Response> resp(count);
    uint64_t seed = 13579;
    for (uint64_t i = 0; i < count; ++i)
    {
        SequenceAlignment::Request &r = reqs[i];
        r.deviceType = SequenceAlignment::programArgs::GPU;
        r.sequenceType = SequenceAlignment::programArgs::DNA;
        r.alignmentType = SequenceAlignment::programArgs::SEMI_GLOBAL;
        r.alphabet = SequenceAlignment::DNA_ALPHABET;
        r.alphabetSize = SequenceAlignment::NUM_DNA_CHARS;
        r.gapPenalty = gapLinear;  // ignored by the affine calls
        std::memcpy(r.scoreMatrix, blast, sizeof(blast));
        r.patternNumBytes = 1 + next(seed) % maxLen;
        r.textNumBytes = 1 + next(seed) % (4 * maxLen);
        r.textBytes = new char[r.textNumBytes];
        r.patternBytes = new char[r.patternNumBytes];
        for (uint64_t x = 0; x < r.textNumBytes; ++x) r.textBytes[x] = (char)(next(seed) % 4);
        // half the patterns are a piece of the text with substitutions and, now and then, a block of
        // letters left out, so long gaps pay; the others are random
        const bool related = (i & 1) == 0;
        uint64_t src = next(seed) % r.textNumBytes;
        for (uint64_t x = 0; x < r.patternNumBytes; ++x, ++src)
        {
            if (related && next(seed) % 64 == 0) src += next(seed) % 12;
            r.patternBytes[x] = related && src < r.textNumBytes && next(seed) % 8 ? r.textBytes[src] : (char)(next(seed) % 4);
        }
    }
    std::vector<int> linear(count), affine(count);
    if (SequenceAlignment::scoreSequencesGPU(reqs.data(), count, device, linear.data())) return 1;
    if (SequenceAlignment::scoreSequencesGPUAffine(reqs.data(), count, device, gapOpen, gapExtend, affine.data())) return 1;
    if (SequenceAlignment::alignSequencesGPUAffine(reqs.data(), resp.data(), count, device, gapOpen, gapExtend)) return 1;
    for (uint64_t i = 0; i < count; ++i)
    {
        const Expected lin = fitAlign(reqs[i], gapLinear, gapLinear), x = fitAlign(reqs[i], gapOpen, gapExtend);
        const SequenceAlignment::Response &g = resp[i];
        const char *field = nullptr;
        if (linear[i] != lin.score) field = "scoreSequencesGPU";
        else if (affine[i] != x.score) field = "scoreSequencesGPUAffine";
        else if (g.score != x.score) field = "score";
        else if (g.numAlignmentBytes != x.text.size()) field = "numAlignmentBytes";
        else if (g.startInAlignedText != x.startText) field = "startInAlignedText";
        else if (g.startInAlignedPattern != 0) field = "startInAlignedPattern";
        else if (std::memcmp(g.alignedTextBytes, x.text.data(), x.text.size()) != 0) field = "alignedTextBytes";
        else if (std::memcmp(g.alignedPatternBytes, x.pattern.data(), x.pattern.size()) != 0) field = "alignedPatternBytes";
        if (field)
        {
            std::cout << "request " << i << " (" << reqs[i].textNumBytes << "x" << reqs[i].patternNumBytes << "): " << field
                      << " differs: gpu scores " << linear[i] << " / " << affine[i] << " / " << g.score << " length "
                      << g.numAlignmentBytes << " start " << (int64_t)g.startInAlignedText << "/"
                      << (int64_t)g.startInAlignedPattern << ", cpu scores " << lin.score << " / " << x.score << " length "
                      << x.text.size() << " start " << (int64_t)x.startText << "\n";
            return 1;
        }
    }
    std::cout << "OK " << count << "\n";
    return 0;
}
