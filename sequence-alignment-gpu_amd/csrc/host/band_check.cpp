// sa_band_check — a C++14 caller of the banded extension (sa_hip.h: cell (i, j) is in band iff
// min(0, n - m) - w <= j - i <= max(0, n - m) + w): N DNA Requests of mixed sizes through
// SequenceAlignment::scoreSequencesGPUBanded and alignSequencesGPUBanded (gap open 11, gap extend 2,
// half-width 24) and, one by one, through the plain banded Gotoh fill and three-state walk below
// (DESIGN.md §3.5); the score and every Response field are compared. A last call with a half-width
// above every length must equal scoreSequencesGPUAffine.
//   usage: sa_band_check global|local <max length> <requests> [device]
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
    uint64_t startText = 0, startPattern = 0;
    std::string text, pattern;
};

enum { LEFT = 0, DIAG = 1, TOP = 2, STOP = 3, EEXT = 4, FEXT = 8 };

// Gotoh's recurrence row by row over the in-band cells with the direction nibble of each (H, E and F
// of every out-of-band cell and E and F of the borders are minus infinity, a value no score
// reaches), then the walk from the scored cell
Expected bandAlign(const SequenceAlignment::Request &r, bool local, int go, int ge, int64_t w)
{
    const int64_t n = (int64_t)r.textNumBytes, m = (int64_t)r.patternNumBytes, NEG = -(1ll << 40);
    const int64_t cols = n + 1, lo = std::min<int64_t>(0, n - m) - w, hi = std::max<int64_t>(0, n - m) + w;
    std::vector<int64_t> H((size_t)((m + 1) * cols), NEG), E((size_t)((m + 1) * cols), NEG), F((size_t)((m + 1) * cols), NEG);
    std::vector<uint8_t> D((size_t)((m + 1) * cols), 0);
    H[0] = 0;
    for (int64_t j = 1; j <= n && j <= hi; ++j) H[j] = local ? 0 : -(go + (j - 1) * (int64_t)ge);
    for (int64_t i = 1; i <= m && -i >= lo; ++i) H[i * cols] = local ? 0 : -(go + (i - 1) * (int64_t)ge);
    int64_t best = 0, bi = 0, bj = 0;
    for (int64_t i = 1; i <= m; ++i)
        for (int64_t j = std::max<int64_t>(1, i + lo); j <= n && j <= i + hi; ++j)
        {
            const int64_t c = i * cols + j;
            const int64_t eExt = E[c - 1] - ge, eOpen = H[c - 1] - go, fExt = F[c - cols] - ge, fOpen = H[c - cols] - go;
            E[c] = std::max(eExt, eOpen);
            F[c] = std::max(fExt, fOpen);
            const int64_t diag = H[c - cols - 1] + r.scoreMatrix[r.patternBytes[i - 1] * r.alphabetSize + r.textBytes[j - 1]];
            const int64_t h = std::max(diag, std::max(E[c], F[c]));
            uint8_t d = diag > std::max(E[c], F[c]) ? DIAG : E[c] >= F[c] ? LEFT : TOP;
            if (local && h <= 0) d = STOP;
            if (eExt > eOpen) d |= EEXT;
            if (fExt > fOpen) d |= FEXT;
            D[c] = d;
            H[c] = local ? std::max<int64_t>(h, 0) : h;
            if (local && H[c] > best)
            {
                best = H[c];
                bi = i;
                bj = j;
            }
        }
    Expected x;
    int64_t i = local ? bi : m, j = local ? bj : n;
    x.score = (int)(local ? best : H[m * cols + n]);
    if (!local && (n == 0 || m == 0)) x.score = std::max(n, m) ? -(go + ((int)std::max(n, m) - 1) * ge) : 0;
    int64_t ti = j - 1, pi = i - 1;
    int state = DIAG;  // H; LEFT: inside a run of E, TOP: of F
    const char GAP = r.alphabet[r.alphabetSize];
    while (local ? (i > 0 && j > 0) : (i > 0 || j > 0))
    {
        int d, nextState = DIAG;
        if (j == 0) d = TOP;
        else if (i == 0) d = LEFT;
        else
        {
            const uint8_t nib = D[i * cols + j];
            d = state == DIAG ? (nib & 3) : state;
            if (d == STOP) break;
            if (d == LEFT) nextState = nib & EEXT ? LEFT : DIAG;
            if (d == TOP) nextState = nib & FEXT ? TOP : DIAG;
        }
        const int tt = d == DIAG || d == LEFT, tp = d == DIAG || d == TOP;
        x.text.push_back(tt ? r.alphabet[(int)r.textBytes[j - 1]] : GAP);
        x.pattern.push_back(tp ? r.alphabet[(int)r.patternBytes[i - 1]] : GAP);
        j -= tt;
        i -= tp;
        state = nextState;
        if (local && (i == 0 || j == 0)) break;
        ti = std::max<int64_t>(ti - tt, 0);
        pi = std::max<int64_t>(pi - tp, 0);
    }
    std::reverse(x.text.begin(), x.text.end());
    std::reverse(x.pattern.begin(), x.pattern.end());
    x.startText = (uint64_t)ti;
    x.startPattern = (uint64_t)pi;
    return x;
}
}  // namespace

int main(int argc, const char *argv[])
{
    if (argc < 4)
    {
        std::cerr << "usage: sa_band_check global|local <max length> <requests> [device]\n";
        return 2;
    }
    const bool local = std::strcmp(argv[1], "local") == 0;
    const uint64_t maxLen = std::max<uint64_t>(1, std::strtoull(argv[2], nullptr, 10)), count = std::strtoull(argv[3], nullptr, 10);
    const int device = argc > 4 ? std::atoi(argv[4]) : 0;
    const int gapOpen = 11, gapExtend = 2, band = 24;
    static const int blast[16] = {5, -4, -4, -4, -4, 5, -4, -4, -4, -4, 5, -4, -4, -4, -4, 5};
    std::vector<SequenceAlignment::Request> reqs(count);
    std::vector<SequenceAlignment::Response> resp(count);
    uint64_t seed = 97531;
    for (uint64_t i = 0; i < count; ++i)
    {
        SequenceAlignment::Request &r = reqs[i];
        r.deviceType = SequenceAlignment::programArgs::GPU;
        r.sequenceType = SequenceAlignment::programArgs::DNA;
        r.alignmentType = local ? SequenceAlignment::programArgs::LOCAL : SequenceAlignment::programArgs::GLOBAL;
        r.alphabet = SequenceAlignment::DNA_ALPHABET;
        r.alphabetSize = SequenceAlignment::NUM_DNA_CHARS;
        r.gapPenalty = 5;  // ignored by the banded calls
        std::memcpy(r.scoreMatrix, blast, sizeof(blast));
        r.textNumBytes = 1 + next(seed) % maxLen;
        r.patternNumBytes = 1 + next(seed) % maxLen;
        r.textBytes = new char[r.textNumBytes];
        r.patternBytes = new char[r.patternNumBytes];
        for (uint64_t x = 0; x < r.textNumBytes; ++x) r.textBytes[x] = (char)(next(seed) % 4);
        // half the patterns are the text with substitutions and, now and then, a block of letters left
        // out, so long gaps pay; the others are random
        const bool related = (i & 1) == 0;
        uint64_t src = 0;
        for (uint64_t x = 0; x < r.patternNumBytes; ++x, ++src)
        {
            if (related && next(seed) % 64 == 0) src += next(seed) % 12;
            r.patternBytes[x] = related && src < r.textNumBytes && next(seed) % 8 ? r.textBytes[src] : (char)(next(seed) % 4);
        }
    }
    std::vector<int> scores(count), wide(count), affine(count);
    if (SequenceAlignment::scoreSequencesGPUBanded(reqs.data(), count, device, gapOpen, gapExtend, band, scores.data())) return 1;
    if (SequenceAlignment::alignSequencesGPUBanded(reqs.data(), resp.data(), count, device, gapOpen, gapExtend, band)) return 1;
    if (SequenceAlignment::scoreSequencesGPUBanded(reqs.data(), count, device, gapOpen, gapExtend, (int)maxLen, wide.data())) return 1;
    if (SequenceAlignment::scoreSequencesGPUAffine(reqs.data(), count, device, gapOpen, gapExtend, affine.data())) return 1;
    for (uint64_t i = 0; i < count; ++i)
    {
        const Expected x = bandAlign(reqs[i], local, gapOpen, gapExtend, band);
        const SequenceAlignment::Response &g = resp[i];
        const char *field = nullptr;
        if (scores[i] != x.score) field = "scoreSequencesGPUBanded";
        else if (wide[i] != affine[i]) field = "scoreSequencesGPUBanded with every cell in band";
        else if (g.score != x.score) field = "score";
        else if (g.numAlignmentBytes != x.text.size()) field = "numAlignmentBytes";
        else if (g.startInAlignedText != x.startText) field = "startInAlignedText";
        else if (g.startInAlignedPattern != x.startPattern) field = "startInAlignedPattern";
        else if (std::memcmp(g.alignedTextBytes, x.text.data(), x.text.size()) != 0) field = "alignedTextBytes";
        else if (std::memcmp(g.alignedPatternBytes, x.pattern.data(), x.pattern.size()) != 0) field = "alignedPatternBytes";
        if (field)
        {
            std::cout << "request " << i << " (" << reqs[i].textNumBytes << "x" << reqs[i].patternNumBytes << "): " << field
                      << " differs: gpu score " << g.score << " length " << g.numAlignmentBytes << " start "
                      << (int64_t)g.startInAlignedText << "/" << (int64_t)g.startInAlignedPattern << ", cpu score " << x.score
                      << " length " << x.text.size() << " start " << (int64_t)x.startText << "/" << (int64_t)x.startPattern << "\n";
            return 1;
        }
    }
    std::cout << "OK " << count << "\n";
    return 0;
}
