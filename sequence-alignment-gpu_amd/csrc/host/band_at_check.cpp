// sa_band_at_check — a C++14 caller of the band-at extension (sa_hip.h: request k counts cell (i, j) iff
// bandLo[k] <= j - i <= bandHi[k]): 48 DNA Requests, each a read of up to <m> letters cut from a text up
// to 300 letters longer at letter c, through SequenceAlignment::scoreSequencesGPUBandAt and
// alignSequencesGPUBandAt (gap open 11, gap extend 2) and, one by one, through the plain banded Gotoh
// fill, result pick and three-state walk below; the score and every Response field are
// compared. The bands are {c - w, c + w} (fit, overlap, local) and {-w - k % 3, n - m + w + k % 5}
// (global: the origin and the end cell must be in band). A last call with the bands {-m, n} must equal
// the unbanded function of the mode.
//   usage: sa_band_at_check global|local|fit|overlap <m> <w> [device]
// Prints the first difference, or "OK <w>" as its last line; exit status 0 iff all equal.
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

enum { LEFT = 0, DIAG = 1, TOP = 2, STOP = 3, EEXT = 4, FEXT = 8 };
enum { TB = 1, TE = 2, PB = 4, PE = 8 };

// Gotoh's recurrence row by row over the in-band cells with the direction nibble of each. H, E and F of
// every out-of-band cell are minus infinity (NEG; a value below NEG / 2 counts as it). Borders: 0 where
// free and in band, one gap run where the cell and the origin are in band, else minus infinity. Then the
// result of the mode over the real candidates and the walk from it. `ends` < 0: global; `local` as is.
Expected bandAtAlign(const SequenceAlignment::Request &r, bool local, int ends, int go, int ge, int64_t lo, int64_t hi)
{
    const int64_t n = (int64_t)r.textNumBytes, m = (int64_t)r.patternNumBytes, NEG = -(1ll << 40);
    const int64_t cols = n + 1;
    const int fl = ends < 0 ? 0 : ends;
    const bool tfree = local || (fl & TB), pfree = local || (fl & PB), origin = lo <= 0 && 0 <= hi;
    auto inb = [&](int64_t i, int64_t j) { return lo <= j - i && j - i <= hi; };
    auto real = [&](int64_t v) { return v > NEG / 2; };
    std::vector<int64_t> H((size_t)((m + 1) * cols), NEG), E((size_t)((m + 1) * cols), NEG), F((size_t)((m + 1) * cols), NEG);
    std::vector<uint8_t> D((size_t)((m + 1) * cols), 0);
    if (origin) H[0] = 0;
    for (int64_t j = 1; j <= n; ++j)
        if (inb(0, j) && (tfree || origin)) H[j] = tfree ? 0 : -(go + (j - 1) * (int64_t)ge);
    for (int64_t i = 1; i <= m; ++i)
        if (inb(i, 0) && (pfree || origin)) H[i * cols] = pfree ? 0 : -(go + (i - 1) * (int64_t)ge);
    int64_t best = 0, bi = 0, bj = 0;
    for (int64_t i = 1; i <= m; ++i)
        for (int64_t j = std::max<int64_t>(1, i + lo); j <= n && j <= i + hi; ++j)
        {
            const int64_t c = i * cols + j;
            const int64_t eExt = E[c - 1] - ge, eOpen = H[c - 1] - go, fExt = F[c - cols] - ge, fOpen = H[c - cols] - go;
            const int64_t e = std::max(eExt, eOpen), f = std::max(fExt, fOpen);
            const int64_t diag = H[c - cols - 1] + r.scoreMatrix[r.patternBytes[i - 1] * r.alphabetSize + r.textBytes[j - 1]];
            const int64_t h = std::max(diag, std::max(e, f));
            uint8_t d = diag > std::max(e, f) ? DIAG : e >= f ? LEFT : TOP;
            if (local && h <= 0) d = STOP;
            if (eExt > eOpen && real(E[c - 1])) d |= EEXT;
            if (fExt > fOpen && real(F[c - cols])) d |= FEXT;
            D[c] = d;
            E[c] = real(e) ? e : NEG;
            F[c] = real(f) ? f : NEG;
            H[c] = local ? std::max<int64_t>(h, 0) : real(h) ? h : NEG;
            if (local && H[c] > best)
            {
                best = H[c];
                bi = i;
                bj = j;
            }
        }
    Expected x;
    int64_t i = m, j = n;
    if (local) i = bi, j = bj, x.score = (int)best;
    else if (ends < 0) x.score = (int)H[m * cols + n];
    else
    {
        // the real candidates in row-major order: an interior one beats a border one of the same value,
        // within each kind the first wins
        int64_t iv = NEG, ii = 0, ij = 0, bv = NEG, bbi = 0, bbj = 0;
        for (int64_t a = 0; a <= m; ++a)
            for (int64_t b = 0; b <= n; ++b)
            {
                if (!((a == m && b == n) || (a == m && (fl & TE)) || (b == n && (fl & PE)))) continue;
                const int64_t v = H[a * cols + b];
                if (!real(v)) continue;
                if (a >= 1 && b >= 1)
                {
                    if (v > iv) iv = v, ii = a, ij = b;
                }
                else if (v > bv) bv = v, bbi = a, bbj = b;
            }
        if (real(iv) && iv >= bv) i = ii, j = ij, x.score = (int)iv;
        else i = bbi, j = bbj, x.score = (int)bv;
    }
    int64_t ti = j - 1, pi = i - 1;
    int state = DIAG;  // H; LEFT: inside a run of E, TOP: of F
    const char GAP = r.alphabet[r.alphabetSize];
    for (;;)
    {
        if (local ? !(i > 0 && j > 0) : ends < 0 ? !(i > 0 || j > 0) : (i == 0 && ((fl & TB) || j == 0)) || (j == 0 && ((fl & PB) || i == 0)))
            break;
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
    // ends-free: the cell the walk ended in; global and local: the reference's indices
    x.startText = (uint64_t)(ends >= 0 ? j : ti);
    x.startPattern = (uint64_t)(ends >= 0 ? i : pi);
    return x;
}
}  // namespace

int main(int argc, const char *argv[])
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (argc < 4 || (mode != "global" && mode != "local" && mode != "fit" && mode != "overlap"))
    {
        std::cerr << "usage: sa_band_at_check global|local|fit|overlap <m> <w> [device]\n";
        return 2;
    }
    const bool local = mode == "local";
    // the mode argument of the C++ functions: -1 reads Request::alignmentType, else the free ends
    const int freeEnds = mode == "overlap" ? 15 : -1;
    const int ends = mode == "fit" ? (TB | TE) : mode == "overlap" ? 15 : -1;  // of the plain fill below
    const uint64_t maxLen = std::max<uint64_t>(1, std::strtoull(argv[2], nullptr, 10)), count = 48;
    const int w = std::atoi(argv[3]);
    const int device = argc > 4 ? std::atoi(argv[4]) : 0;
    const int gapOpen = 11, gapExtend = 2;
    static const int blast[16] = {5, -4, -4, -4, -4, 5, -4, -4, -4, -4, 5, -4, -4, -4, -4, 5};
    std::vector<SequenceAlignment::Request> reqs(count);
    std::vector<SequenceAlignment::Response> resp(count), respFull(count), respUnbanded(count);
    std::vector<int> lo(count), hi(count), loFull(count), hiFull(count);
    uint64_t seed = 86420;
    for (uint64_t i = 0; i < count; ++i)
    {
        SequenceAlignment::Request &r = reqs[i];
        r.deviceType = SequenceAlignment::programArgs::GPU;
        r.sequenceType = SequenceAlignment::programArgs::DNA;
        r.alignmentType = local ? SequenceAlignment::programArgs::LOCAL
                          : mode == "fit" ? SequenceAlignment::programArgs::SEMI_GLOBAL
                                          : SequenceAlignment::programArgs::GLOBAL;
        r.alphabet = SequenceAlignment::DNA_ALPHABET;
        r.alphabetSize = SequenceAlignment::NUM_DNA_CHARS;
        r.gapPenalty = 5;  // ignored by the band-at calls
        std::memcpy(r.scoreMatrix, blast, sizeof(blast));
        r.patternNumBytes = 1 + next(seed) % maxLen;
        const uint64_t extra = next(seed) % 301, c = next(seed) % (extra + 1);
        r.textNumBytes = r.patternNumBytes + extra;
        r.textBytes = new char[r.textNumBytes];
        r.patternBytes = new char[r.patternNumBytes];
        for (uint64_t x = 0; x < r.textNumBytes; ++x) r.textBytes[x] = (char)(next(seed) % 4);
        // the read: the text from letter c on with substitutions and, now and then, a few letters left out
        uint64_t src = c;
        for (uint64_t x = 0; x < r.patternNumBytes; ++x, ++src)
        {
            if (next(seed) % 64 == 0) src += next(seed) % 4;
            r.patternBytes[x] = src < r.textNumBytes && next(seed) % 8 ? r.textBytes[src] : (char)(next(seed) % 4);
        }
        if (mode == "global") lo[i] = -w - (int)(i % 3), hi[i] = (int)extra + w + (int)(i % 5);
        else lo[i] = (int)c - w, hi[i] = (int)c + w;
        loFull[i] = -(int)r.patternNumBytes;
        hiFull[i] = (int)r.textNumBytes;
        if (sa_band_reachable(local ? SA_LOCAL : ends < 0 ? SA_GLOBAL : SA_ENDS_FREE | ends, r.textNumBytes, r.patternNumBytes,
                              sa_band{lo[i], hi[i]}) != 1)
        {
            std::cout << "request " << i << ": its band [" << lo[i] << ", " << hi[i] << "] admits no alignment\n";
            return 1;
        }
    }
    std::vector<int> scores(count), full(count), unbanded(count);
    if (SequenceAlignment::scoreSequencesGPUBandAt(reqs.data(), count, device, gapOpen, gapExtend, freeEnds, lo.data(), hi.data(), scores.data())) return 1;
    if (SequenceAlignment::alignSequencesGPUBandAt(reqs.data(), resp.data(), count, device, gapOpen, gapExtend, freeEnds, lo.data(), hi.data())) return 1;
    if (SequenceAlignment::scoreSequencesGPUBandAt(reqs.data(), count, device, gapOpen, gapExtend, freeEnds, loFull.data(), hiFull.data(), full.data())) return 1;
    if (SequenceAlignment::alignSequencesGPUBandAt(reqs.data(), respFull.data(), count, device, gapOpen, gapExtend, freeEnds, loFull.data(), hiFull.data())) return 1;
    if (freeEnds >= 0)
    {
        if (SequenceAlignment::scoreSequencesGPUEndsFree(reqs.data(), count, device, gapOpen, gapExtend, freeEnds, unbanded.data())) return 1;
        if (SequenceAlignment::alignSequencesGPUEndsFree(reqs.data(), respUnbanded.data(), count, device, gapOpen, gapExtend, freeEnds)) return 1;
    }
    else
    {
        if (SequenceAlignment::scoreSequencesGPUAffine(reqs.data(), count, device, gapOpen, gapExtend, unbanded.data())) return 1;
        if (SequenceAlignment::alignSequencesGPUAffine(reqs.data(), respUnbanded.data(), count, device, gapOpen, gapExtend)) return 1;
    }
    for (uint64_t i = 0; i < count; ++i)
    {
        const Expected x = bandAtAlign(reqs[i], local, ends, gapOpen, gapExtend, lo[i], hi[i]);
        const SequenceAlignment::Response &g = resp[i], &a = respFull[i], &b = respUnbanded[i];
        const char *field = nullptr;
        if (scores[i] != x.score) field = "scoreSequencesGPUBandAt";
        else if (full[i] != unbanded[i]) field = "scoreSequencesGPUBandAt with every cell in band";
        else if (a.score != b.score || a.numAlignmentBytes != b.numAlignmentBytes || a.startInAlignedText != b.startInAlignedText ||
                 a.startInAlignedPattern != b.startInAlignedPattern ||
                 std::memcmp(a.alignedTextBytes, b.alignedTextBytes, a.numAlignmentBytes) != 0 ||
                 std::memcmp(a.alignedPatternBytes, b.alignedPatternBytes, a.numAlignmentBytes) != 0)
            field = "alignSequencesGPUBandAt with every cell in band";
        else if (g.score != x.score) field = "score";
        else if (g.numAlignmentBytes != x.text.size()) field = "numAlignmentBytes";
        else if (g.startInAlignedText != x.startText) field = "startInAlignedText";
        else if (g.startInAlignedPattern != x.startPattern) field = "startInAlignedPattern";
        else if (std::memcmp(g.alignedTextBytes, x.text.data(), x.text.size()) != 0) field = "alignedTextBytes";
        else if (std::memcmp(g.alignedPatternBytes, x.pattern.data(), x.pattern.size()) != 0) field = "alignedPatternBytes";
        if (field)
        {
            std::cout << "request " << i << " (" << reqs[i].textNumBytes << "x" << reqs[i].patternNumBytes << ", band [" << lo[i] << ", "
                      << hi[i] << "]): " << field << " differs: gpu score " << g.score << " length " << g.numAlignmentBytes << " start "
                      << (int64_t)g.startInAlignedText << "/" << (int64_t)g.startInAlignedPattern << ", cpu score " << x.score
                      << " length " << x.text.size() << " start " << (int64_t)x.startText << "/" << (int64_t)x.startPattern << "\n";
            return 1;
        }
    }
    std::cout << "OK " << w << "\n";
    return 0;
}
