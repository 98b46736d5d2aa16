// check_ref.h — the kit of the check programs (csrc/host/*_check.cpp, the list at the top of the Makefile):
// the generator of their requests, the one plain reference aligner that the GPU functions are compared with
// (DESIGN.md §3.5), the comparison of a Response with what the reference expects, and the digests that
// `--expected` prints. Header only, C++14, and nothing here calls into either library: a program that calls
// no library function of its own builds with a plain C++ compiler and links nothing (ref_check.cpp).
#pragma once

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <iostream>
#include <string>
#include <vector>

#include "SequenceAlignment.hpp"
#include "sa_hip.h"

namespace check
{
using SequenceAlignment::Request;
using SequenceAlignment::Response;

inline uint64_t nowUs()
{
    return (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---- requests ----

inline uint64_t next(uint64_t &s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return s >> 33;
}

const int blast[16] = {5, -4, -4, -4, -4, 5, -4, -4, -4, -4, 5, -4, -4, -4, -4, 5};

// the scheme fields of a DNA request: the blast matrix and the linear gap 5, which every function with a gap
// argument of its own ignores
inline void scheme(Request &r, SequenceAlignment::programArgs alignmentType = SequenceAlignment::programArgs::GLOBAL)
{
    r.deviceType = SequenceAlignment::programArgs::GPU;
    r.sequenceType = SequenceAlignment::programArgs::DNA;
    r.alignmentType = alignmentType;
    r.alphabet = SequenceAlignment::DNA_ALPHABET;
    r.alphabetSize = SequenceAlignment::NUM_DNA_CHARS;
    r.gapPenalty = 5;
    std::memcpy(r.scoreMatrix, blast, sizeof(blast));
}

// both sides allocated at the lengths the request holds (one letter at least), the text filled with random letters
inline void randomText(Request &r, uint64_t &seed)
{
    r.textBytes = new char[std::max<uint64_t>(r.textNumBytes, 1)];
    r.patternBytes = new char[std::max<uint64_t>(r.patternNumBytes, 1)];
    for (uint64_t x = 0; x < r.textNumBytes; ++x) r.textBytes[x] = (char)(next(seed) % 4);
}

// The related pattern: its first `relatedLetters` letters are the text from letter `src` on with one
// substitution in eight, the others are random; with `skips`, one letter in 64 leaves a block of up to
// skipLength - 1 text letters out, so long gaps pay. relatedLetters = 0 is a random pattern.
inline void relatedPattern(Request &r, uint64_t &seed, uint64_t src, uint64_t relatedLetters, bool skips, uint64_t skipLength)
{
    for (uint64_t x = 0; x < r.patternNumBytes; ++x, ++src)
    {
        if (skips && next(seed) % 64 == 0) src += next(seed) % skipLength;
        r.patternBytes[x] = x < relatedLetters && src < r.textNumBytes && next(seed) % 8 ? r.textBytes[src] : (char)(next(seed) % 4);
    }
}

// a request over letters [from, from + len) of `src`, forwards, or backwards from letter from + len - 1
inline void slice(Request &r, const Request &src, uint64_t tFrom, uint64_t tLen, uint64_t pFrom, uint64_t pLen, bool reversed)
{
    scheme(r);
    r.textNumBytes = tLen;
    r.patternNumBytes = pLen;
    r.textBytes = new char[std::max<uint64_t>(tLen, 1)];
    r.patternBytes = new char[std::max<uint64_t>(pLen, 1)];
    for (uint64_t x = 0; x < tLen; ++x) r.textBytes[x] = src.textBytes[reversed ? tFrom + tLen - 1 - x : tFrom + x];
    for (uint64_t x = 0; x < pLen; ++x) r.patternBytes[x] = src.patternBytes[reversed ? pFrom + pLen - 1 - x : pFrom + x];
}

// the letters of each side in a pair of aligned strings
inline void countLetters(const Response &g, char gapLetter, uint64_t &text, uint64_t &pattern)
{
    text = pattern = 0;
    for (uint64_t x = 0; x < g.numAlignmentBytes; ++x)
    {
        text += g.alignedTextBytes[x] != gapLetter;
        pattern += g.alignedPatternBytes[x] != gapLetter;
    }
}

// ---- the reference aligner ----

struct Expected
{
    int score = 0;
    uint64_t startText = 0, startPattern = 0;
    std::string text, pattern;
};

inline Expected expectedOf(const Response &r)
{
    Expected x;
    x.score = r.score;
    x.startText = r.startInAlignedText;
    x.startPattern = r.startInAlignedPattern;
    x.text.assign(r.alignedTextBytes, r.numAlignmentBytes);
    x.pattern.assign(r.alignedPatternBytes, r.numAlignmentBytes);
    return x;
}

// the aligned strings of `g` after those of `x`, forwards or from their last column backwards
inline void appendStrings(Expected &x, const Response &g, bool reversed)
{
    for (uint64_t c = 0; c < g.numAlignmentBytes; ++c)
    {
        x.text += g.alignedTextBytes[reversed ? g.numAlignmentBytes - 1 - c : c];
        x.pattern += g.alignedPatternBytes[reversed ? g.numAlignmentBytes - 1 - c : c];
    }
}

// What to align: the mode (global, local, or global with the free ends `ends`, a set of SA_FREE_*), the affine
// gap, and the band: cell (i, j) counts iff lo <= j - i <= hi.
struct Spec
{
    bool local = false;
    int ends = -1;  // < 0: none, the plain global result and the reference's start indices
    int go = 11, ge = 2;
    enum Band { EVERY_CELL, HALF_WIDTH, AT } band = EVERY_CELL;
    int64_t lo = 0, hi = 0;  // AT: the band; HALF_WIDTH: lo is the width

    static Spec global(int go, int ge) { return make(false, -1, go, ge); }
    static Spec localMode(int go, int ge) { return make(true, -1, go, ge); }
    static Spec endsFree(int flags, int go, int ge) { return make(false, flags, go, ge); }
    static Spec fit(int go, int ge) { return make(false, SA_FREE_TEXT_BEGIN | SA_FREE_TEXT_END, go, ge); }
    // within w of the diagonals of the origin and of the end cell (sa_hip.h, the banded extension)
    Spec halfWidth(int64_t w) const { return banded(HALF_WIDTH, w, 0); }
    Spec bandAt(int64_t l, int64_t h) const { return banded(AT, l, h); }

    void range(int64_t n, int64_t m, int64_t &l, int64_t &h) const
    {
        l = band == AT ? lo : band == HALF_WIDTH ? std::min<int64_t>(0, n - m) - lo : -m;
        h = band == AT ? hi : band == HALF_WIDTH ? std::max<int64_t>(0, n - m) + lo : n;
    }

  private:
    static Spec make(bool local, int ends, int go, int ge)
    {
        Spec s;
        s.local = local, s.ends = ends, s.go = go, s.ge = ge;
        return s;
    }
    Spec banded(Band kind, int64_t l, int64_t h) const
    {
        Spec s = *this;
        s.band = kind, s.lo = l, s.hi = h;
        return s;
    }
};

// Gotoh's recurrence row by row over the in-band cells with the direction nibble of each. H, E and F of
// every out-of-band cell are minus infinity (NEG; a value below NEG / 2 counts as it). Borders: 0 where
// free and in band, one gap run where the cell and the origin are in band, else minus infinity. Then the
// result of the mode over the real candidates and the three-state walk from it. go == ge is the linear
// recurrence.
inline Expected align(const Request &r, const Spec &s)
{
    enum { LEFT = 0, DIAG = 1, TOP = 2, STOP = 3, EEXT = 4, FEXT = 8 };
    enum { TB = SA_FREE_TEXT_BEGIN, TE = SA_FREE_TEXT_END, PB = SA_FREE_PATTERN_BEGIN, PE = SA_FREE_PATTERN_END };
    const int64_t n = (int64_t)r.textNumBytes, m = (int64_t)r.patternNumBytes, NEG = -(1ll << 40);
    const int64_t cols = n + 1;
    const bool local = s.local;
    const int ends = s.ends, go = s.go, ge = s.ge, fl = ends < 0 ? 0 : ends;
    int64_t lo, hi;
    s.range(n, m, lo, hi);
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

// the score alone, for the programs that call only a scorer
inline int score(const Request &r, const Spec &s) { return align(r, s).score; }

// ---- the comparison ----

// a score of a score-only function beside the Response, with the name the difference is reported under
struct Scored
{
    const char *name;
    int got, want;
};

// the name of the first thing that differs, the scorers' scores first, or nullptr
inline const char *firstDifference(const Response &g, const Expected &x, std::initializer_list<Scored> scorers = {})
{
    for (const Scored &s : scorers)
        if (s.got != s.want) return s.name;
    if (g.score != x.score) return "score";
    if (g.numAlignmentBytes != x.text.size()) return "numAlignmentBytes";
    if (g.startInAlignedText != x.startText) return "startInAlignedText";
    if (g.startInAlignedPattern != x.startPattern) return "startInAlignedPattern";
    if (std::memcmp(g.alignedTextBytes, x.text.data(), x.text.size()) != 0) return "alignedTextBytes";
    if (std::memcmp(g.alignedPatternBytes, x.pattern.data(), x.pattern.size()) != 0) return "alignedPatternBytes";
    return nullptr;
}

// the first-difference line; `params` names the variant's parameters (flags, band, width, seeds, X-drop) or is
// empty. Returns 1, the exit status of a check that failed.
inline int reportDifference(uint64_t index, const Request &r, const std::string &params, const char *field, const Response &g,
                            const Expected &x, std::initializer_list<Scored> scorers = {})
{
    std::cout << "request " << index << " (" << r.textNumBytes << "x" << r.patternNumBytes << (params.empty() ? "" : ", ") << params
              << "): " << field << " differs: gpu score " << g.score << " length " << g.numAlignmentBytes << " start "
              << (int64_t)g.startInAlignedText << "/" << (int64_t)g.startInAlignedPattern << ", expected score " << x.score << " length "
              << x.text.size() << " start " << (int64_t)x.startText << "/" << (int64_t)x.startPattern;
    for (const Scored &s : scorers) std::cout << "; " << s.name << " " << s.got << ", expected " << s.want;
    std::cout << "\n";
    return 1;
}

// the result line of the programs that count mismatches; returns their exit status
inline int printMismatches(uint64_t count, uint64_t bad, uint64_t gpuUs, uint64_t cpuUs)
{
    std::cout << "{\"requests\": " << count << ", \"mismatches\": " << bad << ", \"gpu_us\": " << gpuUs << ", \"cpu_us\": " << cpuUs << "}\n";
    return bad ? 1 : 0;
}

// ---- --expected ----

// 64-bit FNV-1a over everything a program passes to the GPU functions, or over everything it expects of them;
// numbers go in as eight bytes, low byte first
struct Digest
{
    uint64_t h = 14695981039346656037ull;

    void bytes(const char *p, uint64_t len)
    {
        for (uint64_t x = 0; x < len; ++x) h = (h ^ (uint8_t)p[x]) * 1099511628211ull;
    }
    void number(int64_t v)
    {
        for (int b = 0; b < 8; ++b) h = (h ^ (((uint64_t)v >> (8 * b)) & 255)) * 1099511628211ull;
    }
    template <class T> void numbers(const std::vector<T> &v)
    {
        number((int64_t)v.size());
        for (const T &e : v) number((int64_t)e);
    }
    void request(const Request &r)
    {
        number((int64_t)r.alignmentType);
        number((int64_t)r.textNumBytes);
        number((int64_t)r.patternNumBytes);
        bytes(r.textBytes, r.textNumBytes);
        bytes(r.patternBytes, r.patternNumBytes);
    }
    void requests(const std::vector<Request> &v)
    {
        number((int64_t)v.size());
        for (const Request &r : v) request(r);
    }
    void expected(const Expected &x)
    {
        number(x.score);
        number((int64_t)x.startText);
        number((int64_t)x.startPattern);
        number((int64_t)x.text.size());
        bytes(x.text.data(), x.text.size());
        bytes(x.pattern.data(), x.pattern.size());
    }
    std::string hex() const
    {
        char buf[17];
        std::snprintf(buf, sizeof buf, "%016llx", (unsigned long long)h);
        return buf;
    }
};

// takes --expected off the command line, wherever it stands; true if it was there
inline bool takeExpected(int &argc, char **argv)
{
    int kept = 0;
    bool found = false;
    for (int a = 0; a < argc; ++a)
        if (a > 0 && std::strcmp(argv[a], "--expected") == 0) found = true;
        else argv[kept++] = argv[a];
    argc = kept;
    return found;
}

// the line of --expected: what the program gives the GPU and, with a reference of its own, what it expects
// back (nullptr: it compares library functions with each other). Returns 0, the exit status.
inline int printExpected(const char *program, int argc, char **argv, const Digest &requests, const Digest *expected)
{
    std::cout << "{\"program\": \"" << program << "\", \"args\": [";
    for (int a = 1; a < argc; ++a) std::cout << (a > 1 ? ", " : "") << "\"" << argv[a] << "\"";
    std::cout << "], \"requests\": \"" << requests.hex() << "\", \"expected\": ";
    if (expected) std::cout << "\"" << expected->hex() << "\"";
    else std::cout << "null";
    std::cout << "}\n";
    return 0;
}
}  // namespace check
