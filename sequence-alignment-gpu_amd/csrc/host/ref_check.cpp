// sa_ref_check — the reference aligner of the check programs (check_ref.h) on its own: no GPU, no library.
// 300 DNA pairs of 1..40 letters a side, half of them related, under the gaps 11/2, 5/5 and 3/1; global, local
// and all 16 sets of free ends, each with every cell in band and at the half-width 3, global and local also
// at the half-widths 0 and 24. For every result:
//   - the two strings are equally long and no column holds two gap letters
//   - the columns rescore to `score`, a gap run of L letters costing open + (L - 1) * extend
//   - without their gap letters the strings are the whole sequences (global), the letters from the reported
//     starts on (free ends), or pieces of the sequences (local)
//   - no free ends give global's score and strings, and free text ends (fit) the pattern start 0
//   - a half-width of both lengths or more gives every field of the call with every cell in band
// Prints the first failure, or "OK <cases>" as its last line; exit status 0 iff all hold.
#include "check_ref.h"

namespace
{
using check::Expected;
using check::Spec;

std::string letters(const std::string &aligned, char gapLetter)
{
    std::string s;
    for (char c : aligned)
        if (c != gapLetter) s += c;
    return s;
}

std::string spelled(const char *bytes, uint64_t len, const char *alphabet)
{
    std::string s;
    for (uint64_t x = 0; x < len; ++x) s += alphabet[(int)bytes[x]];
    return s;
}

// what fails in `x` as the result of `spec` on `r`, or nullptr
const char *broken(const SequenceAlignment::Request &r, const Spec &spec, const Expected &x)
{
    const char gapLetter = r.alphabet[r.alphabetSize];
    if (x.text.size() != x.pattern.size()) return "the strings' lengths";
    int64_t rescored = 0;
    for (size_t c = 0; c < x.text.size(); ++c)
    {
        const bool tg = x.text[c] == gapLetter, pg = x.pattern[c] == gapLetter;
        if (tg && pg) return "a column of two gap letters";
        if (tg) rescored -= c > 0 && x.text[c - 1] == gapLetter ? spec.ge : spec.go;
        else if (pg) rescored -= c > 0 && x.pattern[c - 1] == gapLetter ? spec.ge : spec.go;
        else
        {
            const char *alphabetEnd = r.alphabet + r.alphabetSize;
            const int ct = (int)(std::find(r.alphabet, alphabetEnd, x.text[c]) - r.alphabet);
            const int cp = (int)(std::find(r.alphabet, alphabetEnd, x.pattern[c]) - r.alphabet);
            rescored += r.scoreMatrix[cp * r.alphabetSize + ct];
        }
    }
    if (rescored != x.score) return "the score of the columns";
    const std::string text = spelled(r.textBytes, r.textNumBytes, r.alphabet), pattern = spelled(r.patternBytes, r.patternNumBytes, r.alphabet);
    const std::string t = letters(x.text, gapLetter), p = letters(x.pattern, gapLetter);
    if (spec.local)
    {
        if (text.find(t) == std::string::npos || pattern.find(p) == std::string::npos) return "the letters of a local alignment";
    }
    else if (spec.ends < 0)
    {
        if (t != text || p != pattern) return "the letters of a global alignment";
    }
    else if (x.startText > text.size() || x.startPattern > pattern.size() || text.compare(x.startText, t.size(), t) != 0 ||
             pattern.compare(x.startPattern, p.size(), p) != 0)
        return "the letters from the reported starts on";
    return nullptr;
}

bool same(const Expected &a, const Expected &b)
{
    return a.score == b.score && a.startText == b.startText && a.startPattern == b.startPattern && a.text == b.text && a.pattern == b.pattern;
}
}  // namespace

int main()
{
    const int gaps[3][2] = {{11, 2}, {5, 5}, {3, 1}};
    uint64_t seed = 192837, cases = 0;
    for (uint64_t pair = 0; pair < 300; ++pair)
    {
        SequenceAlignment::Request r;
        check::scheme(r);
        r.textNumBytes = 1 + check::next(seed) % 40;
        r.patternNumBytes = 1 + check::next(seed) % 40;
        check::randomText(r, seed);
        const bool related = (pair & 1) == 0;
        check::relatedPattern(r, seed, check::next(seed) % r.textNumBytes, related ? r.patternNumBytes : 0, related, 4);
        const int64_t longer = (int64_t)std::max(r.textNumBytes, r.patternNumBytes);
        for (const int *gap : gaps)
        {
            const Expected global = check::align(r, Spec::global(gap[0], gap[1]));
            // mode 0: global, 1: local, 2 + flags: the free ends `flags`
            for (int mode = 0; mode < 18; ++mode)
            {
                const Spec spec = mode == 0 ? Spec::global(gap[0], gap[1]) : mode == 1 ? Spec::localMode(gap[0], gap[1]) : Spec::endsFree(mode - 2, gap[0], gap[1]);
                const Expected every = check::align(r, spec);
                const char *what = nullptr;
                int64_t at = -1;  // the half-width, -1: every cell
                const auto fail = [&](const char *w, int64_t width) { if (w && !what) what = w, at = width; };
                fail(broken(r, spec, every), -1);
                if (mode == 2 && (every.score != global.score || every.text != global.text || every.pattern != global.pattern))
                    fail("no free ends against global", -1);
                if (mode == 2 + (SA_FREE_TEXT_BEGIN | SA_FREE_TEXT_END) && every.startPattern != 0) fail("the pattern start of a fit", -1);
                if (!same(check::align(r, spec.halfWidth(longer)), every)) fail("a half-width of the longer side against every cell", longer);
                ++cases;
                for (int64_t w : {0, 3, 24})
                {
                    if (w != 3 && mode > 1) continue;
                    fail(broken(r, spec.halfWidth(w), check::align(r, spec.halfWidth(w))), w);
                    ++cases;
                }
                if (what)
                {
                    std::cout << "pair " << pair << " (" << r.textNumBytes << "x" << r.patternNumBytes << "), gap " << gap[0] << "/" << gap[1]
                              << ", mode " << mode << ", half-width " << at << ": " << what << " fails\n";
                    return 1;
                }
            }
        }
    }
    std::cout << "OK " << cases << "\n";
    return 0;
}
