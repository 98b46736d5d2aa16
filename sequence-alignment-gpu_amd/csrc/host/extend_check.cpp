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
// With --expected: the digest of the requests (check_ref.h) and nothing of either library.
#include "check_ref.h"

int main(int argc, char **argv)
{
    const bool expectedOnly = check::takeExpected(argc, argv);
    if (argc < 3)
    {
        std::cout << "usage: sa_extend_check <n> <count> [device]\n";
        return 2;
    }
    const uint64_t maxLen = std::max<uint64_t>(1, std::strtoull(argv[1], nullptr, 10));
    const uint64_t count = std::strtoull(argv[2], nullptr, 10);
    const int device = argc > 3 ? std::atoi(argv[3]) : 0;
    const int gapOpen = 11, gapExtend = 2;
    const int xdrops[2] = {20, SA_NO_XDROP};
    std::vector<SequenceAlignment::Request> reqs(count);
    uint64_t seed = 97531;
    for (uint64_t i = 0; i < count; ++i)
    {
        SequenceAlignment::Request &r = reqs[i];
        check::scheme(r);
        r.textNumBytes = 1 + check::next(seed) % maxLen;
        r.patternNumBytes = 1 + check::next(seed) % maxLen;
        check::randomText(r, seed);
        // the pattern: the text with substitutions and a few letters left out up to letter `related`,
        // unrelated letters from there on
        const uint64_t related = check::next(seed) % (r.patternNumBytes + 1);
        check::relatedPattern(r, seed, 0, related, true, 4);
    }
    if (expectedOnly)
    {
        check::Digest sent;
        sent.requests(reqs);
        for (int xdrop : xdrops) sent.number(xdrop);
        return check::printExpected("sa_extend_check", argc, argv, sent, nullptr);
    }
    std::vector<int> previous(count, 0);
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
            uint64_t endText, endPattern;
            check::countLetters(resp[i], reqs[i].alphabet[reqs[i].alphabetSize], endText, endPattern);
            if (endText > reqs[i].textNumBytes || endPattern > reqs[i].patternNumBytes)
            {
                std::cout << "request " << i << " at xdrop " << xdrop << ": the strings hold more letters than the sequences\n";
                return 1;
            }
            check::slice(pre[i], reqs[i], 0, endText, 0, endPattern, false);
        }
        if (SequenceAlignment::alignSequencesGPUAffine(pre.data(), respPrefix.data(), count, device, gapOpen, gapExtend)) return 1;
        for (uint64_t i = 0; i < count; ++i)
        {
            const SequenceAlignment::Response &g = resp[i];
            // the global alignment of the prefixes, and both starts 0
            check::Expected want = check::expectedOf(respPrefix[i]);
            want.startText = want.startPattern = 0;
            const auto scorers = {check::Scored{"scoreSequencesGPUExtend against alignSequencesGPUExtend", scores[i], g.score}};
            const char *field = check::firstDifference(g, want, scorers);
            if (!field && g.score < 0) field = "a negative score";
            if (!field && xdrop == SA_NO_XDROP && g.score < previous[i]) field = "the score without a drop against the score at xdrop 20";
            if (field)
                return check::reportDifference(i, reqs[i], "xdrop " + std::to_string(xdrop) + ", prefixes " + std::to_string(pre[i].textNumBytes) + "x" +
                                                               std::to_string(pre[i].patternNumBytes),
                                               field, g, want, scorers);
            previous[i] = g.score;
        }
    }
    std::cout << "OK " << count << "\n";
    return 0;
}
