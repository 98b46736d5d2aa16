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
// With --expected: the digest of the requests, seeds and halves (check_ref.h) and nothing of either library.
#include "check_ref.h"

int main(int argc, char **argv)
{
    const bool expectedOnly = check::takeExpected(argc, argv);
    if (argc < 3)
    {
        std::cout << "usage: sa_seeds_check <n> <count> [device]\n";
        return 2;
    }
    const uint64_t maxLen = std::max<uint64_t>(1, std::strtoull(argv[1], nullptr, 10));
    const uint64_t count = std::strtoull(argv[2], nullptr, 10);
    const int device = argc > 3 ? std::atoi(argv[3]) : 0;
    const int gapOpen = 11, gapExtend = 2;
    const int xdrops[2] = {20, SA_NO_XDROP};
    std::vector<SequenceAlignment::Request> reqs(count), left(count), right(count);
    std::vector<uint64_t> ts(count), ps(count), len(count);
    uint64_t seed = 86420;
    for (uint64_t i = 0; i < count; ++i)
    {
        SequenceAlignment::Request &r = reqs[i];
        check::scheme(r);
        r.textNumBytes = 1 + check::next(seed) % maxLen;
        r.patternNumBytes = 1 + check::next(seed) % maxLen;
        ts[i] = check::next(seed) % (r.textNumBytes + 1);
        ps[i] = check::next(seed) % (r.patternNumBytes + 1);
        const uint64_t room = std::min(r.textNumBytes - ts[i], r.patternNumBytes - ps[i]);
        len[i] = i % 5 == 0 ? 0 : check::next(seed) % (std::min<uint64_t>(room, 40) + 1);
        check::randomText(r, seed);
        // the pattern: the text on the seed's diagonal with substitutions within `related` letters of the
        // seed, unrelated letters further out
        const uint64_t related = check::next(seed) % (maxLen + 1);
        for (uint64_t x = 0; x < r.patternNumBytes; ++x)
        {
            const int64_t src = (int64_t)x - (int64_t)ps[i] + (int64_t)ts[i];
            const uint64_t away = x < ps[i] ? ps[i] - x : x - ps[i];
            const bool copy = away < related + len[i] && src >= 0 && src < (int64_t)r.textNumBytes && check::next(seed) % 8;
            r.patternBytes[x] = copy ? r.textBytes[src] : (char)(check::next(seed) % 4);
        }
        check::slice(left[i], r, 0, ts[i], 0, ps[i], true);
        check::slice(right[i], r, ts[i] + len[i], r.textNumBytes - ts[i] - len[i], ps[i] + len[i], r.patternNumBytes - ps[i] - len[i], false);
    }
    if (expectedOnly)
    {
        check::Digest sent;
        sent.requests(reqs);
        sent.numbers(ts), sent.numbers(ps), sent.numbers(len);
        sent.requests(left), sent.requests(right);
        for (int xdrop : xdrops) sent.number(xdrop);
        return check::printExpected("sa_seeds_check", argc, argv, sent, nullptr);
    }
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
            // the left extension backwards, the seed's letters, the right extension
            check::Expected want;
            uint64_t leftText, leftPattern;
            check::countLetters(l, reqs[i].alphabet[reqs[i].alphabetSize], leftText, leftPattern);
            check::appendStrings(want, l, true);
            want.score = l.score + r.score;
            for (uint64_t q = 0; q < len[i]; ++q)
            {
                const int ct = reqs[i].textBytes[ts[i] + q], cp = reqs[i].patternBytes[ps[i] + q];
                want.score += check::blast[cp * 4 + ct];
                want.text += reqs[i].alphabet[ct];
                want.pattern += reqs[i].alphabet[cp];
            }
            check::appendStrings(want, r, false);
            want.startText = ts[i] - leftText;
            want.startPattern = ps[i] - leftPattern;
            const auto scorers = {check::Scored{"scoreSequencesGPUSeeds against alignSequencesGPUSeeds", scores[i], g.score}};
            if (const char *field = check::firstDifference(g, want, scorers))
                return check::reportDifference(i, reqs[i], "seed " + std::to_string(ts[i]) + ":" + std::to_string(ps[i]) + ":" + std::to_string(len[i]) +
                                                               " at xdrop " + std::to_string(xdrop) + ", left " + std::to_string(l.score) + " right " +
                                                               std::to_string(r.score),
                                               field, g, want, scorers);
        }
    }
    std::cout << "OK " << count << "\n";
    return 0;
}
