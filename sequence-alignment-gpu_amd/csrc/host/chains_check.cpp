// sa_chains_check — a C++14 caller of the chained-seeds functions (sa_hip.h sa_score_batch_chains): <count> DNA
// Requests of up to <n> letters a side, each with a random colinear chain of one to <seeds> seeds (some of length
// 0, some adjacent, some with a gap that has an empty side) along which the pattern is a mutated copy of the text,
// through SequenceAlignment::scoreSequencesGPUChains and alignSequencesGPUChains (gap open 11, gap extend 2) at
// X-drop 20 and without a drop. Identity C1 of sa_hip.h is checked against the library's own functions:
// alignSequencesGPUExtend on the two ends, the left one reversed here on the host, and alignSequencesGPUAffine in
// GLOBAL mode on every gap rectangle with two non-empty sides must give the score (with the seeds' substitution
// scores and the closed-form gaps added), the two starts and, joined in order, both strings. The scorer's score
// must equal the aligner's.
//   usage: sa_chains_check <n> <count> [seeds] [device]
// Prints the first difference, or "OK <count>" as its last line; exit status 0 iff all equal.
// With --expected: the digest of the requests, chains and pieces (check_ref.h) and nothing of either library.
#include "check_ref.h"

namespace
{
// a gap rectangle with two non-empty sides: its request and where it lies
struct GapPiece {
    uint64_t request, tFrom, tLen, pFrom, pLen;
};
}  // namespace

int main(int argc, char **argv)
{
    const bool expectedOnly = check::takeExpected(argc, argv);
    if (argc < 3)
    {
        std::cout << "usage: sa_chains_check <n> <count> [seeds] [device]\n";
        return 2;
    }
    const uint64_t maxLen = std::max<uint64_t>(8, std::strtoull(argv[1], nullptr, 10));
    const uint64_t count = std::strtoull(argv[2], nullptr, 10);
    const uint64_t maxSeeds = argc > 3 ? std::max<uint64_t>(1, std::strtoull(argv[3], nullptr, 10)) : 6;
    const int device = argc > 4 ? std::atoi(argv[4]) : 0;
    const int gapOpen = 11, gapExtend = 2;
    std::vector<SequenceAlignment::Request> reqs(count), left(count), right(count);
    std::vector<GapPiece> pieces;
    std::vector<uint64_t> ts, ps, len, num(count), first(count);
    uint64_t seed = 97531;
    for (uint64_t i = 0; i < count; ++i)
    {
        SequenceAlignment::Request &r = reqs[i];
        check::scheme(r);
        r.textNumBytes = 1 + check::next(seed) % maxLen;
        r.textBytes = new char[r.textNumBytes];
        for (uint64_t x = 0; x < r.textNumBytes; ++x) r.textBytes[x] = (char)(check::next(seed) % 4);
        // the pattern: the text with substitutions, insertions and deletions, so that the path drifts
        std::vector<char> pat;
        std::vector<uint64_t> from;  // the text letter a pattern letter was copied from
        for (uint64_t x = 0; x < r.textNumBytes; ++x)
        {
            const uint64_t roll = check::next(seed) % 32;
            if (roll == 0) continue;  // a deletion
            pat.push_back(roll == 1 ? (char)(check::next(seed) % 4) : r.textBytes[x]);
            from.push_back(x);
            if (roll == 2)
            {
                pat.push_back((char)(check::next(seed) % 4));  // an insertion
                from.push_back(x);
            }
        }
        if (pat.empty())
        {
            pat.push_back(0);
            from.push_back(0);
        }
        r.patternNumBytes = pat.size();
        r.patternBytes = new char[pat.size()];
        std::memcpy(r.patternBytes, pat.data(), pat.size());
        // the chain: seeds at ascending pattern letters, each where its letter came from in the text
        first[i] = ts.size();
        const uint64_t want = 1 + check::next(seed) % maxSeeds;
        uint64_t te = 0, pe = 0;
        for (uint64_t k = 0; k < want; ++k)
        {
            const uint64_t kind = check::next(seed) % 6;
            uint64_t p0 = pe + (kind == 0 ? 0 : check::next(seed) % (1 + (pat.size() - pe) / (want - k)));
            if (p0 > pat.size()) break;
            uint64_t t0 = p0 < pat.size() ? from[p0] : r.textNumBytes;
            if (kind == 0 || t0 < te) t0 = te;               // adjacent on the text's side, or kept colinear
            if (kind == 1) p0 = pe;                          // a gap with an empty pattern side
            const uint64_t room = std::min(r.textNumBytes - t0, pat.size() - p0);
            const uint64_t L = kind == 2 ? 0 : check::next(seed) % (std::min<uint64_t>(room, 24) + 1);
            ts.push_back(t0);
            ps.push_back(p0);
            len.push_back(L);
            te = t0 + L;
            pe = p0 + L;
        }
        num[i] = ts.size() - first[i];
        const uint64_t a = first[i], z = ts.size() - 1;
        check::slice(left[i], r, 0, ts[a], 0, ps[a], true);
        check::slice(right[i], r, ts[z] + len[z], r.textNumBytes - ts[z] - len[z], ps[z] + len[z], r.patternNumBytes - ps[z] - len[z], false);
        for (uint64_t k = a; k < z; ++k)
        {
            const uint64_t t0 = ts[k] + len[k], p0 = ps[k] + len[k];
            if (ts[k + 1] > t0 && ps[k + 1] > p0) pieces.push_back(GapPiece{i, t0, ts[k + 1] - t0, p0, ps[k + 1] - p0});
        }
    }
    std::vector<SequenceAlignment::Request> gaps(pieces.size());  // a Request owns its letters: filled in place, never copied
    for (size_t k = 0; k < pieces.size(); ++k) check::slice(gaps[k], reqs[pieces[k].request], pieces[k].tFrom, pieces[k].tLen, pieces[k].pFrom, pieces[k].pLen, false);
    const int xdrops[2] = {20, SA_NO_XDROP};
    if (expectedOnly)
    {
        check::Digest sent;
        sent.requests(reqs);
        sent.numbers(num), sent.numbers(ts), sent.numbers(ps), sent.numbers(len);
        sent.requests(left), sent.requests(right), sent.requests(gaps);
        for (int xdrop : xdrops) sent.number(xdrop);
        return check::printExpected("sa_chains_check", argc, argv, sent, nullptr);
    }
    std::vector<SequenceAlignment::Response> respGaps(gaps.size());
    if (!gaps.empty() && SequenceAlignment::alignSequencesGPUAffine(gaps.data(), respGaps.data(), gaps.size(), device, gapOpen, gapExtend)) return 1;
    for (int xdrop : xdrops)
    {
        std::vector<SequenceAlignment::Response> resp(count), respLeft(count), respRight(count);
        std::vector<int> scores(count);
        if (SequenceAlignment::scoreSequencesGPUChains(reqs.data(), count, device, gapOpen, gapExtend, xdrop, num.data(), ts.data(), ps.data(),
                                                       len.data(), scores.data()))
            return 1;
        if (SequenceAlignment::alignSequencesGPUChains(reqs.data(), resp.data(), count, device, gapOpen, gapExtend, xdrop, num.data(), ts.data(),
                                                       ps.data(), len.data()))
            return 1;
        if (SequenceAlignment::alignSequencesGPUExtend(left.data(), respLeft.data(), count, device, gapOpen, gapExtend, xdrop)) return 1;
        if (SequenceAlignment::alignSequencesGPUExtend(right.data(), respRight.data(), count, device, gapOpen, gapExtend, xdrop)) return 1;
        size_t nextGap = 0;
        for (uint64_t i = 0; i < count; ++i)
        {
            const SequenceAlignment::Response &g = resp[i], &l = respLeft[i], &r = respRight[i];
            const char gapLetter = reqs[i].alphabet[reqs[i].alphabetSize];
            // the left extension backwards, then seeds and gaps in turn, then the right extension
            check::Expected want;
            uint64_t leftText, leftPattern;
            check::countLetters(l, gapLetter, leftText, leftPattern);
            check::appendStrings(want, l, true);
            want.score = l.score + r.score;
            for (uint64_t k = first[i]; k < first[i] + num[i]; ++k)
            {
                for (uint64_t q = 0; q < len[k]; ++q)
                {
                    const int ct = reqs[i].textBytes[ts[k] + q], cp = reqs[i].patternBytes[ps[k] + q];
                    want.score += check::blast[cp * 4 + ct];
                    want.text += reqs[i].alphabet[ct];
                    want.pattern += reqs[i].alphabet[cp];
                }
                if (k + 1 == first[i] + num[i]) break;
                const uint64_t t0 = ts[k] + len[k], p0 = ps[k] + len[k], gn = ts[k + 1] - t0, gm = ps[k + 1] - p0;
                if (gn && gm)
                {
                    const SequenceAlignment::Response &gr = respGaps[nextGap++];
                    want.score += gr.score;
                    check::appendStrings(want, gr, false);
                }
                else if (gn + gm)
                {
                    want.score -= gapOpen + ((int)(gn + gm) - 1) * gapExtend;
                    for (uint64_t q = 0; q < gn + gm; ++q)
                    {
                        want.text += gn ? reqs[i].alphabet[(int)reqs[i].textBytes[t0 + q]] : gapLetter;
                        want.pattern += gm ? reqs[i].alphabet[(int)reqs[i].patternBytes[p0 + q]] : gapLetter;
                    }
                }
            }
            check::appendStrings(want, r, false);
            want.startText = ts[first[i]] - leftText;
            want.startPattern = ps[first[i]] - leftPattern;
            const auto scorers = {check::Scored{"scoreSequencesGPUChains against alignSequencesGPUChains", scores[i], g.score}};
            if (const char *field = check::firstDifference(g, want, scorers))
                return check::reportDifference(i, reqs[i], std::to_string(num[i]) + " seeds from " + std::to_string(ts[first[i]]) + ":" +
                                                               std::to_string(ps[first[i]]) + ":" + std::to_string(len[first[i]]) + " at xdrop " +
                                                               std::to_string(xdrop),
                                               field, g, want, scorers);
        }
    }
    std::cout << "OK " << count << "\n";
    return 0;
}
