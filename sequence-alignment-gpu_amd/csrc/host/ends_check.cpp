// sa_ends_check — a C++14 caller of scoreSequencesGPUEndsFree and alignSequencesGPUEndsFree (sa_hip.h:
// SA_ENDS_FREE, global alignment with free sequence ends): N DNA Requests of mixed sizes, request i
// under the flag set i % 16, so every call takes the requests of one flag set. Scores under the linear
// gap 5 (passed as gap open and gap extend) and under gap open 11 / gap extend 2, alignments under
// 11 / 2, each compared with the plain reference of check_ref.h under the same flags. In half the
// requests the end of the text is a mutated copy of the start of the pattern: two reads that overlap.
//   usage: sa_ends_check <max length> <requests> [device]
// Prints the first difference, or "OK <requests>" as its last line; exit status 0 iff all equal.
// With --expected: the digests of the requests and of the reference's results, and nothing of either library.
#include "check_ref.h"

int main(int argc, char **argv)
{
    const bool expectedOnly = check::takeExpected(argc, argv);
    if (argc < 3)
    {
        std::cerr << "usage: sa_ends_check <max length> <requests> [device]\n";
        return 2;
    }
    const uint64_t maxLen = std::max<uint64_t>(1, std::strtoull(argv[1], nullptr, 10)), count = std::strtoull(argv[2], nullptr, 10);
    const int device = argc > 3 ? std::atoi(argv[3]) : 0;
    const int gapLinear = 5, gapOpen = 11, gapExtend = 2;
    std::vector<SequenceAlignment::Request> reqs(count);
    std::vector<check::Expected> want(count);
    std::vector<int> wantLinear(count);
    uint64_t seed = 24680;
    for (uint64_t i = 0; i < count; ++i)
    {
        SequenceAlignment::Request &r = reqs[i];
        check::scheme(r, SequenceAlignment::programArgs::LOCAL);  // ignored by the ends-free functions
        r.patternNumBytes = 1 + check::next(seed) % maxLen;
        r.textNumBytes = 1 + check::next(seed) % maxLen;
        check::randomText(r, seed);
        for (uint64_t x = 0; x < r.patternNumBytes; ++x) r.patternBytes[x] = (char)(check::next(seed) % 4);
        // two overlapping reads: the last `over` letters of the text are the first letters of the
        // pattern with substitutions and, now and then, a letter left out
        if (((i / 16) & 1) == 0)
        {
            const uint64_t over = 1 + check::next(seed) % std::min(r.textNumBytes, r.patternNumBytes);
            uint64_t src = 0;
            for (uint64_t x = r.textNumBytes - over; x < r.textNumBytes && src < r.patternNumBytes; ++x, ++src)
            {
                if (check::next(seed) % 48 == 0) ++src;
                if (src < r.patternNumBytes && check::next(seed) % 10) r.textBytes[x] = r.patternBytes[src];
            }
        }
        wantLinear[i] = check::score(r, check::Spec::endsFree((int)(i % 16), gapLinear, gapLinear));
        want[i] = check::align(r, check::Spec::endsFree((int)(i % 16), gapOpen, gapExtend));
    }
    // the calls, one per flag set: the requests in the order they are sent, and what is expected of them
    std::vector<std::vector<uint64_t>> ids(16);
    check::Digest sent, wanted;
    for (int flags = 0; flags < 16; ++flags)
    {
        for (uint64_t i = (uint64_t)flags; i < count; i += 16) ids[flags].push_back(i);
        if (ids[flags].empty()) continue;
        sent.number(flags);
        sent.number((int64_t)ids[flags].size());
        for (uint64_t i : ids[flags])
        {
            sent.request(reqs[i]);
            wanted.number(wantLinear[i]);
            wanted.expected(want[i]);
        }
    }
    if (expectedOnly) return check::printExpected("sa_ends_check", argc, argv, sent, &wanted);
    for (int flags = 0; flags < 16; ++flags)
    {
        const size_t num = ids[flags].size();
        if (!num) continue;
        std::vector<SequenceAlignment::Request> sub(num);
        for (size_t q = 0; q < num; ++q) sub[q] = reqs[ids[flags][q]];
        std::vector<SequenceAlignment::Response> resp(num);
        std::vector<int> linear(num), affine(num);
        bool failed = SequenceAlignment::scoreSequencesGPUEndsFree(sub.data(), sub.size(), device, gapLinear, gapLinear, flags, linear.data()) ||
                      SequenceAlignment::scoreSequencesGPUEndsFree(sub.data(), sub.size(), device, gapOpen, gapExtend, flags, affine.data()) ||
                      SequenceAlignment::alignSequencesGPUEndsFree(sub.data(), resp.data(), sub.size(), device, gapOpen, gapExtend, flags);
        for (size_t q = 0; q < num && !failed; ++q)
        {
            const uint64_t i = ids[flags][q];
            const auto scorers = {check::Scored{"scoreSequencesGPUEndsFree (linear)", linear[q], wantLinear[i]},
                                  check::Scored{"scoreSequencesGPUEndsFree", affine[q], want[i].score}};
            if (const char *field = check::firstDifference(resp[q], want[i], scorers))
                failed = check::reportDifference(i, reqs[i], "flags " + std::to_string(flags), field, resp[q], want[i], scorers);
        }
        // the copies in `sub` share the originals' sequences: they must not release them
        for (SequenceAlignment::Request &rq : sub) rq.textBytes = rq.patternBytes = nullptr;
        if (failed) return 1;
    }
    std::cout << "OK " << count << "\n";
    return 0;
}
