// sa_fit_check — a C++14 caller of the three functions that take SEMI_GLOBAL (sa_hip.h: SA_FIT, the
// whole pattern inside the text, the text free at both ends): N DNA Requests of mixed sizes through
// scoreSequencesGPU (linear gap 5), scoreSequencesGPUAffine and alignSequencesGPUAffine (gap open 11,
// gap extend 2), each compared with the plain reference of check_ref.h under the free text ends. Texts
// are a few times longer than the patterns; half the patterns are a mutated piece of their text.
//   usage: sa_fit_check <max pattern length> <requests> [device]
// Prints the first difference, or "OK <requests>" as its last line; exit status 0 iff all equal.
// With --expected: the digests of the requests and of the reference's results, and nothing of either library.
#include "check_ref.h"

int main(int argc, char **argv)
{
    const bool expectedOnly = check::takeExpected(argc, argv);
    if (argc < 3)
    {
        std::cerr << "usage: sa_fit_check <max pattern length> <requests> [device]\n";
        return 2;
    }
    const uint64_t maxLen = std::max<uint64_t>(1, std::strtoull(argv[1], nullptr, 10)), count = std::strtoull(argv[2], nullptr, 10);
    const int device = argc > 3 ? std::atoi(argv[3]) : 0;
    const int gapLinear = 5, gapOpen = 11, gapExtend = 2;
    std::vector<SequenceAlignment::Request> reqs(count);
    std::vector<SequenceAlignment::Response> resp(count);
    std::vector<check::Expected> want(count);
    std::vector<int> wantLinear(count);
    check::Digest sent, wanted;
    uint64_t seed = 13579;
    for (uint64_t i = 0; i < count; ++i)
    {
        SequenceAlignment::Request &r = reqs[i];
        check::scheme(r, SequenceAlignment::programArgs::SEMI_GLOBAL);
        r.patternNumBytes = 1 + check::next(seed) % maxLen;
        r.textNumBytes = 1 + check::next(seed) % (4 * maxLen);
        check::randomText(r, seed);
        // half the patterns are a piece of the text with substitutions and, now and then, a block of
        // letters left out, so long gaps pay; the others are random
        const bool related = (i & 1) == 0;
        const uint64_t src = check::next(seed) % r.textNumBytes;
        check::relatedPattern(r, seed, src, related ? r.patternNumBytes : 0, related, 12);
        wantLinear[i] = check::score(r, check::Spec::fit(gapLinear, gapLinear));
        want[i] = check::align(r, check::Spec::fit(gapOpen, gapExtend));
        want[i].startPattern = 0;  // what a fit promises, whatever cell the reference's walk ends in
        wanted.number(wantLinear[i]);
        wanted.expected(want[i]);
    }
    sent.requests(reqs);
    if (expectedOnly) return check::printExpected("sa_fit_check", argc, argv, sent, &wanted);
    std::vector<int> linear(count), affine(count);
    if (SequenceAlignment::scoreSequencesGPU(reqs.data(), count, device, linear.data())) return 1;
    if (SequenceAlignment::scoreSequencesGPUAffine(reqs.data(), count, device, gapOpen, gapExtend, affine.data())) return 1;
    if (SequenceAlignment::alignSequencesGPUAffine(reqs.data(), resp.data(), count, device, gapOpen, gapExtend)) return 1;
    for (uint64_t i = 0; i < count; ++i)
    {
        const auto scorers = {check::Scored{"scoreSequencesGPU", linear[i], wantLinear[i]},
                              check::Scored{"scoreSequencesGPUAffine", affine[i], want[i].score}};
        if (const char *field = check::firstDifference(resp[i], want[i], scorers))
            return check::reportDifference(i, reqs[i], "", field, resp[i], want[i], scorers);
    }
    std::cout << "OK " << count << "\n";
    return 0;
}
