// sa_align_affine_check — a C++14 caller of the affine alignment extension: N DNA Requests of mixed
// sizes, aligned with one SequenceAlignment::alignSequencesGPUAffine call (gap open 11, gap extend 2)
// and, one by one, with the plain reference of check_ref.h; every Response field is
// compared.
//   usage: sa_align_affine_check global|local <max length> <requests> [device]
// Prints the first difference, or "OK <requests>" as its last line; exit status 0 iff all equal.
// With --expected: the digests of the requests and of the reference's results, and nothing of either library.
#include "check_ref.h"

int main(int argc, char **argv)
{
    const bool expectedOnly = check::takeExpected(argc, argv);
    if (argc < 4)
    {
        std::cerr << "usage: sa_align_affine_check global|local <max length> <requests> [device]\n";
        return 2;
    }
    const bool local = std::strcmp(argv[1], "local") == 0;
    const uint64_t maxLen = std::max<uint64_t>(1, std::strtoull(argv[2], nullptr, 10)), count = std::strtoull(argv[3], nullptr, 10);
    const int device = argc > 4 ? std::atoi(argv[4]) : 0;
    const int gapOpen = 11, gapExtend = 2;
    const check::Spec spec = local ? check::Spec::localMode(gapOpen, gapExtend) : check::Spec::global(gapOpen, gapExtend);
    std::vector<SequenceAlignment::Request> reqs(count);
    std::vector<SequenceAlignment::Response> resp(count);
    std::vector<check::Expected> want(count);
    check::Digest sent, wanted;
    uint64_t seed = 24680;
    for (uint64_t i = 0; i < count; ++i)
    {
        SequenceAlignment::Request &r = reqs[i];
        check::scheme(r, local ? SequenceAlignment::programArgs::LOCAL : SequenceAlignment::programArgs::GLOBAL);
        r.textNumBytes = 1 + check::next(seed) % maxLen;
        r.patternNumBytes = 1 + check::next(seed) % maxLen;
        check::randomText(r, seed);
        // half the patterns are the text with substitutions and, now and then, a block of letters left
        // out, so long gaps pay; the others are random
        const bool related = (i & 1) == 0;
        check::relatedPattern(r, seed, 0, related ? r.patternNumBytes : 0, related, 12);
        want[i] = check::align(r, spec);
        wanted.expected(want[i]);
    }
    sent.requests(reqs);
    if (expectedOnly) return check::printExpected("sa_align_affine_check", argc, argv, sent, &wanted);
    if (SequenceAlignment::alignSequencesGPUAffine(reqs.data(), resp.data(), count, device, gapOpen, gapExtend)) return 1;
    for (uint64_t i = 0; i < count; ++i)
        if (const char *field = check::firstDifference(resp[i], want[i])) return check::reportDifference(i, reqs[i], "", field, resp[i], want[i]);
    std::cout << "OK " << count << "\n";
    return 0;
}
