// sa_score_affine_check — a C++14 caller of the affine score-only extension: N DNA Requests of mixed
// sizes, scored with one SequenceAlignment::scoreSequencesGPUAffine call (gap open 11, gap extend 2)
// and, one by one, with the plain reference of check_ref.h; every score is compared.
//   usage: sa_score_affine_check global|local <requests> <max length> [device]
// Prints one JSON line {"requests", "mismatches", "gpu_us", "cpu_us"}; exit status 0 iff all equal.
// With --expected: the digests of the requests and of the reference's scores, and nothing of either library.
#include "check_ref.h"

int main(int argc, char **argv)
{
    const bool expectedOnly = check::takeExpected(argc, argv);
    if (argc < 4)
    {
        std::cerr << "usage: sa_score_affine_check global|local <requests> <max length> [device]\n";
        return 2;
    }
    const bool local = std::strcmp(argv[1], "local") == 0;
    const uint64_t count = std::strtoull(argv[2], nullptr, 10), maxLen = std::strtoull(argv[3], nullptr, 10);
    const int device = argc > 4 ? std::atoi(argv[4]) : 0;
    const int gapOpen = 11, gapExtend = 2;
    const check::Spec spec = local ? check::Spec::localMode(gapOpen, gapExtend) : check::Spec::global(gapOpen, gapExtend);
    std::vector<SequenceAlignment::Request> reqs(count);
    uint64_t seed = 13579;
    for (uint64_t i = 0; i < count; ++i)
    {
        SequenceAlignment::Request &r = reqs[i];
        check::scheme(r, local ? SequenceAlignment::programArgs::LOCAL : SequenceAlignment::programArgs::GLOBAL);
        r.textNumBytes = 1 + check::next(seed) % maxLen;
        r.patternNumBytes = 1 + check::next(seed) % r.textNumBytes;
        check::randomText(r, seed);
        // half the patterns are the text with substitutions and, now and then, a block of letters left
        // out, so long gaps pay; the others are random
        const bool related = (i & 1) == 0;
        check::relatedPattern(r, seed, 0, related ? r.patternNumBytes : 0, related, 12);
    }
    std::vector<int> gpu(count, 0), cpu(count, 0);
    const uint64_t t1 = check::nowUs();
    for (uint64_t i = 0; i < count; ++i) cpu[i] = check::score(reqs[i], spec);
    const uint64_t t2 = check::nowUs();
    if (expectedOnly)
    {
        check::Digest sent, want;
        sent.requests(reqs);
        want.numbers(cpu);
        return check::printExpected("sa_score_affine_check", argc, argv, sent, &want);
    }
    if (SequenceAlignment::scoreSequencesGPUAffine(reqs.data(), count, device, gapOpen, gapExtend, gpu.data())) return 1;
    const uint64_t t3 = check::nowUs();
    uint64_t bad = 0;
    for (uint64_t i = 0; i < count; ++i)
        if (gpu[i] != cpu[i] && bad++ < 3)
            std::cerr << "request " << i << " (" << reqs[i].textNumBytes << "x" << reqs[i].patternNumBytes
                      << "): gpu score " << gpu[i] << " cpu " << cpu[i] << "\n";
    return check::printMismatches(count, bad, t3 - t2, t2 - t1);
}
