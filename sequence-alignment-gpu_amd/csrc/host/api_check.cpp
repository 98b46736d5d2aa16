// sa_api_check — a C++14 caller of the batch extension: N DNA Requests of mixed sizes (text at least
// as long as the pattern, as parseArguments guarantees, utilities.cpp:225-230), aligned with one
// SequenceAlignment::alignSequenceGPUBatch call over G GPUs and, one by one, with the reference
// semantics of alignSequenceCPU; every Response field and both strings compared.
//   usage: sa_api_check global|local <requests> <max length> <gpus>
// Prints one JSON line {"requests", "mismatches", "gpu_us", "cpu_us"}; exit status 0 iff all equal.
// With --expected: the digest of the requests (check_ref.h) and nothing of either library.
#include "check_ref.h"

int main(int argc, char **argv)
{
    const bool expectedOnly = check::takeExpected(argc, argv);
    if (argc < 5)
    {
        std::cerr << "usage: sa_api_check global|local <requests> <max length> <gpus>\n";
        return 2;
    }
    const bool local = std::strcmp(argv[1], "local") == 0;
    const uint64_t count = std::strtoull(argv[2], nullptr, 10), maxLen = std::strtoull(argv[3], nullptr, 10);
    const int gpus = std::atoi(argv[4]);
    std::vector<SequenceAlignment::Request> reqs(count);
    uint64_t seed = 12345;
    for (uint64_t i = 0; i < count; ++i)
    {
        SequenceAlignment::Request &r = reqs[i];
        check::scheme(r, local ? SequenceAlignment::programArgs::LOCAL : SequenceAlignment::programArgs::GLOBAL);
        r.textNumBytes = 1 + check::next(seed) % maxLen;
        r.patternNumBytes = 1 + check::next(seed) % r.textNumBytes;
        check::randomText(r, seed);
        // half the patterns are copies of the text with substitutions, so alignments are long
        check::relatedPattern(r, seed, 0, i & 1 ? 0 : r.patternNumBytes, false, 0);
    }
    if (expectedOnly)
    {
        check::Digest sent;
        sent.requests(reqs);
        return check::printExpected("sa_api_check", argc, argv, sent, nullptr);
    }
    std::vector<SequenceAlignment::Response> gpu(count), cpu(count);
    const uint64_t t0 = check::nowUs();
    if (SequenceAlignment::alignSequenceGPUBatch(reqs.data(), gpu.data(), count, gpus)) return 1;
    const uint64_t t1 = check::nowUs();
    for (uint64_t i = 0; i < count; ++i)
        if (SequenceAlignment::alignSequenceCPU(reqs[i], &cpu[i])) return 1;
    const uint64_t t2 = check::nowUs();
    uint64_t bad = 0;
    for (uint64_t i = 0; i < count; ++i)
        if (check::firstDifference(gpu[i], check::expectedOf(cpu[i])) && bad++ < 3)
            std::cerr << "request " << i << " (" << reqs[i].textNumBytes << "x" << reqs[i].patternNumBytes
                      << "): gpu score " << gpu[i].score << " cpu " << cpu[i].score << "\n";
    return check::printMismatches(count, bad, t1 - t0, t2 - t1);
}
