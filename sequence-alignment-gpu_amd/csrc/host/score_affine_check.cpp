// sa_score_affine_check — a C++14 caller of the affine score-only extension: N DNA Requests of mixed
// sizes, scored with one SequenceAlignment::scoreSequencesGPUAffine call (gap open 11, gap extend 2)
// and, one by one, with the plain Gotoh loop below; every score is compared.
//   usage: sa_score_affine_check global|local <requests> <max length> [device]
// Prints one JSON line {"requests", "mismatches", "gpu_us", "cpu_us"}; exit status 0 iff all equal.
#include <sys/time.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "SequenceAlignment.hpp"

namespace
{
uint64_t now_us()
{
    timeval t;
    gettimeofday(&t, nullptr);
    return 1000000ull * (uint64_t)t.tv_sec + (uint64_t)t.tv_usec;
}

uint64_t next(uint64_t &s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return s >> 33;
}

// Gotoh's recurrence row by row; E and F of the borders are minus infinity (a value no score reaches)
int gotoh(const SequenceAlignment::Request &r, bool local, int go, int ge)
{
    const int64_t n = (int64_t)r.textNumBytes, m = (int64_t)r.patternNumBytes, NEG = -(1ll << 40);
    std::vector<int64_t> H(n + 1), F(n + 1, NEG);
    H[0] = 0;
    for (int64_t j = 1; j <= n; ++j) H[j] = local ? 0 : -(go + (j - 1) * (int64_t)ge);
    int64_t best = 0;
    for (int64_t i = 1; i <= m; ++i)
    {
        int64_t diag = H[0], E = NEG;
        H[0] = local ? 0 : -(go + (i - 1) * (int64_t)ge);
        for (int64_t j = 1; j <= n; ++j)
        {
            E = std::max(E - ge, H[j - 1] - go);
            F[j] = std::max(F[j] - ge, H[j] - go);
            int64_t h = diag + r.scoreMatrix[r.patternBytes[i - 1] * r.alphabetSize + r.textBytes[j - 1]];
            h = std::max(h, std::max(E, F[j]));
            if (local) h = std::max<int64_t>(h, 0);
            diag = H[j];
            H[j] = h;
            best = std::max(best, h);
        }
    }
    return (int)(local ? best : H[n]);
}
}  // namespace

int main(int argc, const char *argv[])
{
    if (argc < 4)
    {
        std::cerr << "usage: sa_score_affine_check global|local <requests> <max length> [device]\n";
        return 2;
    }
    const bool local = std::strcmp(argv[1], "local") == 0;
    const uint64_t count = std::strtoull(argv[2], nullptr, 10), maxLen = std::strtoull(argv[3], nullptr, 10);
    const int device = argc > 4 ? std::atoi(argv[4]) : 0;
    const int gapOpen = 11, gapExtend = 2;
    static const int blast[16] = {5, -4, -4, -4, -4, 5, -4, -4, -4, -4, 5, -4, -4, -4, -4, 5};
    std::vector<SequenceAlignment::Request> reqs(count);
    uint64_t seed = 13579;
    for (uint64_t i = 0; i < count; ++i)
    {
        SequenceAlignment::Request &r = reqs[i];
        r.deviceType = SequenceAlignment::programArgs::GPU;
        r.sequenceType = SequenceAlignment::programArgs::DNA;
        r.alignmentType = local ? SequenceAlignment::programArgs::LOCAL : SequenceAlignment::programArgs::GLOBAL;
        r.alphabet = SequenceAlignment::DNA_ALPHABET;
        r.alphabetSize = SequenceAlignment::NUM_DNA_CHARS;
        r.gapPenalty = 5;  // ignored by the affine call
        std::memcpy(r.scoreMatrix, blast, sizeof(blast));
        r.textNumBytes = 1 + next(seed) % maxLen;
        r.patternNumBytes = 1 + next(seed) % r.textNumBytes;
        r.textBytes = new char[r.textNumBytes];
        r.patternBytes = new char[r.patternNumBytes];
        for (uint64_t x = 0; x < r.textNumBytes; ++x) r.textBytes[x] = (char)(next(seed) % 4);
        // half the patterns are the text with substitutions and, now and then, a block of letters left
        // out, so long gaps pay; the others are random
        const bool related = (i & 1) == 0;
        uint64_t src = 0;
        for (uint64_t x = 0; x < r.patternNumBytes; ++x, ++src)
        {
            if (related && next(seed) % 64 == 0) src += next(seed) % 12;
            r.patternBytes[x] = related && src < r.textNumBytes && next(seed) % 8 ? r.textBytes[src] : (char)(next(seed) % 4);
        }
    }
    std::vector<int> gpu(count, 0), cpu(count, 0);
    const uint64_t t0 = now_us();
    if (SequenceAlignment::scoreSequencesGPUAffine(reqs.data(), count, device, gapOpen, gapExtend, gpu.data())) return 1;
    const uint64_t t1 = now_us();
    for (uint64_t i = 0; i < count; ++i) cpu[i] = gotoh(reqs[i], local, gapOpen, gapExtend);
    const uint64_t t2 = now_us();
    uint64_t bad = 0;
    for (uint64_t i = 0; i < count; ++i)
        if (gpu[i] != cpu[i] && bad++ < 3)
            std::cerr << "request " << i << " (" << reqs[i].textNumBytes << "x" << reqs[i].patternNumBytes
                      << "): gpu score " << gpu[i] << " cpu " << cpu[i] << "\n";
    std::cout << "{\"requests\": " << count << ", \"mismatches\": " << bad << ", \"gpu_us\": " << (t1 - t0)
              << ", \"cpu_us\": " << (t2 - t1) << "}\n";
    return bad ? 1 : 0;
}
