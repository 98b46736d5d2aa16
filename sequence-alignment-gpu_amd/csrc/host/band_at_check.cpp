// sa_band_at_check — a C++14 caller of the band-at extension (sa_hip.h: request k counts cell (i, j) iff
// bandLo[k] <= j - i <= bandHi[k]): 48 DNA Requests, each a read of up to <m> letters cut from a text up
// to 300 letters longer at letter c, through SequenceAlignment::scoreSequencesGPUBandAt and
// alignSequencesGPUBandAt (gap open 11, gap extend 2) and, one by one, through the plain reference of
// check_ref.h inside the same band; the score and every Response field are
// compared. The bands are {c - w, c + w} (fit, overlap, local) and {-w - k % 3, n - m + w + k % 5}
// (global: the origin and the end cell must be in band). A last call with the bands {-m, n} must equal
// the unbanded function of the mode.
//   usage: sa_band_at_check global|local|fit|overlap <m> <w> [device]
// Prints the first difference, or "OK <w>" as its last line; exit status 0 iff all equal.
// With --expected: the digests of the requests and of the reference's results, and nothing of either library.
#include "check_ref.h"

int main(int argc, char **argv)
{
    const bool expectedOnly = check::takeExpected(argc, argv);
    const std::string mode = argc > 1 ? argv[1] : "";
    if (argc < 4 || (mode != "global" && mode != "local" && mode != "fit" && mode != "overlap"))
    {
        std::cerr << "usage: sa_band_at_check global|local|fit|overlap <m> <w> [device]\n";
        return 2;
    }
    const bool local = mode == "local";
    // the mode argument of the C++ functions: -1 reads Request::alignmentType, else the free ends
    const int freeEnds = mode == "overlap" ? 15 : -1;
    const uint64_t maxLen = std::max<uint64_t>(1, std::strtoull(argv[2], nullptr, 10)), count = 48;
    const int w = std::atoi(argv[3]);
    const int device = argc > 4 ? std::atoi(argv[4]) : 0;
    const int gapOpen = 11, gapExtend = 2;
    const check::Spec spec = local             ? check::Spec::localMode(gapOpen, gapExtend)
                             : mode == "fit"   ? check::Spec::fit(gapOpen, gapExtend)
                             : freeEnds >= 0   ? check::Spec::endsFree(freeEnds, gapOpen, gapExtend)
                                               : check::Spec::global(gapOpen, gapExtend);
    std::vector<SequenceAlignment::Request> reqs(count);
    std::vector<SequenceAlignment::Response> resp(count), respFull(count), respUnbanded(count);
    std::vector<check::Expected> want(count);
    std::vector<int> lo(count), hi(count), loFull(count), hiFull(count);
    check::Digest sent, wanted;
    uint64_t seed = 86420;
    for (uint64_t i = 0; i < count; ++i)
    {
        SequenceAlignment::Request &r = reqs[i];
        check::scheme(r, local ? SequenceAlignment::programArgs::LOCAL
                         : mode == "fit" ? SequenceAlignment::programArgs::SEMI_GLOBAL
                                         : SequenceAlignment::programArgs::GLOBAL);
        r.patternNumBytes = 1 + check::next(seed) % maxLen;
        const uint64_t extra = check::next(seed) % 301, c = check::next(seed) % (extra + 1);
        r.textNumBytes = r.patternNumBytes + extra;
        check::randomText(r, seed);
        // the read: the text from letter c on with substitutions and, now and then, a few letters left out
        check::relatedPattern(r, seed, c, r.patternNumBytes, true, 4);
        if (mode == "global") lo[i] = -w - (int)(i % 3), hi[i] = (int)extra + w + (int)(i % 5);
        else lo[i] = (int)c - w, hi[i] = (int)c + w;
        loFull[i] = -(int)r.patternNumBytes;
        hiFull[i] = (int)r.textNumBytes;
        want[i] = check::align(r, spec.bandAt(lo[i], hi[i]));
        wanted.expected(want[i]);
    }
    sent.requests(reqs);
    sent.number(freeEnds);
    sent.numbers(lo), sent.numbers(hi), sent.numbers(loFull), sent.numbers(hiFull);
    if (expectedOnly) return check::printExpected("sa_band_at_check", argc, argv, sent, &wanted);
    for (uint64_t i = 0; i < count; ++i)
        if (sa_band_reachable(local ? SA_LOCAL : spec.ends < 0 ? SA_GLOBAL : SA_ENDS_FREE | spec.ends, reqs[i].textNumBytes,
                              reqs[i].patternNumBytes, sa_band{lo[i], hi[i]}) != 1)
        {
            std::cout << "request " << i << ": its band [" << lo[i] << ", " << hi[i] << "] admits no alignment\n";
            return 1;
        }
    std::vector<int> scores(count), full(count), unbanded(count);
    if (SequenceAlignment::scoreSequencesGPUBandAt(reqs.data(), count, device, gapOpen, gapExtend, freeEnds, lo.data(), hi.data(), scores.data())) return 1;
    if (SequenceAlignment::alignSequencesGPUBandAt(reqs.data(), resp.data(), count, device, gapOpen, gapExtend, freeEnds, lo.data(), hi.data())) return 1;
    if (SequenceAlignment::scoreSequencesGPUBandAt(reqs.data(), count, device, gapOpen, gapExtend, freeEnds, loFull.data(), hiFull.data(), full.data())) return 1;
    if (SequenceAlignment::alignSequencesGPUBandAt(reqs.data(), respFull.data(), count, device, gapOpen, gapExtend, freeEnds, loFull.data(), hiFull.data())) return 1;
    if (freeEnds >= 0)
    {
        if (SequenceAlignment::scoreSequencesGPUEndsFree(reqs.data(), count, device, gapOpen, gapExtend, freeEnds, unbanded.data())) return 1;
        if (SequenceAlignment::alignSequencesGPUEndsFree(reqs.data(), respUnbanded.data(), count, device, gapOpen, gapExtend, freeEnds)) return 1;
    }
    else
    {
        if (SequenceAlignment::scoreSequencesGPUAffine(reqs.data(), count, device, gapOpen, gapExtend, unbanded.data())) return 1;
        if (SequenceAlignment::alignSequencesGPUAffine(reqs.data(), respUnbanded.data(), count, device, gapOpen, gapExtend)) return 1;
    }
    for (uint64_t i = 0; i < count; ++i)
    {
        const auto scorers = {check::Scored{"scoreSequencesGPUBandAt", scores[i], want[i].score},
                              check::Scored{"scoreSequencesGPUBandAt with every cell in band", full[i], unbanded[i]}};
        const char *field = check::firstDifference(resp[i], want[i], scorers);
        if (!field && check::firstDifference(respFull[i], check::expectedOf(respUnbanded[i])))
            field = "alignSequencesGPUBandAt with every cell in band";
        if (field)
            return check::reportDifference(i, reqs[i], "band [" + std::to_string(lo[i]) + ", " + std::to_string(hi[i]) + "]", field, resp[i],
                                           want[i], scorers);
    }
    std::cout << "OK " << w << "\n";
    return 0;
}
