// sa_cigar_check — a C++14 caller of the CIGAR output (sa_hip.h sa_align_pairs_cigar): <count> DNA Requests of up to
// <n> letters a side, the pattern a mutated copy of the text, through SequenceAlignment::alignSequencesGPUCigar as
// the affine aligner (global and local), the banded aligner, the extension aligner, the seeds aligner (a seed on the
// main diagonal) and the chains aligner (two such seeds), gap open 11 and gap extend 2, under SA_CIGAR_EQX and
// SA_CIGAR_M. Identity G1 of sa_hip.h is checked against the library's own functions: the ops and the counts must be
// sa_cigar_from_strings of the two strings that the align...GPU... function of the same variant returns, and the
// score, the length and the two starts must be that function's.
//   usage: sa_cigar_check <n> <count> [device]
// Prints the first difference, or "OK <count>" as its last line; exit status 0 iff all equal.
// With --expected: the digest of the requests, seeds and chains (check_ref.h) and nothing of either library.
#include "check_ref.h"

namespace
{
sa_align_spec plain(int gapOpen, int gapExtend)
{
    sa_align_spec s;
    s.gap_open = gapOpen;
    s.gap_extend = gapExtend;
    s.band = s.width = -1;
    s.xdrop = SA_NO_XDROP;
    s.extend = 0;
    s.bands = nullptr;
    s.seeds = nullptr;
    s.chain_off = nullptr;
    return s;
}
}  // namespace

int main(int argc, char **argv)
{
    const bool expectedOnly = check::takeExpected(argc, argv);
    if (argc < 3)
    {
        std::cout << "usage: sa_cigar_check <n> <count> [device]\n";
        return 2;
    }
    const uint64_t maxLen = std::max<uint64_t>(8, std::strtoull(argv[1], nullptr, 10));
    const uint64_t count = std::strtoull(argv[2], nullptr, 10);
    const int device = argc > 3 ? std::atoi(argv[3]) : 0;
    const int gapOpen = 11, gapExtend = 2, xdrop = 40, band = 24;
    std::vector<SequenceAlignment::Request> reqs(count);
    std::vector<uint64_t> ts, ps, len, num(count, 2), one(count, 0);
    std::vector<sa_seed> seeds(count), chain;
    std::vector<uint64_t> chainOff(count + 1, 0);
    uint64_t seed = 24681357;
    for (uint64_t i = 0; i < count; ++i)
    {
        SequenceAlignment::Request &r = reqs[i];
        check::scheme(r);
        r.textNumBytes = 1 + check::next(seed) % maxLen;
        r.textBytes = new char[r.textNumBytes];
        for (uint64_t x = 0; x < r.textNumBytes; ++x) r.textBytes[x] = (char)(check::next(seed) % 4);
        std::vector<char> pat;
        for (uint64_t x = 0; x < r.textNumBytes; ++x)
        {
            const uint64_t roll = check::next(seed) % 24;
            if (roll == 0) continue;  // a deletion
            pat.push_back(roll == 1 ? (char)(check::next(seed) % 4) : r.textBytes[x]);
            if (roll == 2) pat.push_back((char)(check::next(seed) % 4));  // an insertion
        }
        if (pat.empty()) pat.push_back(0);
        r.patternNumBytes = pat.size();
        r.patternBytes = new char[pat.size()];
        std::memcpy(r.patternBytes, pat.data(), pat.size());
        // two seeds on the main diagonal, in the first and in the second half of the shorter side
        const uint64_t side = std::min<uint64_t>(r.textNumBytes, r.patternNumBytes), half = side / 2;
        const uint64_t a = check::next(seed) % (half + 1), la = check::next(seed) % (half - a + 1);
        const uint64_t b = half + check::next(seed) % (side - half + 1), lb = check::next(seed) % (side - b + 1);
        seeds[i] = sa_seed{a, a, la};
        chain.push_back(sa_seed{a, a, la});
        chain.push_back(sa_seed{b, b, lb});
        chainOff[i + 1] = chain.size();
        ts.push_back(a), ps.push_back(a), len.push_back(la);
        ts.push_back(b), ps.push_back(b), len.push_back(lb);
    }
    std::vector<uint64_t> sts(count), sps(count), slen(count);
    for (uint64_t i = 0; i < count; ++i) sts[i] = seeds[i].text_pos, sps[i] = seeds[i].pattern_pos, slen[i] = seeds[i].length;

    if (expectedOnly)
    {
        check::Digest sent;
        sent.requests(reqs);
        sent.numbers(sts), sent.numbers(sps), sent.numbers(slen);
        sent.numbers(num), sent.numbers(ts), sent.numbers(ps), sent.numbers(len), sent.numbers(chainOff);
        sent.number(xdrop), sent.number(band);
        return check::printExpected("sa_cigar_check", argc, argv, sent, nullptr);
    }
    const char *names[6] = {"affine global", "affine local", "banded", "extend", "seeds", "chains"};
    for (int variant = 0; variant < 6; ++variant)
    {
        for (uint64_t i = 0; i < count; ++i)
            reqs[i].alignmentType = variant == 1 ? SequenceAlignment::programArgs::LOCAL : SequenceAlignment::programArgs::GLOBAL;
        std::vector<SequenceAlignment::Response> resp(count);
        sa_align_spec spec = plain(gapOpen, gapExtend);
        uint64_t failed = 0;
        switch (variant)
        {
        case 0:
        case 1:
            failed = SequenceAlignment::alignSequencesGPUAffine(reqs.data(), resp.data(), count, device, gapOpen, gapExtend);
            break;
        case 2:
            spec.band = band;
            failed = SequenceAlignment::alignSequencesGPUBanded(reqs.data(), resp.data(), count, device, gapOpen, gapExtend, band);
            break;
        case 3:
            spec.extend = 1, spec.xdrop = xdrop;
            failed = SequenceAlignment::alignSequencesGPUExtend(reqs.data(), resp.data(), count, device, gapOpen, gapExtend, xdrop);
            break;
        case 4:
            spec.extend = 1, spec.xdrop = xdrop, spec.seeds = seeds.data();
            failed = SequenceAlignment::alignSequencesGPUSeeds(reqs.data(), resp.data(), count, device, gapOpen, gapExtend, xdrop, sts.data(),
                                                               sps.data(), slen.data());
            break;
        default:
            spec.extend = 1, spec.xdrop = xdrop, spec.seeds = chain.data(), spec.chain_off = chainOff.data();
            failed = SequenceAlignment::alignSequencesGPUChains(reqs.data(), resp.data(), count, device, gapOpen, gapExtend, xdrop, num.data(),
                                                                ts.data(), ps.data(), len.data());
        }
        if (failed) return 1;
        for (int eqx = 0; eqx < 2; ++eqx)
        {
            std::vector<SequenceAlignment::CigarResponse> got(count);
            if (SequenceAlignment::alignSequencesGPUCigar(reqs.data(), got.data(), count, device, spec, eqx != 0)) return 1;
            for (uint64_t i = 0; i < count; ++i)
            {
                const SequenceAlignment::Response &w = resp[i];
                const SequenceAlignment::CigarResponse &g = got[i];
                std::vector<uint32_t> ops(std::max<uint64_t>(w.numAlignmentBytes, 1));
                sa_cigar_result want;
                if (sa_cigar_from_strings(w.alignedTextBytes, w.alignedPatternBytes, w.numAlignmentBytes, reqs[i].alphabet[reqs[i].alphabetSize],
                                          eqx ? SA_CIGAR_EQX : SA_CIGAR_M, ops.data(), ops.size(), &want) != SA_OK)
                {
                    std::cout << "error: " << sa_last_error() << "\n";
                    return 1;
                }
                ops.resize(want.num_ops);
                const char *field = nullptr;
                if (g.score != w.score) field = "score";
                else if (g.numAlignmentBytes != w.numAlignmentBytes) field = "numAlignmentBytes";
                else if (g.startInAlignedText != w.startInAlignedText || g.startInAlignedPattern != w.startInAlignedPattern) field = "a start";
                else if (g.ops != ops) field = "the ops";
                else if (g.matches != want.matches || g.mismatches != want.mismatches) field = "matches or mismatches";
                else if (g.textGapLetters != want.text_gap_letters || g.patternGapLetters != want.pattern_gap_letters) field = "a gap letter count";
                else if (g.gapOpens != want.gap_opens) field = "gapOpens";
                else if ((uint64_t)g.matches + g.mismatches + g.textGapLetters + g.patternGapLetters != g.numAlignmentBytes) field = "the sum of the counts";
                if (field)
                {
                    std::cout << "request " << i << " (" << reqs[i].textNumBytes << "x" << reqs[i].patternNumBytes << ") as " << names[variant]
                              << (eqx ? " under SA_CIGAR_EQX" : " under SA_CIGAR_M") << ": " << field << " differs: " << g.ops.size()
                              << " ops against " << ops.size() << " from the strings of " << w.numAlignmentBytes << " columns\n";
                    return 1;
                }
            }
        }
    }
    std::cout << "OK " << count << "\n";
    return 0;
}
