// bin/sa_plan_check: the host planner (sa_plan.cpp) as a stand-alone program. No GPU, no ROCm: it
// plans the pair shapes on its command line for a device of a given CU count, under the knobs of
// its environment (the library's own reader), and prints the plan as one JSON object
// (tests/test_plan.py).
//   sa_plan_check --mode global|local|<int> --alphabet A --gap G --matrix blast|blosum50|unit --cus N
//                 [--matrices tests/golden/matrices.json] [--rows-per-lane R] [--strips] NxM[xCOUNT] ...
// NxM is text length x pattern length. A planning error prints {"error": code, "message": text}.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "sa_plan.h"

using namespace sa;

static_assert(sizeof(PairDesc) == 72 && sizeof(StripDesc) == 40, "descriptors without padding: the hash reads raw bytes");

namespace {

int usage(const char *msg)
{
    std::fprintf(stderr, "sa_plan_check: %s\n", msg);
    return 2;
}

// The A x A list of `name` in the golden matrices file ({"name": [v, v, ...], ...}).
bool read_matrix(const std::string &path, const std::string &name, std::vector<int32_t> *out)
{
    std::ifstream f(path);
    if (!f) return false;
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string s = ss.str();
    size_t p = s.find("\"" + name + "\"");
    if (p == std::string::npos || (p = s.find('[', p)) == std::string::npos) return false;
    const size_t end = s.find(']', p);
    if (end == std::string::npos) return false;
    const char *c = s.c_str() + p + 1, *stop = s.c_str() + end;
    while (c < stop)
    {
        char *next = nullptr;
        const long v = std::strtol(c, &next, 10);
        if (next == c) break;
        out->push_back((int32_t)v);
        c = next;
        while (c < stop && (*c == ',' || *c == ' ' || *c == '\n')) ++c;
    }
    return !out->empty();
}

uint64_t fnv1a(uint64_t h, const void *data, size_t bytes)
{
    const unsigned char *b = (const unsigned char *)data;
    for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

void print_strips(const char *key, const std::vector<StripDesc> &v)
{
    std::printf(", \"%s\": [", key);
    for (size_t i = 0; i < v.size(); ++i)
        std::printf("%s{\"pair\": %d, \"row0\": %d, \"flags\": %d, \"nsteps\": %d, \"mask_off\": %llu, \"bnd_in\": %llu, "
                    "\"bnd_out\": %llu}",
                    i ? ", " : "", v[i].pair, v[i].row0, v[i].flags, v[i].nsteps, (unsigned long long)v[i].mask_off,
                    (unsigned long long)v[i].bnd_in, (unsigned long long)v[i].bnd_out);
    std::printf("]");
}

}  // namespace

int main(int argc, char **argv)
{
    sa_params P;
    std::memset(&P, 0, sizeof(P));
    std::string matrix = "blast", matrices = "tests/golden/matrices.json";
    int cus = 256;
    bool strips = false;
    std::vector<sa_pair> pairs;
    for (int i = 1; i < argc; ++i)
    {
        const std::string a = argv[i];
        auto value = [&]() -> const char * { return i + 1 < argc ? argv[++i] : ""; };
        if (a == "--mode")
        {
            const std::string v = value();
            P.mode = v == "global" ? SA_GLOBAL : v == "local" ? SA_LOCAL : std::atoi(v.c_str());
        }
        else if (a == "--alphabet") P.alphabet_size = std::atoi(value());
        else if (a == "--gap") P.gap_penalty = std::atoi(value());
        else if (a == "--matrix") matrix = value();
        else if (a == "--matrices") matrices = value();
        else if (a == "--cus") cus = std::atoi(value());
        else if (a == "--rows-per-lane") P.rows_per_lane = std::atoi(value());
        else if (a == "--strips") strips = true;
        else
        {
            unsigned long long n = 0, m = 0, count = 1;
            if (std::sscanf(a.c_str(), "%llux%llux%llu", &n, &m, &count) < 2) return usage(("bad argument " + a).c_str());
            // offsets as a caller packing the sequences back to back would give them
            for (unsigned long long k = 0; k < count; ++k)
            {
                sa_pair pr;
                pr.text_offset = pairs.empty() ? 0 : pairs.back().text_offset + pairs.back().text_len;
                pr.text_len = n;
                pr.pattern_offset = pairs.empty() ? 0 : pairs.back().pattern_offset + pairs.back().pattern_len;
                pr.pattern_len = m;
                pairs.push_back(pr);
            }
        }
    }
    const int A = P.alphabet_size;
    std::vector<int32_t> S;
    if (matrix == "unit")
    {
        // (sized for any alphabet the limits case asks for, valid or not)
        const int a = std::max(A, 1);
        S.assign((size_t)a * a, -1);
        for (int c = 0; c < a; ++c) S[(size_t)c * a + c] = 1;
    }
    else if (matrix != "blast" && matrix != "blosum50") return usage("matrix must be blast, blosum50 or unit");
    else if (!read_matrix(matrices, matrix, &S)) return usage(("no matrix " + matrix + " in " + matrices).c_str());
    else if ((size_t)A * A != S.size()) return usage("alphabet size does not match the matrix");
    P.score_matrix = S.data();

    Plan pl;
    std::string err;
    const int rc = make_plan(&P, pairs.data(), (int64_t)pairs.size(), cus, knobs(), &pl, &err);
    if (rc != SA_OK)
    {
        std::printf("{\"error\": %d, \"message\": \"%s\"}\n", rc, err.c_str());
        return 0;
    }
    static const char *const kinds[] = {"strips", "band", "pair", "pair_chain", "band3"};  // engine.FILL_KINDS
    uint64_t h = 14695981039346656037ull;
    h = fnv1a(h, pl.pairs.data(), pl.pairs.size() * sizeof(PairDesc));
    h = fnv1a(h, pl.strips.data(), pl.strips.size() * sizeof(StripDesc));
    h = fnv1a(h, pl.bands.data(), pl.bands.size() * sizeof(StripDesc));
    const FillLaunch &g = pl.launch;
    std::printf("{\"mode\": %d, \"A\": %d, \"gap\": %d, \"R\": %d, \"U\": %d, \"W\": %d, \"key_bits\": %d, \"key_rowbits\": %d, "
                "\"sk\": %d, \"chain\": %d, \"chain_solo\": %d, \"band\": %d, \"band_r\": %d, \"strip_w\": %d, \"num_cu\": %d, "
                "\"fill_kind\": \"%s\", \"num_pairs\": %zu, \"num_strips\": %zu, \"num_bands\": %zu, \"tb_groups\": %zu, "
                "\"tb_slots\": %lld, \"max_recs\": %lld, \"code_bytes\": %llu, \"mask_entries\": %llu, \"granules\": %llu, "
                "\"out_bytes\": %llu, \"rec_words\": %llu, \"hash\": \"%016llx\", ",
                pl.mode, pl.A, pl.gap, pl.R, pl.U, pl.W, pl.key_bits, pl.key_rowbits, pl.sk, (int)pl.chain,
                (int)pl.chain_solo, (int)pl.band, pl.band_r, pl.strip_w, pl.num_cu, kinds[fill_kind(pl)], pl.pairs.size(),
                pl.strips.size(), pl.bands.size(), pl.tb_groups.size(), (long long)pl.tb_slots, (long long)pl.max_recs,
                (unsigned long long)pl.code_bytes, (unsigned long long)pl.mask_entries, (unsigned long long)pl.granules,
                (unsigned long long)pl.out_bytes, (unsigned long long)pl.rec_words, (unsigned long long)h);
    std::printf("\"launch\": {\"W\": %d, \"sk\": %d, \"band3\": %d, \"num_groups\": %d, \"num_bands\": %d, "
                "\"num_band_groups\": %d, \"band_wgs\": %d, \"strip_w\": %d, \"grid\": %d, \"chain_lds\": %d, "
                "\"pair_text_len\": %d}",
                g.W, g.sk, (int)g.band3, g.num_groups, g.num_bands, g.num_band_groups, g.band_wgs, g.strip_w, g.grid,
                g.chain_lds, g.pair_text_len);
    if (strips)
    {
        std::printf(", \"pairs\": [");
        for (size_t i = 0; i < pl.pairs.size(); ++i)
            std::printf("%s{\"text_len\": %llu, \"pattern_len\": %llu, \"first_strip\": %d, \"num_strips\": %d}", i ? ", " : "",
                        (unsigned long long)pl.pairs[i].text_len, (unsigned long long)pl.pairs[i].pattern_len,
                        pl.pairs[i].first_strip, pl.pairs[i].num_strips);
        std::printf("]");
        print_strips("strips", pl.strips);
        print_strips("bands", pl.bands);
    }
    std::printf("}\n");
    return 0;
}
