// Host check of the kernels' reciprocal-division functions on inputs that sit on their edges
// (tests/division_edge_inputs.py), compiled for the host with g++ -ffp-contract=off.  It calls the kernels' own functions:
// query_bin_div / query_bin_rcp (correrender_amd/csrc/crf_binned_bins.h) and exact_div / exact_div_guard
// (correrender_amd/csrc/crf_exact_div.h).
//
// usage: division_edges FILE.  FILE is a sequence of records, native byte order:
//   int32 1, float min, float max, int32 num_bins, int64 n, n floats             a bin-edge lattice's samples
//   int32 2, int32 cs, int64 n, cs * n floats (member-major)                     n vectors of cs members
// One line of output per record:
//   lattice min max num_bins: samples, whether the launchers would take the reciprocal form for this range, the samples
//     for which query_bin_rcp and query_bin_div disagree (bin or validity), and the samples whose bin changes when the
//     correction is dropped (q = d * rcp alone)
//   vectors cs n: the vectors that pass exact_div_guard (mean and sd by the reference's sequential fp32 passes), their
//     deviations a for which exact_div(a, sd, 1 / sd) differs in any bit from a / sd, and the deviations of the OTHER
//     vectors for which it differs (what ignoring the guard would cost)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "crf_binned_bins.h"
#include "crf_exact_div.h"

using namespace crf;

static bool same_bits(float a, float b) {
    uint32_t x, y;
    std::memcpy(&x, &a, 4);
    std::memcpy(&y, &b, 4);
    return x == y || (a != a && b != b);
}

template <class T>
static bool get(std::FILE* f, T* v, size_t n = 1) {
    return std::fread(v, sizeof(T), n, f) == n;
}

static bool lattice(std::FILE* f) {
    float mn, mx;
    int32_t nb;
    int64_t n;
    if (!get(f, &mn) || !get(f, &mx) || !get(f, &nb) || !get(f, &n)) return false;
    std::vector<float> y(size_t(n), 0.0f);
    if (!get(f, y.data(), y.size())) return false;
    const float range = mx - mn, rcp = 1.0f / range;
    const double nbd = double(nb);
    long disagree = 0, dropped = 0;
    for (float v : y) {
        bool cd, cr;
        const int bd = query_bin_div(v, mn, range, nbd, nb, &cd);
        const int br = query_bin_rcp(v, mn, range, rcp, nbd, nb, &cr);
        disagree += (bd != br || cd != cr);
        const float q0 = (v - mn) * rcp;  // the mutant: no correction
        dropped += cd && bin_of_normalised(q0, nbd, nb) != bd;
    }
    std::printf("lattice %a %a %d: samples %lld rcp_form %d rcp_vs_div %ld correction_dropped %ld\n", mn, mx, nb,
                (long long)n, int(binned_range_takes_rcp(range)), disagree, dropped);
    return true;
}

static bool vectors(std::FILE* f) {
    int32_t cs;
    int64_t n;
    if (!get(f, &cs) || !get(f, &n)) return false;
    std::vector<float> m(size_t(cs) * size_t(n), 0.0f);
    if (!get(f, m.data(), m.size())) return false;
    const float nn = float(cs), invN = 1.0f / nn, invNm1 = 1.0f / (nn - 1.0f);
    long guarded = 0, wrong_guarded = 0, wrong_unguarded = 0;
    for (int64_t v = 0; v < n; v++) {
        float mean = 0.0f;  // Correlation.cpp:141-174, as pearson_tail (crf_device.h) restates it
        for (int e = 0; e < cs; e++) mean += invN * m[size_t(e) * n + v];
        float var = 0.0f;
        for (int e = 0; e < cs; e++) {
            const float d = m[size_t(e) * n + v] - mean;
            var += invNm1 * d * d;
        }
        const float sd = std::sqrt(var), rcp = 1.0f / sd;
        const bool guard = exact_div_guard(mean, sd);
        guarded += guard;
        for (int e = 0; e < cs; e++) {
            const float a = m[size_t(e) * n + v] - mean;
            const bool same = same_bits(exact_div(a, sd, rcp), a / sd);
            (guard ? wrong_guarded : wrong_unguarded) += !same;
        }
    }
    std::printf("vectors %d %lld: guarded %ld wrong_guarded %ld wrong_unguarded %ld\n", cs, (long long)n, guarded,
                wrong_guarded, wrong_unguarded);
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t kind;
    int records = 0;
    while (get(f, &kind)) {
        if (!(kind == 1 ? lattice(f) : kind == 2 ? vectors(f) : false)) {
            std::printf("FAIL malformed record %d\n", records);
            return 1;
        }
        records++;
    }
    std::fclose(f);
    std::printf("OK division edges: %d records\n", records);
    return 0;
}
