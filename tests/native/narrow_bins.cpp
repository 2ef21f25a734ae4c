// Exhaustive host check of the per-sample bin function of binned mutual information (correrender_amd/csrc/crf_binned_bins.h),
// compiled for the host with g++ -ffp-contract=off.  For every u8, u16 and f16 code, with the value the calculators see of
// it (b / 255.0f, s / 65535.0f, float(h)), and for a list of (min, max, num_bins):
//   1. wherever a launcher would choose the reciprocal form (max - min inside [2^-60, 2^60]) it gives the same bin and the
//      same validity as the division form, for every non-NaN code
//   2. the division form equals the reference's lines evaluated step by step (CorrelationCalculator.cpp:1061-1062,
//      MutualInformation.cpp:64-67), the double -> int conversion being x86's cvttsd2si
//   3. under finite extrema with max > min exactly the f16 NaN codes are skipped, no code of an integer format is
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#if defined(__SSE2__)
#include <emmintrin.h>
#endif

#include "../../include/corrfield.h"
#include "crf_binned_bins.h"

using namespace crf;

static int failures = 0;
static void check(bool ok, const char* what, uint32_t code, int cas, uint32_t got, uint32_t want) {
    if (!ok && failures++ < 20) std::printf("FAIL %s: code 0x%04x case %d: %u vs %u\n", what, code, cas, got, want);
}

// float(h) without relying on a compiler's _Float16: exact for every pattern
static float half_to_float(uint32_t h) {
    const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 0x1Fu, m = h & 0x3FFu;
    uint32_t bits;
    if (e == 0x1Fu) {
        bits = sign | 0x7F800000u | (m << 13);
    } else if (e != 0u) {
        bits = sign | ((e + 112u) << 23) | (m << 13);
    } else {
        const float v = std::ldexp(float(m), -24);  // subnormal: m * 2^-24, exact
        std::memcpy(&bits, &v, 4);
        bits |= sign;
    }
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}

template <int FMT>
static float value_of(uint32_t code) {
    if (FMT == CRF_MEMBER_U8) return float(code) / 255.0f;
    if (FMT == CRF_MEMBER_U16) return float(code) / 65535.0f;
    return half_to_float(code);
}

// int(t) of the reference's x86-64 build: the instruction itself where the compiler offers it
static int x86_double_to_int(double t) {
#if defined(__SSE2__)
    return _mm_cvttsd_si32(_mm_set_sd(t));
#else
    if (!(t > -2147483649.0 && t < 2147483648.0)) return INT_MIN;  // "integer indefinite"
    return int(t);
#endif
}

// The reference, line by line: the normalisation of the query value (CorrelationCalculator.cpp:1061-1062), then the sample
// loop's test and bin (MutualInformation.cpp:64-67, Real = double).  Returns the bin, or kSkippedSampleBin.
static uint32_t reference_bin(float fieldValue, float minFieldValQuery, float maxFieldValQuery, int numBins) {
    volatile float gridPointValue = (fieldValue - minFieldValQuery) / (maxFieldValQuery - minFieldValQuery);
    const double val1 = gridPointValue;
    if (std::isnan(val1)) return kSkippedSampleBin;
    const int binIdx1 = std::clamp(x86_double_to_int(val1 * double(numBins)), 0, numBins - 1);
    return uint32_t(binIdx1);
}

struct Case {
    float min, max;
    int nb;
    bool finite_open;  // finite extrema, max > min: check 3 applies
};

static const Case kCases[] = {
    {0.0f, 1.0f, 80, true},
    {0.0f, 1.0f, 255, true},
    {0.0f, 1.0f, 1, true},
    {0.0f, 1.0f, 2, true},
    {0.25f, 0.75f, 80, true},
    {3.0f / 255.0f, 250.0f / 255.0f, 100, true},
    {0.0f, 0x1p-60f, 80, true},          // range exactly 2^-60: the reciprocal form's lower end
    {0.0f, 0x1p60f, 80, true},           // range exactly 2^60: its upper end
    {0.0f, 0x1p-61f, 80, true},          // just outside: division only
    {0.0f, 0x1p61f, 80, true},
    {0.5f, 0.5f + 0x1p-60f, 80, true},   // (rounds to range 0 in fp32: max == min)
    {0.0f, 1e-8f, 80, true},             // bin index beyond the int range: cvttsd2si gives INT_MIN, bin 0
    {-1.0f, 1.0f, 254, true},
    {-65504.0f, 65504.0f, 255, true},    // the whole finite f16 range
    {0.1f, 0.7f, 7, true},
    {0.5f, 0.5f, 80, false},             // max == min: 0 / 0 is skipped, the rest is +-inf and lands in bin 0
    {0.0f, INFINITY, 80, false},
    {-INFINITY, 1.0f, 80, false},
};

template <int FMT>
static void check_format(uint32_t codes, const char* name) {
    uint64_t nans = 0, rcp_checked = 0, skipped_open = 0;
    for (uint32_t c = 0; c < codes; c++) {
        const float v = value_of<FMT>(c);
        const bool is_nan = v != v;
        nans += is_nan;
        int cas = 0;
        for (const Case& k : kCases) {
            const float range = k.max - k.min;  // the fp32 subtraction of the kernels and of the launchers
            const double nbd = double(k.nb);
            const uint32_t by_div = query_bin_or_skip_div(v, k.min, range, nbd, k.nb);
            check(by_div == reference_bin(v, k.min, k.max, k.nb), "division form vs the reference's lines", c, cas, by_div,
                  reference_bin(v, k.min, k.max, k.nb));
            check(by_div == kSkippedSampleBin || by_div < uint32_t(k.nb), "bin inside [0, num_bins)", c, cas, by_div, 0);
            if (binned_range_takes_rcp(range) && !is_nan) {
                const uint32_t by_rcp = query_bin_or_skip_rcp(v, k.min, range, 1.0f / range, nbd, k.nb);
                check(by_rcp == by_div, "reciprocal form vs division form", c, cas, by_rcp, by_div);
                rcp_checked++;
            }
            if (binned_range_takes_rcp(range) && is_nan)  // (the reciprocal form skips a NaN sample too)
                check(query_bin_or_skip_rcp(v, k.min, range, 1.0f / range, nbd, k.nb) == kSkippedSampleBin,
                      "reciprocal form skips NaN", c, cas, 0, 0);
            if (k.finite_open && range > 0.0f) {
                check((by_div == kSkippedSampleBin) == is_nan, "exactly the NaN codes are skipped", c, cas, by_div, is_nan);
                skipped_open += by_div == kSkippedSampleBin;
            }
            cas++;
        }
    }
    std::printf("%s: %u codes, %llu NaN, %llu reciprocal-form comparisons, %llu skipped under finite extrema\n", name, codes,
                (unsigned long long)nans, (unsigned long long)rcp_checked, (unsigned long long)skipped_open);
}

int main() {
    // the conversion itself, at the edges of the int range
    const double edges[] = {2147483647.5, 2147483648.0, 8e9, -2147483648.5, -2147483649.0, -8e9, INFINITY, -INFINITY, NAN};
    for (double t : edges)
        check(bin_index_x86(t) == x86_double_to_int(t), "bin_index_x86 at the edge", 0, int(&t - edges),
              uint32_t(bin_index_x86(t)), uint32_t(x86_double_to_int(t)));
    check(bin_index_x86(8e9) == INT_MIN && clamp_bin(bin_index_x86(8e9), 80) == 0, "positive overflow lands in bin 0", 0, 0, 0, 0);
    check_format<CRF_MEMBER_U8>(256u, "u8");
    check_format<CRF_MEMBER_U16>(65536u, "u16");
    check_format<CRF_MEMBER_F16>(65536u, "f16");
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("OK narrow bins\n");
    return 0;
}
