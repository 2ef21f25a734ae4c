// Exhaustive host check of the narrow member formats' order keys (correrender_amd/csrc/crf_narrow_keys.h), compiled for
// the host with g++.  For every u8, u16 and f16 code, against the values the calculators see of it (b / 255.0f,
// s / 65535.0f, float(h)):
//   1. the key order of two codes is the float order of their values, and key equality is float equality (+0 == -0):
//      with the codes sorted by key the values never decrease, and neighbours are equal exactly when their keys are;
//      keys of the integer formats are checked against every other code directly (u8) or through the sorted chain (16 bit)
//   2. exactly the f16 NaN codes are classified NaN, no code of an integer format is
//   3. the pad key exceeds every real key, and a (key, slot) composite keeps both parts and their lexicographic order
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "crf_narrow_keys.h"

using namespace crf;

static int failures = 0;
static void check(bool ok, const char* what, uint32_t a, uint32_t b) {
    if (!ok && failures++ < 20) std::printf("FAIL %s: 0x%05x 0x%05x\n", what, a, b);
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

template <int FMT>
static uint64_t check_format(uint32_t codes, const char* name) {
    std::vector<uint32_t> order;
    uint64_t nans = 0;
    for (uint32_t c = 0; c < codes; c++) {
        const uint32_t key = narrow_key<FMT>(c);
        const float v = value_of<FMT>(c);
        check(key < kNarrowPadKey, "pad key above every real key", c, key);
        check(narrow_key_is_nan<FMT>(key) == (v != v), "NaN classification", c, key);
        for (uint32_t slot : {0u, 1u, 127u}) {
            const uint32_t comp = narrow_composite(key, slot);
            check(narrow_composite_key(comp) == key && narrow_composite_slot(comp) == slot, "composite parts", c, slot);
            check(comp < narrow_composite(kNarrowPadKey, 0u), "pad composite above every real one", c, slot);
            if (key > 0u) check(narrow_composite(key - 1u, 127u) < narrow_composite(key, 0u), "key above slot", c, slot);
        }
        if (v != v)
            nans++;
        else
            order.push_back(c);
    }
    check(!narrow_key_is_nan<FMT>(kNarrowPadKey), "pad key is no NaN", kNarrowPadKey, 0);
    // sorted by key, the values must be non-decreasing, and neighbours equal exactly when their keys are: together
    // that is "key order == float order and key equality == float equality" for every pair of non-NaN codes
    std::stable_sort(order.begin(), order.end(), [](uint32_t a, uint32_t b) { return narrow_key<FMT>(a) < narrow_key<FMT>(b); });
    for (size_t i = 1; i < order.size(); i++) {
        const uint32_t a = order[i - 1], b = order[i];
        const float va = value_of<FMT>(a), vb = value_of<FMT>(b);
        const bool same_key = narrow_key<FMT>(a) == narrow_key<FMT>(b);
        check(va <= vb, "values follow the key order", a, b);
        check(same_key == (va == vb), "key equality is float equality", a, b);
    }
    if (codes <= 256u)  // every pair, directly
        for (uint32_t a = 0; a < codes; a++)
            for (uint32_t b = 0; b < codes; b++)
                check((narrow_key<FMT>(a) < narrow_key<FMT>(b)) == (value_of<FMT>(a) < value_of<FMT>(b)), "pairwise order", a, b);
    std::printf("%s: %u codes, %llu NaN\n", name, codes, (unsigned long long)nans);
    return nans;
}

int main() {
    check(check_format<CRF_MEMBER_U8>(256u, "u8") == 0, "u8 NaN count", 0, 0);
    check(check_format<CRF_MEMBER_U16>(65536u, "u16") == 0, "u16 NaN count", 0, 0);
    check(check_format<CRF_MEMBER_F16>(65536u, "f16") == 2046, "f16 NaN count", 0, 0);
    // the two zeros tie; the infinities are ordinary values at the ends of the non-NaN range
    check(narrow_key<CRF_MEMBER_F16>(0x8000u) == narrow_key<CRF_MEMBER_F16>(0x0000u), "+0 and -0", 0x8000u, 0u);
    check(narrow_key<CRF_MEMBER_F16>(0xFC00u) == 0x03FFu && narrow_key<CRF_MEMBER_F16>(0x7C00u) == 0xFC00u, "infinities", 0, 0);
    check(narrow_key<CRF_MEMBER_U16>(65535u) < kNarrowPadKey && narrow_key<CRF_MEMBER_F16>(0x7FFFu) < kNarrowPadKey, "largest keys", 0, 0);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("OK narrow keys\n");
    return 0;
}
