// crf_narrow_keys.h -- order-preserving integer keys of the narrow member formats' stored codes, for the rank kernels that
// read such members as stored (kernels_rank_narrow.hip).  Plain C++, usable from host code (tests/native/narrow_keys.cpp
// checks every code of every format against the float order of the converted values).
//
// A rank estimator needs only the order and the ties of a voxel's values.  The values the calculators see are b / 255.0f,
// s / 65535.0f and float(h) (crf_internal.h): the first two are strictly increasing in the code, the third is exact, so
//   key(a) <  key(b)  <=>  value(a) <  value(b)
//   key(a) == key(b)  <=>  value(a) == value(b)          (-0.0 == +0.0: one key)
// hold for all non-NaN codes with a key of 16 bits.  A seventeenth bit holds the pad key of the guarded kernels, which
// sorts behind every real key -- u16 code 65535 and the f16 NaN patterns above +inf included -- and equals none.
#pragma once
#include <cstdint>

#include "../../include/corrfield.h"

#if defined(__HIPCC__)
#define CRF_HD __host__ __device__
#else
#define CRF_HD
#endif

namespace crf {

constexpr uint32_t kNarrowPadKey = 0x10000u;
constexpr int kNarrowSlotBits = 7;  // slots 0..127 below the key: a composite has 24 significant bits

// u8 / u16: the code.  f16: -0 becomes +0, then the sign-flip map of the 16 bits (negative patterns reversed below the
// positive ones).  Keys of the f16 infinities: 0x03FF and 0xFC00; the NaN patterns lie outside them at either end.
template <int FMT>
CRF_HD inline uint32_t narrow_key(uint32_t code) {
    static_assert(FMT == CRF_MEMBER_U8 || FMT == CRF_MEMBER_U16 || FMT == CRF_MEMBER_F16, "a narrow format");
    if constexpr (FMT == CRF_MEMBER_F16) {
        const uint32_t c = code == 0x8000u ? 0u : code;
        return c ^ ((c & 0x8000u) ? 0xFFFFu : 0x8000u);
    } else {
        return code;
    }
}

// the key belongs to a NaN (f16 only; the integer formats have none)
template <int FMT>
CRF_HD inline bool narrow_key_is_nan(uint32_t key) {
    return FMT == CRF_MEMBER_F16 && (key < 0x03FFu || (key > 0xFC00u && key < kNarrowPadKey));
}

// (key, slot) in one 32-bit word whose unsigned order is the lexicographic order of the pair
CRF_HD inline uint32_t narrow_composite(uint32_t key, uint32_t slot) { return (key << kNarrowSlotBits) | slot; }
CRF_HD inline uint32_t narrow_composite_key(uint32_t c) { return c >> kNarrowSlotBits; }
CRF_HD inline uint32_t narrow_composite_slot(uint32_t c) { return c & ((1u << kNarrowSlotBits) - 1u); }

}  // namespace crf
