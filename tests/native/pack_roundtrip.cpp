// Exhaustive host check of the packed member format (correrender_amd/csrc/crf_internal.h): the encode helpers the
// encode kernel uses and the decode helper the Pearson field kernel uses, compiled for the host with g++.
//   1. every one of the 2^32 bit patterns against one base: the pattern fits iff its exponent field is 0 or within the
//      15 binades above the base, and then decodes to itself from every word position, whatever the other bits of the
//      three words hold
//   2. every exponent field against every base, both signs and a few mantissas
//   3. the segment rule (pack_segment_base)
#include <cstdio>
#include <cstdint>

#include "crf_internal.h"

using namespace crf;

static int failures = 0;
static void check(bool ok, const char* what, uint32_t a, uint32_t b) {
    if (!ok && failures++ < 20) std::printf("FAIL %s: 0x%08x 0x%08x\n", what, a, b);
}

static uint32_t roundtrip(uint32_t bits, uint32_t base, uint32_t junk) {
    const int h = int(junk & 1u), b = int((junk >> 1) & 3u), n = int((junk >> 3) & 7u);
    const uint32_t lo_mask = 0xFFFFu << (16 * h), byte_mask = 0xFFu << (8 * b), code_mask = 0xFu << (4 * n);
    const uint32_t other = junk * 0x9E3779B9u;  // whatever the neighbouring values of the words hold
    const uint32_t lo_word = (pack_lo16(bits) << (16 * h)) | (other & ~lo_mask);
    const uint32_t byte_word = (pack_byte(bits) << (8 * b)) | ((other >> 3) & ~byte_mask);
    const uint32_t code_word = (pack_code(bits, base) << (4 * n)) | ((other << 5) & ~code_mask);
    return unpack_bits(lo_word, h, byte_word, b, code_word, n, base);
}

static bool fits(uint32_t e, uint32_t base) { return e == 0u || (e != 255u && e >= base && e <= base + 14u); }

int main() {
    const uint32_t kBase = 120;
    uint64_t fitting = 0;
    for (uint64_t i = 0; i <= 0xFFFFFFFFull; i++) {
        const uint32_t bits = uint32_t(i);
        const uint32_t e = (bits >> 23) & 0xFFu;
        if (!fits(e, kBase)) continue;
        fitting++;
        const uint32_t code = pack_code(bits, kBase);
        check(code <= 15u && (code == 0u) == (e == 0u), "code range", bits, code);
        check(roundtrip(bits, kBase, bits ^ (bits >> 7)) == bits, "all patterns", bits, kBase);
    }
    check(fitting == (16ull << 23) * 2ull, "fitting count", uint32_t(fitting >> 23), 0);

    const uint32_t mantissas[] = {0u, 1u, 0x7FFFFFu, 0x123456u, 0x400000u, 0x00FFFFu, 0x7F0000u};
    for (uint32_t base = 1; base <= 254; base++) {
        for (uint32_t e = 0; e <= 255; e++) {
            if (!fits(e, base)) continue;
            for (uint32_t s = 0; s < 2; s++)
                for (uint32_t m : mantissas) {
                    const uint32_t bits = (s << 31) | (e << 23) | m;
                    for (uint32_t j = 0; j < 64; j++) check(roundtrip(bits, base, j) == bits, "base x exponent", bits, base);
                }
        }
        // the segment rule: [base, base + 14] fits, one binade more does not, NaN / Inf never
        check(pack_segment_base(base, base, false) == base, "segment single", base, 0);
        if (base + 14u <= 254u) check(pack_segment_base(base, base + 14u, false) == base, "segment 15", base, 0);
        if (base + 15u <= 254u) check(pack_segment_base(base, base + 15u, false) == kPackFallback, "segment 16", base, 0);
        check(pack_segment_base(base, 255u, true) == kPackFallback, "segment special", base, 0);
    }
    check(pack_segment_base(256u, 0u, false) == 1u, "segment zeros", 0, 0);
    check(pack_segment_base(256u, 255u, true) == kPackFallback, "segment zeros + NaN", 0, 0);
    // the layout arithmetic of the header comment
    check(pack_slots(17) == 32 && pack_slots(64) == 64 && pack_slots(65) == 80 && pack_slots(128) == 128, "slots", 0, 0);
    check(pack_tile_bytes(64) == 14u * 1024u && pack_tile_bytes(48) == (6u + 3u + 2u) * 1024u, "tile bytes", 0, 0);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("OK %llu fitting patterns\n", (unsigned long long)fitting);
    return 0;
}
