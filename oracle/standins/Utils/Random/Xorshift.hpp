/*
 * Stand-in for sgl's <Utils/Random/Xorshift.hpp> -- TEST INFRASTRUCTURE, this repository's own code.
 *
 * The reference draws its Kraskov tie-breaking noise from sgl::XorshiftRandomGenerator(seed)
 * .getRandomFloatBetween(0.0f, 1.0f).  sgl's generator is not available, so THIS IS NOT sgl's STREAM: it is this
 * repository's documented stream (oracle/corr_oracle.cpp "Xorshift32"): Marsaglia xorshift32 with shifts
 * (13, 17, 5), seeded with the low 32 bits of the seed, u = (state >> 8) * 2^-24 in [0, 1).
 * On tie-free data the 1e-10 noise cannot change a neighbour count, so results do not depend on the stream; on exactly
 * tied data they do, and agreement with a build that has sgl needs that build's stream (crf_set_kraskov_noise).
 */
#pragma once

#include <cstdint>

namespace sgl {

class XorshiftRandomGenerator {
public:
    explicit XorshiftRandomGenerator(unsigned long seed) : state(uint32_t(seed) ? uint32_t(seed) : 0x9E3779B9u) {}

    float getRandomFloatBetween(float low, float high) {
        state ^= state << 13;
        state ^= state >> 17;
        state ^= state << 5;
        const float u = float(state >> 8) * (1.0f / 16777216.0f);
        return low + u * (high - low);
    }

private:
    uint32_t state;
};

}  // namespace sgl
