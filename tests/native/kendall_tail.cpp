// Runs the host tail of the Kendall calls (correrender_amd/csrc/crf_similarity_tail.h: similarity_kendall_from_counts, no
// HIP in it) without a GPU.  Standard input: any number of cases, each four native 64-bit signed integers -- n, n1, n2, S.
// Prints one line per case: the bits of the float in hex, then n0, n1, n2 and S as the function reports them.
// tests/test_kendall_tail.py compares them with numpy's float64 expression.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "crf_similarity_tail.h"

int main() {
    int64_t in[4];
    while (std::fread(in, sizeof(int64_t), 4, stdin) == 4) {
        long long counts[4];
        const float value = crf::similarity_kendall_from_counts(in[0], in[1], in[2], in[3], counts);
        uint32_t u;
        std::memcpy(&u, &value, sizeof u);
        std::printf("%08x %lld %lld %lld %lld\n", u, counts[0], counts[1], counts[2], counts[3]);
    }
    return 0;
}
