// Runs the host tail of crf_field_similarity's binned measures (correrender_amd/csrc/crf_similarity_tail.h, no HIP in it)
// without a GPU.  Standard input: any number of cases, each as native 64-bit unsigned integers -- num_bins, samples (the
// reference's `es`), then num_bins^2 counts of the joint histogram, x bin major.  Prints one line per case: the bits of
// the float similarity_mi_from_counts returns and the bits of its similarity_mi_to_cc, in hex.
// tests/test_similarity_tail.py compares them with the reference's object code and with a sequential restatement.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "crf_similarity_tail.h"

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, sizeof u);
    return u;
}

int main() {
    uint64_t head[2];
    while (std::fread(head, sizeof(uint64_t), 2, stdin) == 2) {
        if (head[0] < 1 || head[0] > 1024) return 2;
        std::vector<uint64_t> counts(size_t(head[0] * head[0]));
        if (std::fread(counts.data(), sizeof(uint64_t), counts.size(), stdin) != counts.size()) return 3;
        const float mi = crf::similarity_mi_from_counts(counts.data(), int(head[0]), head[1]);
        std::printf("%08x %08x\n", bits(mi), bits(crf::similarity_mi_to_cc(mi)));
    }
    return 0;
}
