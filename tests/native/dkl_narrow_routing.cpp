// Prints dkl_narrow_routed (correrender_amd/csrc/crf_internal.h) -- which DKL calls on narrow members run the native kernel --
// as one line "format members estimator k routed" per combination: every member format id 0..4 (fp32 and an unknown id
// included), 1..2048 members, both estimators, k = 1, 2, 3, 7 and the default ceil(3 cs / 100).
// tests/test_narrow_dkl_routing.py compares the lines with the table of tests/test_gpu_narrow_dkl.py.
#include <cstdio>

#include "crf_internal.h"

static_assert(crf::dkl_narrow_routed(CRF_MEMBER_F32, 64, 0, 1) == false, "fp32 members have no narrow route");

int main() {
    for (int format = 0; format <= 4; format++)
        for (int cs = 1; cs <= crf::kMaxGenericMembers; cs++)
            for (int estimator = 0; estimator <= 1; estimator++) {
                const int def = (3 * cs + 99) / 100 > 1 ? (3 * cs + 99) / 100 : 1;
                const int ks[5] = {1, 2, 3, 7, def};
                for (int k : ks)
                    std::printf("%d %d %d %d %d\n", format, cs, estimator, k,
                                crf::dkl_narrow_routed(format, cs, estimator, k) ? 1 : 0);
            }
    return 0;
}
