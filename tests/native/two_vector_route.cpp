// Prints two_vector_route (correrender_amd/csrc/two_vector_route.h) -- which kernel evaluates a measure between two member
// vectors per item -- as one line "mode measure members k num_bins force route kernel_name" per combination: both modes (0 the
// symmetric field mode, 1 pair requests), the seven measures, 1..2048 members, k = 0, 1, 3, 64, 65, 200, num_bins = 0, 1,
// 80, 255, 256, and both values of the force switch (CRF_SYMMETRIC_DIRECT / CRF_REQUESTS_GENERIC).
// tests/test_two_vector_route.py compares the lines with its own statement of the rules.
#include <cstdio>

#include "two_vector_route.h"

static const char* route_name(crf::TwoVectorKernel kernel) {
    switch (kernel) {
        case crf::TwoVectorKernel::Fill: return "Fill";
        case crf::TwoVectorKernel::PearsonRegister: return "PearsonRegister";
        case crf::TwoVectorKernel::KraskovDirect: return "KraskovDirect";
        case crf::TwoVectorKernel::Sorted: return "Sorted";
        case crf::TwoVectorKernel::DirectSymmetric: return "DirectSymmetric";
        default: return "PairRequest";
    }
}

int main() {
    const int ks[] = {0, 1, 3, 64, 65, 200};
    const int bins[] = {0, 1, 80, 255, 256};
    for (int mode = 0; mode <= 1; mode++)
        for (int measure = CRF_PEARSON; measure <= CRF_KMI_CC; measure++)
            for (int cs = 1; cs <= 2048; cs++)
                for (int k : ks)
                    for (int num_bins : bins)
                        for (int force = 0; force <= 1; force++) {
                            const crf::TwoVectorKernel kernel =
                                crf::two_vector_route(mode == 1, measure, cs, k, num_bins, force == 1);
                            std::printf("%d %d %d %d %d %d %s %s\n", mode, measure, cs, k, num_bins, force,
                                        route_name(kernel), crf::two_vector_kernel_name(kernel, mode == 1, measure));
                        }
    return 0;
}
