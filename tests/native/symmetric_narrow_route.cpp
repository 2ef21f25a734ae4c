// Prints symmetric_narrow_routed (correrender_amd/csrc/symmetric_narrow_route.h) -- whether the symmetric Pearson field reads
// two narrow fields as stored -- as one line "format members routed" per combination: formats -1..5 (crf_member_format is
// 0..3) and 0..300 members.  tests/test_symmetric_narrow_route.py compares the lines with its own statement of the table.
#include <cstdio>

#include "symmetric_narrow_route.h"

// the predicate is usable in constant expressions
static_assert(crf::symmetric_narrow_routed(CRF_MEMBER_U8, 64) && !crf::symmetric_narrow_routed(CRF_MEMBER_F32, 64) &&
                  !crf::symmetric_narrow_routed(CRF_MEMBER_U8, 1) && !crf::symmetric_narrow_routed(CRF_MEMBER_U8, 129),
              "symmetric_narrow_routed");

int main() {
    for (int format = -1; format <= 5; format++)
        for (int cs = 0; cs <= 300; cs++)
            std::printf("%d %d %d\n", format, cs, crf::symmetric_narrow_routed(format, cs) ? 1 : 0);
    return 0;
}
