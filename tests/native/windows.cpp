// Prints the window arithmetic of correrender_amd/csrc/crf_windows.h -- how a grid whose member volumes are 4 GiB or more
// (or, under CRF_WINDOW_VOXELS, any grid with more voxels than one window) is cut into windows -- for
// tests/test_windows.py, which compares the lines with its own statement of the rules in Python integers:
//   "valid VALUE 0|1"                                   window_override_valid
//   "parse [TEXT] VALUE", "parse null VALUE"            parse_window_override (-1: crf_set_grid fails)
//   "grid N OVERRIDE WINDOWED COUNT LAST_LEN SUM FULL MAX_END"
//       WINDOWED grid_windowed, COUNT window_count; over the windows w < COUNT of a windowed grid: LAST_LEN the length of
//       the last one, SUM the sum of all lengths, FULL 1 if every window but the last has window_voxels voxels, MAX_END
//       the largest first voxel + length.  An ordinary grid (COUNT 1) prints its one launch: N N 1 N.
// Sizes go up to 2^32 + 5 voxels, which no GPU test can reach.
#include <cstdio>
#include <initializer_list>

#include "crf_windows.h"

static void grid(size_t n, size_t override_voxels) {
    const bool windowed = crf::grid_windowed(n, override_voxels);
    const size_t count = crf::window_count(n, override_voxels);
    size_t last = n, sum = n, max_end = n;
    int full = 1;
    if (windowed) {
        const size_t window = crf::window_voxels(override_voxels);
        sum = max_end = 0;
        for (size_t w = 0; w < count; w++) {
            const size_t first = crf::window_first(w, window), len = crf::window_length(n, w, window);
            if (w + 1 < count && len != window) full = 0;
            if (first + len > max_end) max_end = first + len;
            sum += len;
            last = len;
        }
        // past the last window there is nothing
        if (crf::window_length(n, count, window) != 0) full = 0;
    }
    std::printf("grid %zu %zu %d %zu %zu %zu %d %zu\n", n, override_voxels, windowed ? 1 : 0, count, last, sum, full, max_end);
}

int main() {
    static_assert(sizeof(size_t) == 8, "the window arithmetic is 64-bit");
    const size_t p29 = size_t(1) << 29, p30 = size_t(1) << 30, p32 = size_t(1) << 32;
    for (long long v : {-1024LL, -1LL, 0LL, 1LL, 1000LL, 1023LL, 1024LL, 1025LL, 2048LL, 65536LL, 65537LL, (long long)p29,
                        (long long)p30 - 1024, (long long)p30, (long long)p32})
        std::printf("valid %lld %d\n", v, crf::window_override_valid(v) ? 1 : 0);
    // the variable's text (printed in brackets: it may be empty)
    for (const char* text : {"", "0", "1024", "65536", "+2048", "1024abc", "abc", "-1", "1000", "1025", "1e5", "2048.0", "0x400",
                             "1073740800", "1073741824", "99999999999999999999", "-99999999999999999999"})
        std::printf("parse [%s] %lld\n", text, crf::parse_window_override(text));
    std::printf("parse null %lld\n", crf::parse_window_override(nullptr));
    // the default rule
    for (size_t n : {size_t(1), size_t(216611), p29, p29 + 1, p30 - 5, p30 - 4, p30 - 3, p30 - 1, p30, p30 + 1, 3 * p29 - 1,
                     3 * p29, 3 * p29 + 1, p32, p32 + 5})
        grid(n, 0);
    // an override
    for (size_t window : {size_t(1024), size_t(65536), p29, p30 - 1024})
        for (size_t n : {size_t(1), window - 1, window, window + 1, 2 * window - 1, 2 * window, 2 * window + 1, 3 * window - 1,
                         size_t(216611), size_t(1025), p30, p32 + 5})
            grid(n, window);
    std::printf("OK windows\n");
    return 0;
}
