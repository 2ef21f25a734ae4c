// crf_windows.h -- the window arithmetic of a grid whose member volumes are too large for one launch (api.cpp:
// ensure_windows, NarrowScope::select_window, for_each_window).  The kernels address a member with 32-bit byte offsets,
// and their out-of-range sentinel offset (crf_device.h: kOutOfRangeOffset = 0xFFFFFFF0) must lie beyond the end of every
// member: a member volume of 4 GiB or more is evaluated in WINDOWS, one launch each, through member-pointer tables advanced
// by the window's first voxel.  Plain C++17 without HIP types, like crf_host_copy.h and two_vector_route.h, so that the
// arithmetic is testable on a machine without a GPU and at sizes no GPU test can reach (tests/test_windows.py).  Everything
// is computed in size_t.  Internal to libcorrfield.so.
#pragma once
#include <cerrno>
#include <cstddef>
#include <cstdlib>

namespace crf {

// 2 GiB of every fp32 member per launch
constexpr size_t kDefaultWindowVoxels = size_t(1) << 29;
// A window starts at a multiple of this many voxels (4 KiB of an fp32 member): every window stays as aligned as the
// members themselves, the argument ensure_host_ranges makes for its ranges.
constexpr size_t kWindowGranule = 1024;
// the first byte offset a kernel cannot use (kOutOfRangeOffset)
constexpr size_t kWindowedFromBytes = size_t(0xFFFFFFF0u);

// the largest window a kernel can address: the last multiple of kWindowGranule whose fp32 bytes stay below the limit
constexpr size_t kMaxWindowVoxels = (kWindowedFromBytes / sizeof(float)) / kWindowGranule * kWindowGranule;

// CRF_WINDOW_VOXELS (a test switch, read by crf_set_grid): 0 or unset keeps the default rule; a positive multiple of
// kWindowGranule, at most kMaxWindowVoxels, is the window size; anything else is refused.
inline bool window_override_valid(long long value) {
    if (value < 0) return false;
    const size_t v = static_cast<size_t>(value);
    return v % kWindowGranule == 0 && v <= kMaxWindowVoxels;
}

// The variable's text as crf_set_grid takes it: null or empty is 0 (unset); one decimal integer that
// window_override_valid accepts is that value; everything else -- trailing text, a fraction, an overflow, a refused value --
// is -1, and crf_set_grid fails.
inline long long parse_window_override(const char* text) {
    if (!text || !*text) return 0;
    char* end = nullptr;
    errno = 0;
    const long long value = std::strtoll(text, &end, 10);
    if (errno != 0 || end == text || *end != '\0' || !window_override_valid(value)) return -1;
    return value;
}

// the voxels of a full window; override_voxels: a valid CRF_WINDOW_VOXELS, 0 for none
inline size_t window_voxels(size_t override_voxels) { return override_voxels ? override_voxels : kDefaultWindowVoxels; }

// Whether a grid of n voxels is evaluated in windows.  Default rule: its fp32 member reaches kWindowedFromBytes (first at
// n = 2^30 - 4).  With an override: it has more voxels than one window.
inline bool grid_windowed(size_t n, size_t override_voxels) {
    return override_voxels ? n > override_voxels : n * sizeof(float) >= kWindowedFromBytes;
}

// the windows of `window` voxels that cover n voxels (written without n + window - 1, which could wrap)
inline size_t windows_covering(size_t n, size_t window) { return n / window + (n % window ? 1 : 0); }

// the launches a per-voxel evaluation of the grid takes: 1 for an ordinary grid
inline size_t window_count(size_t n, size_t override_voxels) {
    return grid_windowed(n, override_voxels) ? windows_covering(n, window_voxels(override_voxels)) : 1;
}

// first voxel of window w
inline size_t window_first(size_t w, size_t window) { return w * window; }

// voxels of window w of a windowed grid of n voxels: every window but the last is full
inline size_t window_length(size_t n, size_t w, size_t window) {
    const size_t first = window_first(w, window);
    if (first >= n) return 0;
    return n - first < window ? n - first : window;
}

}  // namespace crf
