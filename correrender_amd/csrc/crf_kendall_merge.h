// crf_kendall_merge.h -- the partition arithmetic of the inversion count behind crf_kendall_values_device and
// crf_field_kendall_similarity (kernels_kendall_similarity.hip): which sorted runs a merge level pairs, which piece of a
// pair's output a chunk owns, where the chunk's diagonals cut the two runs, and the scalar merge of a piece with its
// inversion count.  No HIP types: the kernel, its launcher and a host program (tests/native/kendall_merge.cpp) run the
// same functions.  Internal to libcorrfield.so.
//
// A level merges sorted runs of `run` values pairwise: pair p is the left run [2 p run, 2 p run + run) and the right run
// after it, both cut at n.  The last run of the array may be ragged; an odd last run is a pair whose right run is empty
// and is carried through (its merge is a copy).  The output of a pair is cut into chunks of `chunk` merged values; every
// pair has the same number of chunks, and those past the end of the last pair are empty.  The first level's runs are the
// tiles the tile kernel leaves sorted.
//
// Ties are taken from the left first.  A right-run value that lands after i values of the left run has len_left - i
// left-run values behind it, all of them strictly greater (the equal ones went first): that many inversions.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define CRF_KENDALL_HD __host__ __device__
#else
#define CRF_KENDALL_HD
#endif

namespace crf {
namespace kendall {

struct MergeChunk {
    uint32_t left, mid, right;  // left run [left, mid), right run [mid, right); mid == right: a carried odd run
    uint32_t first, last;       // the merged values [first, last) of the pair, counted from `left`; first == last: empty
};

// n <= 2^31 - 1 and 1 <= run: the number of levels until one run covers everything (at most 31)
CRF_KENDALL_HD inline int merge_levels(uint32_t n, uint32_t tile) {
    int levels = 0;
    for (uint64_t run = tile; run < n; run *= 2) levels++;
    return levels;
}

// run < n < 2^31 wherever a level is run, so 2 run < 2^32; kept in 64 bits all the same
CRF_KENDALL_HD inline uint32_t chunks_per_pair(uint64_t run, uint32_t chunk) { return uint32_t((2 * run + chunk - 1) / chunk); }
CRF_KENDALL_HD inline uint32_t pair_count(uint32_t n, uint64_t run) { return uint32_t((uint64_t(n) + 2 * run - 1) / (2 * run)); }
// pairs x chunks per pair: below n / chunk + n / (2 run) + 2, which fits 32 bits
CRF_KENDALL_HD inline uint32_t chunk_count(uint32_t n, uint64_t run, uint32_t chunk) {
    return pair_count(n, run) * chunks_per_pair(run, chunk);
}

CRF_KENDALL_HD inline MergeChunk merge_chunk(uint32_t n, uint64_t run, uint32_t chunk, uint32_t index) {
    const uint32_t per_pair = chunks_per_pair(run, chunk);
    const uint32_t pair = index / per_pair, within = index - pair * per_pair;
    const uint64_t start = uint64_t(pair) * 2 * run;  // below n for every index below chunk_count
    const uint64_t left = start < n ? start : n;
    const uint64_t mid = left + run < n ? left + run : n, right = left + 2 * run < n ? left + 2 * run : n;
    const uint64_t len = right - left, first = uint64_t(within) * chunk < len ? uint64_t(within) * chunk : len;
    MergeChunk c;
    c.left = uint32_t(left);
    c.mid = uint32_t(mid);
    c.right = uint32_t(right);
    c.first = uint32_t(first);
    c.last = uint32_t(first + chunk < len ? first + chunk : len);
    return c;
}

// How many of the first d merged values of left[0, nl) and right[0, nr) come from the left run (d <= nl + nr).  The
// interval halves every iteration and starts below 2^32: 32 iterations always suffice.
template <class T>
CRF_KENDALL_HD inline uint32_t merge_path(const T* left, uint32_t nl, const T* right, uint32_t nr, uint32_t d) {
    uint32_t lo = d > nr ? d - nr : 0u, hi = d < nl ? d : nl;
    for (int it = 0; it < 32 && lo < hi; it++) {
        const uint32_t i = lo + (hi - lo) / 2;  // i < hi <= nl, and 1 <= d - i <= nr
        if (left[i] <= right[d - i - 1u]) lo = i + 1u;
        else hi = i;
    }
    return lo;
}

// The merged values [d, d + steps) of left[0, nl) and right[0, nr), cut at nl + nr, into out[0 ..]; returns the
// inversions of the right-run values among them.  left_rest: the values of the whole left run from left[0] on (nl of
// them are here, the others lie behind and are greater still).  A count is at most steps x left_rest.
template <class T>
CRF_KENDALL_HD inline uint64_t merge_count(const T* left, uint32_t nl, const T* right, uint32_t nr, uint32_t d, uint32_t steps,
                                           uint32_t left_rest, T* out) {
    uint32_t i = merge_path(left, nl, right, nr, d), j = d - i;
    uint64_t inversions = 0;
    for (uint32_t k = 0; k < steps; k++) {
        if (i >= nl && j >= nr) break;
        const bool from_left = j >= nr || (i < nl && left[i] <= right[j]);
        if (from_left) {
            out[k] = left[i++];
        } else {
            inversions += left_rest - i;
            out[k] = right[j++];
        }
    }
    return inversions;
}

}  // namespace kendall
}  // namespace crf
