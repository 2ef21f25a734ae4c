// crf_rank_sort.h -- what the users of the device-wide radix sort share: kernels_rank_similarity.hip, which holds the sort
// and ranks with it, and kernels_kendall_similarity.hip, which sorts twice with it and counts inversions.  The key of a
// value, the head bits and run bounds of sorted keys, the scratch layout of a sort, and the launchers of the sort's front
// end.  Device and launcher code; internal to libcorrfield.so.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "crf_internal.h"

namespace crf {
namespace ranksort {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxTileKeys = 4096;    // 16 keys per thread; key and payload staged in 32 KiB of LDS
constexpr int kMaxSortBlocks = 1024;  // rows of the [block][digit] table
constexpr uint32_t kNanKey = 0xFFFFFFFFu;
constexpr uint32_t kNone = 0xFFFFFFFFu;

// u = bits(v == 0 ? +0 : v), key = u ^ (sign ? 0xFFFFFFFF : 0x80000000); every NaN gets 0xFFFFFFFF, which no other value
// has and which sorts last
__device__ __forceinline__ uint32_t sort_key(float v) {
    if (v != v) return kNanKey;
    const uint32_t u = __float_as_uint(v == 0.0f ? 0.0f : v);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// the head bits of the 64 positions a wave looks at: bit l set where position tile + p is the first of a run
__device__ __forceinline__ unsigned long long head_bits(const uint32_t* __restrict__ keys, uint32_t tile, uint32_t p,
                                                        uint32_t tile_len) {
    bool head = false;
    if (p < tile_len) {
        const uint32_t i = tile + p;
        head = i == 0u || keys[i] != keys[i - 1u];
    }
    return __ballot(head);
}

// The heads of one tile of sorted keys, in LDS, for a block of kThreads threads.
struct RunWords {
    unsigned long long heads[kMaxTileKeys / 64];  // word j: positions 64 j .. 64 j + 63 of the tile
    uint32_t word_before[kMaxTileKeys / 64];      // 1 + tile position of the last head in the words before j, 0
    uint32_t word_after[kMaxTileKeys / 64];       // tile position of the first head in the words after j, kNone
};

// fills `words` for the tile; ends with a barrier.  rounds = ceil(tile_keys / kThreads), block-uniform.
__device__ __forceinline__ void tile_head_words(const uint32_t* __restrict__ keys, uint32_t tile, uint32_t tile_len,
                                                int rounds, RunWords& words) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int r = 0; r < rounds; r++) {
        const uint32_t p0 = uint32_t(r * kThreads + w * 64);
        const unsigned long long m = head_bits(keys, tile, p0 + uint32_t(lane), tile_len);
        if (lane == 0) words.heads[p0 >> 6] = m;
    }
    __syncthreads();
    if (w == 0) {  // one wave: at most 64 words
        const int count = rounds * kWaves;
        const unsigned long long m = lane < count ? words.heads[lane] : 0ull;
        uint32_t last = m != 0ull ? uint32_t(lane * 64 + 64 - __clzll((long long)m)) : 0u;
        uint32_t first = m != 0ull ? uint32_t(lane * 64 + __ffsll((long long)m) - 1) : kNone;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {  // inclusive: max from the left, min from the right
            const uint32_t l = __shfl_up(last, off), f = __shfl_down(first, off);
            if (lane >= off) last = max(last, l);
            if (lane + off < 64) first = min(first, f);
        }
        const uint32_t l = __shfl_up(last, 1), f = __shfl_down(first, 1);
        words.word_before[lane] = lane > 0 ? l : 0u;
        words.word_after[lane] = lane < 63 ? f : kNone;
    }
    __syncthreads();
}

// run start *s and run end *e of tile position p = 64 j + lane, as array positions.  carry_start: the last head before
// the tile; carry_end: the first head after it.
__device__ __forceinline__ void run_bounds(const RunWords& words, uint32_t tile, uint32_t p, uint32_t carry_start,
                                           uint32_t carry_end, uint32_t* s, uint32_t* e) {
    const int lane = threadIdx.x & 63;
    const uint32_t j = p >> 6;
    const unsigned long long m = words.heads[j];
    const unsigned long long upto = m & (~0ull >> (63 - lane));                     // heads at or before p
    const unsigned long long past = lane == 63 ? 0ull : m & (~0ull << (lane + 1));  // heads after p
    if (upto != 0ull) *s = tile + j * 64u + uint32_t(63 - __clzll((long long)upto));
    else *s = words.word_before[j] != 0u ? tile + words.word_before[j] - 1u : carry_start;
    if (past != 0ull) *e = tile + j * 64u + uint32_t(__ffsll((long long)past) - 1);
    else *e = words.word_after[j] != kNone ? tile + words.word_after[j] : carry_end;
}

// CRF_RANK_TILE_KEYS (tests): fewer keys per tile, so that a few thousand values span many tiles and blocks
uint32_t tile_keys_setting();

inline size_t align256(size_t v) { return (v + 255) & ~size_t(255); }

// scratch layout of a sort of n keys
struct SortLayout {
    size_t keys[2], payload[2], hist, nans, table, first_head, last_head, bytes;
    explicit SortLayout(size_t n) {
        size_t at = 0;
        auto take = [&](size_t b) {
            const size_t o = at;
            at += align256(b);
            return o;
        };
        for (int i = 0; i < 2; i++) keys[i] = take(n * 4), payload[i] = take(n * 4);
        hist = take(4 * 256 * 4);
        nans = take(4);
        table = take(size_t(kMaxSortBlocks) * 256 * 4);
        const size_t heads = (n + tile_keys_setting() - 1) / tile_keys_setting();
        first_head = take(heads * 4);
        last_head = take(heads * 4);
        bytes = at;
    }
};

// The sort proper: n (key, payload) pairs in keys[cur] / payload[cur], stably by key, least significant digit first
// (rank_count_kernel, rank_scan_kernel, similarity_rank_sort_kernel per digit).  host_hist: the four 256-bin digit
// histograms of the keys, digit 0 = the low byte, on the host; d_hist: the same on the device.  A digit whose histogram
// has one bin holding everything is skipped.  identity: the payload of key i is i, and payload[cur] is not read.  Returns
// the index of the buffers that hold the result; *passes: the passes run (0: nothing moved, and with `identity` no
// payload was written).  wanted_blocks: the persistent grid before CRF_SIMILARITY_MAX_BLOCKS.
int sort_pairs(uint32_t* const keys[2], uint32_t* const payload[2], int cur, uint32_t n, const uint32_t* host_hist,
               const uint32_t* d_hist, uint32_t* d_table, bool identity, int wanted_blocks, hipStream_t s, int* passes);

// For every tile t of the sorted keys: head_before[t], the position of the last head before the tile (0 for tile 0, which
// starts with one), and head_after[t], the position of the first head after it (n: none).  rank_heads_kernel, then
// rank_carry_kernel.  Both arrays hold ceil(n / tile_keys_setting()) entries (SortLayout: last_head, first_head).
void launch_run_carries(const uint32_t* keys, uint32_t n, int wanted_blocks, uint32_t* head_after, uint32_t* head_before,
                        hipStream_t s);

// x and y of every sample of the job, member after member, both NaN where either is (rank_mask_pairs_kernel)
hipError_t launch_mask_pairs(const SimilarityJob& job, float* out_x, float* out_y, hipStream_t s);

}  // namespace ranksort
}  // namespace crf
