// kernels_rank_similarity.hip -- fractional ranks of a device array by a device-wide radix sort (crf_rank_values_device;
// reference: computeRanks, src/Calculators/Correlation.cpp:277-303) and the rank form of the whole-field similarity
// (crf_field_rank_similarity, Spearman; reference: Similarity.cpp:134-143).  Every other sort of this library is a
// per-voxel sort in registers and LDS; this is the only one across the device.
//
// No block waits on another block anywhere in this file: no look-back, no flags, no spinning.  Every ordering between
// blocks is a kernel boundary.
//
//   rank_keys_kernel       one read of the values: the 32-bit sort key of every value (u = bits(v == 0 ? +0 : v),
//                          key = u ^ (sign ? 0xFFFFFFFF : 0x80000000); every NaN gets 0xFFFFFFFF, which no other value
//                          has and which sorts last), all four 256-bin digit histograms (LDS counters, flushed with
//                          integer atomics) and the number of NaNs.  The host reads the histograms back: a digit whose
//                          histogram has one bin holding everything is skipped (constant data: all four).
//   per digit that is not skipped, LSD, each pass stable:
//     rank_count_kernel    the digit counts of every block's share of the keys
//     rank_scan_kernel     one block per digit: exclusive scan in the order [digit][block]
//     similarity_rank_sort_kernel
//                          the stable scatter, tile by tile (the sort proper, and the name crf_last_kernel_name
//                          reports): the offset of a key among the equal digits of its tile comes
//                          from wave-level __ballot match masks (8 ballots per key) and per-wave counts in LDS; key and
//                          payload are staged through LDS in digit order, so that the stores of one digit are contiguous
//   rank_heads_kernel      per tile of the sorted keys: position of the first and of the last head (key[i] != key[i-1])
//   rank_carry_kernel      one block: for every tile the last head before it and the first head after it
//   rank_assign_kernel     run start s and run end e of every sorted position from the tile's head bit masks and the two
//                          carries; rank = fl32(float(s + 1) + float(e - s - 1) * 0.5f) with s an exact integer, scattered
//                          to ranks[payload].  A run may cross any number of tiles or be the whole array.  The scatter
//                          to input order is 4-byte stores at random addresses: the largest single launch.
//   rank_mask_pairs_kernel the samples of the field similarity, in the chunk shape of kernels_similarity.hip: x and y of
//                          every pair, both NaN where either is
//
// Where this departs from the shape first proposed for it, and why (none of it rests on a measurement: the file was
// written before its first run on a device; profiles/field_rank_similarity.md has what was measured afterwards):
//   * Blocks own CONTIGUOUS shares of the tiles and carry their digit offsets from tile to tile in LDS, so the table
//     that is scanned has 256 x blocks entries (at most 1 MiB) instead of 256 x tiles (128 MiB per pass at 2^30 keys), and
//     its scan is one small block per digit (a single block walking the whole table took 0.22 ms per pass, half the
//     time of a sort of 2^24 keys).  Stability holds as with a table per tile: the shares are in index order.
//   * The field similarity does not compact its samples.  A pair with a NaN is masked to (NaN, NaN) in place of being
//     removed: the sort puts NaNs last and leaves them unranked, the moments kernel leaves pairs with a NaN out, and the
//     ranks of the kept values are those of the compacted arrays.  Compaction with an atomic cursor would order the
//     samples differently from call to call and with them the fp64 sums (the value must be reproducible bit for bit); a
//     counted compaction costs a second read of both fields.  Masking needs neither, nor the two compacted arrays.
//   * The first scatter pass takes the identity as payload instead of reading one.
//
// The sort proper (sort_pairs), the run carries and the masking are also what kernels_kendall_similarity.hip starts from:
// crf_rank_sort.h declares them and holds the device helpers both files use.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <limits>
#include <vector>

#include "crf_internal.h"
#include "crf_rank_sort.h"
#include "crf_similarity_chunks.h"

namespace crf {
namespace {

using namespace chunks;
using namespace ranksort;  // the constants, sort_key, head_bits, run_bounds, SortLayout (crf_rank_sort.h)

constexpr int kMaxRounds = kMaxTileKeys / kThreads;
constexpr int kCarryThreads = 1024;
constexpr int kMaskThreads = 256;

// the keys [first, last) of block b: whole tiles, in index order over the blocks
__device__ __forceinline__ void block_share(uint32_t n, uint32_t tile_keys, uint32_t tiles_per_block, uint32_t* first,
                                            uint32_t* last) {
    const unsigned long long a = (unsigned long long)blockIdx.x * tiles_per_block * tile_keys;
    const unsigned long long b = a + (unsigned long long)tiles_per_block * tile_keys;
    *first = uint32_t(a < n ? a : n);
    *last = uint32_t(b < n ? b : n);
}

// exclusive prefix sum over the 256 threads of a block; `waves` holds kWaves counters.  *total: the sum, on every thread
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* waves, uint32_t* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) waves[w] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < kWaves; i++) {
        const uint32_t t = waves[i];
        before += i < w ? t : 0u;
        all += t;
    }
    __syncthreads();  // `waves` may be reused
    *total = all;
    return before + incl - v;
}

// hist: 4 x 256 counters, digit 0 = the low byte;  nans: one counter.  Both zeroed by the launcher.
__global__ __launch_bounds__(kThreads) void rank_keys_kernel(const float* __restrict__ values, uint32_t n,
                                                             uint32_t* __restrict__ keys, uint32_t* __restrict__ hist,
                                                             uint32_t* __restrict__ nans) {
    __shared__ uint32_t bins[4 * 256];
    for (int i = threadIdx.x; i < 4 * 256; i += kThreads) bins[i] = 0u;
    __syncthreads();
    uint32_t nan_count = 0u;
    const uint32_t stride = gridDim.x * uint32_t(kThreads);
    // n < 2^31 and stride <= 2^18: i + stride does not wrap
    for (uint32_t i = blockIdx.x * uint32_t(kThreads) + threadIdx.x; i < n; i += stride) {
        const uint32_t k = sort_key(values[i]);
        keys[i] = k;
        nan_count += k == kNanKey ? 1u : 0u;
#pragma unroll
        for (int d = 0; d < 4; d++) atomicAdd(&bins[d * 256 + ((k >> (8 * d)) & 255u)], 1u);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nan_count += __shfl_xor(nan_count, off);
    if ((threadIdx.x & 63) == 0 && nan_count != 0u) atomicAdd(nans, nan_count);
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * 256; i += kThreads) {
        const uint32_t v = bins[i];
        if (v != 0u) atomicAdd(&hist[i], v);
    }
}

// table[block][digit]: how many keys of the block's share have the digit
__global__ __launch_bounds__(kThreads) void rank_count_kernel(const uint32_t* __restrict__ keys, uint32_t n, int shift,
                                                              uint32_t tile_keys, uint32_t tiles_per_block,
                                                              uint32_t* __restrict__ table) {
    __shared__ uint32_t bins[256];
    bins[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t first, last;
    block_share(n, tile_keys, tiles_per_block, &first, &last);
    for (uint32_t i = first + threadIdx.x; i < last; i += kThreads) atomicAdd(&bins[(keys[i] >> shift) & 255u], 1u);
    __syncthreads();
    table[size_t(blockIdx.x) * 256 + threadIdx.x] = bins[threadIdx.x];
}

// One block per digit d, in place: table[b][d] becomes the destination of the first key with digit d of block b -- the
// keys with a smaller digit (from the digit's histogram of rank_keys_kernel) plus those with digit d in the blocks
// before b.  A column has at most kMaxSortBlocks = 4 x 256 entries: four consecutive ones per thread.
static_assert(kMaxSortBlocks == 4 * kThreads, "rank_scan_kernel: four blocks per thread");
__global__ __launch_bounds__(kThreads) void rank_scan_kernel(uint32_t* __restrict__ table, uint32_t blocks,
                                                             const uint32_t* __restrict__ hist) {
    __shared__ uint32_t waves[kWaves];
    __shared__ uint32_t start;
    const uint32_t d = blockIdx.x;
    uint32_t total;
    const uint32_t smaller = block_exclusive_scan(hist[threadIdx.x], waves, &total);
    if (threadIdx.x == d) start = smaller;
    __syncthreads();
    uint32_t c[4], sum = 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t b = threadIdx.x * 4 + j;
        c[j] = b < blocks ? table[size_t(b) * 256 + d] : 0u;
        sum += c[j];
    }
    uint32_t at = start + block_exclusive_scan(sum, waves, &total);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t b = threadIdx.x * 4 + j;
        if (b < blocks) table[size_t(b) * 256 + d] = at;
        at += c[j];
    }
}

// The stable scatter of one pass.  A tile is cut into four consecutive spans, one per wave; a wave walks its span 64
// keys at a time.  identity: the payload of key i is i (the first pass that runs).
__global__ __launch_bounds__(kThreads) void similarity_rank_sort_kernel(const uint32_t* __restrict__ src_keys,
                                                                const uint32_t* __restrict__ src_payload, uint32_t n,
                                                                int shift, int identity, uint32_t tile_keys,
                                                                uint32_t tiles_per_block, const uint32_t* __restrict__ table,
                                                                uint32_t* __restrict__ dst_keys,
                                                                uint32_t* __restrict__ dst_payload) {
    __shared__ uint32_t stage_keys[kMaxTileKeys];
    __shared__ uint32_t stage_payload[kMaxTileKeys];
    __shared__ uint32_t wave_count[kWaves][256];  // per wave and digit: keys seen so far, then the keys of earlier waves
    __shared__ uint32_t tile_start[256];          // first staging slot of a digit
    __shared__ uint32_t global_base[256];         // destination of staging slot s with digit d: global_base[d] + s (mod 2^32)
    __shared__ uint32_t digit_next[256];          // destination of the block's next key with digit d
    __shared__ uint32_t waves[kWaves];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    volatile uint32_t* my_count = wave_count[w];
    uint32_t first, last;
    block_share(n, tile_keys, tiles_per_block, &first, &last);
    digit_next[threadIdx.x] = table[size_t(blockIdx.x) * 256 + threadIdx.x];
    const int rounds = int((tile_keys + kThreads - 1) / kThreads);  // <= kMaxRounds
    const uint32_t span = uint32_t(rounds) * 64u;
    for (uint32_t tile = first; tile < last; tile += tile_keys) {
        const uint32_t tile_len = min(tile_keys, last - tile);
#pragma unroll
        for (int i = 0; i < kWaves; i++) wave_count[i][threadIdx.x] = 0u;
        __syncthreads();
        uint32_t key[kMaxRounds], payload[kMaxRounds], offset[kMaxRounds];
#pragma unroll
        for (int r = 0; r < kMaxRounds; r++) {
            key[r] = payload[r] = offset[r] = 0u;
            if (r < rounds) {  // block-uniform
                const uint32_t p = uint32_t(w) * span + uint32_t(r) * 64u + uint32_t(lane);
                const bool valid = p < tile_len;
                if (valid) {
                    key[r] = src_keys[tile + p];
                    payload[r] = identity ? tile + p : src_payload[tile + p];
                }
                const uint32_t d = (key[r] >> shift) & 255u;
                unsigned long long peers = __ballot(valid);
#pragma unroll
                for (int bit = 0; bit < 8; bit++) {
                    const bool one = (d >> bit) & 1u;
                    const unsigned long long m = __ballot(valid && one);
                    peers &= one ? m : ~m;
                }
                // the lanes of this wave that hold the same digit in this round; in a wave the LDS operations below
                // run in program order, the reads of all lanes before the leaders' writes
                const uint32_t seen = my_count[d];
                const uint32_t rank = uint32_t(__popcll(peers & below));
                offset[r] = seen + rank;
                if (valid && rank == 0u) my_count[d] = seen + uint32_t(__popcll(peers));
            }
        }
        __syncthreads();
        {  // thread d: the digit's keys in earlier waves, its first staging slot and its destination
            const int d = threadIdx.x;
            uint32_t before = 0u;
#pragma unroll
            for (int i = 0; i < kWaves; i++) {
                const uint32_t c = wave_count[i][d];
                wave_count[i][d] = before;
                before += c;
            }
            uint32_t total;
            const uint32_t start = block_exclusive_scan(before, waves, &total);
            tile_start[d] = start;
            global_base[d] = digit_next[d] - start;
            digit_next[d] += before;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kMaxRounds; r++) {
            if (r < rounds) {
                const uint32_t p = uint32_t(w) * span + uint32_t(r) * 64u + uint32_t(lane);
                if (p < tile_len) {
                    const uint32_t d = (key[r] >> shift) & 255u;
                    const uint32_t slot = tile_start[d] + wave_count[w][d] + offset[r];
                    if (slot < uint32_t(kMaxTileKeys)) {  // always: the slots of a tile are a permutation of [0, tile_len)
                        stage_keys[slot] = key[r];
                        stage_payload[slot] = payload[r];
                    }
                }
            }
        }
        __syncthreads();
        for (uint32_t s = threadIdx.x; s < tile_len; s += kThreads) {
            const uint32_t k = stage_keys[s];
            const uint32_t at = global_base[(k >> shift) & 255u] + s;
            if (at < n) {  // always, when the table counts what this kernel scatters; never store outside the arrays
                dst_keys[at] = k;
                dst_payload[at] = stage_payload[s];
            }
        }
        __syncthreads();
    }
}

// first_head[t]: position of the first head of tile t, kNone if it has none;  last_head[t]: 1 + position of the last, 0
__global__ __launch_bounds__(kThreads) void rank_heads_kernel(const uint32_t* __restrict__ keys, uint32_t n,
                                                              uint32_t tile_keys, uint32_t tiles,
                                                              uint32_t* __restrict__ first_head,
                                                              uint32_t* __restrict__ last_head) {
    __shared__ uint32_t lo[kWaves], hi[kWaves];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int rounds = int((tile_keys + kThreads - 1) / kThreads);
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t tile = t * tile_keys;  // tiles * tile_keys < n + tile_keys: below 2^32
        const uint32_t tile_len = min(tile_keys, n - tile);
        uint32_t first = kNone, last = 0u;
        for (int r = 0; r < rounds; r++) {
            const uint32_t p0 = uint32_t(r * kThreads + w * 64);
            const unsigned long long m = head_bits(keys, tile, p0 + uint32_t(lane), tile_len);
            if (m != 0ull) {
                first = min(first, tile + p0 + uint32_t(__ffsll((long long)m) - 1));
                last = max(last, tile + p0 + uint32_t(64 - __clzll((long long)m)));
            }
        }
        if (lane == 0) lo[w] = first, hi[w] = last;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int i = 1; i < kWaves; i++) first = min(first, lo[i]), last = max(last, hi[i]);
            first_head[t] = first;
            last_head[t] = last;
        }
        __syncthreads();
    }
}

// One block.  In place: last_head[t] becomes the position of the last head BEFORE tile t (0 for tile 0, which starts
// with one), first_head[t] the position of the first head AFTER tile t (n: none).  Every thread owns a contiguous piece.
__global__ __launch_bounds__(kCarryThreads) void rank_carry_kernel(uint32_t* __restrict__ first_head,
                                                                   uint32_t* __restrict__ last_head, uint32_t tiles,
                                                                   uint32_t n) {
    __shared__ uint32_t lo[kCarryThreads], hi[kCarryThreads];
    const uint32_t per = (tiles + kCarryThreads - 1) / kCarryThreads;
    const uint32_t a = min(uint32_t(threadIdx.x) * per, tiles), b = min(a + per, tiles);
    uint32_t first = kNone, last = 0u;
    for (uint32_t t = a; t < b; t++) first = min(first, first_head[t]), last = max(last, last_head[t]);
    lo[threadIdx.x] = first;
    hi[threadIdx.x] = last;
    __syncthreads();
    uint32_t before = 0u, after = kNone;
    for (uint32_t i = 0; i < threadIdx.x; i++) before = max(before, hi[i]);
    for (uint32_t i = threadIdx.x + 1; i < kCarryThreads; i++) after = min(after, lo[i]);
    for (uint32_t t = a; t < b; t++) {  // forward: what lies before
        const uint32_t own = last_head[t];
        last_head[t] = before != 0u ? before - 1u : 0u;
        before = max(before, own);
    }
    for (uint32_t t = b; t > a; t--) {  // backward: what lies after
        const uint32_t own = first_head[t - 1u];
        first_head[t - 1u] = after != kNone ? after : n;
        after = min(after, own);
    }
}

__global__ __launch_bounds__(kThreads) void rank_assign_kernel(const uint32_t* __restrict__ keys,
                                                               const uint32_t* __restrict__ payload, int identity,
                                                               uint32_t n, uint32_t tile_keys, uint32_t tiles,
                                                               const uint32_t* __restrict__ head_after,
                                                               const uint32_t* __restrict__ head_before,
                                                               float* __restrict__ ranks) {
    __shared__ RunWords words;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int rounds = int((tile_keys + kThreads - 1) / kThreads);
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t tile = t * tile_keys;
        const uint32_t tile_len = min(tile_keys, n - tile);
        tile_head_words(keys, tile, tile_len, rounds, words);
        const uint32_t carry_start = head_before[t], carry_end = head_after[t];
        for (int r = 0; r < rounds; r++) {
            const uint32_t p = uint32_t(r * kThreads + w * 64 + lane);
            if (p >= tile_len) continue;
            uint32_t s, e;
            run_bounds(words, tile, p, carry_start, carry_end, &s, &e);
            const uint32_t i = tile + p;
            // one fp32 addition of two rounded terms (the product by 0.5 is exact)
            const float rank = keys[i] == kNanKey ? std::numeric_limits<float>::quiet_NaN()
                                                  : __fadd_rn(float(s + 1u), __fmul_rn(float(e - s - 1u), 0.5f));
            const uint32_t to = identity ? i : payload[i];
            if (to < n) ranks[to] = rank;  // always: the payloads are a permutation of [0, n)
        }
        __syncthreads();
    }
}

// out_x / out_y: members x voxels floats, member after member
template <bool VEC>
__global__ __launch_bounds__(kMaskThreads) void rank_mask_pairs_kernel(Samples s, float* __restrict__ out_x,
                                                                       float* __restrict__ out_y) {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (uint32_t chunk = blockIdx.x; chunk < s.chunks; chunk += gridDim.x) {
        const uint32_t m = chunk / s.chunks_per_member;
        const uint32_t base = (chunk - m * s.chunks_per_member) * uint32_t(kMaskThreads * kLaneVoxels);
        float x[kLaneVoxels], y[kLaneVoxels];
        load_chunk<VEC, kMaskThreads, false>(s.x[m], s.y[m], base, s.voxels, x, y);
        const size_t member = size_t(m) * s.voxels;
#pragma unroll
        for (int e = 0; e < kLaneVoxels; e++) {
            const uint32_t v = base + threadIdx.x * 4 + (e >> 2) * kMaskThreads * 4 + (e & 3);
            if (v < s.voxels) {
                const bool ok = x[e] == x[e] && y[e] == y[e];
                out_x[member + v] = ok ? x[e] : nan;
                out_y[member + v] = ok ? y[e] : nan;
            }
        }
    }
}

}  // namespace

namespace ranksort {

uint32_t tile_keys_setting() {
    const char* v = getenv("CRF_RANK_TILE_KEYS");
    const int t = (v && *v) ? atoi(v) : 0;
    return t > 0 ? uint32_t(std::min(t, kMaxTileKeys)) : uint32_t(kMaxTileKeys);
}

int sort_pairs(uint32_t* const keys[2], uint32_t* const payload[2], int cur, uint32_t n, const uint32_t* host_hist,
               const uint32_t* d_hist, uint32_t* d_table, bool identity, int wanted_blocks, hipStream_t s, int* passes) {
    const uint32_t tile_keys = tile_keys_setting();
    const uint32_t tiles = (n + tile_keys - 1) / tile_keys;
    const uint32_t sort_blocks = grid_blocks(tiles, wanted_blocks);
    const uint32_t tiles_per_block = (tiles + sort_blocks - 1) / sort_blocks;
    const uint32_t used_blocks = (tiles + tiles_per_block - 1) / tiles_per_block;  // the rest would own nothing
    int run = 0;
    for (int d = 0; d < 4; d++) {
        bool one_bin = false;
        for (int b = 0; b < 256; b++) one_bin = one_bin || host_hist[d * 256 + b] == n;
        if (one_bin) continue;  // every key has this digit: the pass would be the identity
        const int shift = 8 * d;
        hipLaunchKernelGGL(rank_count_kernel, dim3(used_blocks), dim3(kThreads), 0, s, keys[cur], n, shift, tile_keys,
                           tiles_per_block, d_table);
        hipLaunchKernelGGL(rank_scan_kernel, dim3(256), dim3(kThreads), 0, s, d_table, used_blocks, d_hist + d * 256);
        hipLaunchKernelGGL(similarity_rank_sort_kernel, dim3(used_blocks), dim3(kThreads), 0, s, keys[cur], payload[cur], n, shift,
                           int(identity && run == 0), tile_keys, tiles_per_block, d_table, keys[cur ^ 1], payload[cur ^ 1]);
        cur ^= 1;
        run++;
    }
    if (passes) *passes = run;
    return cur;
}

void launch_run_carries(const uint32_t* keys, uint32_t n, int wanted_blocks, uint32_t* head_after, uint32_t* head_before,
                        hipStream_t s) {
    const uint32_t tile_keys = tile_keys_setting();
    const uint32_t tiles = (n + tile_keys - 1) / tile_keys;
    hipLaunchKernelGGL(rank_heads_kernel, dim3(grid_blocks(tiles, wanted_blocks)), dim3(kThreads), 0, s, keys, n, tile_keys,
                       tiles, head_after, head_before);
    hipLaunchKernelGGL(rank_carry_kernel, dim3(1), dim3(kCarryThreads), 0, s, head_after, head_before, tiles, n);
}

hipError_t launch_mask_pairs(const SimilarityJob& job, float* out_x, float* out_y, hipStream_t s) {
    int cus = 0;
    if (hipError_t e = compute_units(&cus); e != hipSuccess) return e;
    const Samples smp = make_samples(job, kMaskThreads);
    const uint32_t blocks = grid_blocks(smp.chunks, std::min(4 * cus, kMaxSortBlocks));
    if (job.vec16)
        hipLaunchKernelGGL((rank_mask_pairs_kernel<true>), dim3(blocks), dim3(kMaskThreads), 0, s, smp, out_x, out_y);
    else
        hipLaunchKernelGGL((rank_mask_pairs_kernel<false>), dim3(blocks), dim3(kMaskThreads), 0, s, smp, out_x, out_y);
    return hipGetLastError();
}

}  // namespace ranksort

size_t rank_sort_scratch_bytes(size_t count) { return SortLayout(count).bytes; }

size_t rank_similarity_scratch_bytes(int members, size_t num_voxels) {
    const size_t n = size_t(members) * num_voxels;
    return SortLayout(n).bytes + 2 * align256(n * 4) + 2 * align256(size_t(members) * sizeof(float*));
}

hipError_t launch_rank_values(const float* d_values, size_t count, float* d_ranks, unsigned char* scratch, hipStream_t s,
                              hipEvent_t ev_begin, hipEvent_t ev_end, unsigned long long* ranked, LaunchInfo* info) {
    if (info) info->kernel_name = "similarity_rank_sort_kernel";
    if (count > size_t(0x7FFFFFFF) || !scratch) return hipErrorInvalidValue;
    if (ranked) *ranked = 0;
    if (ev_begin) (void)hipEventRecord(ev_begin, s);
    if (count == 0) {
        if (ev_end) (void)hipEventRecord(ev_end, s);
        return hipSuccess;
    }
    int cus = 0;
    if (hipError_t e = compute_units(&cus); e != hipSuccess) return e;
    const uint32_t n = uint32_t(count);
    const SortLayout lay(count);
    auto u32 = [&](size_t offset) { return reinterpret_cast<uint32_t*>(scratch + offset); };
    uint32_t* keys[2] = {u32(lay.keys[0]), u32(lay.keys[1])};
    uint32_t* payload[2] = {u32(lay.payload[0]), u32(lay.payload[1])};
    const uint32_t tile_keys = tile_keys_setting();
    const uint32_t tiles = (n + tile_keys - 1) / tile_keys;
    // four blocks of four waves per CU, as the streaming kernels of kernels_similarity.hip
    const int wanted = std::min(4 * cus, kMaxSortBlocks);

    if (hipError_t e = hipMemsetAsync(scratch + lay.hist, 0, lay.table - lay.hist, s); e != hipSuccess) return e;
    const uint32_t key_blocks = grid_blocks((n + kThreads - 1) / kThreads, wanted);
    hipLaunchKernelGGL(rank_keys_kernel, dim3(key_blocks), dim3(kThreads), 0, s, d_values, n, keys[0], u32(lay.hist),
                       u32(lay.nans));
    uint32_t host[4 * 256 + 64];  // the histograms, then the NaN counter
    if (hipError_t e = hipMemcpyAsync(host, scratch + lay.hist, sizeof host, hipMemcpyDeviceToHost, s); e != hipSuccess)
        return e;
    if (hipError_t e = hipStreamSynchronize(s); e != hipSuccess) return e;
    if (ranked) *ranked = count - host[4 * 256];

    int passes = 0;
    const int cur = sort_pairs(keys, payload, 0, n, host, u32(lay.hist), u32(lay.table), true, wanted, s, &passes);
    const int identity = passes == 0;
    const uint32_t rank_blocks = grid_blocks(tiles, wanted);
    launch_run_carries(keys[cur], n, wanted, u32(lay.first_head), u32(lay.last_head), s);
    hipLaunchKernelGGL(rank_assign_kernel, dim3(rank_blocks), dim3(kThreads), 0, s, keys[cur], payload[cur], identity, n,
                       tile_keys, tiles, u32(lay.first_head), u32(lay.last_head), d_ranks);
    if (ev_end) (void)hipEventRecord(ev_end, s);
    return hipGetLastError();
}

hipError_t launch_rank_similarity(const SimilarityJob& job, unsigned char* scratch, hipStream_t s, hipEvent_t ev_begin,
                                  hipEvent_t ev_end, LaunchInfo* info) {
    if (info) info->kernel_name = "similarity_rank_sort_kernel";
    const size_t n = size_t(job.members) * job.num_voxels;
    if (job.members < 1 || job.num_voxels < 1 || job.num_voxels >= (size_t(1) << 30) || n > size_t(0x7FFFFFFF) ||
        !job.workspace || !scratch)
        return hipErrorInvalidValue;
    const size_t sort_bytes = SortLayout(n).bytes;
    float* rank_x = reinterpret_cast<float*>(scratch + sort_bytes);
    float* rank_y = reinterpret_cast<float*>(scratch + sort_bytes + align256(n * 4));
    const float** table_x = reinterpret_cast<const float**>(scratch + sort_bytes + 2 * align256(n * 4));
    const float** table_y = table_x + align256(size_t(job.members) * sizeof(float*)) / sizeof(float*);
    // the two rank arrays as the moments kernels take their fields: one slice per member
    std::vector<const float*> slices(size_t(job.members) * 2);
    for (int m = 0; m < job.members; m++) {
        slices[size_t(m)] = rank_x + size_t(m) * job.num_voxels;
        slices[size_t(job.members + m)] = rank_y + size_t(m) * job.num_voxels;
    }
    const size_t table_bytes = size_t(job.members) * sizeof(float*);
    if (hipError_t e = hipMemcpyAsync(table_x, slices.data(), table_bytes, hipMemcpyHostToDevice, s); e != hipSuccess) return e;
    if (hipError_t e = hipMemcpyAsync(table_y, slices.data() + job.members, table_bytes, hipMemcpyHostToDevice, s); e != hipSuccess)
        return e;
    if (ev_begin) (void)hipEventRecord(ev_begin, s);
    if (hipError_t e = launch_mask_pairs(job, rank_x, rank_y, s); e != hipSuccess) return e;
    // in place: the values are read once, into keys, before the first rank is stored
    if (hipError_t e = launch_rank_values(rank_x, n, rank_x, scratch, s, nullptr, nullptr, nullptr, nullptr); e != hipSuccess) return e;
    if (hipError_t e = launch_rank_values(rank_y, n, rank_y, scratch, s, nullptr, nullptr, nullptr, nullptr); e != hipSuccess) return e;
    // slice m starts m * num_voxels floats into a 256-byte aligned array
    SimilarityJob ranks{table_x, table_y, job.members, job.num_voxels, job.num_voxels % 4 == 0, job.workspace};
    if (hipError_t e = launch_similarity_moments(ranks, s, nullptr, nullptr, nullptr); e != hipSuccess) return e;
    if (ev_end) (void)hipEventRecord(ev_end, s);
    return hipGetLastError();
}

}  // namespace crf
