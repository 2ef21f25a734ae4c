// kernels_kendall_similarity.hip -- Kendall's tau-b over ALL samples of two device arrays (crf_kendall_values_device) or of
// two resident fields (crf_field_kendall_similarity); reference: computeKendall<int64_t>, src/Calculators/
// Correlation.cpp:423-455, as computeFieldSimilarity<double> calls it (Similarity.cpp:134-143).  The device leaves four
// integers -- the pairs kept n, the tie sums n1 (x) and n2 (y), and S, the strict inversions of the y sequence in the order
// (x ascending, y ascending among equal x) -- and the host forms the value from them (crf_similarity_tail.h).  Everything
// on the device is an integer; every sum across blocks is a 64-bit integer atomic.  The result is exact and the same from
// call to call.
//
// As in kernels_rank_similarity.hip, whose sort this file uses (crf_rank_sort.h), no block waits on another block: every
// ordering between blocks is a kernel boundary.
//
//   kendall_keys_kernel      one read of x and y: the sort keys of both (a pair with a NaN on either side gets the NaN key
//                            twice), the four digit histograms of either, the number of such pairs
//   sort by the y key, the x key as payload (sort_pairs: rank_count_kernel, rank_scan_kernel, similarity_rank_sort_kernel)
//   rank_heads_kernel, rank_carry_kernel over the sorted y keys, then
//   kendall_run_start_kernel every position i of the y-sorted order gets the start s of its run of equal y: equal y, equal
//                            s; smaller y, smaller s.  Writes (x key, s) as the next sort's (key, payload) and adds
//                            i - s over the non-NaN positions, which over a run of m is m (m - 1) / 2: n2
//   sort by the x key, s as payload: each pass is stable, so the y order survives among equal x
//   rank_heads_kernel, rank_carry_kernel, kendall_run_start_kernel over the sorted x keys, sums only: n1
//   similarity_kendall_tile_kernel
//                            leaves every run of T values of the s sequence sorted and counts the inversions inside it:
//                            one O(T^2) loop over the tile in LDS (reads at one address: a broadcast); for each owned
//                            value, the earlier strictly greater values (its inversions) and the smaller values plus the
//                            equal ones before it (its sorted slot)
//   once per level (crf_kendall_merge.h has the partition and the scalar merge):
//     kendall_partition_kernel
//                            one thread per chunk of merged values: the merge-path search in global memory that
//                            cuts the pair's two runs at the chunk's first diagonal
//     similarity_kendall_merge_kernel
//                            merges neighbouring sorted runs pairwise from one buffer into the other; a block owns
//                            chunks: the two pieces between its cuts are staged in LDS, every thread merges kPerThread
//                            values of them and counts, the merged chunk goes out through LDS in order.  The name
//                            crf_last_kernel_name reports.
//
// The pairs with a NaN sort last in both orders, share the largest s and are left out of the count: only the first n
// entries of the s sequence are counted, so nothing is compacted.
//
// Where this departs from the pipeline first proposed for it, and why:
//   * The masking is fused into the key kernel for crf_kendall_values_device (one read of the inputs, which stay
//     untouched).  The field entry masks with rank_mask_pairs_kernel as the Spearman path does, into the halves of the
//     ping-pong that the first sort pass has not written yet, so the call needs no sample arrays of its own: 16 bytes per
//     sample against the Spearman call's 24.
//   * n1 and n2 are sums of i - s over the positions, not of m - 1 halved: the run end is not needed, and nothing is
//     divided.
//   * One key kernel makes both key arrays and all eight histograms; the x histograms stay valid for the second sort
//     because the first only permutes the x keys.
//   * The cuts of a level are found by a kernel of their own, one thread per chunk, not by the block that merges the
//     chunk: a search is up to 31 dependent loads, which a block would sit out once per chunk and which half a million
//     threads sit out together.  It costs 4 bytes per chunk of scratch and a launch per level.
//   * A level's chunk holds 256, 512, 1024 or 2048 merged values: the smallest of them that holds a whole pair of runs, so
//     that the levels after small tiles run full chunks with every thread merging.
//   * T = 256 comes from a measured sweep (64 to 1024; profiles/field_kendall_similarity.md): the O(T^2) tile kernel
//     grows with T, the number of merge levels falls with it.  The full chunk of 2048 values was not swept: a full level
//     already moves its 8 bytes per sample at about 3 TB/s.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "crf_internal.h"
#include "crf_kendall_merge.h"
#include "crf_rank_sort.h"
#include "crf_similarity_chunks.h"

namespace crf {
namespace {

using namespace chunks;
using namespace ranksort;
using namespace kendall;

constexpr int kMaxTile = 2048;  // values of a tile of the inversion count: 8 per thread, 8 KiB of LDS
constexpr int kDefaultTile = 256;
constexpr int kMaxTileRounds = kMaxTile / kThreads;
constexpr int kPerThread = 8;  // merged values per thread of a full chunk: 2048 values, twice 8 KiB of LDS

// Merged values per thread at the level that merges runs of `run` values: the fewest of 1, 2, 4, 8 with which one chunk
// holds a whole pair, so that the first levels after small tiles fill their chunks and keep every thread merging; 8 from
// pairs of 2048 values on.
int level_per_thread(unsigned long long run) {
    int per = 1;
    while (per < kPerThread && uint64_t(kThreads) * per < 2 * run) per *= 2;
    return per;
}

// the sum over the block, on thread 0.  `waves`: kWaves entries.
__device__ __forceinline__ unsigned long long block_sum(unsigned long long v, unsigned long long* waves) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long all = 0;
    if (threadIdx.x == 0)
#pragma unroll
        for (int i = 0; i < kWaves; i++) all += waves[i];
    __syncthreads();  // `waves` may be reused
    return all;
}

// hist_y, hist_x: 4 x 256 counters each, digit 0 = the low byte;  nans: one counter.  All zeroed by the launcher.
// x and y are only read and may be the same array.
__global__ __launch_bounds__(kThreads) void kendall_keys_kernel(const float* x, const float* y, uint32_t n,
                                                                uint32_t* __restrict__ keys_y, uint32_t* __restrict__ keys_x,
                                                                uint32_t* __restrict__ hist_y, uint32_t* __restrict__ hist_x,
                                                                uint32_t* __restrict__ nans) {
    __shared__ uint32_t bins[8 * 256];  // y, then x
    for (int i = threadIdx.x; i < 8 * 256; i += kThreads) bins[i] = 0u;
    __syncthreads();
    uint32_t nan_count = 0u;
    const uint32_t stride = gridDim.x * uint32_t(kThreads);
    // n < 2^31 and stride <= 2^18: i + stride does not wrap
    for (uint32_t i = blockIdx.x * uint32_t(kThreads) + threadIdx.x; i < n; i += stride) {
        uint32_t kx = sort_key(x[i]), ky = sort_key(y[i]);
        if (kx == kNanKey || ky == kNanKey) kx = ky = kNanKey, nan_count++;
        keys_y[i] = ky;
        keys_x[i] = kx;
#pragma unroll
        for (int d = 0; d < 4; d++) {
            atomicAdd(&bins[d * 256 + ((ky >> (8 * d)) & 255u)], 1u);
            atomicAdd(&bins[1024 + d * 256 + ((kx >> (8 * d)) & 255u)], 1u);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nan_count += __shfl_xor(nan_count, off);
    if ((threadIdx.x & 63) == 0 && nan_count != 0u) atomicAdd(nans, nan_count);
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * 256; i += kThreads) {
        const uint32_t vy = bins[i], vx = bins[1024 + i];
        if (vy != 0u) atomicAdd(&hist_y[i], vy);
        if (vx != 0u) atomicAdd(&hist_x[i], vx);
    }
}

// Over sorted keys: *ties += the sum of i - s over the positions whose key is not the NaN key.  WRITE: next_keys[i] =
// payload[i] and next_payload[i] = s (neither may be `keys` or `payload`: other tiles still read those).
template <bool WRITE>
__global__ __launch_bounds__(kThreads) void kendall_run_start_kernel(const uint32_t* __restrict__ keys,
                                                                     const uint32_t* __restrict__ payload, uint32_t n,
                                                                     uint32_t tile_keys, uint32_t tiles,
                                                                     const uint32_t* __restrict__ head_before,
                                                                     uint32_t* __restrict__ next_keys,
                                                                     uint32_t* __restrict__ next_payload,
                                                                     unsigned long long* __restrict__ ties) {
    __shared__ RunWords words;
    __shared__ unsigned long long waves[kWaves];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int rounds = int((tile_keys + kThreads - 1) / kThreads);
    unsigned long long sum = 0;  // every term is below 2^31, a thread adds at most 2^31 of them
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t tile = t * tile_keys;  // tiles * tile_keys < n + tile_keys: below 2^32
        const uint32_t tile_len = min(tile_keys, n - tile);
        tile_head_words(keys, tile, tile_len, rounds, words);
        const uint32_t carry_start = head_before[t];
        for (int r = 0; r < rounds; r++) {
            const uint32_t p = uint32_t(r * kThreads + w * 64 + lane);
            if (p >= tile_len) continue;
            uint32_t s, e;
            run_bounds(words, tile, p, carry_start, n, &s, &e);
            const uint32_t i = tile + p;
            if (keys[i] != kNanKey) sum += i - s;
            if (WRITE) {  // i < n: tile_len cuts the last tile
                next_keys[i] = payload[i];
                next_payload[i] = s;
            }
        }
        __syncthreads();
    }
    const unsigned long long all = block_sum(sum, waves);
    if (threadIdx.x == 0 && all != 0ull) atomicAdd(ties, all);
}

// dst: every tile of `tile` values of src[0, n) sorted (equal values in their order); *inversions += the strict
// inversions inside the tiles.  tile <= kMaxTile.
__global__ __launch_bounds__(kThreads) void similarity_kendall_tile_kernel(const uint32_t* __restrict__ src, uint32_t n,
                                                                           uint32_t tile, uint32_t tiles,
                                                                           uint32_t* __restrict__ dst,
                                                                           unsigned long long* __restrict__ inversions) {
    __shared__ uint32_t vals[kMaxTile];
    __shared__ unsigned long long waves[kWaves];
    const int rounds = int((tile + kThreads - 1) / kThreads);  // <= kMaxTileRounds
    unsigned long long sum = 0;
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t base = t * tile;  // tiles * tile < n + tile: below 2^32
        const uint32_t len = min(tile, n - base);
        uint32_t mine[kMaxTileRounds], greater[kMaxTileRounds], slot[kMaxTileRounds];  // both counts at most kMaxTile
#pragma unroll
        for (int r = 0; r < kMaxTileRounds; r++) {
            const uint32_t p = uint32_t(r * kThreads) + threadIdx.x;
            mine[r] = greater[r] = slot[r] = 0u;
            if (r < rounds && p < len) vals[p] = mine[r] = src[base + p];
        }
        __syncthreads();
        for (uint32_t q = 0; q < len; q++) {
            const uint32_t v = vals[q];
#pragma unroll
            for (int r = 0; r < kMaxTileRounds; r++) {
                if (r < rounds) {  // block-uniform
                    const bool before = q < uint32_t(r * kThreads) + threadIdx.x;
                    greater[r] += (before && v > mine[r]) ? 1u : 0u;
                    slot[r] += (v < mine[r] || (before && v == mine[r])) ? 1u : 0u;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kMaxTileRounds; r++) {
            const uint32_t p = uint32_t(r * kThreads) + threadIdx.x;
            if (r < rounds && p < len) {
                sum += greater[r];
                // always: the slots of a tile are a permutation of [0, len); never store outside the array
                if (slot[r] < len) dst[base + slot[r]] = mine[r];
            }
        }
        __syncthreads();
    }
    const unsigned long long all = block_sum(sum, waves);
    if (threadIdx.x == 0 && all != 0ull) atomicAdd(inversions, all);
}

// cuts[index]: how many values of the left run lie before the first merged value of chunk `index`
__global__ __launch_bounds__(kThreads) void kendall_partition_kernel(const uint32_t* __restrict__ src, uint32_t n,
                                                                     unsigned long long run, uint32_t chunk,
                                                                     uint32_t chunks, uint32_t* __restrict__ cuts) {
    const uint32_t stride = gridDim.x * uint32_t(kThreads);
    // chunks < 2^31 and stride <= 2^21: index + stride does not wrap
    for (uint32_t index = blockIdx.x * uint32_t(kThreads) + threadIdx.x; index < chunks; index += stride) {
        const MergeChunk c = merge_chunk(n, run, chunk, index);
        cuts[index] = merge_path(src + c.left, c.mid - c.left, src + c.mid, c.right - c.mid, c.first);
    }
}

// One level: dst = src with the sorted runs of `run` values merged pairwise; *inversions += the inversions between the
// two runs of every pair.  PER merged values per thread, chunks of kThreads x PER.
template <int PER>
__global__ __launch_bounds__(kThreads) void similarity_kendall_merge_kernel(const uint32_t* __restrict__ src, uint32_t n,
                                                                            unsigned long long run, uint32_t chunks,
                                                                            const uint32_t* __restrict__ cuts,
                                                                            uint32_t* __restrict__ dst,
                                                                            unsigned long long* __restrict__ inversions) {
    constexpr uint32_t chunk = uint32_t(kThreads * PER);
    __shared__ uint32_t in[chunk];   // the left piece, then the right piece
    __shared__ uint32_t out[chunk];  // the merged chunk
    __shared__ unsigned long long waves[kWaves];
    unsigned long long sum = 0;  // the block's share of S, which is at most n0 < 2^61
    for (uint32_t index = blockIdx.x; index < chunks; index += gridDim.x) {
        const MergeChunk c = merge_chunk(n, run, chunk, index);
        if (c.first == c.last) continue;  // block-uniform: past the end of the last pair
        const uint32_t len_left = c.mid - c.left;
        // the last chunk of a pair ends where the pair does; every other one where the next chunk of the pair begins
        const uint32_t i0 = cuts[index], i1 = c.last == c.right - c.left ? len_left : cuts[index + 1u];
        const uint32_t j0 = c.first - i0, j1 = c.last - i1;
        const uint32_t nl = i1 - i0, nr = j1 - j0, len = c.last - c.first;  // nl + nr == len <= chunk
        for (uint32_t t = threadIdx.x; t < len; t += kThreads)  // c.left + i1 <= c.mid and c.mid + j1 <= c.right <= n
            in[t] = t < nl ? src[c.left + i0 + t] : src[c.mid + j0 + (t - nl)];
        __syncthreads();
        const uint32_t d = min(threadIdx.x * uint32_t(PER), len);
        sum += merge_count(in, nl, in + nl, nr, d, uint32_t(PER), len_left - i0, out + d);
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < len; t += kThreads) {
            const uint32_t at = c.left + c.first + t;
            if (at < n) dst[at] = out[t];  // always: c.left + c.last <= c.right <= n; never store outside the array
        }
        // no barrier here: the next chunk's first barrier lies between these reads of out[] and its next writes
    }
    const unsigned long long all = block_sum(sum, waves);
    if (threadIdx.x == 0 && all != 0ull) atomicAdd(inversions, all);
}

// CRF_KENDALL_TILE_KEYS (tests): shorter sorted runs out of the tile kernel, so that a few thousand values take many
// merge levels
uint32_t tile_setting() {
    const char* v = getenv("CRF_KENDALL_TILE_KEYS");
    const int t = (v && *v) ? atoi(v) : 0;
    return t > 0 ? uint32_t(std::min(t, kMaxTile)) : uint32_t(kDefaultTile);
}

// the sort's scratch, then what this file adds to it
struct KendallLayout {
    SortLayout sort;
    size_t hist_x, counters, cuts, bytes;
    explicit KendallLayout(size_t n) : sort(n) {
        hist_x = sort.bytes;
        counters = hist_x + align256(4 * 256 * 4);
        cuts = counters + align256(3 * sizeof(unsigned long long));  // n2, n1, S
        uint32_t most = 1;  // chunks of a level: of every level that any number of kept pairs up to n can take
        for (unsigned long long run = tile_setting(); run < n; run *= 2)
            most = std::max(most, chunk_count(uint32_t(n), run, uint32_t(kThreads * level_per_thread(run))));
        bytes = cuts + align256(size_t(most) * 4);
    }
};

// The pairs are keys: y keys in keys[0], x keys in payload[0] of the layout, every histogram filled.  Leaves n1, n2 and S
// in `counts` (host) and synchronises the stream.
hipError_t count_from_keys(uint32_t n, unsigned char* scratch, const KendallLayout& lay, int wanted, hipStream_t s,
                           hipEvent_t ev_end, unsigned long long* kept, long long counts[3]) {
    auto u32 = [&](size_t offset) { return reinterpret_cast<uint32_t*>(scratch + offset); };
    uint32_t* keys[2] = {u32(lay.sort.keys[0]), u32(lay.sort.keys[1])};
    uint32_t* payload[2] = {u32(lay.sort.payload[0]), u32(lay.sort.payload[1])};
    unsigned long long* counters = reinterpret_cast<unsigned long long*>(scratch + lay.counters);
    uint32_t host_y[4 * 256 + 64], host_x[4 * 256];  // y: the histograms, then the NaN counter
    if (hipError_t e = hipMemcpyAsync(host_y, scratch + lay.sort.hist, sizeof host_y, hipMemcpyDeviceToHost, s); e != hipSuccess)
        return e;
    if (hipError_t e = hipMemcpyAsync(host_x, scratch + lay.hist_x, sizeof host_x, hipMemcpyDeviceToHost, s); e != hipSuccess)
        return e;
    if (hipError_t e = hipStreamSynchronize(s); e != hipSuccess) return e;
    const uint32_t pairs = n - host_y[4 * 256];
    *kept = pairs;

    const uint32_t tile_keys = tile_keys_setting();
    const uint32_t tiles = (n + tile_keys - 1) / tile_keys;
    const uint32_t run_blocks = grid_blocks(tiles, wanted);
    uint32_t* head_after = u32(lay.sort.first_head);
    uint32_t* head_before = u32(lay.sort.last_head);
    int cur = sort_pairs(keys, payload, 0, n, host_y, u32(lay.sort.hist), u32(lay.sort.table), false, wanted, s, nullptr);
    launch_run_carries(keys[cur], n, wanted, head_after, head_before, s);
    hipLaunchKernelGGL((kendall_run_start_kernel<true>), dim3(run_blocks), dim3(kThreads), 0, s, keys[cur], payload[cur], n,
                       tile_keys, tiles, head_before, keys[cur ^ 1], payload[cur ^ 1], counters + 0);
    cur ^= 1;
    cur = sort_pairs(keys, payload, cur, n, host_x, u32(lay.hist_x), u32(lay.sort.table), false, wanted, s, nullptr);
    launch_run_carries(keys[cur], n, wanted, head_after, head_before, s);
    hipLaunchKernelGGL((kendall_run_start_kernel<false>), dim3(run_blocks), dim3(kThreads), 0, s, keys[cur], payload[cur], n,
                       tile_keys, tiles, head_before, nullptr, nullptr, counters + 1);

    // the s sequence is payload[cur]; the x keys are done with, and the merge levels go to and fro between them and the
    // other key buffer
    if (pairs > 1u) {
        const uint32_t tile = tile_setting();
        const uint32_t count_tiles = (pairs + tile - 1) / tile;
        hipLaunchKernelGGL(similarity_kendall_tile_kernel, dim3(grid_blocks(count_tiles, wanted)), dim3(kThreads), 0, s,
                           payload[cur], pairs, tile, count_tiles, keys[cur], counters + 2);
        int at = cur;
        for (unsigned long long run = tile; run < pairs; run *= 2) {
            const int per = level_per_thread(run);
            const uint32_t chunks = chunk_count(pairs, run, uint32_t(kThreads * per));
            hipLaunchKernelGGL(kendall_partition_kernel, dim3(grid_blocks((chunks + kThreads - 1) / kThreads, 8 * wanted)),
                               dim3(kThreads), 0, s, keys[at], pairs, run, uint32_t(kThreads * per), chunks, u32(lay.cuts));
            const auto merge = per == 1 ? similarity_kendall_merge_kernel<1> : per == 2 ? similarity_kendall_merge_kernel<2>
                             : per == 4 ? similarity_kendall_merge_kernel<4> : similarity_kendall_merge_kernel<8>;
            hipLaunchKernelGGL(merge, dim3(grid_blocks(chunks, wanted)), dim3(kThreads), 0, s, keys[at], pairs, run, chunks,
                               u32(lay.cuts), keys[at ^ 1], counters + 2);
            at ^= 1;
        }
    }
    if (ev_end) (void)hipEventRecord(ev_end, s);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    unsigned long long host[3];
    if (hipError_t e = hipMemcpyAsync(host, counters, sizeof host, hipMemcpyDeviceToHost, s); e != hipSuccess) return e;
    if (hipError_t e = hipStreamSynchronize(s); e != hipSuccess) return e;
    counts[0] = (long long)host[1];  // n1: ties of x
    counts[1] = (long long)host[0];  // n2: ties of y
    counts[2] = (long long)host[2];  // S
    return hipSuccess;
}

// zeroes the histograms and counters, makes the keys of (x, y) and runs the count
hipError_t count_pairs(const float* d_x, const float* d_y, uint32_t n, unsigned char* scratch, const KendallLayout& lay,
                       hipStream_t s, hipEvent_t ev_end, unsigned long long* kept, long long counts[3]) {
    int cus = 0;
    if (hipError_t e = compute_units(&cus); e != hipSuccess) return e;
    // four blocks of four waves per CU, as the sort
    const int wanted = std::min(4 * cus, kMaxSortBlocks);
    auto u32 = [&](size_t offset) { return reinterpret_cast<uint32_t*>(scratch + offset); };
    if (hipError_t e = hipMemsetAsync(scratch + lay.sort.hist, 0, lay.sort.table - lay.sort.hist, s); e != hipSuccess) return e;
    if (hipError_t e = hipMemsetAsync(scratch + lay.hist_x, 0, lay.cuts - lay.hist_x, s); e != hipSuccess) return e;
    const uint32_t key_blocks = grid_blocks((n + kThreads - 1) / kThreads, wanted);
    hipLaunchKernelGGL(kendall_keys_kernel, dim3(key_blocks), dim3(kThreads), 0, s, d_x, d_y, n, u32(lay.sort.keys[0]),
                       u32(lay.sort.payload[0]), u32(lay.sort.hist), u32(lay.hist_x), u32(lay.sort.nans));
    return count_from_keys(n, scratch, lay, wanted, s, ev_end, kept, counts);
}

}  // namespace

size_t kendall_scratch_bytes(size_t count) { return KendallLayout(count).bytes; }

hipError_t launch_kendall_values(const float* d_x, const float* d_y, size_t count, unsigned char* scratch, hipStream_t s,
                                 hipEvent_t ev_begin, hipEvent_t ev_end, unsigned long long* kept, long long counts[3],
                                 LaunchInfo* info) {
    if (info) info->kernel_name = "similarity_kendall_merge_kernel";
    if (count < 1 || count > size_t(0x7FFFFFFF) || !scratch || !kept || !counts) return hipErrorInvalidValue;
    if (ev_begin) (void)hipEventRecord(ev_begin, s);
    return count_pairs(d_x, d_y, uint32_t(count), scratch, KendallLayout(count), s, ev_end, kept, counts);
}

hipError_t launch_kendall_similarity(const SimilarityJob& job, unsigned char* scratch, hipStream_t s, hipEvent_t ev_begin,
                                     hipEvent_t ev_end, unsigned long long* kept, long long counts[3], LaunchInfo* info) {
    if (info) info->kernel_name = "similarity_kendall_merge_kernel";
    const size_t n = size_t(job.members) * job.num_voxels;
    if (job.members < 1 || job.num_voxels < 1 || job.num_voxels >= (size_t(1) << 30) || n > size_t(0x7FFFFFFF) || !scratch ||
        !kept || !counts)
        return hipErrorInvalidValue;
    const KendallLayout lay(n);
    // the masked samples go where the first sort pass writes only after the key kernel has read them
    float* x = reinterpret_cast<float*>(scratch + lay.sort.keys[1]);
    float* y = reinterpret_cast<float*>(scratch + lay.sort.payload[1]);
    if (ev_begin) (void)hipEventRecord(ev_begin, s);
    if (hipError_t e = launch_mask_pairs(job, x, y, s); e != hipSuccess) return e;
    return count_pairs(x, y, uint32_t(n), scratch, lay, s, ev_end, kept, counts);
}

}  // namespace crf
