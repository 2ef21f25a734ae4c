// Drives the partition arithmetic of the Kendall inversion count (correrender_amd/csrc/crf_kendall_merge.h, no HIP in it)
// without a GPU, the way kernels_kendall_similarity.hip does: tiles of `tile` values sorted and counted with the tile
// kernel's two counts per value, then one level per doubling of the run -- a cut per chunk (merge_path at the chunk's first
// diagonal), the two pieces between a chunk's cuts copied into a buffer of exactly their size, merge_count per `per_thread`
// merged values.  Per level it checks that the chunks tile the output exactly once, that no index leaves its run, and
// that every pair of runs comes out sorted; at the end that the summed counts equal the O(n^2) count of strict
// inversions and that the output is the sorted input.  Sequences: random, few levels, all equal, ascending, descending,
// sawtooth, every left run above its right run; run counts 1, 2, 3, 5 and 65 with a last run of one value, a full one and
// a ragged one.  Also the arithmetic alone at 2^31 - 1 values.  tests/test_kendall_merge.py builds it plain and under
// AddressSanitizer + UBSan.  Prints "OK kendall merge".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "crf_kendall_merge.h"

using namespace crf::kendall;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

static uint64_t quadratic(const std::vector<uint32_t>& v) {
    uint64_t s = 0;
    for (size_t i = 0; i < v.size(); i++)
        for (size_t j = i + 1; j < v.size(); j++) s += v[j] < v[i] ? 1u : 0u;
    return s;
}

// the tile kernel: for each value, the earlier strictly greater values and its slot among the tile's values
static uint64_t sort_tiles(const std::vector<uint32_t>& src, uint32_t tile, std::vector<uint32_t>& dst) {
    const uint32_t n = uint32_t(src.size());
    uint64_t inversions = 0;
    std::vector<int> written(n, 0);
    for (uint32_t base = 0; base < n; base += tile) {
        const uint32_t len = std::min(tile, n - base);
        for (uint32_t p = 0; p < len; p++) {
            uint32_t greater = 0, slot = 0;
            for (uint32_t q = 0; q < len; q++) {
                const uint32_t v = src[base + q], mine = src[base + p];
                greater += (q < p && v > mine) ? 1u : 0u;
                slot += (v < mine || (q < p && v == mine)) ? 1u : 0u;
            }
            CHECK(slot < len);
            dst[base + slot] = src[base + p];
            written[base + slot]++;
            inversions += greater;
        }
    }
    for (uint32_t i = 0; i < n; i++) CHECK(written[i] == 1);
    return inversions;
}

static uint64_t merge_level(const std::vector<uint32_t>& src, uint64_t run, uint32_t chunk, uint32_t per_thread,
                            std::vector<uint32_t>& dst) {
    const uint32_t n = uint32_t(src.size());
    const uint32_t chunks = chunk_count(n, run, chunk);
    CHECK(chunks == pair_count(n, run) * chunks_per_pair(run, chunk));
    std::vector<uint32_t> cuts(chunks);
    for (uint32_t index = 0; index < chunks; index++) {  // the partition kernel
        const MergeChunk c = merge_chunk(n, run, chunk, index);
        CHECK(c.left <= c.mid && c.mid <= c.right && c.right <= n && c.left < n);
        CHECK(c.left % (2 * run) == 0 && c.mid - c.left <= run && c.right - c.mid <= run);
        CHECK(c.first <= c.last && c.last <= c.right - c.left && c.last - c.first <= chunk);
        cuts[index] = merge_path(src.data() + c.left, c.mid - c.left, src.data() + c.mid, c.right - c.mid, c.first);
    }
    std::vector<int> written(n, 0);
    uint64_t inversions = 0;
    for (uint32_t index = 0; index < chunks; index++) {  // the merge kernel
        const MergeChunk c = merge_chunk(n, run, chunk, index);
        if (c.first == c.last) continue;
        const uint32_t len_left = c.mid - c.left, len_right = c.right - c.mid;
        if (c.last != c.right - c.left) CHECK(index + 1 < chunks && merge_chunk(n, run, chunk, index + 1).left == c.left);
        const uint32_t i0 = cuts[index], i1 = c.last == c.right - c.left ? len_left : cuts[index + 1];
        CHECK(i0 <= i1 && i1 <= len_left && i0 <= c.first && i1 <= c.last);
        const uint32_t j0 = c.first - i0, j1 = c.last - i1;
        CHECK(j0 <= j1 && j1 <= len_right);
        const uint32_t nl = i1 - i0, nr = j1 - j0, len = c.last - c.first;
        CHECK(nl + nr == len);
        std::vector<uint32_t> in(len), out(len);  // exactly: the sanitizer sees any index outside the pieces
        for (uint32_t t = 0; t < len; t++) in[t] = t < nl ? src[c.left + i0 + t] : src[c.mid + j0 + (t - nl)];
        const uint32_t threads = (chunk + per_thread - 1) / per_thread;
        for (uint32_t thread = 0; thread < threads; thread++) {
            const uint32_t d = std::min(thread * per_thread, len);
            inversions += merge_count(in.data(), nl, in.data() + nl, nr, d, per_thread, len_left - i0, out.data() + d);
        }
        for (uint32_t t = 0; t < len; t++) {
            const uint32_t at = c.left + c.first + t;
            CHECK(at < c.right);
            dst[at] = out[t];
            written[at]++;
        }
    }
    for (uint32_t i = 0; i < n; i++) CHECK(written[i] == 1);
    for (uint64_t left = 0; left < n; left += 2 * run)
        CHECK(std::is_sorted(dst.begin() + left, dst.begin() + std::min<uint64_t>(left + 2 * run, n)));
    return inversions;
}

static void run_case(const std::vector<uint32_t>& data, uint32_t tile, uint32_t chunk, uint32_t per_thread) {
    const uint32_t n = uint32_t(data.size());
    std::vector<uint32_t> a(n), b(n);
    uint64_t inversions = n ? sort_tiles(data, tile, a) : 0;
    int levels = 0;
    for (uint64_t run = tile; run < n; run *= 2, levels++) {
        inversions += merge_level(a, run, chunk, per_thread, b);
        a.swap(b);
    }
    CHECK(levels == merge_levels(n, tile));
    CHECK(inversions == quadratic(data));
    std::vector<uint32_t> sorted(data);
    std::sort(sorted.begin(), sorted.end());
    CHECK(a == sorted);
}

static std::vector<uint32_t> sequence(int kind, uint32_t n, uint32_t tile, std::mt19937& rng) {
    std::vector<uint32_t> v(n);
    for (uint32_t i = 0; i < n; i++) {
        switch (kind) {
            case 0: v[i] = rng(); break;                                  // random, tie-free in practice
            case 1: v[i] = rng() % 5u; break;                             // a handful of levels
            case 2: v[i] = 7u; break;                                     // all equal
            case 3: v[i] = i; break;                                      // ascending: no inversion
            case 4: v[i] = n - i; break;                                  // descending: every pair
            case 5: v[i] = i % 3u; break;                                 // sawtooth
            case 6: v[i] = (n / tile + 1u - i / tile) * 4u + rng() % 4u; break;  // every run above the next
            default: v[i] = (i * 2654435761u) >> 20; break;
        }
    }
    return v;
}

int main() {
    std::mt19937 rng(12345);
    const uint32_t configs[][3] = {{16, 32, 4}, {5, 4, 3}, {64, 2048, 8}, {7, 64, 8}, {1, 2, 1}};  // tile, chunk, per thread
    const uint32_t run_counts[] = {1, 2, 3, 5, 65};
    int cases = 0;
    for (const auto& cfg : configs) {
        const uint32_t tile = cfg[0];
        for (uint32_t runs : run_counts) {
            // the last run: one value, a full one, a ragged one
            const uint32_t sizes[] = {(runs - 1) * tile + 1, runs * tile, (runs - 1) * tile + (tile + 1) / 2};
            for (uint32_t n : sizes)
                for (int kind = 0; kind < 8; kind++, cases++) run_case(sequence(kind, n, tile, rng), tile, cfg[1], cfg[2]);
        }
        run_case({}, tile, cfg[1], cfg[2]);
    }
    // the arithmetic alone at the largest size: 2^31 - 1 values, runs of 2^30 from tiles of 1024, chunks of 2048
    const uint32_t n = 0x7FFFFFFFu;
    CHECK(merge_levels(n, 1024) == 21);
    for (uint64_t run = 1024; run < n; run *= 2) {
        const uint32_t chunks = chunk_count(n, run, 2048);
        uint64_t covered = 0;
        const uint32_t probe[] = {0, 1, chunks / 2, chunks - 2, chunks - 1};
        for (uint32_t index : probe) {
            const MergeChunk c = merge_chunk(n, run, 2048, index);
            CHECK(c.left <= c.mid && c.mid <= c.right && c.right <= n && c.first <= c.last && c.last <= c.right - c.left);
        }
        const uint32_t per_pair = chunks_per_pair(run, 2048);
        for (uint32_t pair = 0; pair < pair_count(n, run); pair += std::max(1u, pair_count(n, run) / 64)) {
            const MergeChunk first = merge_chunk(n, run, 2048, pair * per_pair), last = merge_chunk(n, run, 2048, (pair + 1) * per_pair - 1);
            CHECK(first.first == 0 && first.left == last.left && last.last == last.right - last.left);
        }
        const MergeChunk end = merge_chunk(n, run, 2048, chunks - 1);
        covered = uint64_t(end.left) + end.last;
        CHECK(covered == n);
    }
    std::printf("%d cases\nOK kendall merge\n", cases);
    return 0;
}
