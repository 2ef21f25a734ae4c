// crf_host_copy.h -- the host half of a host-output evaluation (api.cpp, compute_to_host): how the grid is cut into voxel
// ranges, how a range is shared among the copier threads, how destination pages are faulted in ahead of the copy, and
// the loop every copier thread runs.  No HIP and no context: tests/native/host_copy.cpp drives all of it with a scripted
// producer on a real SpinPool (crf_pool.h).  Internal to libcorrfield.so.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <immintrin.h>
#include <sys/mman.h>

constexpr int kMaxHostChunks = 16;  // z-chunks of a host-output evaluation (kernel of chunk i+1 under the D2H of chunk i)

namespace crf {

constexpr int kMadvPopulateWrite = 23;  // MADV_POPULATE_WRITE (Linux 5.14), not in every libc header
constexpr size_t kPage = 4096;

// The populate step of fault_in: 0 when [addr, addr + len) is resident and writable afterwards.  A seam: a test passes a
// function that fails, which is what a kernel before 5.14 or a mapping that refuses the advice looks like.
using PopulateFn = int (*)(void* addr, size_t len);
inline int populate_write(void* addr, size_t len) { return madvise(addr, len, kMadvPopulateWrite); }

// faults [lo, hi) of the caller's buffer in (write access); mode 0: leave it to the copy, 1: touch, 2: populate
inline void fault_in(char* base, size_t lo, size_t hi, int mode, PopulateFn populate = populate_write) {
    if (mode == 0 || lo >= hi) return;
    const uintptr_t a = (reinterpret_cast<uintptr_t>(base) + lo) & ~(kPage - 1);
    const uintptr_t e = (reinterpret_cast<uintptr_t>(base) + hi + kPage - 1) & ~(kPage - 1);
    if (mode == 2 && populate(reinterpret_cast<void*>(a), e - a) == 0) return;
    // fallback / mode 1: one write per page.  The bytes written are inside the caller's buffer and are overwritten by
    // the result afterwards (copy_ranges never faults a share in that it has copied).
    for (size_t off = lo; off < hi; off += kPage) static_cast<volatile char*>(base)[off] = 0;
    static_cast<volatile char*>(base)[hi - 1] = 0;
}

// thread w's share of byte range [r_lo, r_hi) among `workers` threads, split on page boundaries
inline void thread_share(size_t r_lo, size_t r_hi, int w, int workers, size_t* lo, size_t* hi) {
    const size_t per = (((r_hi - r_lo) + size_t(workers) - 1) / size_t(workers) + kPage - 1) & ~(kPage - 1);
    *lo = std::min(r_hi, r_lo + size_t(w) * per);
    *hi = std::min(r_hi, *lo + per);
}

// "3,6,6" -> {3, 6, 6}: the comma-separated shares of 64 of CRF_HOST_SHARES (host_range_partition decides if they count)
inline std::vector<int> parse_shares(const char* text) {
    std::vector<int> v;
    for (const char* q = text; q && *q;) {
        v.push_back(atoi(q));
        while (*q && *q != ',') q++;
        if (*q == ',') q++;
    }
    return v;
}

// The voxel ranges of a host-output evaluation over n voxels: the first voxel of every range, then n.  Range lengths are
// multiples of 1024 voxels (4 KiB: every range stays as aligned as the members themselves).
// forced >= 1 (experiments): that many equal ranges, at most max_chunks.
// Else shares of 64, `shares` when it is 1..max_chunks entries that sum to 64 (experiments), the default otherwise.
inline std::vector<size_t> host_range_partition(size_t n, int forced, const std::vector<int>& shares, int max_chunks) {
    std::vector<size_t> first{0};
    if (forced >= 1) {
        size_t per = (n + size_t(forced) - 1) / size_t(forced);
        per = (per + 1023) & ~size_t(1023);
        for (size_t at = per; at < n && int(first.size()) < max_chunks; at += per) first.push_back(at);
    } else {
        // Shares of 64, consecutive ranges alternating between two streams: 3 6 6 6 6 6 6 6 6 5 4 2 2.  The two streams'
        // kernels run concurrently and share the link; with the FIRST range half the size of the others the kernel ends
        // alternate (B0 A0 B1 A1 ...), so results land every ~1/11 of the run from early on, the copier threads always
        // have a landed range to move, and the last ranges are small: only their copy is not hidden behind a kernel.
        // Same-process A/B at 256^3 (tools/measure_host_path.py ab, profiles/r03_host_boundary_variants.txt), resident /
        // fresh destination: 13 ranges 1.326 / 1.391 ms; 11 ranges (4 8x6 6 3 2 1) 1.336 / 1.452; 8 staggered ranges
        // 1.369 / 1.467; 8 shrinking ranges 16 14 11 8 6 4 3 2 (pairs end together) 1.378 / 1.527; 8 equal 1.450 / 1.644.
        std::vector<int> use = {3, 6, 6, 6, 6, 6, 6, 6, 6, 5, 4, 2, 2};
        int sum = 0;
        for (int s : shares) sum += s;
        if (sum == 64 && shares.size() >= 1 && shares.size() <= size_t(max_chunks)) use = shares;
        size_t acc = 0;
        for (int j = 0; j + 1 < int(use.size()); j++) {
            acc += size_t(use[size_t(j)]);
            const size_t at = (n / 64 * acc + 1023) & ~size_t(1023);
            if (at > first.back() && at < n) first.push_back(at);
        }
    }
    first.push_back(n);
    return first;
}

// What copier thread w of `threads` does in one evaluation: for every range j (voxels first[j] .. first[j + 1]) wait
// until ready[j] leaves 0, then copy its share of the range from the staging buffer to the caller's; while it waits it
// faults its shares of the ranges ahead in.  ready[j] < 0: the evaluation failed, nothing more is copied.
inline int copy_ranges(char* dst, const char* src, const size_t* first, int ranges, int threads, const std::atomic<int>* ready,
                       int fault_mode, int w, PopulateFn populate = populate_write) {
    if (w >= threads) return 0;
    int faulted = 0;  // ranges whose share this thread has faulted in, or copied, already
    for (int j = 0; j < ranges; j++) {
        size_t lo, hi;
        while (ready[j].load(std::memory_order_acquire) == 0) {
            if (faulted < ranges) {
                thread_share(first[faulted] * sizeof(float), first[faulted + 1] * sizeof(float), w, threads, &lo, &hi);
                fault_in(dst, lo, hi, fault_mode, populate);
                faulted++;
            } else {
                _mm_pause();
            }
        }
        if (ready[j].load(std::memory_order_acquire) < 0) return 0;  // the evaluation failed: nothing to copy
        thread_share(first[j] * sizeof(float), first[j + 1] * sizeof(float), w, threads, &lo, &hi);
        if (lo < hi) memcpy(dst + lo, src + lo, hi - lo);
        // a range that landed before this thread got to fault it in: touching it now would write into the result
        faulted = std::max(faulted, j + 1);
    }
    return 0;
}

}  // namespace crf
