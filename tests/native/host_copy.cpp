// The host half of a host-output evaluation (correrender_amd/csrc/crf_host_copy.h) on the real thread pool
// (crf_pool.h), with this program in the place of compute_to_host: it starts the copier job, then releases the ranges
// on a scripted schedule.  No GPU, no HIP.  Built plain and under ThreadSanitizer / AddressSanitizer + UBSan by
// tests/test_host_copy.py; every failed check is printed, the last line is "OK host copy" only when none failed.
//
//   1. host_range_partition and thread_share: the properties api.cpp relies on, at the voxel counts where they can break
//   2. copy_ranges: destination == source byte for byte and both canaries intact, over release schedules (among them a
//      copier that finds ranges landed before it looks: it must not fault in what it has copied), fault modes (with a
//      populate step that fails, so that mode 2 falls back to touching), thread counts, range counts, sizes and
//      destination alignments; and the abort of an evaluation
//   3. SpinPool: every worker runs every job once, statuses, barriers, start after start, destruction with a job in flight
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include <sys/mman.h>

#include "crf_host_copy.h"
#include "crf_pool.h"

namespace {

using crf::kPage;

int g_failures = 0;

#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            g_failures++;                     \
            if (g_failures <= 200) {          \
                printf("FAILED %s: ", #cond); \
                printf(__VA_ARGS__);          \
                printf("\n");                 \
            }                                 \
        }                                     \
    } while (0)

struct Lcg {
    uint64_t s;
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return uint32_t(s >> 33);
    }
};

double seconds_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// short pauses are polled: a sleep takes 60 us at the least
void pause_us(int us) {
    if (us >= 100) {
        std::this_thread::sleep_for(std::chrono::microseconds(us));
    } else if (us > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        while (seconds_since(t0) < us * 1e-6) _mm_pause();
    }
}

// ---- 1. the range partition and the thread shares ---------------------------------------------------------------------
const std::vector<int> kDefaultShares = {3, 6, 6, 6, 6, 6, 6, 6, 6, 5, 4, 2, 2};

void check_shares_of_ranges(const std::vector<size_t>& first, const char* what) {
    for (size_t j = 0; j + 1 < first.size(); j++) {
        const size_t r_lo = first[j] * sizeof(float), r_hi = first[j + 1] * sizeof(float);
        for (int workers = 1; workers <= 16; workers++) {
            size_t at = r_lo;
            for (int w = 0; w < workers; w++) {
                size_t lo, hi;
                crf::thread_share(r_lo, r_hi, w, workers, &lo, &hi);
                CHECK(lo == at && hi >= lo && hi <= r_hi, "%s range %zu, worker %d of %d: [%zu, %zu) after %zu", what, j, w,
                      workers, lo, hi, at);
                if (hi < r_hi) CHECK((hi - r_lo) % kPage == 0, "%s range %zu, worker %d of %d: cut at %zu", what, j, w, workers, hi);
                at = hi;
            }
            CHECK(at == r_hi, "%s range %zu, %d workers: the shares end at %zu, the range at %zu", what, j, workers, at, r_hi);
        }
    }
}

// the properties of every partition; used_shares: the share list that must have decided it (null: a forced count)
void check_partition(size_t n, int forced, const std::vector<int>& shares, const std::vector<int>* used_shares, const char* what) {
    const std::vector<size_t> first = crf::host_range_partition(n, forced, shares, kMaxHostChunks);
    const std::string where = std::string(what) + ", n=" + std::to_string(n);
    CHECK(first.size() >= 2 && first.front() == 0 && first.back() == n, "%s", where.c_str());
    CHECK(int(first.size()) - 1 <= kMaxHostChunks, "%s: %zu ranges", where.c_str(), first.size() - 1);
    for (size_t j = 0; j + 1 < first.size(); j++) {
        CHECK(first[j] < first[j + 1], "%s: boundary %zu", where.c_str(), j);
        if (j > 0) CHECK(first[j] % 1024 == 0, "%s: boundary %zu = %zu", where.c_str(), j, first[j]);
    }
    if (used_shares) {
        // every boundary is a share boundary rounded up to 1024 voxels, in order; all of them at these voxel counts
        std::vector<size_t> want;
        size_t acc = 0;
        for (size_t j = 0; j + 1 < used_shares->size(); j++) {
            acc += size_t((*used_shares)[j]);
            want.push_back(n / 64 * acc);
        }
        CHECK(first.size() - 2 == want.size(), "%s: %zu inner boundaries, %zu shares", where.c_str(), first.size() - 2,
              used_shares->size());
        for (size_t j = 0; j < want.size() && j + 2 < first.size(); j++)
            CHECK(first[j + 1] >= want[j] && first[j + 1] - want[j] < 1024, "%s: boundary %zu = %zu, share boundary %zu",
                  where.c_str(), j + 1, first[j + 1], want[j]);
    } else {
        CHECK(int(first.size()) - 1 == std::min(forced, kMaxHostChunks), "%s: %zu ranges", where.c_str(), first.size() - 1);
    }
    check_shares_of_ranges(first, where.c_str());
}

void test_partition() {
    const size_t counts[] = {size_t(1) << 21, (size_t(1) << 21) + 1, 2106041, size_t(1) << 24, (size_t(1) << 29) - 1,
                             (size_t(1) << 29) + 1, size_t(0xFFFFFFF0u) / 4 - 1};
    struct List {
        const char* text;
        bool counts;  // sums to 64 in 1..kMaxHostChunks entries
    };
    const List lists[] = {{"32,32", true}, {"64", true}, {"1,2,4,8,16,33", true}, {"4,4,4,4,4,4,4,4,4,4,4,4,4,4,4,4", true},
                          {"32,16", false}, {"", false}, {"2,2,2,2,2,2,2,2,2,2,2,2,2,2,2,2,32", false}};
    for (size_t n : counts) {
        check_partition(n, 0, {}, &kDefaultShares, "default shares");
        for (const List& l : lists) {
            const std::vector<int> v = crf::parse_shares(l.text);
            check_partition(n, 0, v, l.counts ? &v : &kDefaultShares, l.text);
            if (!l.counts)
                CHECK(crf::host_range_partition(n, 0, v, kMaxHostChunks) == crf::host_range_partition(n, 0, {}, kMaxHostChunks),
                      "shares '%s' must be ignored (n=%zu)", l.text, n);
        }
        for (int forced : {1, 2, 13, 16, 1000}) check_partition(n, forced, {}, nullptr, ("forced " + std::to_string(forced)).c_str());
    }
    CHECK(crf::parse_shares(nullptr).empty(), "no share list");
    CHECK((crf::parse_shares("3,6,55") == std::vector<int>{3, 6, 55}), "parse_shares");
    CHECK((crf::host_range_partition(2106041, 0, {}, kMaxHostChunks) ==
           std::vector<size_t>{0, 99328, 296960, 494592, 691200, 888832, 1086464, 1284096, 1481728, 1678336, 1843200, 1975296,
                               2040832, 2106041}),
          "the default ranges of 161 x 127 x 103");
}

// ---- 2. the copier loop -----------------------------------------------------------------------------------------------
constexpr unsigned char kCanary = 0xC5, kFill = 0xEE;
constexpr size_t kFront = 2 * kPage, kBack = 2 * kPage;  // canaries: at least kFront before the destination, kBack after it

std::atomic<long> g_populate_refused{0};
int populate_refuses(void*, size_t) {
    g_populate_refused.fetch_add(1, std::memory_order_relaxed);
    errno = EINVAL;
    return -1;
}

struct FaultConfig {
    int mode;
    crf::PopulateFn populate;
    const char* name;
    bool may_touch;
};
const FaultConfig kFaultConfigs[] = {{0, crf::populate_write, "mode 0", false},
                                     {1, crf::populate_write, "mode 1 (touch)", true},
                                     {2, crf::populate_write, "mode 2 (populate)", true},  // touches where the kernel refuses
                                     {2, populate_refuses, "mode 2, populate fails (touch)", true}};
constexpr int kFaultConfigCount = 4;

enum Schedule { kPre, kStepwise, kAtOnce };

struct Bench {
    char* arena = nullptr;
    size_t arena_bytes = 0;
    std::vector<char> src;
    std::unique_ptr<crf::SpinPool> pool;  // as ensure_copy_pool builds it; copy_ranges uses the first `threads` workers
    int pool_size = 0;
    std::atomic<int> ready[kMaxHostChunks];
    long cases = 0;
    long differing_by_config[kFaultConfigCount] = {};
    long failed_by_config[kFaultConfigCount] = {};

    explicit Bench(size_t max_voxels) {
        arena_bytes = kFront + kPage + max_voxels * sizeof(float) + kBack + kPage;
        void* p = mmap(nullptr, arena_bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (p == MAP_FAILED) {
            printf("mmap of %zu bytes failed\n", arena_bytes);
            exit(2);
        }
        arena = static_cast<char*>(p);
        src.resize(max_voxels * sizeof(float));
        for (size_t i = 0; i < src.size(); i++) src[i] = char(1 + (i * 131 + (i >> 12) * 7 + (i >> 20)) % 255);  // never 0
    }
    ~Bench() {
        pool.reset();
        munmap(arena, arena_bytes);
    }
    // a pool of 4 for up to 3 copier threads (one worker always finds nothing to do), of 16 for 16: one pool at a time
    void use_pool_for(int threads) {
        const int size = threads <= 3 ? 4 : 16;
        if (size == pool_size) return;
        pool.reset();
        pool = std::make_unique<crf::SpinPool>(size, nullptr, 300e-6);
        pool_size = size;
    }

    // the destination of `bytes` at `offset` past a page boundary, canaries around it; fresh: its whole pages are given
    // back to the kernel first, so they are faulted in again (and read as 0)
    char* prepare(size_t bytes, size_t offset, bool fresh, unsigned char* fill) {
        char* dst = arena + kFront + offset;
        memset(arena, kCanary, kFront + offset);
        memset(dst + bytes, kCanary, kBack);
        *fill = fresh ? 0 : kFill;
        const uintptr_t a = (reinterpret_cast<uintptr_t>(dst) + kPage - 1) & ~(kPage - 1);
        const uintptr_t e = (reinterpret_cast<uintptr_t>(dst) + bytes) & ~(kPage - 1);
        if (fresh && e > a) {  // whole pages come back zero-filled; the ragged ends are cleared by hand
            memset(dst, 0, a - reinterpret_cast<uintptr_t>(dst));
            memset(reinterpret_cast<void*>(e), 0, reinterpret_cast<uintptr_t>(dst) + bytes - e);
            CHECK(madvise(reinterpret_cast<void*>(a), e - a, MADV_DONTNEED) == 0, "MADV_DONTNEED: errno %d", errno);
        } else {
            memset(dst, *fill, bytes);
        }
        return dst;
    }
    long canary_damage(const char* dst, size_t bytes) const {
        long bad = 0;
        for (const char* p = arena; p < dst; p++) bad += (static_cast<unsigned char>(*p) != kCanary);
        for (const char* p = dst + bytes; p < dst + bytes + kBack; p++) bad += (static_cast<unsigned char>(*p) != kCanary);
        return bad;
    }

    // One evaluation.  released: ranges [0, released) are released, the others (an aborted evaluation) set to -1.
    // kStepwise: one by one, each after a pause in which the copiers run out of ranges to fault in; kPre: ranges [0, k]
    // are ready before the copiers start (they are late for them), the others follow stepwise; kAtOnce: all together.
    void run(const std::vector<size_t>& first, int threads, int config, size_t offset, Schedule schedule, int k, int pause,
             bool fresh, int released) {
        const FaultConfig& fc = kFaultConfigs[config];
        const int ranges = int(first.size()) - 1;
        const size_t bytes = first[size_t(ranges)] * sizeof(float);
        unsigned char fill;
        char* dst = prepare(bytes, offset, fresh, &fill);
        const char* s = src.data();
        const size_t* f = first.data();
        const std::atomic<int>* rd = ready;
        for (int j = 0; j < ranges; j++) ready[j].store(0, std::memory_order_relaxed);
        const std::function<int(int)> job = [=](int w) -> int {
            return crf::copy_ranges(dst, s, f, ranges, threads, rd, fc.mode, w, fc.populate);
        };
        auto release = [&](int j) { ready[j].store(j < released ? 1 : -1, std::memory_order_release); };
        use_pool_for(threads);
        int next = 0;
        if (schedule == kPre)
            for (; next <= k; next++) release(next);
        pool->start(job);
        if (schedule == kPre) pause_us(4 * pause);  // the copiers copy what they found ready, then wait for the next range
        for (; next < ranges; next++) {
            if (schedule != kAtOnce) pause_us(pause);
            release(next);
        }
        const int status = pool->wait();
        cases++;

        char what[256];
        snprintf(what, sizeof what, "%s, %zu voxels in %d ranges, %d threads, destination at page + %zu%s, %s k=%d, %d released",
                 fc.name, first[size_t(ranges)], ranges, threads, offset, fresh ? " (fresh pages)" : "",
                 schedule == kPre ? "ready before start" : schedule == kStepwise ? "stepwise" : "at once", k, released);
        CHECK(status == 0, "%s: status %d", what, status);
        const size_t good = first[size_t(released)] * sizeof(float);
        long differing = 0;
        if (memcmp(dst, s, good) != 0)
            for (size_t i = 0; i < good; i++) differing += (dst[i] != s[i]);
        if (differing) {
            differing_by_config[config] += differing;
            failed_by_config[config]++;
        }
        CHECK(differing == 0, "%s: %ld bytes of the destination differ from the source", what, differing);
        // ranges of an aborted evaluation: as they were, but for the bytes that faulting in touched
        long foreign = 0;
        for (size_t i = good; i < bytes; i++) {
            const unsigned char b = static_cast<unsigned char>(dst[i]);
            foreign += !(b == fill || (fc.may_touch && b == 0));
        }
        CHECK(foreign == 0, "%s: %ld bytes written into ranges that were not released", what, foreign);
        const long damage = canary_damage(dst, bytes);
        CHECK(damage == 0, "%s: %ld canary bytes overwritten", what, damage);
    }
};

const size_t kOffsets[] = {0, 4, 4092};
const int kThreads[] = {1, 2, 3, 16};

// the four range counts on n voxels: 1, 2, the default shares, kMaxHostChunks
std::vector<std::vector<size_t>> partitions_of(size_t n) {
    return {crf::host_range_partition(n, 1, {}, kMaxHostChunks), crf::host_range_partition(n, 2, {}, kMaxHostChunks),
            crf::host_range_partition(n, 0, {}, kMaxHostChunks), crf::host_range_partition(n, kMaxHostChunks, {}, kMaxHostChunks)};
}

// every schedule of one configuration: ready before the start for k = 0 .. ranges-1, stepwise, at once; with all three
// destination offsets, or with one that rotates through the cases
void run_schedules(Bench& b, const std::vector<size_t>& first, int ti, int config, bool every_offset, int pause, bool fresh) {
    const int ranges = int(first.size()) - 1;
    for (int sched = 0; sched < ranges + 2; sched++) {
        const Schedule schedule = sched < ranges ? kPre : sched == ranges ? kStepwise : kAtOnce;
        const int k = sched < ranges ? sched : -1;
        for (int oi = 0; oi < 3; oi++)
            if (every_offset || oi == (sched + ti + config) % 3)
                b.run(first, kThreads[ti], config, kOffsets[oi], schedule, k, pause, fresh, ranges);
    }
}

// aborts: ranges [0, released) released, the others -1, for every released < ranges (ends_only: 0, 1 and ranges - 1);
// decided before the copiers start, and after it with the released ranges handed over one by one.  The offset rotates.
void run_aborts(Bench& b, const std::vector<size_t>& first, int ti, int config, bool ends_only, int pause) {
    const int ranges = int(first.size()) - 1;
    for (int released = 0; released < ranges; released++) {
        if (ends_only && released > 1 && released < ranges - 1) continue;
        const size_t offset = kOffsets[(released + ti + config) % 3];
        b.run(first, kThreads[ti], config, offset, kPre, ranges - 1, 0, false, released);
        b.run(first, kThreads[ti], config, offset, kStepwise, -1, pause, false, released);
    }
}

// Small grids: schedules, fault modes and range counts all crossed for 1, 2 and 3 threads, with every destination
// offset for 3 threads and a rotating one for the others.  For 16 threads (oversubscribing a small host) the one-page ranges
// come in 2 only, and the aborts are the ends.  (Under ThreadSanitizer a hand-off of the spinning pool costs
// milliseconds, so the number of evaluations is what the run time buys.)  Large grids: see below.
void test_copier() {
    const size_t big[] = {size_t(1) << 21, 2106041};
    const size_t kFlagship = 2;  // index of the default ranges in partitions_of
    Bench b(big[1]);
    std::vector<std::vector<size_t>> tiny;  // one-page ranges: 16 threads on one page leave all shares but the first empty
    for (int ranges : {1, 2, 13, kMaxHostChunks}) {
        tiny.push_back(crf::host_range_partition(size_t(ranges) * 1024, ranges, {}, kMaxHostChunks));
        CHECK(int(tiny.back().size()) - 1 == ranges, "%d one-page ranges", ranges);
    }
    // a small ragged grid in the default shares: ranges of 3 to 6 pages and a ragged last one
    const std::vector<size_t> small = crf::host_range_partition(64 * 1024 + 1000 + 37, 0, {}, kMaxHostChunks);
    CHECK(small.size() == 14, "small default partition: %zu ranges", small.size() - 1);
    const std::vector<std::vector<size_t>> parts[2] = {partitions_of(big[0]), partitions_of(big[1])};

    for (int ti = 0; ti < 4; ti++) {
        const auto t0 = std::chrono::steady_clock::now();
        const long cases0 = b.cases;
        const bool few = kThreads[ti] <= 3, every_offset = kThreads[ti] == 3;
        for (int config = 0; config < kFaultConfigCount; config++) {
            for (size_t i = 0; i < tiny.size(); i++) {
                if (!few && i != 1) continue;
                run_schedules(b, tiny[i], ti, config, every_offset, 30, false);
                if (few) run_aborts(b, tiny[i], ti, config, false, 30);
            }
            for (bool fresh : {false, true})
                if (few || !fresh) run_schedules(b, small, ti, config, every_offset, 30, fresh);
            run_aborts(b, small, ti, config, !few, 30);
        }
        printf("copier, %d threads: %ld evaluations of small grids in %.2f s\n", kThreads[ti], b.cases - cases0, seconds_since(t0));
    }
    for (int ti = 0; ti < 4; ti++) {
        const auto t0 = std::chrono::steady_clock::now();
        const long cases0 = b.cases;
        for (int config = 0; config < kFaultConfigCount; config++) {
            // 2^21 and 161 x 127 x 103 voxels.  One evaluation costs three passes over 8 MiB (tens of milliseconds each
            // under ThreadSanitizer), so: every range count x fault mode x thread count once, at one size or the other;
            // the schedule (ready before the start with k = 0 and with k = ranges / 2, stepwise, at once) rotates so
            // that any two of the three meet every schedule; the offset and never-touched pages rotate too ...
            for (int si = 0; si < 2; si++)
                for (size_t pi = 0; pi < 4; pi++) {
                    if ((ti + config + si) % 2) continue;
                    const std::vector<size_t>& first = parts[si][pi];
                    const int ranges = int(first.size()) - 1;
                    const int pick = (ti + int(pi) + config) % 4;
                    const size_t offset = kOffsets[(ti + 2 * int(pi) + config + si) % 3];
                    b.run(first, kThreads[ti], config, offset, pick <= 1 ? kPre : pick == 2 ? kStepwise : kAtOnce,
                          pick == 0 ? 0 : pick == 1 ? ranges / 2 : -1, 300, (ti + int(pi)) % 2 == 0, ranges);
                }
        }
        printf("copier, %d threads: %ld evaluations of large grids in %.2f s\n", kThreads[ti], b.cases - cases0, seconds_since(t0));
    }
    const auto t_default = std::chrono::steady_clock::now();
    const long cases_default = b.cases;
    // ... and at 161 x 127 x 103 voxels in the default ranges on 3 threads, what crf_compute does by default: five
    // schedules in the two modes that touch, two in the others; never-touched destination pages; two aborts
    {
        const std::vector<size_t>& first = parts[1][kFlagship];
        const int ranges = int(first.size()) - 1;
        for (int config = 0; config < kFaultConfigCount; config++) {
            if (kFaultConfigs[config].mode == 1 || kFaultConfigs[config].populate == populate_refuses) {
                for (int k : {0, 1, ranges / 2, ranges - 1})
                    b.run(first, 3, config, kOffsets[(k + config) % 3], kPre, k, 300, false, ranges);
                b.run(first, 3, config, kOffsets[0], kStepwise, -1, 300, false, ranges);
            } else {
                b.run(first, 3, config, kOffsets[1], kPre, 0, 300, false, ranges);
                b.run(first, 3, config, kOffsets[0], kStepwise, -1, 300, false, ranges);
            }
            b.run(first, 3, config, kOffsets[config % 3], kPre, 0, 300, true, ranges);
            b.run(first, 3, config, kOffsets[(1 + config) % 3], kPre, ranges - 1, 0, false, 1);
            b.run(first, 3, config, kOffsets[(2 + config) % 3], kStepwise, -1, 300, false, ranges - 1);
        }
    }
    // the case the defect was first seen in: 4 equal ranges, 3 threads, range 0 ready before the start
    {
        const std::vector<size_t> first = crf::host_range_partition(big[1], 4, {}, kMaxHostChunks);
        for (int config = 0; config < kFaultConfigCount; config++) b.run(first, 3, config, 0, kPre, 0, 300, false, 4);
    }
    printf("copier, default ranges: %ld evaluations in %.2f s\n", b.cases - cases_default, seconds_since(t_default));
    CHECK(g_populate_refused.load() > 0, "the failing populate step was never asked");
    printf("copier: %ld evaluations\n", b.cases);
    for (int config = 0; config < kFaultConfigCount; config++)
        printf("copier, %s: %ld evaluations with a wrong destination, %ld differing bytes\n", kFaultConfigs[config].name,
               b.failed_by_config[config], b.differing_by_config[config]);
}

// ---- 3. the pool ------------------------------------------------------------------------------------------------------
struct Generation {
    std::vector<int> ran;     // [worker]: times the job ran there (written by that worker only)
    std::vector<int> status;  // [worker]: what the job returns there
    int id = 0;
};

void test_pool_at(int workers, double spin_seconds, int generations, Lcg& rng) {
    std::vector<long> slot(size_t(workers), -1);  // written by its worker before the first barrier, read by all after it
    std::atomic<long> wrong_reads{0};
    long total_ran = 0;
    char what[96];
    snprintf(what, sizeof what, "pool of %d, spin %.0f us", workers, spin_seconds * 1e6);
    {
        crf::SpinPool pool(workers, nullptr, spin_seconds);
        CHECK(pool.size() == workers, "%s", what);
        CHECK(pool.wait() == 0, "%s: wait() with nothing started", what);
        auto make_job = [&](Generation& g) {
            return std::function<int(int)>([&g, &slot, &wrong_reads, &pool, workers](int w) -> int {
                g.ran[size_t(w)]++;
                slot[size_t(w)] = long(g.id) * 1000 + w;
                pool.barrier();
                for (int i = 0; i < workers; i++)
                    if (slot[size_t(i)] != long(g.id) * 1000 + i) wrong_reads.fetch_add(1, std::memory_order_relaxed);
                pool.barrier();
                slot[size_t(w)] = -2;  // the next write phase: after every read of this one
                return g.status[size_t(w)];
            });
        };
        auto fresh = [&](Generation& g, int id) {
            g.id = id;
            g.ran.assign(size_t(workers), 0);
            g.status.assign(size_t(workers), 0);
            if (rng.next() % 3 == 0)  // some workers fail; wait() reports the one with the lowest index
                for (int w = 0; w < workers; w++)
                    if (rng.next() % 3 == 0) g.status[size_t(w)] = 100 + w + 1000 * int(rng.next() % 7);
        };
        auto first_status = [](const Generation& g) {
            for (int s : g.status)
                if (s) return s;
            return 0;
        };
        auto ran_once = [&](const Generation& g, const char* how) {
            for (int w = 0; w < workers; w++) {
                CHECK(g.ran[size_t(w)] == 1, "%s, generation %d (%s): worker %d ran the job %d times", what, g.id, how, w, g.ran[size_t(w)]);
                total_ran += g.ran[size_t(w)];
            }
        };
        Generation a, b;
        for (int gen = 0; gen < generations;) {
            // workers are found spinning (short pauses) and, where the spin time allows it, asleep (longer ones)
            const uint32_t r = rng.next() % 16;
            pause_us(r < 6 ? 0 : r < 14 ? int(rng.next() % 120) : 500);
            fresh(a, gen);
            const std::function<int(int)> job_a = make_job(a);
            switch (rng.next() % 3) {
            case 0: {
                CHECK(pool.run(job_a) == first_status(a), "%s, generation %d: status of run()", what, gen);
                ran_once(a, "run");
                gen += 1;
                break;
            }
            case 1: {
                pool.start(job_a);
                pause_us(int(rng.next() % 4) * 20);
                CHECK(pool.wait() == first_status(a), "%s, generation %d: status of wait()", what, gen);
                CHECK(pool.wait() == 0, "%s, generation %d: a second wait()", what, gen);
                ran_once(a, "start, wait");
                gen += 1;
                break;
            }
            default: {  // start directly after start: the second one waits for the first job
                fresh(b, gen + 1);
                const std::function<int(int)> job_b = make_job(b);
                pool.start(job_a);
                pool.start(job_b);
                ran_once(a, "start, start");
                CHECK(pool.wait() == first_status(b), "%s, generation %d: status of wait() after start, start", what, gen + 1);
                ran_once(b, "start, start, wait");
                gen += 2;
                break;
            }
            }
        }
    }
    CHECK(wrong_reads.load() == 0, "%s: %ld reads after the barrier did not see the writes before it", what, wrong_reads.load());
    CHECK(total_ran >= long(generations) * workers, "%s: %ld job runs", what, total_ran);
}

void test_pool_destroyed_with_a_job_in_flight(double spin_seconds) {
    constexpr int kWorkers = 5;
    std::vector<int> ran(kWorkers, 0);
    std::atomic<int> entered{0};
    const std::function<int(int)> job = [&](int w) -> int {
        entered.fetch_add(1, std::memory_order_relaxed);
        pause_us(200 * w);  // still running when the destructor starts
        ran[size_t(w)]++;
        return w;
    };
    {
        crf::SpinPool pool(kWorkers, nullptr, spin_seconds);
        pool.start(job);
    }
    for (int w = 0; w < kWorkers; w++) CHECK(ran[size_t(w)] == 1, "destroyed in flight (spin %.0f us): worker %d ran %d times", spin_seconds * 1e6, w, ran[size_t(w)]);
    CHECK(entered.load() == kWorkers, "destroyed in flight: %d workers entered", entered.load());
    {
        crf::SpinPool idle(3, nullptr, spin_seconds);  // never used: workers spinning or asleep, then stopped
        pause_us(spin_seconds > 0 && spin_seconds < 1e-3 ? 300 : 0);
    }
}

void test_pool() {
    Lcg rng{20261020};
    int total = 0;
    for (double spin : {0.0, 50e-6, 2000e-6})  // every hand-off sleeps / mixed / never sleeps
        for (int workers : {1, 3, 8, 16}) {
            const int generations = workers == 16 ? 40 : workers == 8 ? 160 : 500;  // 16 oversubscribe a small host
            test_pool_at(workers, spin, generations, rng);
            total += generations;
        }
    for (double spin : {0.0, 50e-6, 2000e-6}) test_pool_destroyed_with_a_job_in_flight(spin);
    printf("pool: %d generations\n", total);
}

}  // namespace

int main() {
    unsetenv("CRF_POOL_SPIN_US");  // the spin times are the test's
    setvbuf(stdout, nullptr, _IOLBF, 0);
    auto t0 = std::chrono::steady_clock::now();
    test_partition();
    printf("partition: %.2f s\n", seconds_since(t0));
    t0 = std::chrono::steady_clock::now();
    test_pool();
    printf("pool: %.2f s\n", seconds_since(t0));
    test_copier();
    if (g_failures) {
        printf("%d checks FAILED\n", g_failures);
        return 1;
    }
    printf("OK host copy\n");
    return 0;
}
