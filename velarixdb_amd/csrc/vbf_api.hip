// vbf_api.hip -- the C ABI (include/vbf.h) over the gfx950 kernels.
//
// Host-side responsibilities: argument checks that mirror the reference's asserts/panics,
// sizing arithmetic (bf.rs:230-239), the filter handle (bf.rs:38-58 semantics: clones share
// one bit array behind a mutex, like Arc<Mutex<BitVec>>), and the chunked, double-buffered
// H2D pipeline for keys that arrive in host memory (memtable / compaction output).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <utility>
#include <atomic>
#include <cstdarg>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <unistd.h>

#include "../../include/vbf.h"
#include "sip13.hpp"
#include "vbf_kernels.hpp"

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

inline int ok() {
    g_err.clear();
    return VBF_OK;
}

// On failure the thread's sticky HIP error is cleared (hipGetLastError resets it) after it is
// reported, so it cannot resurface as a later launch's hipGetLastError on the same thread -- e.g.
// the next asynchronous set a device's worker thread runs after one whose allocation failed.
#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            (void)hipGetLastError();                                                          \
            int code_ = (e_ == hipErrorOutOfMemory) ? VBF_ENOMEM : VBF_EHIP;                  \
            return fail(code_, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
        }                                                                                     \
    } while (0)

// Switches the calling thread to `device` for the scope, restoring the previous one.
// HIP does not survive fork(): a child of a process that used the GPU through this library must not
// call into HIP (such calls can hang or fault).  The first device scope records the process that
// uses HIP; a forked child's device scopes fail with VBF_EINVAL before any HIP call.
std::atomic<pid_t> g_hip_pid{0};

bool hip_forked() {
    const pid_t owner = g_hip_pid.load();
    return owner != 0 && owner != getpid();
}

// Records the calling process as the one that uses HIP (the first call wins); false in a child
// forked from it.
bool hip_owner() {
    const pid_t me = getpid();
    pid_t owner = 0;
    return g_hip_pid.compare_exchange_strong(owner, me) || owner == me;
}

int fail_forked() {
    return fail(VBF_EINVAL, "process %d forked from %d, which uses the GPU: HIP cannot be used in the child",
                (int)getpid(), (int)g_hip_pid.load());
}

// The stateless device-pointer entry points (no DeviceGuard: they run on the caller's current
// device) check the same at their start.
#define FORK_GUARD()                          \
    do {                                      \
        if (!hip_owner()) return fail_forked(); \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    bool forked = false;
    explicit DeviceGuard(int device) {
        if (!hip_owner()) {
            forked = true;
            err = hipErrorNotSupported;
            return;
        }
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) err = hipSetDevice(device);
    }
    ~DeviceGuard() {
        if (forked) return;
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

#define DEVICE_SCOPE(dev)                                                                     \
    DeviceGuard guard_(dev);                                                                  \
    if (guard_.forked) return fail_forked();                                                  \
    if (guard_.err != hipSuccess)                                                             \
        return fail(VBF_ENODEV, "hipSetDevice(%d): %s", (int)(dev), hipGetErrorString(guard_.err))

// Rust `f64 as u32`: saturating, NaN -> 0, truncation toward zero.
uint32_t f64_as_u32(double x) {
    if (std::isnan(x) || x <= 0.0) return 0;
    if (x >= 4294967295.0) return 4294967295u;
    return (uint32_t)x;
}

int check_keys(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n) {
    if (n == 0) return VBF_OK;
    if (!keys && !offsets && stride) return fail(VBF_EINVAL, "keys is NULL");
    if (offsets == nullptr && stride == 0) return VBF_OK;  // n empty keys
    return VBF_OK;
}

int check_mk(uint32_t m, uint32_t k, uint64_t n) {
    if (m == 0 && k > 0 && n > 0)
        return fail(VBF_EDIVZERO, "m == 0 with k = %u > 0: the reference divides by zero (bf.rs:88)", k);
    return VBF_OK;
}

vbf::KeyBatch batch(const uint8_t* keys, const uint64_t* offsets, uint64_t off_base,
                    uint64_t stride, uint64_t n, int lp) {
    return vbf::KeyBatch{keys, offsets, off_base, stride, n, lp != 0};
}

// ---------------------------------------------------------------------------------------
// Partitioned-build workspace: one grow-only buffer per (device, stream), so concurrent
// builds on different streams never share scratch.
// ---------------------------------------------------------------------------------------
enum WsSlot {
    kWsBuild = 0,
    kWsSstScratch = 1,
    kWsSstKeys = 2,
    kWsSstInput = 3,
    kWsMulti = 4,
    kWsMultiKeys = 5,
    kWsCompact = 6,
    kWsCompactIn = 7,
    kWsGather = 8,
    kWsProbe = 9,
    kWsCount = 10,
    kWsMultiGroup = 11,
    kWsSstEnc = 12,
    kWsSstEncIO = 13,
    kWsCompactOut = 14,
    kWsTableOpen = 15,
    kWsTableDesc = 16,
    kWsTableIO = 17,
    kWsTableScanPairs = 18,
    kWsTableScan = 19,
    kWsTableScanIO = 20,
    kWsVlog = 21,
    kWsVlogIO = 22,
    kWsVlogOut = 23,
    kWsVlogEnc = 24,
    kWsVlogEncIO = 25,
    kWsMemSort = 26,
    kWsMemIO = 27,
    kWsMemOut = 28,
    kWsFilterInsert = 29,
    kWsFilterInsertIO = 30,
    kWsVlogWalk = 31,
    kWsVlogWalkOut = 32,
    kWsGc = 33,
    kWsGcOut = 34,
    kWsMemOpen = 35,
    kWsMemGetDesc = 36,
    kWsMemGetIO = 37,
    kWsStoreIO = 38,
    kWsStoreScanDesc = 39,
    kWsStoreScanIn = 40,
    kWsStoreScanPairs = 41,
    kWsStoreScan = 42,
    kWsStoreScanOut = 43,
};
struct Workspace {
    int device;
    hipStream_t stream;
    int slot;
    void* ptr;
    uint64_t bytes;
};
std::mutex g_ws_mu;
std::vector<Workspace> g_ws;

// VBF_WS_MAX_BYTES (read per call): the largest single workspace the library may allocate -- for a
// caller sharing the GPU; a build whose default chunk needs more runs in smaller chunks (do_build)
uint64_t ws_max_bytes() {
    const char* e = getenv("VBF_WS_MAX_BYTES");
    return e ? strtoull(e, nullptr, 10) : ~0ull;
}

int get_workspace(hipStream_t s, uint64_t bytes, void** out, int slot = kWsBuild) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    bytes = std::max<uint64_t>(bytes, 256);
    if (bytes > ws_max_bytes())
        return fail(VBF_ENOMEM, "workspace of %llu bytes above VBF_WS_MAX_BYTES", (unsigned long long)bytes);
    std::lock_guard<std::mutex> lk(g_ws_mu);
    for (auto& w : g_ws) {
        if (w.device == dev && w.stream == s && w.slot == slot) {
            if (w.bytes < bytes) {
                HIP_TRY(hipStreamSynchronize(s));  // the old buffer may still be in use on s
                HIP_TRY(hipFree(w.ptr));
                w.ptr = nullptr;
                w.bytes = 0;
                HIP_TRY(hipMalloc(&w.ptr, bytes));
                w.bytes = bytes;
            }
            *out = w.ptr;
            return VBF_OK;
        }
    }
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, bytes));
    g_ws.push_back(Workspace{dev, s, slot, p, bytes});
    *out = p;
    return VBF_OK;
}

constexpr uint64_t kAutoPartitionMinIdx = 1ull << 22;
// batched multi-SST probe: below this many keys every filter is probed one lane per key
constexpr uint64_t kMultiGroupMinKeys = 1ull << 20;

// The build every entry point funnels into.  strategy: VBF_BUILD_AUTO / _ATOMIC / _PARTITIONED.
// atomic_merge: another writer may touch `words` concurrently (the partitioned path then
// merges its segments with word atomics instead of load+store).
int do_build(const vbf::KeyBatch& kb, uint32_t m, uint32_t k, uint32_t* words, int strategy,
             bool atomic_merge, hipStream_t s) {
    const bool fresh = (strategy & VBF_BUILD_FRESH) != 0;
    strategy &= ~VBF_BUILD_FRESH;
    // a fresh filter the segment pass cannot write whole (atomic strategy, no keys, several
    // chunks or several workgroups per segment) is zeroed first: BitVec::from_elem(m, false)
    auto zero = [&]() -> int {
        if (fresh && m) HIP_TRY(hipMemsetAsync(words, 0, ((uint64_t)m + 31) / 32 * 4, s));
        return VBF_OK;
    };
    if (kb.n == 0 || k == 0) return zero();
    bool part;
    if (strategy == VBF_BUILD_ATOMIC) {
        part = false;
    } else if (strategy == VBF_BUILD_PARTITIONED) {
        if (!vbf::partition_supported(m, k))
            return fail(VBF_EINVAL, "partitioned build needs 1 <= k <= 32 and m > 0 (k = %u)", k);
        part = true;
    } else if (strategy == VBF_BUILD_AUTO) {
        part = vbf::partition_supported(m, k) && kb.n * (uint64_t)k >= kAutoPartitionMinIdx;
    } else {
        return fail(VBF_EINVAL, "unknown build strategy %d", strategy);
    }
    if (!part) {
        if (int rc = zero()) return rc;
        HIP_TRY(vbf::launch_build(kb, m, k, words, s));
        return VBF_OK;
    }
    // The workspace holds one chunk of bit indices (kBuildChunkIdx = 2^32: ~10.7 GB).  When it
    // cannot be allocated (other streams' workspaces, the caller's own memory), the chunk is halved
    // down to 2^28 indices -- more segment passes, the same words.
    uint64_t chunk = vbf::build_chunk_default(), need = 0;
    void* ws = nullptr;
    for (;;) {
        need = vbf::partition_workspace_bytes(kb.n, m, k, chunk);
        const int rc = get_workspace(s, need, &ws);
        if (rc == VBF_OK) break;
        if (rc != VBF_ENOMEM || chunk <= (1ull << 28)) return rc;
        chunk /= 2;
    }
    const bool fused = fresh && !atomic_merge && vbf::partition_fresh_ok(kb.n, m, k, chunk);
    if (fresh && !fused)
        if (int rc = zero()) return rc;
    HIP_TRY(vbf::launch_build_partitioned(kb, m, k, words, ws, need, atomic_merge, s, fused, chunk));
    return VBF_OK;
}

// The probe every entry point funnels into: out (answer bytes) or count (hits).  The per-key
// early-exit gather costs ~1 + (k-1)*hit_rate random filter loads per key; the partitioned probe
// costs all k hashes per key but no random loads.  AUTO (large batches over large filters) probes
// the first 64K keys with the gather, reads the hit count back (one stream sync) and takes the
// partitioned path when at least 35 % of them hit (measured crossover: 100M keys, k = 10).
constexpr uint64_t kAutoProbePartitionMinIdx = 1ull << 24;
constexpr uint64_t kProbeSample = 1ull << 16;

int do_probe(const vbf::KeyBatch& kb, uint32_t m, uint32_t k, const uint32_t* words, uint8_t* out,
             unsigned long long* count, int strategy, hipStream_t s) {
    if (kb.n == 0) return VBF_OK;
    bool part;
    if (strategy == VBF_BUILD_ATOMIC) {
        part = false;
    } else if (strategy == VBF_BUILD_PARTITIONED) {
        if (!vbf::probe_partition_supported(m, k))
            return fail(VBF_EINVAL, "partitioned probe needs 1 <= k <= 32 and a filter of at least 1 segment (k = %u)", k);
        part = true;
    } else if (strategy == VBF_BUILD_AUTO) {
        part = k > 1 && vbf::probe_partition_supported(m, k) && kb.n * (uint64_t)k >= kAutoProbePartitionMinIdx &&
               m >= (64u << 20);
        if (part) {  // sample the hit rate
            vbf::KeyBatch sb = kb;
            sb.n = std::min<uint64_t>(kb.n, kProbeSample);
            const uint64_t np = vbf::count_partials(sb.n);
            void* pw = nullptr;
            int rc = get_workspace(s, np * 4 + 256, &pw, kWsCount);
            if (rc) return rc;
            auto* c = reinterpret_cast<unsigned long long*>(static_cast<char*>(pw) + np * 4);
            c = reinterpret_cast<unsigned long long*>(((uintptr_t)c + 7) & ~(uintptr_t)7);
            HIP_TRY(hipMemsetAsync(c, 0, 8, s));
            HIP_TRY(vbf::launch_count(sb, m, k, words, c, static_cast<uint32_t*>(pw), s));
            unsigned long long hits = 0;
            HIP_TRY(hipMemcpyAsync(&hits, c, 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            part = hits * 100 >= sb.n * 35;
        }
    } else {
        return fail(VBF_EINVAL, "unknown probe strategy %d", strategy);
    }
    if (!part || k == 0) {
        if (count) {
            void* pw = nullptr;
            int rc = get_workspace(s, vbf::count_partials(kb.n) * 4, &pw, kWsCount);
            if (rc) return rc;
            HIP_TRY(vbf::launch_count(kb, m, k, words, count, static_cast<uint32_t*>(pw), s));
        } else {
            HIP_TRY(vbf::launch_probe(kb, m, k, words, out, s));
        }
        return VBF_OK;
    }
    const uint64_t need = vbf::probe_workspace_bytes(kb.n, m, k);
    void* ws = nullptr;
    int rc = get_workspace(s, need, &ws, kWsProbe);
    if (rc) return rc;
    HIP_TRY(vbf::launch_probe_partitioned(kb, m, k, words, out, count, ws, need, s));
    return VBF_OK;
}

// ---------------------------------------------------------------------------------------
// Host -> device staging: two pinned buffers and two streams per device; chunk c uses
// buffer (c & 1), so the H2D copy of chunk c+1 overlaps the kernel of chunk c.
// ---------------------------------------------------------------------------------------
constexpr uint64_t kChunkBytes = 64ull << 20;

// Host copy into / out of the pinned staging buffers, split over up to 8 threads
// (VBF_COPY_THREADS): one thread's memcpy into pinned memory runs well below the PCIe rate.  The
// helper threads are a persistent pool (creating 7 threads per 16 MiB chunk cost ~0.1 ms each
// chunk); concurrent callers take turns.
class CopyPool {
  public:
    static CopyPool& get() {
        static std::mutex mu;
        static CopyPool* p = nullptr;  // never destroyed: workers outlive static teardown
        std::lock_guard<std::mutex> lk(mu);
        // a forked child (e.g. a multiprocessing fork) inherits the pool but not its threads:
        // it gets a pool of its own
        if (!p || p->pid_ != getpid()) p = new CopyPool();
        return *p;
    }
    unsigned threads() const { return nt_; }
    // Runs f(0 .. parts-1) with part 0 on the calling thread.
    template <class F>
    void run(unsigned parts, F&& f) {
        std::lock_guard<std::mutex> caller(call_mu_);
        {
            std::lock_guard<std::mutex> lk(mu_);
            job_ = [&f](unsigned i) { f(i); };
            parts_ = parts;
            next_ = 1;
            done_ = 1;
            ++gen_;
        }
        cv_.notify_all();
        f(0);
        std::unique_lock<std::mutex> lk(mu_);
        done_cv_.wait(lk, [&] { return done_ == parts_; });
        job_ = nullptr;
    }

  private:
    CopyPool() : pid_(getpid()) {
        const char* e = getenv("VBF_COPY_THREADS");
        const unsigned hw = std::thread::hardware_concurrency();
        const int v = e ? atoi(e) : (int)std::min(8u, hw ? hw : 1u);
        nt_ = (unsigned)std::max(1, v);
        for (unsigned t = 1; t < nt_; ++t) std::thread([this] { loop(); }).detach();
    }
    void loop() {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            cv_.wait(lk, [&] { return gen_ != seen; });
            seen = gen_;
            while (next_ < parts_) {
                const unsigned i = next_++;
                auto job = job_;
                lk.unlock();
                job(i);
                lk.lock();
                if (++done_ == parts_) done_cv_.notify_one();
            }
        }
    }
    const pid_t pid_;
    unsigned nt_ = 1;
    std::mutex call_mu_, mu_;
    std::condition_variable cv_, done_cv_;
    std::function<void(unsigned)> job_;
    unsigned parts_ = 0, next_ = 0, done_ = 0;
    uint64_t gen_ = 0;
};

void par_memcpy(void* dst, const void* src, size_t n) {
    constexpr size_t kMinPerThread = 2u << 20;
    CopyPool& pool = CopyPool::get();
    const unsigned nt = (unsigned)std::min<size_t>(pool.threads(), n / kMinPerThread);
    if (nt <= 1) {
        std::memcpy(dst, src, n);
        return;
    }
    const size_t per = (n / nt + 4095) & ~(size_t)4095;
    pool.run(nt, [=](unsigned t) {
        const size_t a = (size_t)t * per;
        if (a < n) std::memcpy(static_cast<char*>(dst) + a, static_cast<const char*>(src) + a, std::min(per, n - a));
    });
}

struct Staging {
    std::mutex mu;
    // The device's shared stream (filter_stream) and the workspaces cached on it belong to one host
    // entry point at a time: HostCall takes it before the call's first get_workspace on that stream
    // and releases it after draining the stream, on every return.  A lock of its own, not `mu`: `mu`
    // guards the two staging streams and their buffers, which no holder of host_mu touches, so a long
    // vbf_build_host keeps overlapping the read path's gets and scans as before.
    // Lock order: filter lock(s) (Storage::mu, address order), then host_mu.  No holder waits for a
    // device worker's job (jobs_cv) or takes another device's host_mu.
    std::mutex host_mu;
    int device = -1;
    hipStream_t stream[2] = {nullptr, nullptr};
    hipEvent_t done[2] = {nullptr, nullptr};
    uint8_t* h_keys[2] = {nullptr, nullptr};
    uint8_t* d_keys[2] = {nullptr, nullptr};
    uint64_t key_cap[2] = {0, 0};
    uint64_t* h_offs[2] = {nullptr, nullptr};
    uint64_t* d_offs[2] = {nullptr, nullptr};
    uint64_t off_cap[2] = {0, 0};
    uint8_t* h_out[2] = {nullptr, nullptr};
    uint8_t* d_out[2] = {nullptr, nullptr};
    uint64_t out_cap[2] = {0, 0};
    uint32_t* d_words = nullptr;  // scratch filter for the one-shot host API
    uint64_t words_cap = 0;
    uint8_t* h_xfer[2] = {nullptr, nullptr};  // pinned bounce buffers for large filter copies
    hipEvent_t first = nullptr;  // a fresh filter's first chunk built: the other chunks OR after it

    int init(int dev) {
        if (device == dev) return VBF_OK;
        device = dev;
        for (int b = 0; b < 2; ++b) {
            HIP_TRY(hipStreamCreateWithFlags(&stream[b], hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&done[b], hipEventDisableTiming));
        }
        HIP_TRY(hipEventCreateWithFlags(&first, hipEventDisableTiming));
        return VBF_OK;
    }
    template <class T>
    static int grow(T** h, T** d, uint64_t* cap, uint64_t count) {
        if (count <= *cap) return VBF_OK;
        if (h && *h) HIP_TRY(hipHostFree(*h));
        if (*d) HIP_TRY(hipFree(*d));
        if (h) *h = nullptr;
        *d = nullptr;
        *cap = 0;
        uint64_t want = count + count / 4 + 64;
        if (h) HIP_TRY(hipHostMalloc((void**)h, want * sizeof(T), hipHostMallocDefault));
        HIP_TRY(hipMalloc((void**)d, want * sizeof(T)));
        *cap = want;
        return VBF_OK;
    }
};

// Large host <-> device copies (filter words) bounce through two pinned chunk buffers, so the
// DMA of chunk c+1 overlaps the (threaded) host copy of chunk c; pageable hipMemcpy runs at a
// fraction of the link rate.  Small copies go direct.  Caller holds st.mu and has ordered src.
constexpr uint64_t kXferDirect = 8ull << 20;
// bounce chunk: small enough that the last chunk's host copy (not overlapped) is short
constexpr uint64_t kXferChunk = 16ull << 20;

int xfer_bufs(Staging& st) {
    for (int b = 0; b < 2; ++b)
        if (!st.h_xfer[b]) HIP_TRY(hipHostMalloc((void**)&st.h_xfer[b], kChunkBytes, hipHostMallocDefault));
    return VBF_OK;
}

bool d2h_direct() {  // VBF_D2H_DIRECT=1: pageable hipMemcpy instead of the bounce (A/B)
    static const bool v = [] { const char* e = getenv("VBF_D2H_DIRECT"); return e && atoi(e) != 0; }();
    return v;
}

int xfer_d2h(Staging& st, void* dst, const void* src, uint64_t bytes) {
    if (bytes < kXferDirect || d2h_direct()) {
        HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
        return VBF_OK;
    }
    int rc = xfer_bufs(st);
    if (rc) return rc;
    const uint64_t nc = (bytes + kXferChunk - 1) / kXferChunk;
    for (uint64_t c = 0; c <= nc; ++c) {
        if (c < nc) {
            const int b = (int)(c & 1);
            const uint64_t off = c * kXferChunk, len = std::min<uint64_t>(kXferChunk, bytes - off);
            HIP_TRY(hipMemcpyAsync(st.h_xfer[b], static_cast<const char*>(src) + off, len, hipMemcpyDeviceToHost,
                                   st.stream[b]));
            HIP_TRY(hipEventRecord(st.done[b], st.stream[b]));
        }
        if (c > 0) {
            const int pb = (int)((c - 1) & 1);
            const uint64_t off = (c - 1) * kXferChunk, len = std::min<uint64_t>(kXferChunk, bytes - off);
            HIP_TRY(hipEventSynchronize(st.done[pb]));
            par_memcpy(static_cast<char*>(dst) + off, st.h_xfer[pb], len);
        }
    }
    return VBF_OK;
}

// H2D on st.stream[0..1]; returns with both streams synchronized.
int xfer_h2d(Staging& st, void* dst, const void* src, uint64_t bytes) {
    if (bytes < kXferDirect) {
        HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
        return VBF_OK;
    }
    int rc = xfer_bufs(st);
    if (rc) return rc;
    const uint64_t nc = (bytes + kXferChunk - 1) / kXferChunk;
    for (uint64_t c = 0; c < nc; ++c) {
        const int b = (int)(c & 1);
        const uint64_t off = c * kXferChunk, len = std::min<uint64_t>(kXferChunk, bytes - off);
        if (c >= 2) HIP_TRY(hipEventSynchronize(st.done[b]));  // buffer b's previous DMA finished
        par_memcpy(st.h_xfer[b], static_cast<const char*>(src) + off, len);
        HIP_TRY(hipMemcpyAsync(static_cast<char*>(dst) + off, st.h_xfer[b], len, hipMemcpyHostToDevice, st.stream[b]));
        HIP_TRY(hipEventRecord(st.done[b], st.stream[b]));
    }
    for (int b = 0; b < 2; ++b) HIP_TRY(hipStreamSynchronize(st.stream[b]));
    return VBF_OK;
}

// VBF_H2D_DIRECT=0 forces the pinned bounce for key chunks (A/B); default: direct.
bool h2d_direct() {
    static const bool v = [] { const char* e = getenv("VBF_H2D_DIRECT"); return !e || atoi(e) != 0; }();
    return v;
}

std::mutex g_staging_mu;
std::vector<std::unique_ptr<Staging>> g_staging;

Staging* staging_for(int device) {
    std::lock_guard<std::mutex> lk(g_staging_mu);
    if ((int)g_staging.size() <= device) g_staging.resize(device + 1);
    if (!g_staging[device]) g_staging[device].reset(new Staging());
    return g_staging[device].get();
}

// Streams host keys through the staging buffers, calling launch(batch_on_device, first_key,
// buffer_index, stream) per chunk.  After the loop both streams are synchronized.
template <class Launch, class AfterChunk>
int pipeline_host_keys(Staging& st, const uint8_t* keys, const uint64_t* offsets, uint64_t stride,
                       uint64_t n, int lp, bool need_out, Launch&& launch, AfterChunk&& after) {
    uint64_t lo = 0;
    int c = 0;
    uint64_t pending_lo[2] = {0, 0}, pending_n[2] = {0, 0};
    bool pending[2] = {false, false};
    while (lo < n) {
        // choose the chunk [lo, hi)
        uint64_t hi, bytes, base = 0;
        if (offsets) {
            // largest hi with offsets[hi] - offsets[lo] <= kChunkBytes (a single huge key alone)
            base = offsets[lo];
            const uint64_t* ub = std::upper_bound(offsets + lo + 1, offsets + n + 1, base + kChunkBytes);
            hi = (uint64_t)(ub - offsets) - 1;
            if (hi <= lo) hi = lo + 1;
            bytes = offsets[hi] - base;
        } else {
            uint64_t per = stride ? (kChunkBytes / stride) : n;
            if (per == 0) per = 1;
            hi = (n - lo) < per ? n : lo + per;
            bytes = (hi - lo) * stride;
        }
        const int b = c & 1;
        HIP_TRY(hipEventSynchronize(st.done[b]));  // buffer b free again
        if (pending[b]) {
            int rc = after(b, pending_lo[b], pending_n[b]);
            if (rc) return rc;
            pending[b] = false;
        }
        const uint8_t* src = keys + (offsets ? base : lo * stride);
        int rc;
        if (h2d_direct()) {
            // the runtime's own pageable path runs at the link rate: no host bounce copy
            rc = Staging::grow<uint8_t>(nullptr, &st.d_keys[b], &st.key_cap[b], bytes ? bytes : 1);
            if (rc) return rc;
            HIP_TRY(hipMemcpyAsync(st.d_keys[b], src, bytes, hipMemcpyHostToDevice, st.stream[b]));
        } else {
            rc = Staging::grow(&st.h_keys[b], &st.d_keys[b], &st.key_cap[b], bytes ? bytes : 1);
            if (rc) return rc;
            if (bytes) par_memcpy(st.h_keys[b], src, bytes);
            HIP_TRY(hipMemcpyAsync(st.d_keys[b], st.h_keys[b], bytes, hipMemcpyHostToDevice, st.stream[b]));
        }
        const uint64_t* d_off = nullptr;
        if (offsets) {
            rc = Staging::grow(&st.h_offs[b], &st.d_offs[b], &st.off_cap[b], hi - lo + 1);
            if (rc) return rc;
            par_memcpy(st.h_offs[b], offsets + lo, (hi - lo + 1) * sizeof(uint64_t));
            HIP_TRY(hipMemcpyAsync(st.d_offs[b], st.h_offs[b], (hi - lo + 1) * sizeof(uint64_t),
                                   hipMemcpyHostToDevice, st.stream[b]));
            d_off = st.d_offs[b];
        }
        if (need_out) {
            rc = Staging::grow(&st.h_out[b], &st.d_out[b], &st.out_cap[b], hi - lo);
            if (rc) return rc;
        }
        vbf::KeyBatch kb = batch(st.d_keys[b], d_off, base, stride, hi - lo, lp);
        rc = launch(kb, lo, b, st.stream[b]);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(st.done[b], st.stream[b]));
        pending[b] = true;
        pending_lo[b] = lo;
        pending_n[b] = hi - lo;
        lo = hi;
        ++c;
    }
    for (int b = 0; b < 2; ++b) {
        HIP_TRY(hipStreamSynchronize(st.stream[b]));
        if (pending[b]) {
            int rc = after(b, pending_lo[b], pending_n[b]);
            if (rc) return rc;
            pending[b] = false;
        }
    }
    return VBF_OK;
}

// ---------------------------------------------------------------------------------------
// Filter handle.  Storage is shared between clones (bf.rs:249 clones the Arc).
// ---------------------------------------------------------------------------------------
struct Storage {
    int device = 0;  // VBF_DEVICE_HOST: the bits live in host memory (h_words), no HIP at all
    uint32_t m = 0;
    uint64_t nwords = 0;
    uint32_t* d_words = nullptr;
    // Host-resident bits.  Allocated on first use (host_words): a filter that is created on the
    // host and moved to a GPU before any set -- the compaction filter, bf.rs:62-81 then
    // build_filter_from_entries -- never zero-fills m/8 bytes of host memory.
    // Empty while pristine and never touched = all zero.
    std::vector<uint32_t> h_words;
    // The last asynchronous operation on d_words (a _dev call on the caller's stream): later
    // calls on other streams wait for it on the device, host-side calls wait for it on the host,
    // so every operation on one filter is ordered as the reference's Mutex<BitVec> orders them.
    hipEvent_t last = nullptr;
    bool pending = false;
    std::mutex mu;  // the reference's Mutex<BitVec>
    // Asynchronous set_host jobs (vbf_filter_set_host_async) queued on the device's worker and
    // not yet run.  Every other call on the filter first waits for them (storage_drain), so calls
    // stay ordered as the reference's Mutex orders them; a failed job's status is reported by the
    // next call that drains.
    uint64_t jobs_queued = 0, jobs_done = 0;
    pid_t jobs_pid = 0;  // the process whose worker runs the queued jobs (a forked child has none)
    std::condition_variable jobs_cv;
    int async_rc = VBF_OK;
    std::string async_msg;
    // Host mirror of d_words (device-resident filters only): a pinned copy that answers
    // single-key contains on the CPU, as the reference's read path calls it once per SST per get
    // (key_range/range.rs:130,136,171).  Valid while no device write happened since it was
    // filled; filled lazily by the first small contains (one D2H), or queued right after every
    // device write in VBF_MIRROR_EAGER mode.
    int mirror_mode = -1;  // -1: the process default (VBF_MIRROR, default lazy)
    // No bit was ever set since the array was created or cleared (BitVec::from_elem(m, false),
    // bf.rs:71): a migrate allocates zeroed words on the target instead of copying them.
    bool pristine = true;
    uint32_t* mirror = nullptr;
    bool mirror_ok = false;
    // vbf_filter_words_dev handed out d_words: a caller kernel may write the bits behind the
    // library's back, so the mirror is not trusted (every host read copies the words again) until
    // the caller declares its write with vbf_filter_stream_record.
    bool ext_write = false;
    bool mirror_current() const { return mirror_ok && !ext_write; }
    bool host() const { return device == VBF_DEVICE_HOST; }
    void free_mirror() {
        if (mirror && !hip_forked()) (void)hipHostFree(mirror);
        mirror = nullptr;
        mirror_ok = false;
    }
    ~Storage() {
        if (hip_forked()) {  // a forked child: the allocations are the parent's, and HIP is off limits
            mirror = nullptr;
            return;
        }
        if (d_words) {
            int prev = -1;
            (void)hipGetDevice(&prev);
            (void)hipSetDevice(device);
            if (pending) (void)hipEventSynchronize(last);
            (void)hipFree(d_words);
            if (prev >= 0) (void)hipSetDevice(prev);
        }
        free_mirror();
        if (last) (void)hipEventDestroy(last);
    }
};

// Caller holds s.mu, host-resident storage: the words, allocated (zeroed) on first use.
uint32_t* host_words(Storage& s) {
    if (s.h_words.size() != s.nwords) s.h_words.assign(s.nwords, 0u);
    return s.h_words.data();
}

// Caller holds s.mu: true when every queued asynchronous job has run.  Jobs queued by the parent
// of a forked child never run in the child (the worker thread stayed in the parent): the child
// counts them as failed instead of waiting for them forever.
bool storage_jobs_settled(Storage& s) {
    if (s.jobs_done == s.jobs_queued) return true;
    if (s.jobs_pid != getpid()) {
        s.jobs_done = s.jobs_queued;
        if (s.async_rc == VBF_OK) {
            s.async_rc = VBF_EINVAL;
            s.async_msg = "the process forked while an asynchronous set was queued; its bits are not in this copy";
        }
        return true;
    }
    return false;
}

// Caller holds `lk` on s.mu: waits until every asynchronous set_host job queued on the filter
// has run (the worker takes s.mu to run one, the wait releases it), then reports a failed job.
int storage_drain(Storage& s, std::unique_lock<std::mutex>& lk) {
    s.jobs_cv.wait(lk, [&] { return storage_jobs_settled(s); });
    if (s.async_rc != VBF_OK) {
        const int rc = s.async_rc;
        const std::string m = s.async_msg;
        s.async_rc = VBF_OK;
        s.async_msg.clear();
        return fail(rc, "an earlier asynchronous set on this filter failed: %s", m.c_str());
    }
    return VBF_OK;
}

int mirror_default() {
    static const int v = [] {
        const char* e = getenv("VBF_MIRROR");
        return e ? std::max(0, std::min(2, atoi(e))) : (int)VBF_MIRROR_LAZY;
    }();
    return v;
}
inline int mirror_mode(const Storage& s) { return s.mirror_mode < 0 ? mirror_default() : s.mirror_mode; }
// contains_host batches of at most this many keys answer from the mirror (~0.1 us per key on
// one core, against ~27 us for the staged GPU round trip)
uint64_t mirror_max_keys() {
    static const uint64_t v = [] {
        const char* e = getenv("VBF_MIRROR_MAX_KEYS");
        return e ? (uint64_t)strtoull(e, nullptr, 10) : (uint64_t)256;
    }();
    return v;
}

// Caller holds s.mu.  The stream `st` (any, including the legacy NULL stream) waits for the
// filter's last asynchronous operation.
int storage_wait(Storage& s, hipStream_t st) {
    if (s.pending) HIP_TRY(hipStreamWaitEvent(st, s.last, 0));
    return VBF_OK;
}
// Caller holds s.mu: the operation just queued on `st` is now the filter's last one.
int storage_mark(Storage& s, hipStream_t st) {
    if (!s.last) HIP_TRY(hipEventCreateWithFlags(&s.last, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(s.last, st));
    s.pending = true;
    return VBF_OK;
}
// Caller holds s.mu: the host waits until the filter's last asynchronous operation finished.
int storage_sync(Storage& s) {
    if (s.pending) {
        HIP_TRY(hipEventSynchronize(s.last));
        s.pending = false;
    }
    return VBF_OK;
}

// Caller holds s.mu, on s.device: a device write was just queued on `st` (and marked).  The
// mirror is stale; in eager mode its refresh is queued behind the write on the same stream, so
// it is valid once the filter's last event completes (every host reader syncs that first).
int mirror_after_write(Storage& s, hipStream_t st) {
    s.mirror_ok = false;
    if (mirror_mode(s) != VBF_MIRROR_EAGER || !s.nwords) return VBF_OK;
    if (!s.mirror) HIP_TRY(hipHostMalloc((void**)&s.mirror, s.nwords * 4, hipHostMallocDefault));
    HIP_TRY(hipMemcpyAsync(s.mirror, s.d_words, s.nwords * 4, hipMemcpyDeviceToHost, st));
    s.mirror_ok = true;
    return storage_mark(s, st);
}

// ---------------------------------------------------------------------------------------
// Host-resident filters (VBF_DEVICE_HOST): the memtable's filter, built one key per put
// (memtable/mem.rs:207-221: contains, then set) and probed one key per get (:223-230).  A GPU
// launch per key would cost two PCIe round trips per put, so these run on the CPU in the
// library, with the same SipHash-1-3 rounds as the kernels (sip13.hpp, compiled for the host)
// and Rust's `hash % m` (bf.rs:88,99).
// ---------------------------------------------------------------------------------------
vbf::Prefix host_prefix(const uint8_t* key, uint64_t len, bool lp) {
    vbf::Sip st = vbf::sip_init();
    if (lp) vbf::sip_compress(st, len);  // Hash for [u8]: write_usize(len) first
    uint64_t c = 0;
    for (; c + 8 <= len; c += 8) {
        uint64_t w;
        std::memcpy(&w, key + c, 8);  // little-endian block
        vbf::sip_compress(st, w);
    }
    vbf::Prefix p;
    p.st = st;
    p.r = (uint32_t)(len & 7);
    uint64_t t = 0;
    if (p.r) std::memcpy(&t, key + c, p.r);
    p.tail = t;
    p.total = (uint32_t)((len + (lp ? 8 : 0) + 8) & 0xff);
    return p;
}

inline void host_key(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t j,
                     const uint8_t** kp, uint64_t* len) {
    if (offsets) {
        *kp = keys + offsets[j];
        *len = offsets[j + 1] - offsets[j];
    } else {
        *kp = keys + j * stride;
        *len = stride;
    }
}

// bf.rs:84-92 per key (the caller counts the elements).
void host_set(uint32_t* w, uint32_t m, uint32_t k, const uint8_t* keys, const uint64_t* offsets, uint64_t stride,
              uint64_t n, bool lp) {
    for (uint64_t j = 0; j < n; ++j) {
        const uint8_t* kp;
        uint64_t len;
        host_key(keys, offsets, stride, j, &kp, &len);
        const vbf::Prefix p = host_prefix(kp, len, lp);
        for (uint32_t i = 0; i < k; ++i) {
            const uint32_t idx = (uint32_t)(vbf::prefix_hash(p, i) % (uint64_t)m);
            w[idx >> 5] |= 1u << (idx & 31);
        }
    }
}

// bf.rs:95-105 per key: early exit on the first clear bit; k == 0 answers true.
void host_contains(const uint32_t* w, uint32_t m, uint32_t k, const uint8_t* keys, const uint64_t* offsets,
                   uint64_t stride, uint64_t n, bool lp, uint8_t* out) {
    for (uint64_t j = 0; j < n; ++j) {
        const uint8_t* kp;
        uint64_t len;
        host_key(keys, offsets, stride, j, &kp, &len);
        const vbf::Prefix p = host_prefix(kp, len, lp);
        uint8_t hit = 1;
        for (uint32_t i = 0; i < k; ++i) {
            const uint32_t idx = (uint32_t)(vbf::prefix_hash(p, i) % (uint64_t)m);
            if (!((w[idx >> 5] >> (idx & 31)) & 1u)) {
                hit = 0;
                break;
            }
        }
        out[j] = hit;
    }
}

std::mutex g_stream_mu;
std::vector<hipStream_t> g_filter_streams;

int filter_stream(int device, hipStream_t* out) {
    std::lock_guard<std::mutex> lk(g_stream_mu);
    if ((int)g_filter_streams.size() <= device) g_filter_streams.resize(device + 1, nullptr);
    if (!g_filter_streams[device]) HIP_TRY(hipStreamCreateWithFlags(&g_filter_streams[device], hipStreamNonBlocking));
    *out = g_filter_streams[device];
    return VBF_OK;
}

inline uint64_t align256(uint64_t x) { return (x + 255) & ~255ull; }

// One host entry point's scope on `device` (HOST_CALL): the device's shared stream `s` and the
// call's turn on that stream and its workspaces (Staging::host_mu).  Every return that does not
// follow finish (or settled) drains the stream in the destructor, before the lock is released and,
// HOST_CALL's device guard being older, before the previous device is restored: no failing return
// leaves work in flight that reads or writes the caller's buffers, the call's locals or a workspace
// the next holder may grow.  Declared after the locals its copies use; filter locks and their drain
// are taken before it (host_mu's lock order).
struct HostCall {
    std::unique_lock<std::mutex> lk;
    hipStream_t s = nullptr;
    bool drained = false;
    std::vector<std::vector<uint64_t>> rebased;  // up_rebased's sources, kept until the drain

    ~HostCall() {
        if (s && !drained) (void)hipStreamSynchronize(s);
    }
    int begin(int device) {  // on `device` (DEVICE_SCOPE)
        if (int rc = filter_stream(device, &s)) return rc;
        lk = std::unique_lock<std::mutex>(staging_for(device)->host_mu);
        return VBF_OK;
    }
    // Host <-> device copies of `count` elements; nothing when count == 0 or the host side is NULL.
    int copy(void* dst, const void* src, uint64_t bytes, hipMemcpyKind kind) {
        if (bytes) HIP_TRY(hipMemcpyAsync(dst, src, bytes, kind, s));
        return VBF_OK;
    }
    template <class T>
    int up(T* dst, const T* src, uint64_t count) {
        return src ? copy(dst, src, count * sizeof(T), hipMemcpyHostToDevice) : VBF_OK;
    }
    template <class T>
    int down(T* dst, const T* src, uint64_t count) {
        return dst ? copy(dst, src, count * sizeof(T), hipMemcpyDeviceToHost) : VBF_OK;
    }
    // offsets[i] - offsets[0]: positions in a device copy that starts at the first offset.
    int up_rebased(uint64_t* dst, const uint64_t* offsets, uint64_t count) {
        if (!count || !offsets) return VBF_OK;
        rebased.emplace_back(offsets, offsets + count);
        for (auto& x : rebased.back()) x -= offsets[0];
        return up(dst, rebased.back().data(), count);
    }
    int sync() {  // the mid-call drains
        HIP_TRY(hipStreamSynchronize(s));
        return VBF_OK;
    }
    int finish() {  // the success path's last drain
        int rc = sync();
        drained = !rc;
        return rc ? rc : ok();
    }
    // For a success path that enqueued nothing, or ends in a core call that returns synchronised.
    void settled() { drained = true; }
};

// DEVICE_SCOPE, then the host call's scope `name`; returns either's error.
#define HOST_CALL(name, dev) \
    DEVICE_SCOPE(dev);       \
    HostCall name;           \
    if (int hrc_ = name.begin(dev)) return hrc_

// A device image: parts laid end to end in the order added, each on a 256-byte boundary.
template <class T>
struct Part {
    uint64_t off;
    bool present;
};
struct DevImage {
    uint64_t bytes = 0;  // the last part's end
    void* base = nullptr;
    template <class T>
    Part<T> add(uint64_t count, bool present = true) {
        const Part<T> p{align256(bytes), present};
        bytes = p.off + (present ? count * sizeof(T) : 0);
        return p;
    }
    int alloc(HostCall& call, int slot) { return get_workspace(call.s, bytes, &base, slot); }
    template <class T>
    T* ptr(Part<T> p) const {
        return p.present ? reinterpret_cast<T*>(static_cast<char*>(base) + p.off) : nullptr;
    }
};

// For offsets that are absolute positions in the caller's arena: the pointer they index, given the
// device copy `dev` of the arena's bytes from `first` on.
const uint8_t* arena_base(const uint8_t* dev, uint64_t first) {
    return reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(dev) - first);
}

// Caller holds s.mu (drained), on s.device: the mirror holds the current bits (one D2H when
// it is stale).
int mirror_fill(Storage& s) {
    int rc = storage_sync(s);
    if (rc) return rc;
    if (s.mirror_current() || !s.nwords) return VBF_OK;
    if (!s.mirror) HIP_TRY(hipHostMalloc((void**)&s.mirror, s.nwords * 4, hipHostMallocDefault));
    hipStream_t fs;
    if ((rc = filter_stream(s.device, &fs))) return rc;
    HIP_TRY(hipMemcpyAsync(s.mirror, s.d_words, s.nwords * 4, hipMemcpyDeviceToHost, fs));
    HIP_TRY(hipStreamSynchronize(fs));
    s.mirror_ok = true;
    return VBF_OK;
}

int new_storage(int device, uint32_t m, std::shared_ptr<Storage>* out) {
    auto s = std::make_shared<Storage>();
    s->device = device;
    s->m = m;
    s->nwords = ((uint64_t)m + 31) / 32;
    if (device == VBF_DEVICE_HOST) {
        // BitVec::from_elem(m, false) (bf.rs:71): allocated on first use (host_words)
    } else if (s->nwords) {
        hipStream_t st;
        int rc = filter_stream(device, &st);
        if (rc) return rc;
        HIP_TRY(hipMalloc((void**)&s->d_words, s->nwords * 4));
        // zeroed on the filter's stream, not waited for: every later use of the words is ordered
        // after the filter's last event (storage_wait / storage_sync)
        HIP_TRY(hipMemsetAsync(s->d_words, 0, s->nwords * 4, st));
        if ((rc = storage_mark(*s, st))) return rc;
    }
    *out = std::move(s);
    return VBF_OK;
}

// ---------------------------------------------------------------------------------------
// Phase profiling: when enabled, every kernel phase is bracketed by hipEvents on its stream.
// ---------------------------------------------------------------------------------------
std::atomic<bool> g_prof{false};
std::mutex g_prof_mu;
struct PhaseRec {
    int phase;
    hipEvent_t a, b;
};
std::vector<PhaseRec> g_prof_recs;
thread_local hipEvent_t g_open[vbf::kNumPhases] = {};

}  // namespace

namespace vbf {
void phase_begin(int phase, hipStream_t s) {
    if (!g_prof.load(std::memory_order_relaxed)) return;
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return;
    (void)hipEventRecord(e, s);
    g_open[phase] = e;
}
void phase_end(int phase, hipStream_t s) {
    if (!g_prof.load(std::memory_order_relaxed) || !g_open[phase]) return;
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return;
    (void)hipEventRecord(e, s);
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_recs.push_back(PhaseRec{phase, g_open[phase], e});
    g_open[phase] = nullptr;
}
}  // namespace vbf

namespace {

// ---------------------------------------------------------------------------------------
// SST data.db decode (vbf_sst.hip): count pass + scan, one 16-byte readback (entry total and
// error word) so the caller can size or validate, then the emit pass queued on the stream.
// ---------------------------------------------------------------------------------------
int sst_count_pass(const uint8_t* data, uint64_t len, const uint32_t* blocks, uint64_t nblocks,
                   hipStream_t s, vbf::SstArgs* a, uint64_t* n_out, uint32_t* uniform_len = nullptr) {
    *a = vbf::SstArgs{};
    *n_out = 0;
    if (uniform_len) *uniform_len = 0xFFFFFFFFu;
    if (len && (!data || !blocks || !nblocks))
        return fail(VBF_EINVAL, "data.db of %llu bytes needs its block start offsets (index.db)",
                    (unsigned long long)len);
    if (!len && nblocks) return fail(VBF_EINVAL, "%llu block offsets for an empty data.db", (unsigned long long)nblocks);
    if (nblocks >= 0x7FFFFFFFull) return fail(VBF_EINVAL, "too many blocks (%llu)", (unsigned long long)nblocks);
    if (!len) return VBF_OK;
    size_t tmpb = 0, tmpr = 0;
    HIP_TRY(vbf::sst_scan(nullptr, nullptr, nblocks + 1, nullptr, &tmpb, s));
    HIP_TRY(vbf::sst_len_range(nullptr, nullptr, nblocks, nullptr, nullptr, &tmpr, s));
    tmpb = std::max(tmpb, tmpr);
    const uint64_t o_ebase = align256((nblocks + 1) * 4);
    const uint64_t o_pos = o_ebase + align256((nblocks + 1) * 8);
    const uint64_t o_lmin = o_pos + align256(vbf::sst_pos_bytes(nblocks));
    const uint64_t o_lmax = o_lmin + align256(nblocks * 4);
    const uint64_t o_err = o_lmax + align256(nblocks * 4);
    const uint64_t o_tmp = o_err + 256;
    void* ws = nullptr;
    int rc = get_workspace(s, o_tmp + tmpb, &ws, kWsSstScratch);
    if (rc) return rc;
    char* base = static_cast<char*>(ws);
    uint32_t* counts = reinterpret_cast<uint32_t*>(base);
    uint64_t* ebase = reinterpret_cast<uint64_t*>(base + o_ebase);
    uint32_t* err = reinterpret_cast<uint32_t*>(base + o_err);
    HIP_TRY(hipMemsetAsync(counts, 0, (nblocks + 1) * 4, s));
    HIP_TRY(hipMemsetAsync(err, 0, 4, s));
    HIP_TRY(hipMemsetAsync(err + 1, 0xFF, 12, s));
    uint16_t* pos = reinterpret_cast<uint16_t*>(base + o_pos);
    static const uint32_t walk_v = [] {  // VBF_SST_WALK=0: the scalar entry walk (A/B)
        const char* e = getenv("VBF_SST_WALK");
        return e ? (uint32_t)(atoi(e) != 0) : 1u;
    }();
    static const uint32_t abl = [] {
        const char* e = VBF_ABLATION_BUILD ? getenv("VBF_ABLATE") : nullptr;
        return e ? (uint32_t)atoi(e) : 0u;
    }();
    uint32_t* lmin = reinterpret_cast<uint32_t*>(base + o_lmin);
    uint32_t* lmax = reinterpret_cast<uint32_t*>(base + o_lmax);
    *a = vbf::SstArgs{data, len, blocks, nblocks, counts, pos, lmin, lmax, ebase, nullptr, nullptr, nullptr, nullptr,
                      nullptr, err, abl, walk_v};
    vbf::phase_begin(vbf::kPhaseSstWalk, s);
    HIP_TRY(vbf::sst_count(*a, s));
    vbf::phase_end(vbf::kPhaseSstWalk, s);
    vbf::phase_begin(vbf::kPhaseSstScan, s);
    HIP_TRY(vbf::sst_scan(counts, ebase, nblocks + 1, base + o_tmp, &tmpb, s));
    if (uniform_len) HIP_TRY(vbf::sst_len_range(lmin, lmax, nblocks, err + 2, base + o_tmp, &tmpb, s));
    vbf::phase_end(vbf::kPhaseSstScan, s);
    uint64_t total = 0;
    uint32_t ev[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(&total, ebase + nblocks, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(ev, err, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (ev[0]) {
        const char* what = (ev[0] & 8) ? "block offsets not increasing / not starting at 0 / past the end"
                         : (ev[0] & 4) ? "block larger than 65535 bytes"
                         : (ev[0] & 2) ? "more than 256 entries in a block"
                                       : "entry crosses the block end (truncated data.db or wrong index)";
        return fail(VBF_EINVAL, "malformed data.db at block %u: %s", ev[1], what);
    }
    if (len < 17 * total) return fail(VBF_EINVAL, "inconsistent entry count %llu", (unsigned long long)total);
    *n_out = total;
    if (uniform_len && total && ev[2] == ev[3] && a->ablate == 0) *uniform_len = ev[2];
    return VBF_OK;
}

// vbf_sst_decode_*: the caller's outputs (NULL = not asked for) hold n entries and kb key bytes.
int sst_decode_caps(bool entry_arrays, bool offsets, bool keys, uint64_t entries_cap, uint64_t keys_cap, uint64_t n,
                    uint64_t kb) {
    if (entry_arrays && entries_cap < n)
        return fail(VBF_EINVAL, "entry arrays hold %llu < %llu entries", (unsigned long long)entries_cap,
                    (unsigned long long)n);
    if (offsets && entries_cap < n + 1)
        return fail(VBF_EINVAL, "offsets holds %llu < %llu entries", (unsigned long long)entries_cap,
                    (unsigned long long)(n + 1));
    if (keys && keys_cap < kb)
        return fail(VBF_EINVAL, "keys holds %llu < %llu bytes", (unsigned long long)keys_cap, (unsigned long long)kb);
    return VBF_OK;
}

int sst_emit_pass(vbf::SstArgs a, uint8_t* keys, uint64_t* offsets, uint32_t* val_off, uint64_t* created,
                  uint8_t* tomb, hipStream_t s) {
    if (!a.len) {
        if (offsets) HIP_TRY(hipMemsetAsync(offsets, 0, 8, s));
        return VBF_OK;
    }
    if (keys && ((uintptr_t)keys & 3)) return fail(VBF_EINVAL, "keys buffer must be 4-byte aligned");
    a.keys = keys;
    a.offsets = offsets;
    a.val_off = val_off;
    a.created = created;
    a.tomb = tomb;
    if (!keys && !offsets && !val_off && !created && !tomb) return VBF_OK;
    vbf::phase_begin(vbf::kPhaseSstEmit, s);
    HIP_TRY(vbf::sst_emit(a, s));
    vbf::phase_end(vbf::kPhaseSstEmit, s);
    return VBF_OK;
}

// ---------------------------------------------------------------------------------------
// SST data.db / index.db encode (vbf_sst_write.hip) on device pointers: the block segmentation
// and the scan that places the index records, one readback (the sizes and the error word), then
// the emit passes queued on the stream.  The three sizes are written whenever they are known,
// so a too-small capacity still reports them.
// ---------------------------------------------------------------------------------------
int sst_encode(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n, const uint32_t* val_off,
               const int64_t* created, const uint8_t* tomb, uint8_t* data, uint64_t data_cap, uint64_t* data_len,
               uint8_t* index, uint64_t index_cap, uint64_t* index_len, uint32_t* blocks, uint64_t blocks_cap,
               uint64_t* nblocks, hipStream_t s) {
    if (!data_len || !index_len || !nblocks) return fail(VBF_EINVAL, "data_len / index_len / nblocks is NULL");
    *data_len = *index_len = *nblocks = 0;
    if (n == 0) return VBF_OK;
    constexpr uint64_t kMaxKey = 4096 - 17;
    if (!offsets && stride > kMaxKey)
        return fail(VBF_EINVAL, "entry of %llu bytes exceeds a 4096-byte block (BlockIsFull)",
                    (unsigned long long)(stride + 17));
    if (!keys && !offsets && stride) return fail(VBF_EINVAL, "keys is NULL");
    if (n >= (1ull << 32) / 17)
        return fail(VBF_EINVAL, "data.db of %llu entries reaches 2^32 bytes: index.db's u32 block offsets cannot address it",
                    (unsigned long long)n);
    vbf::SstEncArgs a{};
    a.keys = keys;
    a.offsets = offsets;
    a.stride = stride;
    a.n = n;
    a.val_off = val_off;
    a.created = created;
    a.tomb = tomb;
    uint64_t dl, il, nb;
    if (!offsets) {  // equal entries: 4096 / (stride + 17) per block, nothing to compute on the device
        const uint64_t es = stride + 17, per = 4096 / es;
        dl = n * es;
        nb = (n + per - 1) / per;
        il = nb * (stride + 8);
    } else {
        a.ntiles = (n + vbf::kEncTile - 1) / vbf::kEncTile;
        a.ngroups = (a.ntiles + vbf::kEncGroup - 1) / vbf::kEncGroup;
        const uint64_t tiles_pad = a.ngroups * vbf::kEncGroup;
        size_t tmpb = 0;
        HIP_TRY(vbf::scan_u64(nullptr, &tmpb, nullptr, nullptr, a.ntiles + 1, s));
        const uint64_t o_tab = align256(n), o_gtab = o_tab + align256(tiles_pad * vbf::kEncReach);
        const uint64_t o_gep = o_gtab + align256(a.ngroups * vbf::kEncReach), o_ep = o_gep + align256(a.ngroups);
        const uint64_t o_tsum = o_ep + align256(tiles_pad), o_tbase = o_tsum + align256((a.ntiles + 1) * 8);
        const uint64_t o_err = o_tbase + align256((a.ntiles + 1) * 8), o_tmp = o_err + 256;
        void* ws = nullptr;
        int rc = get_workspace(s, o_tmp + tmpb, &ws, kWsSstEnc);
        if (rc) return rc;
        char* b = static_cast<char*>(ws);
        a.delta = reinterpret_cast<uint8_t*>(b);
        a.tab = reinterpret_cast<uint8_t*>(b + o_tab);
        a.gtab = reinterpret_cast<uint8_t*>(b + o_gtab);
        a.gep = reinterpret_cast<uint8_t*>(b + o_gep);
        a.ep = reinterpret_cast<uint8_t*>(b + o_ep);
        a.tsum = reinterpret_cast<uint64_t*>(b + o_tsum);
        uint64_t* tbase = reinterpret_cast<uint64_t*>(b + o_tbase);
        a.tbase = tbase;
        a.err = reinterpret_cast<uint32_t*>(b + o_err);
        HIP_TRY(hipMemsetAsync(a.err, 0, 4, s));
        HIP_TRY(hipMemsetAsync(a.err + 1, 0xFF, 4, s));
        HIP_TRY(hipMemsetAsync(a.tsum + a.ntiles, 0, 8, s));
        HIP_TRY(vbf::sst_enc_segment(a, s));
        HIP_TRY(vbf::scan_u64(b + o_tmp, &tmpb, a.tsum, tbase, a.ntiles + 1, s));
        vbf::phase_end(vbf::kPhaseEncScan, s);
        uint64_t tot = 0, oe[2] = {0, 0};
        uint32_t ev[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(&tot, tbase + a.ntiles, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&oe[0], offsets, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&oe[1], offsets + n, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(ev, a.err, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (ev[0] & vbf::kEncErrOrder) return fail(VBF_EINVAL, "offsets descend at entry %u", ev[1]);
        if (ev[0] & vbf::kEncErrBig)
            return fail(VBF_EINVAL, "entry %u exceeds a 4096-byte block (BlockIsFull): keys hold at most 4079 bytes", ev[1]);
        dl = (oe[1] - oe[0]) + 17 * n;
        nb = tot >> 40;
        il = tot & ((1ull << 40) - 1);
    }
    if (dl >= (1ull << 32))
        return fail(VBF_EINVAL, "data.db of %llu bytes reaches 2^32: index.db's u32 block offsets cannot address it",
                    (unsigned long long)dl);
    if (!keys && dl > 17 * n) return fail(VBF_EINVAL, "keys is NULL");
    *data_len = dl;
    *index_len = il;
    *nblocks = nb;
    if (data && data_cap < dl)
        return fail(VBF_EINVAL, "data holds %llu < %llu bytes", (unsigned long long)data_cap, (unsigned long long)dl);
    if (index && index_cap < il)
        return fail(VBF_EINVAL, "index holds %llu < %llu bytes", (unsigned long long)index_cap, (unsigned long long)il);
    if (blocks && blocks_cap < nb)
        return fail(VBF_EINVAL, "blocks holds %llu < %llu offsets", (unsigned long long)blocks_cap, (unsigned long long)nb);
    a.data = data;
    a.index = index;
    a.blocks = blocks;
    if (data || index || blocks) HIP_TRY(vbf::sst_enc_emit(a, s));
    return VBF_OK;
}

// index.db (indexer.rs:151-170: u32 key_len | key | u32 block offset per block) -> offsets.
int parse_index(const uint8_t* index, uint64_t len, std::vector<uint32_t>* out) {
    out->clear();
    uint64_t p = 0;
    while (p < len) {
        if (len - p < 4) return fail(VBF_EINVAL, "index.db truncated at byte %llu", (unsigned long long)p);
        uint32_t L;
        memcpy(&L, index + p, 4);
        if (len - p - 4 < (uint64_t)L + 4) return fail(VBF_EINVAL, "index.db truncated at byte %llu", (unsigned long long)p);
        uint32_t off;
        memcpy(&off, index + p + 4 + L, 4);
        out->push_back(off);
        p += (uint64_t)L + 8;
    }
    return VBF_OK;
}

// ---------------------------------------------------------------------------------------
// Host keys into a device-resident filter.  Caller holds s.mu (drained), on s.device: the keys
// stream through the device's staging pipeline (H2D of chunk c+1 under the kernels of chunk c)
// and the bits are merged into d_words; returns with the work finished.
// ---------------------------------------------------------------------------------------
int device_set_host(Storage& s, uint32_t k, const uint8_t* keys, const uint64_t* offsets, uint64_t stride,
                    uint64_t n, int lp) {
    Staging* st = staging_for(s.device);
    std::lock_guard<std::mutex> lk2(st->mu);
    int rc = st->init(s.device);
    if (rc) return rc;
    if ((rc = storage_sync(s))) return rc;  // earlier _dev work on this filter, any stream
    s.mirror_ok = false;
    // A pristine filter (new or cleared, never written: the compaction filter, sized.rs:192-193)
    // takes its first chunk as BloomFilter::new fused with the build (VBF_BUILD_FRESH: the segment
    // pass writes its words without reading them, where one chunk and one workgroup per segment
    // allow), as the benchmark's step does; the other chunks wait for it on the device, then OR
    // in with word atomics as before.
    const bool fresh = s.pristine;
    s.pristine = false;
    rc = pipeline_host_keys(
        *st, keys, offsets, stride, n, lp, false,
        [&](const vbf::KeyBatch& kb, uint64_t lo, int, hipStream_t hs) -> int {
            if (fresh && lo == 0) {
                int r = do_build(kb, s.m, k, s.d_words, VBF_BUILD_AUTO | VBF_BUILD_FRESH, false, hs);
                if (r) return r;
                HIP_TRY(hipEventRecord(st->first, hs));
                return VBF_OK;
            }
            if (fresh) HIP_TRY(hipStreamWaitEvent(hs, st->first, 0));
            return do_build(kb, s.m, k, s.d_words, VBF_BUILD_AUTO, true, hs);
        },
        [](int, uint64_t, uint64_t) { return VBF_OK; });
    if (rc) return rc;
    return mirror_after_write(s, st->stream[0]);
}

// ---------------------------------------------------------------------------------------
// Asynchronous set_host (vbf_filter_set_host_async): one worker thread per device runs the
// queued jobs in order, each exactly as a synchronous set_host would under the filter's lock.
// The submitting thread returns at once, so a serial caller -- the compaction loop that builds
// one filter per merged table (compactors/sized.rs:170-200) -- keeps merging the next table
// while the GPUs build, one filter per device with VBF_DEVICE_AUTO placement.
// ---------------------------------------------------------------------------------------
struct AsyncJob {
    std::shared_ptr<Storage> s;
    uint32_t k = 0;
    const uint8_t* keys = nullptr;
    const uint64_t* offsets = nullptr;
    uint64_t stride = 0, n = 0;
    int lp = 1;
    std::unique_ptr<uint8_t[]> own_keys;  // the library's copy when the caller passed no release
    std::unique_ptr<uint64_t[]> own_offs;
    void (*release)(void*) = nullptr;
    void* ctx = nullptr;
};

class AsyncQueue {
  public:
    static AsyncQueue& get(int device) {
        static std::mutex mu;
        static std::vector<AsyncQueue*> qs;  // never destroyed: the workers outlive static teardown
        std::lock_guard<std::mutex> lk(mu);
        if ((int)qs.size() <= device) qs.resize(device + 1, nullptr);
        // a forked child inherits the queue objects but not their threads: start new ones
        if (!qs[device] || qs[device]->pid_ != getpid()) qs[device] = new AsyncQueue();
        return *qs[device];
    }
    void push(AsyncJob* j) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            q_.push_back(j);
        }
        cv_.notify_one();
    }

  private:
    AsyncQueue() : pid_(getpid()) { std::thread([this] { loop(); }).detach(); }
    void loop() {
        for (;;) {
            AsyncJob* j;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return !q_.empty(); });
                j = q_.front();
                q_.erase(q_.begin());
            }
            run(*j);
            Storage& s = *j->s;
            {
                std::lock_guard<std::mutex> lk(s.mu);
                ++s.jobs_done;
            }
            s.jobs_cv.notify_all();
            // after the job counts as done: a release callback may call back into the library
            // (vbf_filter_sync, or a free in a Rust Drop) without waiting for its own job
            if (j->release) j->release(j->ctx);
            delete j;
        }
    }
    static void run(AsyncJob& j) {
        Storage& s = *j.s;
        std::lock_guard<std::mutex> lk(s.mu);
        int rc;
        {
            DeviceGuard g(s.device);
            if (g.forked) {
                rc = fail_forked();
            } else if (g.err != hipSuccess) {
                rc = fail(VBF_ENODEV, "hipSetDevice(%d): %s", s.device, hipGetErrorString(g.err));
            } else {
                (void)hipGetLastError();  // no earlier job's failure is this job's
                rc = device_set_host(s, j.k, j.keys, j.offsets, j.stride, j.n, j.lp);
            }
        }
        if (rc && s.async_rc == VBF_OK) {  // the first failure is reported by the next call that drains
            s.async_rc = rc;
            s.async_msg = g_err;
        }
    }
    const pid_t pid_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::vector<AsyncJob*> q_;
};

std::atomic<uint64_t> g_auto_rr{0};

// xor over words of (w_i * G + (i + 1) * C), 64-bit wrapping: velarixdb_amd/filter_file.py's
// fast_checksum, the integrity word of the persisted bit array.
uint64_t words_checksum(const uint32_t* w, uint64_t nwords) {
    constexpr uint64_t G = 0x9E3779B97F4A7C15ull, C = 0xC2B2AE3D27D4EB4Full;
    CopyPool& pool = CopyPool::get();
    const unsigned nt = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(pool.threads(), nwords >> 20));
    std::vector<uint64_t> part(nt, 0);
    auto body = [&](unsigned t) {
        const uint64_t a = nwords * t / nt, b = nwords * (t + 1) / nt;
        uint64_t x = 0;
        for (uint64_t i = a; i < b; ++i) x ^= (uint64_t)w[i] * G + (i + 1) * C;
        part[t] = x;
    };
    if (nt == 1) body(0);
    else pool.run(nt, body);
    uint64_t x = 0;
    for (uint64_t v : part) x ^= v;
    return x;
}

}  // namespace

struct vbf_filter {
    std::shared_ptr<Storage> bits;
    uint32_t k = 0;
    std::atomic<uint32_t> n{0};
    double p = 0.0;
    // Binding bookkeeping that lives in the handle, so a binding's BloomFilter needs no private
    // fields (velarixdb builds `BloomFilter { file_path, ..Default::default() }` outside
    // filter::bf: db/recovery.rs:143-146, tests/workload.rs:309-312).  Per handle, copied by clone
    // like the struct's other plain fields (bf.rs:242-254).
    std::atomic<uint64_t> sst_entries{VBF_EXT_NONE};  // the SST's entry count (build_filter_from_entries)
    std::atomic<int> restored{0};  // vbf_filter_recover_ext loaded persisted bits (not yet taken)
};

extern "C" {

const char* vbf_version(void) { return "velarixdb_amd-vbf 0.2.0 gfx950"; }

int vbf_profile_enable(int on) {
    g_prof.store(on != 0);
    return ok();
}

int vbf_profile_read(double* ms, uint64_t* launches, int nphases) {
    FORK_GUARD();
    if (!ms || !launches || nphases < 0) return fail(VBF_EINVAL, "NULL argument");
    for (int i = 0; i < nphases; ++i) {
        ms[i] = 0.0;
        launches[i] = 0;
    }
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto& r : g_prof_recs) {
        float t = 0.f;
        HIP_TRY(hipEventSynchronize(r.b));
        HIP_TRY(hipEventElapsedTime(&t, r.a, r.b));
        if (r.phase < nphases) {
            ms[r.phase] += t;
            launches[r.phase] += 1;
        }
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    g_prof_recs.clear();
    return ok();
}

const char* vbf_last_error(void) { return g_err.c_str(); }

int vbf_device_count(int* count) {
    if (!count) return fail(VBF_EINVAL, "count is NULL");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        *count = 0;
        return fail(VBF_ENODEV, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = c;
    return ok();
}

uint32_t vbf_num_bits(uint64_t n, double p) {
    const double ln2 = std::log(2.0);
    const double x = ((double)n * std::log(p)) / (ln2 * ln2);  // powi(2) == one multiply
    return f64_as_u32(-std::ceil(x));
}

uint32_t vbf_num_hash_functions(uint32_t m, uint32_t n) {
    const double x = ((double)m / (double)n) * std::ceil(std::log(2.0));  // ln2.ceil() == 1
    return f64_as_u32(x);
}

int vbf_size(double p, uint64_t n, uint32_t* m, uint32_t* k) {
    if (!m || !k) return fail(VBF_EINVAL, "NULL output");
    if (!(p >= 0.0)) return fail(VBF_EINVAL, "False positive rate can not be less than or equal to zero");
    if (n == 0) return fail(VBF_EINVAL, "No of elements should be greater than 0");
    *m = vbf_num_bits(n, p);
    *k = vbf_num_hash_functions(*m, (uint32_t)n);
    return ok();
}

void vbf_meta_serialize(uint32_t k, uint32_t n, double p, uint8_t out[16]) {
    uint64_t pb;
    std::memcpy(&pb, &p, 8);
    for (int i = 0; i < 4; ++i) out[i] = (uint8_t)(k >> (8 * i));
    for (int i = 0; i < 4; ++i) out[4 + i] = (uint8_t)(n >> (8 * i));
    for (int i = 0; i < 8; ++i) out[8 + i] = (uint8_t)(pb >> (8 * i));
}

int vbf_meta_parse(const uint8_t* in, size_t len, uint32_t* k, uint32_t* n, double* p) {
    if (!in || !k || !n || !p) return fail(VBF_EINVAL, "NULL argument");
    if (len < 16) return fail(VBF_EINVAL, "filter metadata truncated: %zu < 16 bytes (unexpected EOF)", len);
    uint32_t kk = 0, nn = 0;
    uint64_t pb = 0;
    for (int i = 3; i >= 0; --i) kk = (kk << 8) | in[i];
    for (int i = 3; i >= 0; --i) nn = (nn << 8) | in[4 + i];
    for (int i = 7; i >= 0; --i) pb = (pb << 8) | in[8 + i];
    *k = kk;
    *n = nn;
    std::memcpy(p, &pb, 8);
    return ok();
}

// ---- stateless device-pointer entry points ----

int vbf_build_dev(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                  int len_prefix, uint32_t m, uint32_t k, uint32_t* words, void* stream) {
    return vbf_build_dev_ex(keys, offsets, stride, n, len_prefix, m, k, words, VBF_BUILD_AUTO, stream);
}

uint64_t vbf_build_workspace_bytes(uint64_t n, uint32_t m, uint32_t k) {
    return vbf::partition_workspace_bytes(n, m, k);
}

int vbf_release_workspaces(void) {
    if (hip_forked()) {  // the parent's buffers: forget them, free nothing
        std::lock_guard<std::mutex> lk(g_ws_mu);
        g_ws.clear();
        return ok();
    }
    // every device's host calls are kept out while their workspaces are freed: a new caller waits
    // in staging_for, one in flight is waited for.  _dev calls on caller streams are the caller's
    // to keep away (vbf.h).
    std::lock_guard<std::mutex> sl(g_staging_mu);
    std::vector<std::unique_lock<std::mutex>> held;
    for (auto& st : g_staging)
        if (st) {
            held.emplace_back(st->host_mu);
            held.emplace_back(st->mu);
        }
    std::lock_guard<std::mutex> lk(g_ws_mu);
    for (auto& w : g_ws) {
        int prev = -1;
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(w.device);
        (void)hipStreamSynchronize(w.stream);
        (void)hipFree(w.ptr);
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    g_ws.clear();
    return ok();
}

int vbf_build_dev_ex(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                     int len_prefix, uint32_t m, uint32_t k, uint32_t* words, int strategy, void* stream) {
    FORK_GUARD();
    int rc = check_mk(m, k, n);
    if (rc) return rc;
    if ((rc = check_keys(keys, offsets, stride, n))) return rc;
    if (n && k && !words) return fail(VBF_EINVAL, "words is NULL");
    vbf::KeyBatch kb = batch(keys, offsets, 0, stride, n, len_prefix);
    if ((rc = do_build(kb, m, k, words, strategy, false, (hipStream_t)stream))) return rc;
    return ok();
}

int vbf_probe_dev_ex(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                     int len_prefix, uint32_t m, uint32_t k, const uint32_t* words, uint8_t* out,
                     int strategy, void* stream) {
    FORK_GUARD();
    int rc = check_mk(m, k, n);
    if (rc) return rc;
    if ((rc = check_keys(keys, offsets, stride, n))) return rc;
    if (n && !out) return fail(VBF_EINVAL, "out is NULL");
    vbf::KeyBatch kb = batch(keys, offsets, 0, stride, n, len_prefix);
    if ((rc = do_probe(kb, m, k, words, out, nullptr, strategy, (hipStream_t)stream))) return rc;
    return ok();
}

int vbf_probe_dev(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                  int len_prefix, uint32_t m, uint32_t k, const uint32_t* words, uint8_t* out,
                  void* stream) {
    return vbf_probe_dev_ex(keys, offsets, stride, n, len_prefix, m, k, words, out, VBF_BUILD_AUTO, stream);
}

int vbf_probe_count_dev_ex(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                           int len_prefix, uint32_t m, uint32_t k, const uint32_t* words,
                           unsigned long long* count_dev, int strategy, void* stream) {
    FORK_GUARD();
    int rc = check_mk(m, k, n);
    if (rc) return rc;
    if ((rc = check_keys(keys, offsets, stride, n))) return rc;
    if (!count_dev) return fail(VBF_EINVAL, "count_dev is NULL");
    vbf::KeyBatch kb = batch(keys, offsets, 0, stride, n, len_prefix);
    if ((rc = do_probe(kb, m, k, words, nullptr, count_dev, strategy, (hipStream_t)stream))) return rc;
    return ok();
}

int vbf_probe_count_dev(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                        int len_prefix, uint32_t m, uint32_t k, const uint32_t* words,
                        unsigned long long* count_dev, void* stream) {
    return vbf_probe_count_dev_ex(keys, offsets, stride, n, len_prefix, m, k, words, count_dev, VBF_BUILD_AUTO,
                                  stream);
}

int vbf_hashes_dev(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                   int len_prefix, uint32_t k, uint64_t* out, void* stream) {
    FORK_GUARD();
    int rc = check_keys(keys, offsets, stride, n);
    if (rc) return rc;
    if (n && k && !out) return fail(VBF_EINVAL, "out is NULL");
    vbf::KeyBatch kb = batch(keys, offsets, 0, stride, n, len_prefix);
    HIP_TRY(vbf::launch_hashes(kb, k, out, (hipStream_t)stream));
    return ok();
}

int vbf_or_words_dev(uint32_t* dst, const uint32_t* src, uint64_t nwords, void* stream) {
    FORK_GUARD();
    if (nwords && (!dst || !src)) return fail(VBF_EINVAL, "NULL words");
    HIP_TRY(vbf::launch_or_words(dst, src, nwords, (hipStream_t)stream));
    return ok();
}

extern "C++" {
namespace vbf {  // vbf_kernels.hip
hipError_t launch_or_fold(uint32_t* dst, const uint32_t* src, uint64_t nwords, uint32_t parts, uint64_t pstride,
                          hipStream_t s);
}
}

int vbf_or_fold_dev(uint32_t* dst, const uint32_t* src, uint64_t nwords, uint32_t nparts, uint64_t part_stride,
                    void* stream) {
    FORK_GUARD();
    if (nwords && nparts && (!dst || !src)) return fail(VBF_EINVAL, "NULL words");
    if (nparts > 1 && part_stride < nwords) return fail(VBF_EINVAL, "parts overlap (stride %llu < %llu words)",
                                                        (unsigned long long)part_stride, (unsigned long long)nwords);
    const hipError_t e = vbf::launch_or_fold(dst, src, nwords, nparts, part_stride, (hipStream_t)stream);
    if (e == hipErrorInvalidValue) return fail(VBF_EINVAL, "vbf_or_fold_dev needs 16-byte aligned words and a stride of whole 4-word units");
    HIP_TRY(e);
    return ok();
}

int vbf_popcount_dev(const uint32_t* words, uint64_t nwords, unsigned long long* count_dev, void* stream) {
    FORK_GUARD();
    if (!count_dev || (nwords && !words)) return fail(VBF_EINVAL, "NULL argument");
    HIP_TRY(vbf::launch_popcount(words, nwords, count_dev, (hipStream_t)stream));
    return ok();
}

int vbf_gen_fixed_dev(uint64_t seed, uint64_t base, uint64_t n, uint32_t len, uint8_t* out, void* stream) {
    FORK_GUARD();
    if (n && len && !out) return fail(VBF_EINVAL, "out is NULL");
    HIP_TRY(vbf::launch_gen_fixed(seed, base, n, len, out, (hipStream_t)stream));
    return ok();
}

int vbf_gen_var_dev(uint64_t seed, uint64_t base, uint64_t n, const uint64_t* offsets, uint8_t* out,
                    void* stream) {
    FORK_GUARD();
    if (n && (!offsets || !out)) return fail(VBF_EINVAL, "NULL argument");
    HIP_TRY(vbf::launch_gen_var(seed, base, n, offsets, out, (hipStream_t)stream));
    return ok();
}

int vbf_gen_sst_fixed_dev(uint64_t seed, uint64_t base, uint64_t n, uint32_t len, uint8_t* data,
                          uint32_t* blocks, void* stream) {
    FORK_GUARD();
    if (n && (!data || !blocks)) return fail(VBF_EINVAL, "NULL argument");
    if (len + 17 > 4096) return fail(VBF_EINVAL, "an entry of %u + 17 bytes exceeds a 4096-byte block", len);
    HIP_TRY(vbf::gen_sst_fixed(seed, base, n, len, data, blocks, (hipStream_t)stream));
    return ok();
}

// ---- one-shot host-pointer entry points ----

int vbf_build_host(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                   int len_prefix, uint32_t m, uint32_t k, uint32_t* words, uint64_t nwords,
                   int device) {
    int rc = check_mk(m, k, n);
    if (rc) return rc;
    if ((rc = check_keys(keys, offsets, stride, n))) return rc;
    const uint64_t need = ((uint64_t)m + 31) / 32;
    if (nwords < need || (need && !words)) return fail(VBF_EINVAL, "words holds %llu < ceil(m/32) = %llu",
                                                       (unsigned long long)nwords, (unsigned long long)need);
    if (n == 0 || k == 0) return ok();
    DEVICE_SCOPE(device);
    Staging* st = staging_for(device);
    std::lock_guard<std::mutex> lk(st->mu);
    if ((rc = st->init(device))) return rc;
    if ((rc = Staging::grow<uint32_t>(nullptr, &st->d_words, &st->words_cap, need))) return rc;
    if ((rc = xfer_h2d(*st, st->d_words, words, need * 4))) return rc;
    rc = pipeline_host_keys(
        *st, keys, offsets, stride, n, len_prefix, false,
        [&](const vbf::KeyBatch& kb, uint64_t, int, hipStream_t s) -> int {
            return do_build(kb, m, k, st->d_words, VBF_BUILD_AUTO, true, s);
        },
        [](int, uint64_t, uint64_t) { return VBF_OK; });
    if (rc) return rc;
    if ((rc = xfer_d2h(*st, words, st->d_words, need * 4))) return rc;
    return ok();
}

int vbf_build_shards_host(vbf_shard* shards, uint64_t nshards, const int* devices, int ndevices) {
    if (nshards && !shards) return fail(VBF_EINVAL, "shards is NULL");
    if (nshards && (!devices || ndevices <= 0)) return fail(VBF_EINVAL, "no devices given");
    std::vector<std::string> msg(nshards);
    auto work = [&](int d) {
        for (uint64_t s = (uint64_t)d; s < nshards; s += (uint64_t)ndevices) {
            vbf_shard& sh = shards[s];
            sh.status = vbf_build_host(sh.keys, sh.offsets, sh.stride, sh.n, sh.len_prefix, sh.m, sh.k, sh.words,
                                       sh.nwords, devices[d]);
            if (sh.status) msg[s] = g_err;
        }
    };
    const int nt = (int)std::min<uint64_t>((uint64_t)ndevices, nshards);
    std::vector<std::thread> th;
    th.reserve(nt > 0 ? nt - 1 : 0);
    for (int d = 1; d < nt; ++d) th.emplace_back(work, d);
    if (nt > 0) work(0);
    for (auto& t : th) t.join();
    for (uint64_t s = 0; s < nshards; ++s)
        if (shards[s].status) return fail(shards[s].status, "shard %llu: %s", (unsigned long long)s, msg[s].c_str());
    return ok();
}

int vbf_probe_host(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                   int len_prefix, uint32_t m, uint32_t k, const uint32_t* words, uint64_t nwords,
                   uint8_t* out, int device) {
    int rc = check_mk(m, k, n);
    if (rc) return rc;
    if ((rc = check_keys(keys, offsets, stride, n))) return rc;
    const uint64_t need = ((uint64_t)m + 31) / 32;
    if (nwords < need || (need && !words)) return fail(VBF_EINVAL, "words too short");
    if (n && !out) return fail(VBF_EINVAL, "out is NULL");
    if (n == 0) return ok();
    DEVICE_SCOPE(device);
    Staging* st = staging_for(device);
    std::lock_guard<std::mutex> lk(st->mu);
    if ((rc = st->init(device))) return rc;
    if ((rc = Staging::grow<uint32_t>(nullptr, &st->d_words, &st->words_cap, need ? need : 1))) return rc;
    if (need) HIP_TRY(hipMemcpyAsync(st->d_words, words, need * 4, hipMemcpyHostToDevice, st->stream[0]));
    HIP_TRY(hipEventRecord(st->done[0], st->stream[0]));
    HIP_TRY(hipStreamWaitEvent(st->stream[1], st->done[0], 0));
    rc = pipeline_host_keys(
        *st, keys, offsets, stride, n, len_prefix, true,
        [&](const vbf::KeyBatch& kb, uint64_t, int b, hipStream_t s) -> int {
            if (int rc2 = do_probe(kb, m, k, st->d_words, st->d_out[b], nullptr, VBF_BUILD_AUTO, s)) return rc2;
            HIP_TRY(hipMemcpyAsync(st->h_out[b], st->d_out[b], kb.n, hipMemcpyDeviceToHost, s));
            return VBF_OK;
        },
        [&](int b, uint64_t lo, uint64_t cnt) {
            par_memcpy(out + lo, st->h_out[b], cnt);
            return VBF_OK;
        });
    if (rc) return rc;
    return ok();
}

// ---- filter handle ----
//
// Every entry point takes the filter's lock (Storage::mu, the reference's Mutex<BitVec>) BEFORE
// it looks at where the bits live: vbf_filter_migrate changes device / d_words / h_words under
// that lock and clones share the Storage, so a residency read outside it could send a call down
// the wrong path.  Then it drains the filter's queued asynchronous sets (storage_drain).

static int make_filter(int device, uint32_t m, uint32_t k, double p, vbf_filter** out) {
    if (!out) return fail(VBF_EINVAL, "out is NULL");
    std::unique_ptr<vbf_filter> f(new vbf_filter());
    if (device == VBF_DEVICE_HOST) {
        int rc = new_storage(device, m, &f->bits);
        if (rc) return rc;
    } else {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
            return fail(VBF_ENODEV, "no HIP device available");
        // placement policy: filters created with VBF_DEVICE_AUTO go round-robin over the devices,
        // so one serial caller's successive filters (one per merged table) land on different GPUs
        if (device == VBF_DEVICE_AUTO) device = (int)(g_auto_rr.fetch_add(1) % (uint64_t)count);
        if (device < 0 || device >= count)
            return fail(VBF_ENODEV, "device %d out of range (%d devices)", device, count);
        DEVICE_SCOPE(device);
        int rc = new_storage(device, m, &f->bits);
        if (rc) return rc;
    }
    f->k = k;
    f->p = p;
    *out = f.release();
    return ok();
}

static int host_resident(const char* what) {
    return fail(VBF_EINVAL, "%s: the filter is host-resident (VBF_DEVICE_HOST); use the _host entry points", what);
}

int vbf_filter_new(double p, uint64_t no_of_elements, int device, vbf_filter** out) {
    uint32_t m, k;
    int rc = vbf_size(p, no_of_elements, &m, &k);
    if (rc) return rc;
    return make_filter(device, m, k, p, out);
}

int vbf_filter_default(int device, vbf_filter** out) { return make_filter(device, 0, 0, 0.0, out); }

int vbf_filter_new_sized(uint32_t m, uint32_t k, double p, int device, vbf_filter** out) {
    return make_filter(device, m, k, p, out);
}

int vbf_filter_recover(const uint8_t* meta, size_t len, int device, vbf_filter** out) {
    uint32_t k, n;
    double p;
    int rc = vbf_meta_parse(meta, len, &k, &n, &p);
    if (rc) return rc;
    // bf.rs:144-147: m is recomputed from the STORED element count (usize) and p.
    rc = make_filter(device, vbf_num_bits((uint64_t)n, p), k, p, out);
    if (rc) return rc;
    (*out)->n.store(n);
    return ok();
}

int vbf_filter_clone(const vbf_filter* f, vbf_filter** out) {
    if (!f || !out) return fail(VBF_EINVAL, "NULL argument");
    vbf_filter* c = new vbf_filter();
    c->bits = f->bits;
    c->k = f->k;
    c->n.store(f->n.load());  // bf.rs:248: the clone's counter is a copy, the bits are shared
    c->p = f->p;
    c->sst_entries.store(f->sst_entries.load());
    c->restored.store(f->restored.load());
    *out = c;
    return ok();
}

void vbf_filter_free(vbf_filter* f) { delete f; }

uint32_t vbf_filter_num_bits(const vbf_filter* f) { return f ? f->bits->m : 0; }
uint32_t vbf_filter_num_elements(const vbf_filter* f) { return f ? f->n.load() : 0; }
uint32_t vbf_filter_num_hash_functions(const vbf_filter* f) { return f ? f->k : 0; }
double vbf_filter_false_positive_rate(const vbf_filter* f) { return f ? f->p : 0.0; }
int vbf_filter_device(const vbf_filter* f) {
    if (!f) return VBF_DEVICE_HOST - 1;
    std::lock_guard<std::mutex> lk(f->bits->mu);
    return f->bits->device;
}
uint64_t vbf_filter_host_bytes(const vbf_filter* f) {
    if (!f) return 0;
    Storage& s = *f->bits;
    std::lock_guard<std::mutex> lk(s.mu);
    return (uint64_t)s.h_words.size() * 4 + (s.mirror ? s.nwords * 4 : 0);
}

uint32_t* vbf_filter_words_dev(const vbf_filter* f) {
    if (!f) return nullptr;
    Storage& s = *f->bits;
    std::lock_guard<std::mutex> lk(s.mu);
    // the caller's kernels are not ordered after the filter's last event (e.g. the asynchronous
    // zeroing of a new filter's words): wait for it here
    if (!hip_forked() && storage_sync(s) != VBF_OK) return nullptr;
    if (s.d_words) {
        // the caller may write through the pointer: the bits are no longer known to be zero, and
        // the host mirror is bypassed until the write is declared (vbf_filter_stream_record)
        s.pristine = false;
        s.mirror_ok = false;
        s.ext_write = true;
    }
    return s.d_words;
}

const uint32_t* vbf_filter_words_dev_read(const vbf_filter* f) {
    if (!f) return nullptr;
    Storage& s = *f->bits;
    std::lock_guard<std::mutex> lk(s.mu);
    if (!hip_forked() && storage_sync(s) != VBF_OK) return nullptr;  // as vbf_filter_words_dev
    return s.d_words;  // read-only use: the mirror and `pristine` stay trusted
}

int vbf_filter_set_num_elements(vbf_filter* f, uint32_t n) {
    if (!f) return fail(VBF_EINVAL, "filter is NULL");
    f->n.store(n);
    return ok();
}

int vbf_filter_set_sst_entries(vbf_filter* f, uint64_t entries) {
    if (!f) return fail(VBF_EINVAL, "filter is NULL");
    f->sst_entries.store(entries);
    return ok();
}
uint64_t vbf_filter_sst_entries(const vbf_filter* f) { return f ? f->sst_entries.load() : VBF_EXT_NONE; }
int vbf_filter_take_restored(vbf_filter* f) {
    if (!f) return fail(VBF_EINVAL, "filter is NULL");
    return f->restored.exchange(0);
}

int vbf_filter_serialize(const vbf_filter* f, uint8_t out[16]) {
    if (!f || !out) return fail(VBF_EINVAL, "NULL argument");
    vbf_meta_serialize(f->k, f->n.load(), f->p, out);
    return ok();
}

int vbf_filter_set_dev(vbf_filter* f, const uint8_t* keys, const uint64_t* offsets, uint64_t stride,
                       uint64_t n, int len_prefix, void* stream) {
    if (!f) return fail(VBF_EINVAL, "filter is NULL");
    Storage& s = *f->bits;
    std::unique_lock<std::mutex> lk(s.mu);
    int rc = storage_drain(s, lk);
    if (rc) return rc;
    if (s.host()) return host_resident("vbf_filter_set_dev");
    if ((rc = check_mk(s.m, f->k, n))) return rc;
    if ((rc = check_keys(keys, offsets, stride, n))) return rc;
    if (n && f->k) {
        DEVICE_SCOPE(s.device);
        const hipStream_t hs = (hipStream_t)stream;
        if ((rc = storage_wait(s, hs))) return rc;
        vbf::KeyBatch kb = batch(keys, offsets, 0, stride, n, len_prefix);
        s.mirror_ok = false;
        s.pristine = false;
        if ((rc = do_build(kb, s.m, f->k, s.d_words, VBF_BUILD_AUTO, true, hs))) return rc;
        if ((rc = storage_mark(s, hs))) return rc;
        if ((rc = mirror_after_write(s, hs))) return rc;
    }
    f->n.fetch_add((uint32_t)n);
    return ok();
}

int vbf_filter_set_host(vbf_filter* f, const uint8_t* keys, const uint64_t* offsets, uint64_t stride,
                        uint64_t n, int len_prefix) {
    if (!f) return fail(VBF_EINVAL, "filter is NULL");
    Storage& s = *f->bits;
    int rc = check_mk(s.m, f->k, n);
    if (rc) return rc;
    if ((rc = check_keys(keys, offsets, stride, n))) return rc;
    std::unique_lock<std::mutex> lk(s.mu);
    if ((rc = storage_drain(s, lk))) return rc;
    if (n && f->k) {
        if (s.host()) {
            s.pristine = false;
            host_set(host_words(s), s.m, f->k, keys, offsets, stride, n, len_prefix != 0);
        } else {
            DEVICE_SCOPE(s.device);
            if ((rc = device_set_host(s, f->k, keys, offsets, stride, n, len_prefix))) return rc;
        }
    }
    f->n.fetch_add((uint32_t)n);
    return ok();
}

int vbf_filter_set_host_async(vbf_filter* f, const uint8_t* keys, const uint64_t* offsets, uint64_t stride,
                              uint64_t n, int len_prefix, void (*release)(void*), void* release_ctx) {
    if (!f) return fail(VBF_EINVAL, "filter is NULL");
    Storage& s = *f->bits;
    int rc = check_mk(s.m, f->k, n);
    if (rc) return rc;
    if ((rc = check_keys(keys, offsets, stride, n))) return rc;
    std::unique_ptr<AsyncJob> j(new AsyncJob());
    j->s = f->bits;
    j->k = f->k;
    j->stride = stride;
    j->n = n;
    j->lp = len_prefix;
    j->release = release;
    j->ctx = release_ctx;
    if (n && f->k && !release) {
        // no release callback: the caller may reuse its buffers on return, so the job runs from
        // the library's own copy
        const uint64_t base = offsets ? offsets[0] : 0;
        const uint64_t bytes = offsets ? offsets[n] - base : n * stride;
        j->own_keys.reset(new (std::nothrow) uint8_t[bytes ? bytes : 1]);
        if (!j->own_keys) return fail(VBF_ENOMEM, "copying %llu key bytes", (unsigned long long)bytes);
        if (bytes) par_memcpy(j->own_keys.get(), keys + base, bytes);
        if (offsets) {
            j->own_offs.reset(new (std::nothrow) uint64_t[n + 1]);
            if (!j->own_offs) return fail(VBF_ENOMEM, "copying %llu offsets", (unsigned long long)(n + 1));
            for (uint64_t i = 0; i <= n; ++i) j->own_offs[i] = offsets[i] - base;
        }
        j->keys = j->own_keys.get();
        j->offsets = j->own_offs.get();
    } else {
        j->keys = keys;
        j->offsets = offsets;
    }
    std::unique_lock<std::mutex> lk(s.mu);
    if (s.host() || !n || !f->k) {  // nothing to overlap with: the CPU set runs now
        if ((rc = storage_drain(s, lk))) return rc;
        if (n && f->k) {
            s.pristine = false;
            host_set(host_words(s), s.m, f->k, j->keys, j->offsets, stride, n, len_prefix != 0);
        }
        lk.unlock();
        if (release) release(release_ctx);
    } else {
        // a forked child: a device-resident filter's set never runs here (HIP is the parent's), so
        // fail before anything is queued or counted -- no job, no worker thread, no n += N
        if (hip_forked()) return fail_forked();
        if (s.jobs_pid != getpid() && s.jobs_done != s.jobs_queued) {
            // forked while the parent had sets queued on this filter: they never run here.  Report
            // that now (as every other call does) instead of overwriting jobs_pid, which would make
            // the parent's jobs look like this process's and every later drain wait forever
            // (ADVICE r04).  The caller keeps its buffers: release is not called on an error.
            (void)storage_jobs_settled(s);
            if ((rc = storage_drain(s, lk))) return rc;
        }
        ++s.jobs_queued;
        s.jobs_pid = getpid();
        s.pristine = false;
        // s.device cannot change while the job is queued: migrate drains first
        AsyncQueue::get(s.device).push(j.release());
    }
    f->n.fetch_add((uint32_t)n);
    return ok();
}

int vbf_filter_sync(vbf_filter* f) {
    if (!f) return fail(VBF_EINVAL, "filter is NULL");
    Storage& s = *f->bits;
    std::unique_lock<std::mutex> lk(s.mu);
    int rc = storage_drain(s, lk);
    if (rc) return rc;
    if (!s.host()) {
        DEVICE_SCOPE(s.device);
        if ((rc = storage_sync(s))) return rc;
    }
    return ok();
}

int vbf_filter_busy(const vbf_filter* f) {
    if (!f) return fail(VBF_EINVAL, "filter is NULL");
    Storage& s = *f->bits;
    std::lock_guard<std::mutex> lk(s.mu);
    if (!storage_jobs_settled(s)) return 1;
    if (s.host() || !s.pending) return 0;
    DEVICE_SCOPE(s.device);
    const hipError_t e = hipEventQuery(s.last);
    if (e == hipErrorNotReady) return 1;
    if (e != hipSuccess) return fail(VBF_EHIP, "hipEventQuery: %s", hipGetErrorString(e));
    return 0;
}

int vbf_filter_stream_wait(const vbf_filter* f, void* stream) {
    if (!f) return fail(VBF_EINVAL, "filter is NULL");
    Storage& s = *f->bits;
    std::unique_lock<std::mutex> lk(s.mu);
    int rc = storage_drain(s, lk);
    if (rc) return rc;
    if (s.host()) return host_resident("vbf_filter_stream_wait");
    DEVICE_SCOPE(s.device);
    if ((rc = storage_wait(s, (hipStream_t)stream))) return rc;
    return ok();
}

int vbf_filter_stream_record(vbf_filter* f, void* stream) {
    if (!f) return fail(VBF_EINVAL, "filter is NULL");
    Storage& s = *f->bits;
    std::unique_lock<std::mutex> lk(s.mu);
    int rc = storage_drain(s, lk);
    if (rc) return rc;
    if (s.host()) return host_resident("vbf_filter_stream_record");
    DEVICE_SCOPE(s.device);
    s.pristine = false;
    s.ext_write = false;  // the write is declared: the mirror is refreshed behind it from here on
    if ((rc = storage_mark(s, (hipStream_t)stream))) return rc;
    if ((rc = mirror_after_write(s, (hipStream_t)stream))) return rc;
    return ok();
}

int vbf_filter_set_mirror(vbf_filter* f, int mode) {
    if (!f) return fail(VBF_EINVAL, "filter is NULL");
    if (mode < VBF_MIRROR_OFF || mode > VBF_MIRROR_EAGER) return fail(VBF_EINVAL, "unknown mirror mode %d", mode);
    Storage& s = *f->bits;
    std::unique_lock<std::mutex> lk(s.mu);
    int rc = storage_drain(s, lk);
    if (rc) return rc;
    if (!s.host()) {
        DEVICE_SCOPE(s.device);
        if ((rc = storage_sync(s))) return rc;  // a queued eager refresh must land before a free
    }
    s.mirror_mode = mode;
    if (mode == VBF_MIRROR_OFF) s.free_mirror();
    return ok();
}

int vbf_filter_contains_dev(const vbf_filter* f, const uint8_t* keys, const uint64_t* offsets,
                            uint64_t stride, uint64_t n, int len_prefix, uint8_t* out, void* stream) {
    if (!f) return fail(VBF_EINVAL, "filter is NULL");
    Storage& s = *f->bits;
    std::unique_lock<std::mutex> lk(s.mu);
    int rc = storage_drain(s, lk);
    if (rc) return rc;
    if (s.host()) return host_resident("vbf_filter_contains_dev");
    if ((rc = check_mk(s.m, f->k, n))) return rc;
    if ((rc = check_keys(keys, offsets, stride, n))) return rc;
    if (n && !out) return fail(VBF_EINVAL, "out is NULL");
    if (n == 0) return ok();
    DEVICE_SCOPE(s.device);
    const hipStream_t hs = (hipStream_t)stream;
    if ((rc = storage_wait(s, hs))) return rc;
    vbf::KeyBatch kb = batch(keys, offsets, 0, stride, n, len_prefix);
    if ((rc = do_probe(kb, s.m, f->k, s.d_words, out, nullptr, VBF_BUILD_AUTO, hs))) return rc;
    if ((rc = storage_mark(s, hs))) return rc;  // a later clear / load must not overtake the reads
    return ok();
}

int vbf_filter_contains_host(const vbf_filter* f, const uint8_t* keys, const uint64_t* offsets,
                             uint64_t stride, uint64_t n, int len_prefix, uint8_t* out) {
    if (!f) return fail(VBF_EINVAL, "filter is NULL");
    Storage& s = *f->bits;
    int rc = check_mk(s.m, f->k, n);
    if (rc) return rc;
    if ((rc = check_keys(keys, offsets, stride, n))) return rc;
    if (n && !out) return fail(VBF_EINVAL, "out is NULL");
    if (n == 0) return ok();
    std::unique_lock<std::mutex> lk(s.mu);
    if ((rc = storage_drain(s, lk))) return rc;
    if (s.host()) {
        host_contains(host_words(s), s.m, f->k, keys, offsets, stride, n, len_prefix != 0, out);
        return ok();
    }
    DEVICE_SCOPE(s.device);
    if (mirror_mode(s) != VBF_MIRROR_OFF && n <= mirror_max_keys()) {
        // the read path's single-key probes (range.rs:130,136,171) answer from the host mirror
        if ((rc = mirror_fill(s))) return rc;
        host_contains(s.mirror, s.m, f->k, keys, offsets, stride, n, len_prefix != 0, out);
        return ok();
    }
    Staging* st = staging_for(s.device);
    std::lock_guard<std::mutex> lk2(st->mu);
    if ((rc = st->init(s.device))) return rc;
    if ((rc = storage_sync(s))) return rc;
    rc = pipeline_host_keys(
        *st, keys, offsets, stride, n, len_prefix, true,
        [&](const vbf::KeyBatch& kb, uint64_t, int b, hipStream_t hs) -> int {
            if (int rc2 = do_probe(kb, s.m, f->k, s.d_words, st->d_out[b], nullptr, VBF_BUILD_AUTO, hs)) return rc2;
            HIP_TRY(hipMemcpyAsync(st->h_out[b], st->d_out[b], kb.n, hipMemcpyDeviceToHost, hs));
            return VBF_OK;
        },
        [&](int b, uint64_t lo, uint64_t cnt) {
            par_memcpy(out + lo, st->h_out[b], cnt);
            return VBF_OK;
        });
    if (rc) return rc;
    return ok();
}

int vbf_filter_clear(vbf_filter* f, vbf_filter** out) {
    if (!f || !out) return fail(VBF_EINVAL, "NULL argument");
    Storage& s = *f->bits;
    int device;
    {
        std::unique_lock<std::mutex> lk(s.mu);
        int rc = storage_drain(s, lk);
        if (rc) return rc;
        if (s.host()) {
            std::fill(s.h_words.begin(), s.h_words.end(), 0u);
        } else {
            DEVICE_SCOPE(s.device);
            hipStream_t fs;
            if ((rc = filter_stream(s.device, &fs))) return rc;
            if ((rc = storage_wait(s, fs))) return rc;  // a pending set_dev must not undo the clear
            if (s.nwords) HIP_TRY(hipMemsetAsync(s.d_words, 0, s.nwords * 4, fs));
            HIP_TRY(hipStreamSynchronize(fs));
            s.pending = false;
            if (s.mirror) {  // the mirror stays exact: all zero too
                std::memset(s.mirror, 0, s.nwords * 4);
                s.mirror_ok = true;
            }
        }
        s.pristine = true;
        device = s.device;
    }
    return make_filter(device, s.m, f->k, f->p, out);
}

// Caller holds s.mu (drained).
static int words_to_host_locked(Storage& s, uint32_t* out) {
    if (!s.nwords) return VBF_OK;
    if (s.host()) {
        if (s.h_words.empty()) std::memset(out, 0, s.nwords * 4);  // never written: all zero
        else std::memcpy(out, s.h_words.data(), s.nwords * 4);
        return VBF_OK;
    }
    DEVICE_SCOPE(s.device);
    int rc = storage_sync(s);  // this filter's pending work only: other filters keep running
    if (rc) return rc;
    if (s.mirror_current()) {  // current host copy: no PCIe transfer
        par_memcpy(out, s.mirror, s.nwords * 4);
        return VBF_OK;
    }
    Staging* st = staging_for(s.device);
    std::lock_guard<std::mutex> lk2(st->mu);
    rc = st->init(s.device);
    if (!rc) rc = xfer_d2h(*st, out, s.d_words, s.nwords * 4);
    return rc;
}

int vbf_filter_words_to_host(const vbf_filter* f, uint32_t* out, uint64_t nwords) {
    if (!f) return fail(VBF_EINVAL, "filter is NULL");
    Storage& s = *f->bits;
    if (nwords < s.nwords || (s.nwords && !out)) return fail(VBF_EINVAL, "out holds %llu < %llu words",
                                                            (unsigned long long)nwords, (unsigned long long)s.nwords);
    std::unique_lock<std::mutex> lk(s.mu);
    int rc = storage_drain(s, lk);
    if (!rc) rc = words_to_host_locked(s, out);
    return rc ? rc : ok();
}

// Caller holds s.mu (drained).
static int words_from_host_locked(Storage& s, const uint32_t* in) {
    if (!s.nwords) return VBF_OK;
    s.pristine = false;
    if (s.host()) {
        std::memcpy(host_words(s), in, s.nwords * 4);
        return VBF_OK;
    }
    DEVICE_SCOPE(s.device);
    int rc = storage_sync(s);
    if (rc) return rc;
    s.mirror_ok = false;
    Staging* st = staging_for(s.device);
    std::lock_guard<std::mutex> lk2(st->mu);
    rc = st->init(s.device);
    if (!rc) rc = xfer_h2d(*st, s.d_words, in, s.nwords * 4);
    if (!rc && mirror_mode(s) == VBF_MIRROR_EAGER) {
        if (!s.mirror) HIP_TRY(hipHostMalloc((void**)&s.mirror, s.nwords * 4, hipHostMallocDefault));
        par_memcpy(s.mirror, in, s.nwords * 4);
        s.mirror_ok = true;
    }
    return rc;
}

int vbf_filter_words_from_host(vbf_filter* f, const uint32_t* in, uint64_t nwords) {
    if (!f) return fail(VBF_EINVAL, "filter is NULL");
    Storage& s = *f->bits;
    if (nwords != s.nwords || (s.nwords && !in)) return fail(VBF_EINVAL, "expected %llu words, got %llu",
                                                            (unsigned long long)s.nwords, (unsigned long long)nwords);
    std::unique_lock<std::mutex> lk(s.mu);
    int rc = storage_drain(s, lk);
    if (!rc) rc = words_from_host_locked(s, in);
    return rc ? rc : ok();
}

int vbf_filter_migrate(vbf_filter* f, int device) {
    if (!f) return fail(VBF_EINVAL, "filter is NULL");
    Storage& s = *f->bits;
    if (device != VBF_DEVICE_HOST) {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return fail(VBF_ENODEV, "no HIP device available");
        if (device == VBF_DEVICE_AUTO) device = (int)(g_auto_rr.fetch_add(1) % (uint64_t)count);
        if (device < 0 || device >= count) return fail(VBF_ENODEV, "device %d out of range (%d devices)", device, count);
    }
    std::unique_lock<std::mutex> lk(s.mu);
    int rc = storage_drain(s, lk);
    if (rc) return rc;
    if (device == s.device) return ok();
    std::vector<uint32_t> w;
    const bool zeros = s.pristine;  // nothing to copy: the target gets zeroed words
    if (s.host()) {
        w.swap(s.h_words);
        if (!zeros && w.size() != s.nwords) w.assign(s.nwords, 0u);  // written words are allocated
    } else {
        DEVICE_SCOPE(s.device);
        if ((rc = storage_sync(s))) return rc;
        if (!zeros) w.resize(s.nwords);  // to the host, a pristine filter stays unallocated
        if (s.nwords && !zeros) HIP_TRY(hipMemcpy(w.data(), s.d_words, s.nwords * 4, hipMemcpyDeviceToHost));
    }
    uint32_t* nd = nullptr;
    if (device != VBF_DEVICE_HOST && s.nwords) {
        DEVICE_SCOPE(device);
        hipError_t e = hipMalloc((void**)&nd, s.nwords * 4);
        // a pristine filter's words are zeroed asynchronously below (no copy, no host wait)
        if (e == hipSuccess && !zeros) e = hipMemcpy(nd, w.data(), s.nwords * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) {  // the filter stays where it was, bits intact
            (void)hipGetLastError();
            if (nd) (void)hipFree(nd);
            if (s.host()) s.h_words.swap(w);
            return fail(e == hipErrorOutOfMemory ? VBF_ENOMEM : VBF_EHIP, "moving the bits to device %d: %s",
                        device, hipGetErrorString(e));
        }
    }
    if (!s.host()) {  // release the old device copy (its work is finished: storage_sync above)
        DEVICE_SCOPE(s.device);
        if (s.d_words) (void)hipFree(s.d_words);
        if (s.last) (void)hipEventDestroy(s.last);
        s.last = nullptr;
        s.pending = false;
    }
    // a mirror of the old device copy still holds the bits; moving to the host makes it moot
    if (device == VBF_DEVICE_HOST) s.free_mirror();
    s.d_words = nd;
    if (device == VBF_DEVICE_HOST) s.h_words.swap(w);
    s.device = device;
    if (nd && zeros) {  // on the filter's stream; every later use waits for the filter's last event
        DEVICE_SCOPE(device);
        hipStream_t fs;
        if ((rc = filter_stream(device, &fs))) return rc;
        HIP_TRY(hipMemsetAsync(nd, 0, s.nwords * 4, fs));
        if ((rc = storage_mark(s, fs))) return rc;
    }
    return ok();
}

// ---- persisted bit array ----

static constexpr uint32_t kExtMagic = 0x57464256u;  // "VBFW"
static constexpr uint32_t kExtVersion = 2;
static constexpr uint64_t kExtBytes = 32;  // u32 magic | u32 version | u32 m | u32 nwords | u64 entries | u64 checksum

static inline void put_u32(uint8_t* p, uint32_t v) { std::memcpy(p, &v, 4); }
static inline void put_u64(uint8_t* p, uint64_t v) { std::memcpy(p, &v, 8); }
static inline uint32_t get_u32(const uint8_t* p) {
    uint32_t v;
    std::memcpy(&v, p, 4);
    return v;
}
static inline uint64_t get_u64(const uint8_t* p) {
    uint64_t v;
    std::memcpy(&v, p, 8);
    return v;
}

int vbf_filter_serialize_ext(const vbf_filter* f, const uint8_t* keys, const uint64_t* offsets, uint64_t stride,
                             uint64_t entries, int len_prefix, uint8_t* buf, uint64_t cap, uint64_t* len) {
    if (!f || !len) return fail(VBF_EINVAL, "NULL argument");
    Storage& s = *f->bits;
    const uint32_t k = f->k, n = f->n.load();
    const double p = f->p;
    // recover_meta (bf.rs:144-147) recreates m from the stored n; persisted bits are useful only
    // in that shape
    const uint32_t m_rec = vbf_num_bits((uint64_t)n, p);
    const uint64_t nw = ((uint64_t)m_rec + 31) / 32;
    enum { kHeaderOnly, kOwnWords, kFromKeys } mode = kHeaderOnly;
    if (entries != VBF_EXT_NONE && !(m_rec == 0 && k > 0 && entries > 0)) {
        if (s.m == m_rec) mode = kOwnWords;
        else if (keys || offsets || entries == 0) mode = kFromKeys;
    }
    if (mode == kFromKeys) {
        int rc = check_keys(keys, offsets, stride, entries);
        if (rc) return rc;
    }
    const uint64_t need = 16 + (mode == kHeaderOnly ? 0 : kExtBytes + nw * 4);
    *len = need;
    if (!buf) return ok();  // size query
    if (cap < need) return fail(VBF_EINVAL, "buffer holds %llu < %llu bytes", (unsigned long long)cap,
                                (unsigned long long)need);
    vbf_meta_serialize(k, n, p, buf);
    if (mode == kHeaderOnly) return ok();
    uint8_t* body = buf + 16 + kExtBytes;
    const bool aligned = ((uintptr_t)body & 3) == 0;
    std::vector<uint32_t> tmp;
    uint32_t* w = reinterpret_cast<uint32_t*>(body);
    if (!aligned) {
        tmp.resize(nw);
        w = tmp.data();
    }
    int rc = VBF_OK;
    if (mode == kOwnWords) {
        std::unique_lock<std::mutex> lk(s.mu);
        rc = storage_drain(s, lk);
        if (!rc) rc = words_to_host_locked(s, w);
    } else {
        std::memset(w, 0, nw * 4);
        if (entries && k) {
            int device;
            {
                std::lock_guard<std::mutex> lk(s.mu);
                device = s.device;
            }
            if (device == VBF_DEVICE_HOST) host_set(w, m_rec, k, keys, offsets, stride, entries, len_prefix != 0);
            else rc = vbf_build_host(keys, offsets, stride, entries, len_prefix, m_rec, k, w, nw, device);
        }
    }
    if (rc) return rc;
    if (!aligned) std::memcpy(body, tmp.data(), nw * 4);
    uint8_t* e = buf + 16;
    put_u32(e, kExtMagic);
    put_u32(e + 4, kExtVersion);
    put_u32(e + 8, m_rec);
    put_u32(e + 12, (uint32_t)nw);
    put_u64(e + 16, entries);
    put_u64(e + 24, words_checksum(w, nw));
    return ok();
}

int vbf_filter_recover_ext(const uint8_t* bytes, uint64_t len, int device, vbf_filter** out, int* restored) {
    if (!bytes || !out) return fail(VBF_EINVAL, "NULL argument");
    if (restored) *restored = 0;
    vbf_filter* f = nullptr;
    int rc = vbf_filter_recover(bytes, (size_t)len, device, &f);
    if (rc) return rc;
    const uint32_t m = f->bits->m;
    const uint64_t nw = ((uint64_t)m + 31) / 32;
    if (len >= 16 + kExtBytes) {
        const uint8_t* e = bytes + 16;
        const uint8_t* body = e + kExtBytes;
        if (get_u32(e) == kExtMagic && get_u32(e + 4) == kExtVersion && get_u32(e + 8) == m &&
            get_u32(e + 12) == nw && len - 16 - kExtBytes == nw * 4) {
            std::vector<uint32_t> tmp;
            const uint32_t* w = reinterpret_cast<const uint32_t*>(body);
            if ((uintptr_t)body & 3) {
                tmp.resize(nw);
                std::memcpy(tmp.data(), body, nw * 4);
                w = tmp.data();
            }
            if (words_checksum(w, nw) == get_u64(e + 24)) {
                if ((rc = vbf_filter_words_from_host(f, w, nw))) {
                    vbf_filter_free(f);
                    return rc;
                }
                // recover_meta + build_filter_from_entries (range.rs:121-124): stored n + entries
                f->n.store((uint32_t)(f->n.load() + get_u64(e + 16)));
                f->restored.store(1);
                if (restored) *restored = 1;
            }
        }
    }
    *out = f;
    return ok();
}

// ---- SST data.db decode ----

int vbf_sst_index_blocks(const uint8_t* index, uint64_t len, uint32_t* offsets, uint64_t cap, uint64_t* nblocks) {
    if (!nblocks || (len && !index)) return fail(VBF_EINVAL, "NULL argument");
    std::vector<uint32_t> v;
    int rc = parse_index(index, len, &v);
    if (rc) return rc;
    *nblocks = v.size();
    if (offsets && cap) memcpy(offsets, v.data(), 4 * std::min<uint64_t>(cap, v.size()));
    return ok();
}

int vbf_sst_decode_dev(const uint8_t* data, uint64_t len, const uint32_t* blocks, uint64_t nblocks, uint8_t* keys,
                       uint64_t keys_cap, uint64_t* offsets, uint32_t* val_offsets, uint64_t* created_ms,
                       uint8_t* tombstones, uint64_t entries_cap, uint64_t* n_out, void* stream) {
    FORK_GUARD();
    if (!n_out) return fail(VBF_EINVAL, "n_out is NULL");
    hipStream_t s = (hipStream_t)stream;
    vbf::SstArgs a;
    int rc = sst_count_pass(data, len, blocks, nblocks, s, &a, n_out);
    if (rc) return rc;
    if ((rc = sst_decode_caps(val_offsets || created_ms || tombstones, offsets, keys, entries_cap, keys_cap, *n_out,
                              len - 17 * *n_out)))
        return rc;
    if ((rc = sst_emit_pass(a, keys, offsets, val_offsets, created_ms, tombstones, s))) return rc;
    return ok();
}

int vbf_sst_decode_host(const uint8_t* data, uint64_t len, const uint8_t* index, uint64_t index_len, uint8_t* keys,
                        uint64_t keys_cap, uint64_t* offsets, uint32_t* val_offsets, uint64_t* created_ms,
                        uint8_t* tombstones, uint64_t entries_cap, uint64_t* n_out, int device) {
    if (!n_out || (len && !data) || (index_len && !index)) return fail(VBF_EINVAL, "NULL argument");
    std::vector<uint32_t> blk;
    int rc = parse_index(index, index_len, &blk);
    if (rc) return rc;
    HOST_CALL(call, device);
    // device image: data | blocks, then the outputs (count pass first, to size them)
    DevImage in;
    const auto p_data = in.add<uint8_t>(len);
    const auto p_blk = in.add<uint32_t>(blk.size());
    if ((rc = in.alloc(call, kWsSstInput))) return rc;
    if ((rc = call.up(in.ptr(p_data), data, len)) || (rc = call.up(in.ptr(p_blk), blk.data(), blk.size()))) return rc;
    vbf::SstArgs a;
    if ((rc = sst_count_pass(in.ptr(p_data), len, in.ptr(p_blk), blk.size(), call.s, &a, n_out))) return rc;
    const uint64_t n = *n_out, kb = len - 17 * n;
    if ((rc = sst_decode_caps(val_offsets || created_ms || tombstones, offsets, keys, entries_cap, keys_cap, n, kb)))
        return rc;
    DevImage out;  // keys | offsets | val | created | tombstones
    const auto p_keys = out.add<uint8_t>(kb, keys);
    const auto p_off = out.add<uint64_t>(n + 1, offsets);
    const auto p_val = out.add<uint32_t>(n, val_offsets);
    const auto p_cr = out.add<uint64_t>(n, created_ms);
    const auto p_tb = out.add<uint8_t>(n, tombstones);
    if ((rc = out.alloc(call, kWsSstKeys))) return rc;
    if ((rc = sst_emit_pass(a, out.ptr(p_keys), out.ptr(p_off), out.ptr(p_val), out.ptr(p_cr), out.ptr(p_tb), call.s)))
        return rc;
    if ((rc = call.down(keys, out.ptr(p_keys), kb)) || (rc = call.down(offsets, out.ptr(p_off), n + 1)) ||
        (rc = call.down(val_offsets, out.ptr(p_val), n)) || (rc = call.down(created_ms, out.ptr(p_cr), n)) ||
        (rc = call.down(tombstones, out.ptr(p_tb), n)))
        return rc;
    return call.finish();
}

// ---- SST data.db / index.db encode ----

int vbf_sst_encode_dev(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                       const uint32_t* val_offsets, const int64_t* created_ms, const uint8_t* tombstones, uint8_t* data,
                       uint64_t data_cap, uint64_t* data_len, uint8_t* index, uint64_t index_cap, uint64_t* index_len,
                       uint32_t* blocks, uint64_t blocks_cap, uint64_t* nblocks, void* stream) {
    FORK_GUARD();
    int rc = sst_encode(keys, offsets, stride, n, val_offsets, created_ms, tombstones, data, data_cap, data_len, index,
                        index_cap, index_len, blocks, blocks_cap, nblocks, (hipStream_t)stream);
    return rc ? rc : ok();
}

int vbf_sst_encode_host(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                        const uint32_t* val_offsets, const int64_t* created_ms, const uint8_t* tombstones, uint8_t* data,
                        uint64_t data_cap, uint64_t* data_len, uint8_t* index, uint64_t index_cap, uint64_t* index_len,
                        uint32_t* blocks, uint64_t blocks_cap, uint64_t* nblocks, int device) {
    if (!data_len || !index_len || !nblocks) return fail(VBF_EINVAL, "data_len / index_len / nblocks is NULL");
    *data_len = *index_len = *nblocks = 0;
    if (n == 0) return ok();
    if (!offsets && stride > 4079)
        return fail(VBF_EINVAL, "entry of %llu bytes exceeds a 4096-byte block (BlockIsFull)",
                    (unsigned long long)(stride + 17));
    if (offsets && offsets[n] < offsets[0]) return fail(VBF_EINVAL, "offsets descend (last below first)");
    const uint64_t k0 = offsets ? offsets[0] : 0, kb = offsets ? offsets[n] - k0 : n * stride;
    if (!keys && kb) return fail(VBF_EINVAL, "keys is NULL");
    if (n >= (1ull << 32) / 17 || kb >= (1ull << 32))
        return fail(VBF_EINVAL, "data.db reaches 2^32 bytes: index.db's u32 block offsets cannot address it");
    HOST_CALL(call, device);
    int rc;
    // device image: keys | offsets | val | created | tombstones | data | index | blocks, the outputs
    // at the sizes that always suffice (or the caller's capacity when that is smaller)
    const uint64_t dcap = data ? std::min(data_cap, kb + 17 * n) : 0, icap = index ? std::min(index_cap, kb + 8 * n) : 0;
    const uint64_t bcap = blocks ? std::min(blocks_cap, n) : 0;
    DevImage img;
    const auto p_keys = img.add<uint8_t>(kb);
    const auto p_off = img.add<uint64_t>(n + 1, offsets);
    const auto p_val = img.add<uint32_t>(n, val_offsets);
    const auto p_cr = img.add<int64_t>(n, created_ms);
    const auto p_tb = img.add<uint8_t>(n, tombstones);
    const auto p_data = img.add<uint8_t>(dcap, data);
    const auto p_idx = img.add<uint8_t>(icap, index);
    const auto p_blk = img.add<uint32_t>(bcap, blocks);
    if ((rc = img.alloc(call, kWsSstEncIO))) return rc;
    if ((rc = call.up(img.ptr(p_keys), kb ? keys + k0 : nullptr, kb)) || (rc = call.up(img.ptr(p_off), offsets, n + 1)) ||
        (rc = call.up(img.ptr(p_val), val_offsets, n)) || (rc = call.up(img.ptr(p_cr), created_ms, n)) ||
        (rc = call.up(img.ptr(p_tb), tombstones, n)))
        return rc;
    // offsets are absolute positions in `keys`: the device copy starts at keys + offsets[0]
    if ((rc = sst_encode(arena_base(img.ptr(p_keys), k0), img.ptr(p_off), stride, n, img.ptr(p_val), img.ptr(p_cr),
                         img.ptr(p_tb), img.ptr(p_data), dcap, data_len, img.ptr(p_idx), icap, index_len,
                         img.ptr(p_blk), bcap, nblocks, call.s)))
        return rc;
    if ((rc = call.down(data, img.ptr(p_data), *data_len)) || (rc = call.down(index, img.ptr(p_idx), *index_len)) ||
        (rc = call.down(blocks, img.ptr(p_blk), *nblocks)))
        return rc;
    return call.finish();
}

// range.rs:117-128 (load_entries_from_file + build_filter_from_entries) on the device: decode
// data.db into packed keys/offsets and OR their bits into the filter; no_of_elements += n.
// Caller holds s.mu (drained), on s.device; the filter is device-resident.
static int rebuild_locked(vbf_filter* f, Storage& s, const uint8_t* data, uint64_t len, const uint32_t* blocks,
                          uint64_t nblocks, uint64_t* n_out, hipStream_t st) {
    uint64_t n = 0;
    vbf::SstArgs a;
    uint32_t ulen = 0xFFFFFFFFu;
    int rc = sst_count_pass(data, len, blocks, nblocks, st, &a, &n, &ulen);
    if (rc) return rc;
    if (n_out) *n_out = n;
    if ((rc = check_mk(s.m, f->k, n))) return rc;
    if (n && f->k) {
        const uint64_t kb = len - 17 * n, o_off = align256(kb);
        void* out = nullptr;
        if ((rc = get_workspace(st, o_off + (n + 1) * 8, &out, kWsSstKeys))) return rc;
        uint8_t* d_keys = static_cast<uint8_t*>(out);
        uint64_t* d_off = reinterpret_cast<uint64_t*>(d_keys + o_off);
        // every key the same length (the common case): packed keys are a fixed-stride batch, which
        // the build reads with its aligned fast path instead of through offsets
        const bool uniform = ulen != 0xFFFFFFFFu && ulen > 0;
        if ((rc = sst_emit_pass(a, d_keys, uniform ? nullptr : d_off, nullptr, nullptr, nullptr, st))) return rc;
        if ((rc = storage_wait(s, st))) return rc;
        vbf::KeyBatch kb2 = uniform ? batch(d_keys, nullptr, 0, ulen, n, 1) : batch(d_keys, d_off, 0, 0, n, 1);
        s.mirror_ok = false;
        s.pristine = false;
        if ((rc = do_build(kb2, s.m, f->k, s.d_words, VBF_BUILD_AUTO, true, st))) return rc;
        if ((rc = storage_mark(s, st))) return rc;
        if ((rc = mirror_after_write(s, st))) return rc;
    }
    f->n.fetch_add((uint32_t)n);
    return VBF_OK;
}

int vbf_filter_rebuild_from_sst_dev(vbf_filter* f, const uint8_t* data, uint64_t len, const uint32_t* blocks,
                                    uint64_t nblocks, uint64_t* n_out, void* stream) {
    if (!f) return fail(VBF_EINVAL, "filter is NULL");
    Storage& s = *f->bits;
    std::unique_lock<std::mutex> lk(s.mu);
    int rc = storage_drain(s, lk);
    if (rc) return rc;
    if (s.host()) return host_resident("vbf_filter_rebuild_from_sst_dev");
    DEVICE_SCOPE(s.device);
    if ((rc = rebuild_locked(f, s, data, len, blocks, nblocks, n_out, (hipStream_t)stream))) return rc;
    return ok();
}

int vbf_filter_rebuild_from_sst_host(vbf_filter* f, const uint8_t* data, uint64_t len, const uint8_t* index,
                                     uint64_t index_len, uint64_t* n_out) {
    if (!f || (len && !data) || (index_len && !index)) return fail(VBF_EINVAL, "NULL argument");
    Storage& s = *f->bits;
    std::vector<uint32_t> blk;
    int rc = parse_index(index, index_len, &blk);
    if (rc) return rc;
    std::unique_lock<std::mutex> lk(s.mu);
    if ((rc = storage_drain(s, lk))) return rc;
    if (s.host()) return host_resident("vbf_filter_rebuild_from_sst_host");
    HOST_CALL(call, s.device);  // after the filter's lock and its drain
    DevImage in;  // data | blocks
    const auto p_data = in.add<uint8_t>(len);
    const auto p_blk = in.add<uint32_t>(blk.size());
    if ((rc = in.alloc(call, kWsSstInput))) return rc;
    if ((rc = call.up(in.ptr(p_data), data, len)) || (rc = call.up(in.ptr(p_blk), blk.data(), blk.size()))) return rc;
    if ((rc = rebuild_locked(f, s, in.ptr(p_data), len, in.ptr(p_blk), blk.size(), n_out, call.s))) return rc;
    return call.finish();
}

}  // extern "C"

// ---- batched probe across SSTs ----

namespace {
// Locks every distinct storage of `filters` in address order (clones share one), so two
// concurrent multi-probes over overlapping sets cannot deadlock; then drains each filter's
// queued asynchronous sets.
struct MultiLock {
    std::vector<std::unique_lock<std::mutex>> locks;
    std::vector<Storage*> v;
    explicit MultiLock(const vbf_filter* const* filters, uint32_t nsst) {
        for (uint32_t s = 0; s < nsst; ++s)
            if (filters[s]) v.push_back(filters[s]->bits.get());
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
        for (Storage* st : v) locks.emplace_back(st->mu);
    }
    // A device's worker runs its queued jobs in order, each under its own filter's lock.  Waiting
    // for filter A's job while holding B's lock would deadlock when B's job is queued ahead of
    // A's on the same worker.  So: with every lock held, find a filter whose jobs are
    // not all done; if there is one, release every lock, wait for that filter alone, take the
    // locks again (address order) and look again.  Only once all are settled are failures
    // reported (storage_drain no longer waits then).
    int drain() {
        for (;;) {
            Storage* behind = nullptr;
            for (Storage* st : v)
                if (!storage_jobs_settled(*st)) {
                    behind = st;
                    break;
                }
            if (!behind) break;
            for (auto& l : locks) l.unlock();
            {
                std::unique_lock<std::mutex> lk(behind->mu);
                behind->jobs_cv.wait(lk, [&] { return storage_jobs_settled(*behind); });
            }
            for (auto& l : locks) l.lock();
        }
        for (size_t i = 0; i < v.size(); ++i)
            if (int rc = storage_drain(*v[i], locks[i])) return rc;
        return VBF_OK;
    }
};

// Rust's Ord for [u8]: bytewise, then shorter first.
int cmp_host(const uint8_t* a, uint64_t la, const uint8_t* b, uint64_t lb) {
    const int c = std::memcmp(a, b, std::min(la, lb));
    if (c) return c < 0 ? -1 : 1;
    return la < lb ? -1 : (la > lb ? 1 : 0);
}

// The read path's small batches (one get: one key against every in-range SST,
// range.rs:101-136) answered on the CPU from the filters' host mirrors; the same answers as the
// k_multi_probe kernel.  Caller holds every filter's lock (drained).  The filters may live on
// different GPUs (compaction places them round-robin, VBF_DEVICE_AUTO): each mirror is filled on
// its own device.
static int mirror_fill_on_device(Storage& s) {
    DEVICE_SCOPE(s.device);
    return mirror_fill(s);
}

int multi_probe_mirror(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n, int len_prefix,
                       uint32_t nsst, const vbf_filter* const* filters, const uint8_t* bounds,
                       const uint64_t* bounds_off, uint8_t* out) {
    for (uint32_t i = 0; i < nsst; ++i)
        if (int rc = mirror_fill_on_device(*filters[i]->bits)) return rc;
    for (uint64_t j = 0; j < n; ++j) {
        const uint8_t* kp;
        uint64_t kl;
        host_key(keys, offsets, stride, j, &kp, &kl);
        for (uint32_t i = 0; i < nsst; ++i) {
            const Storage& st = *filters[i]->bits;
            const uint32_t k = filters[i]->k;
            bool hit = true;
            if (bounds_off)  // range.rs:118
                hit = cmp_host(kp, kl, bounds + bounds_off[2 * i], bounds_off[2 * i + 1] - bounds_off[2 * i]) >= 0 &&
                      cmp_host(kp, kl, bounds + bounds_off[2 * i + 1], bounds_off[2 * i + 2] - bounds_off[2 * i + 1]) <= 0;
            if (hit && k > 0 && st.m == 0)
                return fail(VBF_EDIVZERO, "a key inside an SST's range reaches its filter with m == 0 < k "
                                          "(bf.rs:100 divides by zero)");
            uint8_t h = hit ? 1 : 0;
            if (hit && k > 0) host_contains(st.mirror, st.m, k, kp, nullptr, kl, 1, len_prefix != 0, &h);
            out[j * nsst + i] = h;
        }
    }
    return VBF_OK;
}

int multi_probe(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n, int len_prefix,
                uint32_t nsst, const vbf_filter* const* filters, const uint8_t* bounds, const uint64_t* bounds_off,
                uint8_t* out, hipStream_t s) {
    if (nsst && !filters) return fail(VBF_EINVAL, "filters is NULL");
    bool zero_m = false;
    for (uint32_t i = 0; i < nsst; ++i) {
        if (!filters[i]) return fail(VBF_EINVAL, "filters[%u] is NULL", i);
        if (filters[i]->bits->host()) return host_resident("vbf_multi_probe");
        if (filters[i]->bits->device != filters[0]->bits->device)
            return fail(VBF_EINVAL, "filters[%u] lives on device %d, filters[0] on %d", i, filters[i]->bits->device,
                        filters[0]->bits->device);
        // bf.rs:100 divides by m: the reference panics once a key reaches such a filter.  Without
        // key ranges every key reaches every filter; with them only keys inside its range do.
        if (filters[i]->bits->m == 0 && filters[i]->k > 0 && n) {
            if (!bounds_off)
                return fail(VBF_EDIVZERO, "filters[%u]: m == 0 with k = %u (bf.rs:100 divides by zero)", i,
                            filters[i]->k);
            zero_m = true;
        }
    }
    if (bounds_off) {
        for (uint32_t i = 0; i < 2 * nsst; ++i)
            if (bounds_off[i + 1] < bounds_off[i]) return fail(VBF_EINVAL, "bounds_off not nondecreasing at %u", i);
        if (bounds_off[2 * nsst] && !bounds) return fail(VBF_EINVAL, "bounds is NULL");
    }
    if (!n || !nsst) return VBF_OK;
    if (!out) return fail(VBF_EINVAL, "out is NULL");
    // Filters sharing (m, k) test the same positions for a key: interleave up to 8 of them and
    // probe them together (vbf_multi_part.hip) when the batch is large; the rest one lane per key.
    const char* menv = getenv("VBF_MULTI");  // A/B knob, read per call
    const int mode = menv ? atoi(menv) : 0;
    std::vector<vbf::MultiGroup> groups;
    std::vector<char> grouped(nsst, 0);
    if (mode != 1 && (mode == 2 || n >= kMultiGroupMinKeys)) {
        std::vector<uint32_t> order(nsst);
        for (uint32_t i = 0; i < nsst; ++i) order[i] = i;
        auto key_of = [&](uint32_t i) { return std::make_pair(filters[i]->bits->m, filters[i]->k); };
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key_of(a) < key_of(b); });
        for (uint32_t x = 0; x < nsst;) {
            uint32_t y = x;
            while (y < nsst && key_of(order[y]) == key_of(order[x])) ++y;
            const uint32_t m = filters[order[x]]->bits->m, k = filters[order[x]]->k;
            if (y - x >= 2 && vbf::multi_group_supported(m, k)) {
                for (uint32_t a = x; a < y; a += vbf::kMaxGroup) {
                    vbf::MultiGroup g{};
                    g.m = m;
                    g.k = k;
                    g.G = std::min<uint32_t>(vbf::kMaxGroup, y - a);
                    for (uint32_t q = 0; q < g.G; ++q) {
                        const uint32_t i = order[a + q];
                        g.words[q] = filters[i]->bits->d_words;
                        g.col[q] = i;
                        if (bounds_off) {
                            g.lo_beg[q] = bounds_off[2 * i];
                            g.lo_end[q] = g.hi_beg[q] = bounds_off[2 * i + 1];
                            g.hi_end[q] = bounds_off[2 * i + 2];
                        }
                        grouped[i] = 1;
                    }
                    groups.push_back(g);
                }
            }
            x = y;
        }
    }
    std::vector<vbf::MultiSst> tab;
    for (uint32_t i = 0; i < nsst; ++i) {
        if (grouped[i]) continue;
        const Storage& st = *filters[i]->bits;
        vbf::MultiSst e{st.d_words, st.m, st.m ? ~0ull / st.m : 0, filters[i]->k, i, 0, 0, 0, 0};
        if (bounds_off) {
            e.lo_beg = bounds_off[2 * i];
            e.lo_end = e.hi_beg = bounds_off[2 * i + 1];
            e.hi_end = bounds_off[2 * i + 2];
        }
        tab.push_back(e);
    }
    const uint64_t nb = bounds_off ? bounds_off[2 * nsst] : 0;
    const uint64_t o_b = align256(nsst * sizeof(vbf::MultiSst));
    const uint64_t o_err = o_b + align256(nb + 8);
    void* ws = nullptr;
    int rc = get_workspace(s, o_err + 256, &ws, kWsMulti);
    if (rc) return rc;
    uint32_t* d_err = reinterpret_cast<uint32_t*>(static_cast<char*>(ws) + o_err);
    // the table is read by this launch only; the stream orders reuse by the next call
    if (!tab.empty())
        HIP_TRY(hipMemcpyAsync(ws, tab.data(), tab.size() * sizeof(vbf::MultiSst), hipMemcpyHostToDevice, s));
    uint8_t* d_bounds = nullptr;
    if (bounds_off) {
        d_bounds = static_cast<uint8_t*>(ws) + o_b;
        if (nb) HIP_TRY(hipMemcpyAsync(d_bounds, bounds, nb, hipMemcpyHostToDevice, s));
    }
    if (zero_m) HIP_TRY(hipMemsetAsync(d_err, 0, 4, s));
    HIP_TRY(hipStreamSynchronize(s));  // pageable sources: keep them alive only for this call
    // every filter's pending work (set_dev on another stream) lands before the probe reads it
    for (uint32_t i = 0; i < nsst; ++i)
        if ((rc = storage_wait(*filters[i]->bits, s))) return rc;
    const vbf::KeyBatch kb = batch(keys, offsets, 0, stride, n, len_prefix);
    for (const vbf::MultiGroup& g : groups) {
        const uint64_t need = vbf::multi_group_workspace_bytes(n, g.m, g.k);
        void* gw = nullptr;
        if ((rc = get_workspace(s, need, &gw, kWsMultiGroup))) return rc;
        HIP_TRY(vbf::launch_multi_probe_group(kb, g, d_bounds, out, nsst, gw, need, s));
    }
    if (!tab.empty()) {
        vbf::MultiArgs a{keys, offsets, 0, stride, n, (uint32_t)tab.size(),
                         static_cast<const vbf::MultiSst*>(ws), d_bounds, out, d_err, nsst};
        HIP_TRY(vbf::launch_multi_probe(a, len_prefix != 0, s));
    }
    for (uint32_t i = 0; i < nsst; ++i)
        if ((rc = storage_mark(*filters[i]->bits, s))) return rc;
    if (zero_m) {  // rare (Default / p > 1 filters): one readback decides whether the reference panics
        uint32_t e = 0;
        HIP_TRY(hipMemcpyAsync(&e, d_err, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (e) return fail(VBF_EDIVZERO, "a key inside an SST's range reaches its filter with m == 0 < k "
                                         "(bf.rs:100 divides by zero)");
    }
    return VBF_OK;
}
}  // namespace

extern "C" {

int vbf_multi_probe_dev(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n, int len_prefix,
                        uint32_t nsst, const vbf_filter* const* filters, const uint8_t* bounds,
                        const uint64_t* bounds_off, uint8_t* out, void* stream) {
    FORK_GUARD();
    int rc = check_keys(keys, offsets, stride, n);
    if (rc) return rc;
    if (nsst && filters && filters[0]) {
        MultiLock lk(filters, nsst);
        if ((rc = lk.drain())) return rc;
        if (filters[0]->bits->host()) return host_resident("vbf_multi_probe_dev");
        DEVICE_SCOPE(filters[0]->bits->device);
        if ((rc = multi_probe(keys, offsets, stride, n, len_prefix, nsst, filters, bounds, bounds_off, out,
                              (hipStream_t)stream)))
            return rc;
        return ok();
    }
    if ((rc = multi_probe(keys, offsets, stride, n, len_prefix, nsst, filters, bounds, bounds_off, out,
                          (hipStream_t)stream)))
        return rc;
    return ok();
}

}  // extern "C"

namespace {
// The device path of vbf_multi_probe_host for filters that all live on `device`: the keys are
// staged to it and the answers copied back.  Caller holds every filter's lock (drained).
int multi_probe_host_device(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                            int len_prefix, uint32_t nsst, const vbf_filter* const* filters, const uint8_t* bounds,
                            const uint64_t* bounds_off, uint8_t* out, int device) {
    HOST_CALL(call, device);  // this device's part only: the multi-device path takes each in turn
    int rc;
    const uint64_t k0 = offsets ? offsets[0] : 0, kbytes = offsets ? offsets[n] - k0 : n * stride;
    DevImage img;  // keys | offsets | answers
    const auto p_keys = img.add<uint8_t>(kbytes);
    const auto p_off = img.add<uint64_t>(n + 1, offsets);
    const auto p_out = img.add<uint8_t>(n * nsst);
    if ((rc = img.alloc(call, kWsMultiKeys))) return rc;
    if ((rc = call.up(img.ptr(p_keys), kbytes ? keys + k0 : nullptr, kbytes))) return rc;
    // absolute positions in the device copy
    if (offsets && ((rc = call.up_rebased(img.ptr(p_off), offsets, n + 1)) || (rc = call.sync()))) return rc;
    if ((rc = multi_probe(img.ptr(p_keys), img.ptr(p_off), stride, n, len_prefix, nsst, filters, bounds, bounds_off,
                          img.ptr(p_out), call.s)))
        return rc;
    if ((rc = call.down(out, img.ptr(p_out), n * nsst))) return rc;
    return call.finish();
}

// vbf_multi_probe_host over filters split into groups (group[i] of filter i; the multi-device
// path groups by device): each group is probed on the device of its first filter, with the keys
// staged there, its filters' bound bytes re-based into a bounds array of their own, and its answer
// columns scattered back into out[n][nsst].  Caller holds every filter's lock (drained).
int multi_probe_host_groups(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                            int len_prefix, uint32_t nsst, const vbf_filter* const* filters, const uint8_t* bounds,
                            const uint64_t* bounds_off, uint8_t* out, const int* group) {
    std::vector<int> gs;
    for (uint32_t i = 0; i < nsst; ++i)
        if (std::find(gs.begin(), gs.end(), group[i]) == gs.end()) gs.push_back(group[i]);
    std::vector<const vbf_filter*> sub;
    std::vector<uint32_t> cols;
    std::vector<uint8_t> sb, tmp;
    std::vector<uint64_t> so;
    for (const int g : gs) {
        sub.clear();
        cols.clear();
        sb.clear();
        so.assign(1, 0);
        for (uint32_t i = 0; i < nsst; ++i) {
            if (group[i] != g) continue;
            sub.push_back(filters[i]);
            cols.push_back(i);
            if (bounds_off) {  // this filter's [lo, hi) bound bytes, re-based
                sb.insert(sb.end(), bounds + bounds_off[2 * i], bounds + bounds_off[2 * i + 1]);
                so.push_back(sb.size());
                sb.insert(sb.end(), bounds + bounds_off[2 * i + 1], bounds + bounds_off[2 * i + 2]);
                so.push_back(sb.size());
            }
        }
        const uint32_t ns = (uint32_t)sub.size();
        const int dev = sub[0]->bits->device;
        for (const vbf_filter* f : sub)
            if (f->bits->device != dev)
                return fail(VBF_EINVAL, "a group's filters live on devices %d and %d", dev, f->bits->device);
        tmp.resize(n * ns);
        if (int rc = multi_probe_host_device(keys, offsets, stride, n, len_prefix, ns, sub.data(),
                                             bounds_off ? sb.data() : nullptr, bounds_off ? so.data() : nullptr,
                                             tmp.data(), dev))
            return rc;
        for (uint64_t j = 0; j < n; ++j)
            for (uint32_t q = 0; q < ns; ++q) out[j * nsst + cols[q]] = tmp[j * ns + q];
    }
    return VBF_OK;
}
}  // namespace

extern "C" {

int vbf_multi_probe_host(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n, int len_prefix,
                         uint32_t nsst, const vbf_filter* const* filters, const uint8_t* bounds,
                         const uint64_t* bounds_off, uint8_t* out) {
    int rc = check_keys(keys, offsets, stride, n);
    if (rc) return rc;
    if (!nsst || !n) {
        if ((rc = multi_probe(keys, offsets, stride, n, len_prefix, nsst, filters, bounds, bounds_off, out, nullptr)))
            return rc;
        return ok();
    }
    if (!filters) return fail(VBF_EINVAL, "filters is NULL");
    for (uint32_t i = 0; i < nsst; ++i)
        if (!filters[i]) return fail(VBF_EINVAL, "filters[%u] is NULL", i);
    if (!out) return fail(VBF_EINVAL, "out is NULL");
    if (bounds_off) {
        for (uint32_t i = 0; i < 2 * nsst; ++i)
            if (bounds_off[i + 1] < bounds_off[i]) return fail(VBF_EINVAL, "bounds_off not nondecreasing at %u", i);
        if (bounds_off[2 * nsst] && !bounds) return fail(VBF_EINVAL, "bounds is NULL");
    }
    MultiLock lk(filters, nsst);
    if ((rc = lk.drain())) return rc;
    bool mirrored = n <= mirror_max_keys();
    std::vector<int> devices;
    for (uint32_t i = 0; i < nsst; ++i) {
        const Storage& st = *filters[i]->bits;
        if (st.host()) return host_resident("vbf_multi_probe_host");
        if (mirror_mode(st) == VBF_MIRROR_OFF) mirrored = false;
        if (std::find(devices.begin(), devices.end(), st.device) == devices.end()) devices.push_back(st.device);
    }
    if (mirrored) {  // the read path's one-key gets: no kernel, any mix of devices
        if ((rc = multi_probe_mirror(keys, offsets, stride, n, len_prefix, nsst, filters, bounds, bounds_off, out)))
            return rc;
        return ok();
    }
    if (devices.size() == 1) {
        if ((rc = multi_probe_host_device(keys, offsets, stride, n, len_prefix, nsst, filters, bounds, bounds_off, out,
                                          devices[0])))
            return rc;
        return ok();
    }
    // filters on several GPUs: each device probes its own filters
    std::vector<int> group(nsst);
    for (uint32_t i = 0; i < nsst; ++i) group[i] = filters[i]->bits->device;
    if ((rc = multi_probe_host_groups(keys, offsets, stride, n, len_prefix, nsst, filters, bounds, bounds_off, out,
                                      group.data())))
        return rc;
    return ok();
}

int vbf_multi_probe_host_grouped(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                                 int len_prefix, uint32_t nsst, const vbf_filter* const* filters,
                                 const uint8_t* bounds, const uint64_t* bounds_off, const int* group, uint8_t* out) {
    int rc = check_keys(keys, offsets, stride, n);
    if (rc) return rc;
    if (!nsst || !n) return ok();
    if (!filters || !group || !out) return fail(VBF_EINVAL, "NULL argument");
    for (uint32_t i = 0; i < nsst; ++i)
        if (!filters[i]) return fail(VBF_EINVAL, "filters[%u] is NULL", i);
    if (bounds_off) {
        for (uint32_t i = 0; i < 2 * nsst; ++i)
            if (bounds_off[i + 1] < bounds_off[i]) return fail(VBF_EINVAL, "bounds_off not nondecreasing at %u", i);
        if (bounds_off[2 * nsst] && !bounds) return fail(VBF_EINVAL, "bounds is NULL");
    }
    MultiLock lk(filters, nsst);
    if ((rc = lk.drain())) return rc;
    for (uint32_t i = 0; i < nsst; ++i)
        if (filters[i]->bits->host()) return host_resident("vbf_multi_probe_host_grouped");
    if ((rc = multi_probe_host_groups(keys, offsets, stride, n, len_prefix, nsst, filters, bounds, bounds_off, out,
                                      group)))
        return rc;
    return ok();
}

}  // extern "C"

// ---- compaction merge ----

namespace {
// The merge's argument checks, all on the host and before any device work, shared by the _dev and
// _host entry points so that both give the same code and message.  hipcub's selects and scans run
// over the entry count, so it stays below 2^31; that check precedes the NULL checks (a count that
// large is wrong whatever the pointers are).  *total = run_off[nruns], 0 for no tables.
int compact_validate(const uint64_t* offsets, const int64_t* created, const uint8_t* tomb, const uint64_t* run_off,
                     uint32_t nruns, const uint8_t* map_keys, const uint64_t* map_off, const int64_t* map_time,
                     uint64_t map_n, bool need_out_ids, const uint32_t* out_ids, uint64_t* total) {
    *total = 0;
    if (nruns == 0) return VBF_OK;
    if (!run_off) return fail(VBF_EINVAL, "run_off is NULL");
    if (run_off[0] != 0) return fail(VBF_EINVAL, "run_off must start at 0");
    for (uint32_t r = 0; r < nruns; ++r)
        if (run_off[r + 1] < run_off[r]) return fail(VBF_EINVAL, "run_off not nondecreasing at %u", r);
    const uint64_t n = run_off[nruns];
    if (n > 0x7FFFFFFFull) return fail(VBF_EINVAL, "too many entries (%llu > 2^31 - 1)", (unsigned long long)n);
    if (n && (!offsets || !created || !tomb || (need_out_ids && !out_ids))) return fail(VBF_EINVAL, "NULL argument");
    if (map_n && (!map_keys || !map_off || !map_time)) return fail(VBF_EINVAL, "map arrays are NULL");
    *total = n;
    return VBF_OK;
}

// The merge levels over first-level segments [bnd[i], bnd[i + 1]): per level the segment
// boundaries (`all`) and every pair's first tile (`tiles_all`), in the layout merge_levels_from
// walks.  No level for a single segment.
struct MergeGeometry {
    std::vector<uint64_t> all, tiles_all, ntiles_lv;
    std::vector<uint32_t> nseg_lv;
    uint64_t max_tiles = 1;
    explicit MergeGeometry(std::vector<uint64_t> bnd) {
        const uint64_t tile = vbf::compact_tile();
        uint32_t nseg = (uint32_t)bnd.size() - 1;
        while (nseg > 1) {
            all.insert(all.end(), bnd.begin(), bnd.end());
            nseg_lv.push_back(nseg);
            uint64_t t = 0;
            for (uint32_t i = 0; i < nseg; i += 2) {
                tiles_all.push_back(t);
                const uint64_t len = bnd[std::min(i + 2, nseg)] - bnd[i];
                t += (len + tile - 1) / tile;
            }
            tiles_all.push_back(t);
            ntiles_lv.push_back(t);
            max_tiles = std::max(max_tiles, t);
            std::vector<uint64_t> nb;
            for (uint32_t i = 0; i < nseg; i += 2) nb.push_back(bnd[i]);
            nb.push_back(bnd[nseg]);
            bnd.swap(nb);
            nseg = (uint32_t)bnd.size() - 1;
        }
    }
};

int compact_merge(const uint8_t* keys, const uint64_t* offsets, const int64_t* created, const uint8_t* tomb,
                  const uint64_t* run_off, uint32_t nruns, const uint8_t* map_keys, const uint64_t* map_off,
                  const int64_t* map_time, uint64_t map_n, int use_ttl, uint64_t entry_ttl_ms, uint64_t tomb_ttl_ms,
                  uint64_t now_ms, uint32_t* out_ids, uint64_t* n_out, uint32_t* upd_ids, int64_t* upd_time,
                  uint64_t* n_upd, hipStream_t s) {
    if (!n_out) return fail(VBF_EINVAL, "n_out is NULL");
    *n_out = 0;
    if (n_upd) *n_upd = 0;
    uint64_t total = 0;
    int rc = compact_validate(offsets, created, tomb, run_off, nruns, map_keys, map_off, map_time, map_n, true,
                              out_ids, &total);
    if (rc) return rc;
    if (total == 0) return VBF_OK;
    // merge levels: segment boundaries and per-pair tile starts per level, all uploaded at once
    const MergeGeometry geo(std::vector<uint64_t>(run_off, run_off + nruns + 1));
    const std::vector<uint64_t>& all = geo.all;
    const std::vector<uint64_t>& tiles_all = geo.tiles_all;
    const std::vector<uint64_t>& ntiles_lv = geo.ntiles_lv;
    const std::vector<uint32_t>& nseg_lv = geo.nseg_lv;
    const uint64_t max_tiles = geo.max_tiles;
    size_t t1 = 0, t2 = 0, t3 = 0;
    HIP_TRY(vbf::select_u32(nullptr, &t1, nullptr, nullptr, nullptr, nullptr, total, s));
    HIP_TRY(vbf::select_i64(nullptr, &t2, nullptr, nullptr, nullptr, nullptr, total, s));
    t3 = std::max(t1, t2);
    const uint64_t o_pong = align256(total * 4), o_keep = o_pong + align256(total * 4);
    const uint64_t o_sel = o_keep + align256(total), o_upd = o_sel + align256(total * 4);
    const uint64_t o_ut = o_upd + align256(total), o_ro = o_ut + align256(total * 8);
    const uint64_t o_bnd = o_ro + align256((nruns + 1) * 8), o_tl = o_bnd + align256(all.size() * 8 + 8);
    const uint64_t o_pp = o_tl + align256(tiles_all.size() * 8 + 8), o_pq = o_pp + align256(total * 8);
    const uint64_t o_split = o_pq + align256(total * 8), o_misc = o_split + align256(max_tiles * 8);
    const uint64_t o_tmp = o_misc + 256, bytes = o_tmp + t3;
    void* ws = nullptr;
    if ((rc = get_workspace(s, bytes, &ws, kWsCompact))) return rc;
    char* b = static_cast<char*>(ws);
    uint32_t* ping = reinterpret_cast<uint32_t*>(b);
    uint32_t* pong = reinterpret_cast<uint32_t*>(b + o_pong);
    uint8_t* keep = reinterpret_cast<uint8_t*>(b + o_keep);
    uint32_t* sel = reinterpret_cast<uint32_t*>(b + o_sel);
    uint8_t* upd = reinterpret_cast<uint8_t*>(b + o_upd);
    int64_t* ut = reinterpret_cast<int64_t*>(b + o_ut);
    uint64_t* d_ro = reinterpret_cast<uint64_t*>(b + o_ro);
    uint64_t* d_bnd = reinterpret_cast<uint64_t*>(b + o_bnd);
    uint64_t* d_tl = reinterpret_cast<uint64_t*>(b + o_tl);
    uint64_t* pping = reinterpret_cast<uint64_t*>(b + o_pp);
    uint64_t* ppong = reinterpret_cast<uint64_t*>(b + o_pq);
    uint64_t* split = reinterpret_cast<uint64_t*>(b + o_split);
    uint64_t* misc = reinterpret_cast<uint64_t*>(b + o_misc);  // [0] n_out, [1] n_upd, [2] sort error
    HIP_TRY(hipMemcpyAsync(d_ro, run_off, (nruns + 1) * 8, hipMemcpyHostToDevice, s));
    if (!all.empty()) HIP_TRY(hipMemcpyAsync(d_bnd, all.data(), all.size() * 8, hipMemcpyHostToDevice, s));
    if (!tiles_all.empty())
        HIP_TRY(hipMemcpyAsync(d_tl, tiles_all.data(), tiles_all.size() * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(misc, 0, 16, s));
    HIP_TRY(hipMemsetAsync(misc + 2, 0xFF, 8, s));
    vbf::CompactArgs a{keys, offsets, created, tomb, d_ro, nruns, map_keys, map_off, map_time, map_n, use_ttl,
                       entry_ttl_ms, tomb_ttl_ms, now_ms, total};
    vbf::phase_begin(vbf::kPhaseMergeLevels, s);
    HIP_TRY(vbf::compact_check_sorted(a, reinterpret_cast<uint32_t*>(misc + 2), s));
    uint32_t* order = nullptr;
    uint64_t* opfx = nullptr;
    HIP_TRY(vbf::compact_merge_levels(a, d_bnd, d_tl, nseg_lv.data(), ntiles_lv.data(), (uint32_t)nseg_lv.size(),
                                      ping, pong, pping, ppong, split, &order, &opfx, s));
    vbf::phase_end(vbf::kPhaseMergeLevels, s);
    vbf::phase_begin(vbf::kPhaseFold, s);
    HIP_TRY(vbf::compact_fold(a, order, opfx, total, keep, sel, upd, ut, s));
    vbf::phase_end(vbf::kPhaseFold, s);
    vbf::phase_begin(vbf::kPhaseSelect, s);
    size_t tb = t3;
    HIP_TRY(vbf::select_u32(b + o_tmp, &tb, sel, keep, out_ids, misc, total, s));
    if (upd_ids && upd_time) {
        tb = t3;
        HIP_TRY(vbf::select_u32(b + o_tmp, &tb, order, upd, upd_ids, misc + 1, total, s));
        tb = t3;
        HIP_TRY(vbf::select_i64(b + o_tmp, &tb, ut, upd, upd_time, misc + 1, total, s));
    }
    vbf::phase_end(vbf::kPhaseSelect, s);
    uint64_t hv[3];
    HIP_TRY(hipMemcpyAsync(hv, misc, 24, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint32_t bad = (uint32_t)hv[2];
    if (bad != 0xFFFFFFFFu)
        return fail(VBF_EINVAL, "run entries not strictly increasing at entry %u (tables are SkipMaps)", bad);
    *n_out = hv[0];
    if (n_upd) *n_upd = (upd_ids && upd_time) ? hv[1] : 0;
    return VBF_OK;
}

int gather_entries(const uint8_t* keys, const uint64_t* offsets, const int64_t* created, const uint8_t* tomb,
                   const uint32_t* val, const uint32_t* ids, uint64_t n, uint8_t* out_keys, uint64_t out_keys_cap,
                   uint64_t* out_offsets, int64_t* out_created, uint8_t* out_tomb, uint32_t* out_val,
                   uint64_t* key_bytes, hipStream_t s) {
    // the offsets' scan runs over n + 1 items, which stay below 2^31 (hipcub's count)
    if (n >= 0x7FFFFFFFull) return fail(VBF_EINVAL, "too many entries (%llu > 2^31 - 2)", (unsigned long long)n);
    if (!out_offsets) return fail(VBF_EINVAL, "out_offsets is NULL");
    if (n && (!offsets || !ids)) return fail(VBF_EINVAL, "NULL argument");
    if ((out_created && !created) || (out_tomb && !tomb) || (out_val && !val))
        return fail(VBF_EINVAL, "an output array without its input");
    size_t tmpb = 0;
    HIP_TRY(vbf::scan_u64(nullptr, &tmpb, nullptr, nullptr, n + 1, s));
    const uint64_t o_tmp = align256((n + 1) * 8);
    void* ws = nullptr;
    int rc = get_workspace(s, o_tmp + tmpb, &ws, kWsGather);
    if (rc) return rc;
    uint64_t* lens = static_cast<uint64_t*>(ws);
    HIP_TRY(vbf::gather_lens(offsets, ids, n, lens, s));
    HIP_TRY(vbf::scan_u64(static_cast<char*>(ws) + o_tmp, &tmpb, lens, out_offsets, n + 1, s));
    uint64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, out_offsets + n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (key_bytes) *key_bytes = total;
    if (total > out_keys_cap || (total && !out_keys))
        return fail(VBF_EINVAL, "out_keys holds %llu < %llu bytes", (unsigned long long)out_keys_cap,
                    (unsigned long long)total);
    vbf::GatherArgs g{keys, offsets, created, tomb, val, ids, n, out_keys, out_offsets, out_created, out_tomb, out_val};
    HIP_TRY(vbf::gather(g, s));
    return VBF_OK;
}

// The device image of vbf_compact_merge_host and _write_host: the arena (keys | offsets | created |
// tombstones | val_offsets, write only | map keys | map offsets | map times), then the merge's
// outputs (ids | updated ids | updated times).
struct CompactImage : DevImage {
    Part<uint8_t> keys, tb, mk;
    Part<uint64_t> off, mo;
    Part<int64_t> cr, mt, ut;
    Part<uint32_t> val, ids, ui;
};

// Lays the image out, allocates it and uploads the arena (one stream synchronisation: the sources
// are pageable).  with_val without the caller's val_offsets: that part is zero-filled.
int compact_stage(HostCall& c, CompactImage& m, const uint8_t* keys, const uint64_t* offsets, const int64_t* created,
                  const uint8_t* tomb, uint64_t total, bool with_val, const uint32_t* val_offsets,
                  const uint8_t* map_keys, const uint64_t* map_off, const int64_t* map_time, uint64_t map_n,
                  bool want_upd) {
    const uint64_t kb = offsets[total], mkb = map_n ? map_off[map_n] : 0;
    m.keys = m.add<uint8_t>(kb);
    m.off = m.add<uint64_t>(total + 1);
    m.cr = m.add<int64_t>(total);
    m.tb = m.add<uint8_t>(total);
    m.val = m.add<uint32_t>(total, with_val);
    m.mk = m.add<uint8_t>(mkb, map_n);
    m.mo = m.add<uint64_t>(map_n + 1, map_n);
    m.mt = m.add<int64_t>(map_n, map_n);
    m.ids = m.add<uint32_t>(total);
    m.ui = m.add<uint32_t>(total, want_upd);
    m.ut = m.add<int64_t>(total, want_upd);
    int rc = m.alloc(c, kWsCompactIn);
    if (rc || (rc = c.up(m.ptr(m.keys), keys, kb)) || (rc = c.up(m.ptr(m.off), offsets, total + 1)) ||
        (rc = c.up(m.ptr(m.cr), created, total)) || (rc = c.up(m.ptr(m.tb), tomb, total)) ||
        (rc = c.up(m.ptr(m.val), val_offsets, total)))
        return rc;
    if (with_val && !val_offsets) HIP_TRY(hipMemsetAsync(m.ptr(m.val), 0, total * 4, c.s));
    if (map_n && ((rc = c.up(m.ptr(m.mk), map_keys, mkb)) || (rc = c.up(m.ptr(m.mo), map_off, map_n + 1)) ||
                  (rc = c.up(m.ptr(m.mt), map_time, map_n))))
        return rc;
    return c.sync();
}
}  // namespace

extern "C" {

int vbf_compact_merge_dev(const uint8_t* keys, const uint64_t* offsets, const int64_t* created_ms,
                          const uint8_t* tombstones, const uint64_t* run_off, uint32_t nruns, const uint8_t* map_keys,
                          const uint64_t* map_off, const int64_t* map_time, uint64_t map_n, int use_ttl,
                          uint64_t entry_ttl_ms, uint64_t tombstone_ttl_ms, uint64_t now_ms, uint32_t* out_ids,
                          uint64_t* n_out, uint32_t* upd_ids, int64_t* upd_time, uint64_t* n_upd, void* stream) {
    FORK_GUARD();
    int rc = compact_merge(keys, offsets, created_ms, tombstones, run_off, nruns, map_keys, map_off, map_time, map_n,
                           use_ttl, entry_ttl_ms, tombstone_ttl_ms, now_ms, out_ids, n_out, upd_ids, upd_time, n_upd,
                           (hipStream_t)stream);
    return rc ? rc : ok();
}

int vbf_gather_entries_dev(const uint8_t* keys, const uint64_t* offsets, const int64_t* created_ms,
                           const uint8_t* tombstones, const uint32_t* val_offsets, const uint32_t* ids, uint64_t n,
                           uint8_t* out_keys, uint64_t out_keys_cap, uint64_t* out_offsets, int64_t* out_created_ms,
                           uint8_t* out_tombstones, uint32_t* out_val_offsets, uint64_t* key_bytes, void* stream) {
    FORK_GUARD();
    int rc = gather_entries(keys, offsets, created_ms, tombstones, val_offsets, ids, n, out_keys, out_keys_cap,
                            out_offsets, out_created_ms, out_tombstones, out_val_offsets, key_bytes, (hipStream_t)stream);
    return rc ? rc : ok();
}

int vbf_compact_merge_host(const uint8_t* keys, const uint64_t* offsets, const int64_t* created_ms,
                           const uint8_t* tombstones, const uint64_t* run_off, uint32_t nruns, const uint8_t* map_keys,
                           const uint64_t* map_off, const int64_t* map_time, uint64_t map_n, int use_ttl,
                           uint64_t entry_ttl_ms, uint64_t tombstone_ttl_ms, uint64_t now_ms, uint32_t* out_ids,
                           uint64_t* n_out, uint32_t* upd_ids, int64_t* upd_time, uint64_t* n_upd, int device) {
    if (!n_out) return fail(VBF_EINVAL, "n_out is NULL");
    *n_out = 0;
    if (n_upd) *n_upd = 0;
    uint64_t total = 0;
    int rc = compact_validate(offsets, created_ms, tombstones, run_off, nruns, map_keys, map_off, map_time, map_n, true,
                              out_ids, &total);
    if (rc) return rc;
    if (total == 0) return ok();  // no entries: nothing to merge, no device needed
    HOST_CALL(call, device);
    const bool want_upd = upd_ids && upd_time;
    CompactImage m;
    if ((rc = compact_stage(call, m, keys, offsets, created_ms, tombstones, total, false, nullptr, map_keys, map_off,
                            map_time, map_n, want_upd)))
        return rc;
    uint64_t nu = 0;
    if ((rc = compact_merge(m.ptr(m.keys), m.ptr(m.off), m.ptr(m.cr), m.ptr(m.tb), run_off, nruns, m.ptr(m.mk),
                            m.ptr(m.mo), m.ptr(m.mt), map_n, use_ttl, entry_ttl_ms, tombstone_ttl_ms, now_ms,
                            m.ptr(m.ids), n_out, m.ptr(m.ui), m.ptr(m.ut), &nu, call.s)))
        return rc;
    if ((rc = call.down(out_ids, m.ptr(m.ids), *n_out)) ||
        (want_upd && ((rc = call.down(upd_ids, m.ptr(m.ui), nu)) || (rc = call.down(upd_time, m.ptr(m.ut), nu)))) ||
        (rc = call.finish()))
        return rc;
    if (n_upd) *n_upd = nu;
    return ok();
}

// One bucket through to the merged table's files and filter: merge -> gather -> encode -> build,
// all on `device` from one upload of the arena.
int vbf_compact_write_host(const uint8_t* keys, const uint64_t* offsets, const int64_t* created_ms,
                           const uint8_t* tombstones, const uint64_t* run_off, uint32_t nruns, const uint8_t* map_keys,
                           const uint64_t* map_off, const int64_t* map_time, uint64_t map_n, int use_ttl,
                           uint64_t entry_ttl_ms, uint64_t tombstone_ttl_ms, uint64_t now_ms,
                           const uint32_t* val_offsets, double false_positive, vbf_filter** filter_out, uint8_t* data,
                           uint64_t data_cap, uint64_t* data_len, uint8_t* index, uint64_t index_cap,
                           uint64_t* index_len, uint64_t* n_out, uint32_t* upd_ids, int64_t* upd_time, uint64_t* n_upd,
                           int device) {
    if (!n_out || !data_len || !index_len || !filter_out) return fail(VBF_EINVAL, "NULL argument");
    *n_out = *data_len = *index_len = 0;
    *filter_out = nullptr;
    if (n_upd) *n_upd = 0;
    uint64_t total = 0;
    int rc = compact_validate(offsets, created_ms, tombstones, run_off, nruns, map_keys, map_off, map_time, map_n, false,
                              nullptr, &total);
    if (rc) return rc;
    if (total == 0) return fail(VBF_EINVAL, "empty merge: BloomFilter::new asserts no_of_elements > 0 (bf.rs:67)");
    uint32_t m_probe, k_probe;  // bf.rs:63-66: the rate is checked before any work
    if ((rc = vbf_size(false_positive, total, &m_probe, &k_probe))) return rc;
    // The one place a filter lock is taken under the device's: the merged table's filter is created
    // below and no other thread can reach it before this call returns it.
    HOST_CALL(call, device);
    const bool want_upd = upd_ids && upd_time;
    CompactImage m;
    if ((rc = compact_stage(call, m, keys, offsets, created_ms, tombstones, total, true, val_offsets, map_keys, map_off,
                            map_time, map_n, want_upd)))
        return rc;
    uint64_t n = 0, nu = 0;
    if ((rc = compact_merge(m.ptr(m.keys), m.ptr(m.off), m.ptr(m.cr), m.ptr(m.tb), run_off, nruns, m.ptr(m.mk),
                            m.ptr(m.mo), m.ptr(m.mt), map_n, use_ttl, entry_ttl_ms, tombstone_ttl_ms, now_ms,
                            m.ptr(m.ids), &n, m.ptr(m.ui), m.ptr(m.ut), &nu, call.s)))
        return rc;
    // the map updates happen during the fold, before the merged table is looked at (sized.rs:286-320)
    if (want_upd && nu) {
        if ((rc = call.down(upd_ids, m.ptr(m.ui), nu)) || (rc = call.down(upd_time, m.ptr(m.ut), nu)) ||
            (rc = call.sync()))
            return rc;
    }
    if (n_upd) *n_upd = nu;
    if (n == 0) return fail(VBF_EINVAL, "empty merge: BloomFilter::new asserts no_of_elements > 0 (bf.rs:67)");
    // merged table in the build's key layout, then its files; capacities that always suffice
    const uint64_t kb = offsets[total];
    DevImage q;  // keys | offsets | created | tombstones | val | data.db | index.db
    const auto q_keys = q.add<uint8_t>(kb);
    const auto q_off = q.add<uint64_t>(n + 1);
    const auto q_cr = q.add<int64_t>(n);
    const auto q_tb = q.add<uint8_t>(n);
    const auto q_val = q.add<uint32_t>(n);
    const auto q_data = q.add<uint8_t>(kb + 17 * n, data);
    const auto q_idx = q.add<uint8_t>(kb + 8 * n, index);
    if ((rc = q.alloc(call, kWsCompactOut))) return rc;
    uint8_t* g_keys = q.ptr(q_keys);
    uint64_t* g_off = q.ptr(q_off);
    uint64_t gkb = 0;
    if ((rc = gather_entries(m.ptr(m.keys), m.ptr(m.off), m.ptr(m.cr), m.ptr(m.tb), m.ptr(m.val), m.ptr(m.ids), n,
                             g_keys, kb, g_off, q.ptr(q_cr), q.ptr(q_tb), q.ptr(q_val), &gkb, call.s)))
        return rc;
    uint64_t nb = 0;
    if ((rc = sst_encode(g_keys, g_off, 0, n, q.ptr(q_val), q.ptr(q_cr), q.ptr(q_tb), q.ptr(q_data), kb + 17 * n,
                         data_len, q.ptr(q_idx), kb + 8 * n, index_len, nullptr, 0, &nb, call.s)))
        return rc;
    *n_out = n;
    if (data && data_cap < *data_len)
        return fail(VBF_EINVAL, "data holds %llu < %llu bytes", (unsigned long long)data_cap,
                    (unsigned long long)*data_len);
    if (index && index_cap < *index_len)
        return fail(VBF_EINVAL, "index holds %llu < %llu bytes", (unsigned long long)index_cap,
                    (unsigned long long)*index_len);
    // BloomFilter::new(false_positive, n) + build_filter_from_entries (sized.rs:192-193)
    vbf_filter* f = nullptr;
    if ((rc = vbf_filter_new(false_positive, n, device, &f))) return rc;
    std::unique_ptr<vbf_filter> hold(f);  // freed on any failure below
    if ((rc = vbf_filter_set_dev(f, g_keys, g_off, 0, n, 1, call.s))) return rc;
    if ((rc = call.down(data, q.ptr(q_data), *data_len)) || (rc = call.down(index, q.ptr(q_idx), *index_len)) ||
        (rc = call.finish()))
        return rc;
    *filter_out = hold.release();
    return ok();
}

}  // extern "C"

// ---- memtable flush: MemTable::insert's order and filter step, Flusher::flush (vbf_memtable.hip) ----

namespace {

// vbf_filter_insert_*: one u32 of scratch per filter bit, so at most 2^30 bits (4 GiB).
constexpr uint64_t kInsertMaxBits = 1ull << 30;

// Shared by the _dev and _host sorts, before any device work.  The entry limit first, as in the
// merge: a count that large is wrong whatever the pointers are.
int memtable_check(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n, const uint32_t* out_ids,
                   uint64_t* n_out) {
    if (!n_out) return fail(VBF_EINVAL, "n_out is NULL");
    *n_out = 0;
    if (n > 0x7FFFFFFFull) return fail(VBF_EINVAL, "too many entries (%llu > 2^31 - 1)", (unsigned long long)n);
    if (n == 0) return VBF_OK;
    if (!out_ids) return fail(VBF_EINVAL, "out_ids is NULL");
    return check_keys(keys, offsets, stride, n);
}

int offsets_ascend(const uint64_t* offsets, uint64_t n) {
    if (offsets)
        for (uint64_t i = 0; i < n; ++i)
            if (offsets[i + 1] < offsets[i])
                return fail(VBF_EINVAL, "offsets descend at entry %llu", (unsigned long long)i);
    return VBF_OK;
}

// The sort on device pointers, n in [1, 2^31): out_ids[0 .. *n_out) = the distinct keys in
// ascending order, each by its last put.  One stream synchronisation, for the count and the
// offsets' check.  *soff_out (optional): the sort's own n + 1 offsets into `keys`, valid until the
// next sort on the stream.
// Workspace: 33 bytes per entry (offsets 8, two id buffers 4 + 4, two prefix buffers 8 + 8, the
// keep flags 1), the levels' geometry (16 bytes per tile) and the select's scratch.
int memtable_sort(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n, uint32_t* out_ids,
                  uint64_t* n_out, const uint64_t** soff_out, hipStream_t s) {
    const uint64_t tile = vbf::memtable_tile();
    std::vector<uint64_t> bnd;
    for (uint64_t b = 0; b < n; b += tile) bnd.push_back(b);
    bnd.push_back(n);
    const MergeGeometry geo(std::move(bnd));
    size_t tsel = 0;
    HIP_TRY(vbf::select_u32(nullptr, &tsel, nullptr, nullptr, nullptr, nullptr, n, s));
    DevImage w;
    const auto p_soff = w.add<uint64_t>(n + 1);
    const auto p_ping = w.add<uint32_t>(n);
    const auto p_pong = w.add<uint32_t>(n);
    const auto p_pp = w.add<uint64_t>(n);
    const auto p_pq = w.add<uint64_t>(n);
    const auto p_keep = w.add<uint8_t>(n);
    const auto p_bnd = w.add<uint64_t>(geo.all.size() + 1);
    const auto p_tl = w.add<uint64_t>(geo.tiles_all.size() + 1);
    const auto p_split = w.add<uint64_t>(geo.max_tiles);
    const auto p_misc = w.add<uint64_t>(2);  // [0] the distinct keys, [1] low word: the first descending offset
    const auto p_tmp = w.add<uint8_t>(tsel);
    int rc = get_workspace(s, w.bytes, &w.base, kWsMemSort);
    if (rc) return rc;
    uint64_t* soff = w.ptr(p_soff);
    uint64_t* misc = w.ptr(p_misc);
    if (!geo.all.empty())
        HIP_TRY(hipMemcpyAsync(w.ptr(p_bnd), geo.all.data(), geo.all.size() * 8, hipMemcpyHostToDevice, s));
    if (!geo.tiles_all.empty())
        HIP_TRY(hipMemcpyAsync(w.ptr(p_tl), geo.tiles_all.data(), geo.tiles_all.size() * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(misc, 0, 8, s));
    HIP_TRY(hipMemsetAsync(misc + 1, 0xFF, 8, s));
    vbf::CompactArgs a{};
    a.keys = keys;
    a.offsets = soff;
    a.run_off_host_total = n;
    vbf::phase_begin(vbf::kPhaseMemSort, s);
    HIP_TRY(vbf::memtable_prefixes(keys, offsets, stride, n, reinterpret_cast<uint32_t*>(misc + 1), soff, w.ptr(p_ping),
                                   w.ptr(p_pp), s));
    HIP_TRY(vbf::memtable_tile_sort(a, n, w.ptr(p_ping), w.ptr(p_pp), s));
    vbf::phase_end(vbf::kPhaseMemSort, s);
    vbf::phase_begin(vbf::kPhaseMemMerge, s);
    uint32_t* order = nullptr;
    uint64_t* opfx = nullptr;
    HIP_TRY(vbf::merge_levels_from(a, w.ptr(p_bnd), w.ptr(p_tl), geo.nseg_lv.data(), geo.ntiles_lv.data(),
                                   (uint32_t)geo.nseg_lv.size(), w.ptr(p_ping), w.ptr(p_pong), w.ptr(p_pp), w.ptr(p_pq),
                                   w.ptr(p_split), &order, &opfx, s));
    HIP_TRY(vbf::memtable_keep(a, order, opfx, n, w.ptr(p_keep), s));
    size_t tb = tsel;
    HIP_TRY(vbf::select_u32(w.ptr(p_tmp), &tb, order, w.ptr(p_keep), out_ids, misc, n, s));
    vbf::phase_end(vbf::kPhaseMemMerge, s);
    uint64_t hv[2];
    HIP_TRY(hipMemcpyAsync(hv, misc, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint32_t bad = (uint32_t)hv[1];
    if (bad != 0xFFFFFFFFu) return fail(VBF_EINVAL, "offsets descend at entry %u", bad);
    *n_out = hv[0];
    if (soff_out) *soff_out = soff;
    return VBF_OK;
}

// A batch of host keys as the sort and the filter step take it on the device: the key bytes from
// the first offset on, and the offsets rebased to that copy.
struct KeyImage : DevImage {
    Part<uint8_t> keys;
    Part<uint64_t> off;
    uint64_t kb = 0;
    void lay(const uint64_t* offsets, uint64_t stride, uint64_t n) {
        kb = offsets ? offsets[n] - offsets[0] : n * stride;
        keys = add<uint8_t>(kb);
        off = add<uint64_t>(n + 1, offsets);
    }
    int upload(HostCall& c, const uint8_t* k, const uint64_t* offsets, uint64_t n) {
        int rc = c.up(ptr(keys), kb ? k + (offsets ? offsets[0] : 0) : nullptr, kb);
        return rc ? rc : c.up_rebased(ptr(off), offsets, n + 1);
    }
};

int filter_insert_check(const vbf_filter* f, const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                        uint64_t* n_new) {
    if (n_new) *n_new = 0;
    if (!f) return fail(VBF_EINVAL, "filter is NULL");
    if (n > 0xFFFFFFFEull) return fail(VBF_EINVAL, "too many keys (%llu > 2^32 - 2)", (unsigned long long)n);
    if (f->bits->m > kInsertMaxBits)
        return fail(VBF_EINVAL, "filter of %u bits above the insert's cap of 2^30 bits (one u32 of scratch per bit)",
                    f->bits->m);
    int rc = check_mk(f->bits->m, f->k, n);
    return rc ? rc : check_keys(keys, offsets, stride, n);
}

// mem.rs:209-211 replayed over the batch on a host-resident filter; returns the sets that ran.
uint64_t host_insert(uint32_t* w, uint32_t m, uint32_t k, const uint8_t* keys, const uint64_t* offsets, uint64_t stride,
                     uint64_t n, bool lp) {
    uint64_t fresh = 0;
    std::vector<uint32_t> idx(k);
    for (uint64_t j = 0; j < n; ++j) {
        const uint8_t* kp;
        uint64_t len;
        host_key(keys, offsets, stride, j, &kp, &len);
        const vbf::Prefix p = host_prefix(kp, len, lp);
        bool contained = true;
        for (uint32_t i = 0; i < k; ++i) {
            idx[i] = (uint32_t)(vbf::prefix_hash(p, i) % (uint64_t)m);
            contained = contained && ((w[idx[i] >> 5] >> (idx[i] & 31)) & 1u);
        }
        if (contained) continue;
        for (uint32_t i = 0; i < k; ++i) w[idx[i] >> 5] |= 1u << (idx[i] & 31);
        ++fresh;
    }
    return fresh;
}

// The filter step on a device-resident filter and device keys.  Caller holds s.mu (drained), on
// s.device; n, k > 0.  Counts the keys not contained at their turn, then ORs every key's bits in
// (the skipped sets would have changed nothing).  One stream synchronisation, for the count.
int filter_insert_device(Storage& s, vbf_filter* f, const vbf::KeyBatch& kb, uint64_t* fresh, hipStream_t hs) {
    int rc = storage_wait(s, hs);
    if (rc) return rc;
    const uint64_t np = vbf::filter_insert_partials(kb.n);
    DevImage w;
    const auto p_first = w.add<uint32_t>(s.m);
    const auto p_part = w.add<uint32_t>(np);
    const auto p_cnt = w.add<unsigned long long>(1);
    if ((rc = get_workspace(hs, w.bytes, &w.base, kWsFilterInsert))) return rc;
    HIP_TRY(hipMemsetAsync(w.ptr(p_cnt), 0, 8, hs));
    vbf::phase_begin(vbf::kPhaseFilterInsert, hs);
    HIP_TRY(vbf::filter_insert_count(kb, s.m, f->k, s.d_words, w.ptr(p_first), w.ptr(p_part), w.ptr(p_cnt), hs));
    s.mirror_ok = false;
    s.pristine = false;
    if ((rc = do_build(kb, s.m, f->k, s.d_words, VBF_BUILD_AUTO, true, hs))) return rc;
    vbf::phase_end(vbf::kPhaseFilterInsert, hs);
    if ((rc = storage_mark(s, hs)) || (rc = mirror_after_write(s, hs))) return rc;
    unsigned long long c = 0;
    HIP_TRY(hipMemcpyAsync(&c, w.ptr(p_cnt), 8, hipMemcpyDeviceToHost, hs));
    HIP_TRY(hipStreamSynchronize(hs));
    *fresh = c;
    return VBF_OK;
}

}  // namespace

extern "C" {

int vbf_memtable_sort_dev(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n, uint32_t* out_ids,
                          uint64_t* n_out, void* stream) {
    int rc = memtable_check(keys, offsets, stride, n, out_ids, n_out);
    if (rc) return rc;
    if (n == 0) return ok();
    FORK_GUARD();
    rc = memtable_sort(keys, offsets, stride, n, out_ids, n_out, nullptr, (hipStream_t)stream);
    return rc ? rc : ok();
}

int vbf_memtable_sort_host(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n, uint32_t* out_ids,
                           uint64_t* n_out, int device) {
    int rc = memtable_check(keys, offsets, stride, n, out_ids, n_out);
    if (rc) return rc;
    if (n == 0) return ok();  // no entries: no device needed
    if ((rc = offsets_ascend(offsets, n))) return rc;
    HOST_CALL(call, device);
    KeyImage m;
    m.lay(offsets, stride, n);
    const auto p_ids = m.add<uint32_t>(n);
    if ((rc = m.alloc(call, kWsMemIO)) || (rc = m.upload(call, keys, offsets, n))) return rc;
    if ((rc = memtable_sort(m.ptr(m.keys), m.ptr(m.off), stride, n, m.ptr(p_ids), n_out, nullptr, call.s))) return rc;
    if ((rc = call.down(out_ids, m.ptr(p_ids), *n_out))) return rc;
    return call.finish();
}

int vbf_filter_insert_dev(vbf_filter* f, const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                          int len_prefix, uint64_t* n_new, void* stream) {
    int rc = filter_insert_check(f, keys, offsets, stride, n, n_new);
    if (rc) return rc;
    Storage& s = *f->bits;
    std::unique_lock<std::mutex> lk(s.mu);
    if ((rc = storage_drain(s, lk))) return rc;
    if (s.host()) return host_resident("vbf_filter_insert_dev");
    uint64_t fresh = 0;
    if (n && f->k) {
        DEVICE_SCOPE(s.device);
        if ((rc = filter_insert_device(s, f, batch(keys, offsets, 0, stride, n, len_prefix), &fresh,
                                       (hipStream_t)stream)))
            return rc;
    }
    f->n.fetch_add((uint32_t)fresh);
    if (n_new) *n_new = fresh;
    return ok();
}

int vbf_filter_insert_host(vbf_filter* f, const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                           int len_prefix, uint64_t* n_new) {
    int rc = filter_insert_check(f, keys, offsets, stride, n, n_new);
    if (rc) return rc;
    if ((rc = offsets_ascend(offsets, n))) return rc;
    Storage& s = *f->bits;
    std::unique_lock<std::mutex> lk(s.mu);
    if ((rc = storage_drain(s, lk))) return rc;
    uint64_t fresh = 0;
    if (n && f->k) {
        if (s.host()) {
            fresh = host_insert(host_words(s), s.m, f->k, keys, offsets, stride, n, len_prefix != 0);
            if (fresh) s.pristine = false;
        } else {
            HOST_CALL(call, s.device);  // after the filter's lock and its drain
            KeyImage m;
            m.lay(offsets, stride, n);
            if ((rc = m.alloc(call, kWsFilterInsertIO)) || (rc = m.upload(call, keys, offsets, n))) return rc;
            if ((rc = filter_insert_device(s, f, batch(m.ptr(m.keys), m.ptr(m.off), 0, stride, n, len_prefix), &fresh,
                                           call.s)))
                return rc;
            if ((rc = call.finish())) return rc;
        }
    }
    f->n.fetch_add((uint32_t)fresh);
    if (n_new) *n_new = fresh;
    return ok();
}

// One batch of puts through to the SST's files: sort -> gather -> encode (-> the filter step), all
// on `device` from one upload.
int vbf_flush_write_host(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                         const uint32_t* val_offsets, const int64_t* created_ms, const uint8_t* tombstones,
                         vbf_filter* filter, uint8_t* data, uint64_t data_cap, uint64_t* data_len, uint8_t* index,
                         uint64_t index_cap, uint64_t* index_len, uint32_t* out_ids, uint64_t* n_out, int device) {
    if (!data_len || !index_len || !n_out) return fail(VBF_EINVAL, "data_len / index_len / n_out is NULL");
    *data_len = *index_len = *n_out = 0;
    if (n > 0x7FFFFFFFull) return fail(VBF_EINVAL, "too many entries (%llu > 2^31 - 1)", (unsigned long long)n);
    if (n == 0) return fail(VBF_EINVAL, "Cannot flush an empty table (flusher.rs:40-44, table.rs:262-264)");
    int rc = check_keys(keys, offsets, stride, n);
    if (rc || (rc = offsets_ascend(offsets, n))) return rc;
    if (!offsets && stride > 4079)
        return fail(VBF_EINVAL, "entry of %llu bytes exceeds a 4096-byte block (BlockIsFull)",
                    (unsigned long long)(stride + 17));
    const uint64_t kb = offsets ? offsets[n] - offsets[0] : n * stride;
    if (!keys && kb) return fail(VBF_EINVAL, "keys is NULL");
    if (n >= (1ull << 32) / 17 || kb >= (1ull << 32))
        return fail(VBF_EINVAL, "data.db reaches 2^32 bytes: index.db's u32 block offsets cannot address it");
    // lock order: the filter's, then the device's
    std::unique_lock<std::mutex> flk;
    if (filter) {
        Storage& fs = *filter->bits;
        if ((rc = filter_insert_check(filter, keys, offsets, stride, n, nullptr))) return rc;
        flk = std::unique_lock<std::mutex>(fs.mu);
        if ((rc = storage_drain(fs, flk))) return rc;
        if (fs.host())
            return fail(VBF_EINVAL, "vbf_flush_write_host: the filter is host-resident (VBF_DEVICE_HOST); a memtable's "
                                    "own host filter stays with its caller (pass NULL)");
        if (fs.device != device)
            return fail(VBF_EINVAL, "the filter lives on device %d, the flush runs on device %d", fs.device, device);
    }
    HOST_CALL(call, device);
    KeyImage m;  // keys | offsets | val | created | tombstones | ids
    m.lay(offsets, stride, n);
    const auto p_val = m.add<uint32_t>(n, val_offsets);
    const auto p_cr = m.add<int64_t>(n, created_ms);
    const auto p_tb = m.add<uint8_t>(n, tombstones);
    const auto p_ids = m.add<uint32_t>(n);
    if ((rc = m.alloc(call, kWsMemIO)) || (rc = m.upload(call, keys, offsets, n)) ||
        (rc = call.up(m.ptr(p_val), val_offsets, n)) || (rc = call.up(m.ptr(p_cr), created_ms, n)) ||
        (rc = call.up(m.ptr(p_tb), tombstones, n)))
        return rc;
    uint64_t nd = 0;
    const uint64_t* soff = nullptr;
    if ((rc = memtable_sort(m.ptr(m.keys), m.ptr(m.off), stride, n, m.ptr(p_ids), &nd, &soff, call.s))) return rc;
    // the table in key order in the encoder's layout, then its files; capacities that always suffice
    DevImage q;  // keys | offsets | created | tombstones | val | data.db | index.db
    const auto q_keys = q.add<uint8_t>(kb);
    const auto q_off = q.add<uint64_t>(nd + 1);
    const auto q_cr = q.add<int64_t>(nd, created_ms);
    const auto q_tb = q.add<uint8_t>(nd, tombstones);
    const auto q_val = q.add<uint32_t>(nd, val_offsets);
    const auto q_data = q.add<uint8_t>(kb + 17 * nd, data);
    const auto q_idx = q.add<uint8_t>(kb + 8 * nd, index);
    if ((rc = q.alloc(call, kWsMemOut))) return rc;
    uint64_t gkb = 0, nb = 0;
    if ((rc = gather_entries(m.ptr(m.keys), soff, m.ptr(p_cr), m.ptr(p_tb), m.ptr(p_val), m.ptr(p_ids), nd,
                             q.ptr(q_keys), kb, q.ptr(q_off), q.ptr(q_cr), q.ptr(q_tb), q.ptr(q_val), &gkb, call.s)))
        return rc;
    if ((rc = sst_encode(q.ptr(q_keys), q.ptr(q_off), 0, nd, q.ptr(q_val), q.ptr(q_cr), q.ptr(q_tb), q.ptr(q_data),
                         kb + 17 * nd, data_len, q.ptr(q_idx), kb + 8 * nd, index_len, nullptr, 0, &nb, call.s)))
        return rc;
    *n_out = nd;
    if (data && data_cap < *data_len)
        return fail(VBF_EINVAL, "data holds %llu < %llu bytes", (unsigned long long)data_cap,
                    (unsigned long long)*data_len);
    if (index && index_cap < *index_len)
        return fail(VBF_EINVAL, "index holds %llu < %llu bytes", (unsigned long long)index_cap,
                    (unsigned long long)*index_len);
    // MemTable::insert's filter step over every put, in arrival order (mem.rs:209-211)
    if (filter && filter->k) {
        uint64_t fresh = 0;
        if ((rc = filter_insert_device(*filter->bits, filter, batch(m.ptr(m.keys), m.ptr(m.off), 0, stride, n, 1), &fresh,
                                       call.s)))
            return rc;
        filter->n.fetch_add((uint32_t)fresh);
    }
    if ((rc = call.down(data, q.ptr(q_data), *data_len)) || (rc = call.down(index, q.ptr(q_idx), *index_len)) ||
        (rc = call.down(out_ids, m.ptr(p_ids), nd)))
        return rc;
    return call.finish();
}

}  // extern "C"

// ---- point lookups in SST tables ----

// A device-resident SST: the three file buffers (borrowed from the caller, or uploaded into
// `files`) and the side tables of vbf_table.hip in `side`.  Immutable once opened.
struct vbf_table {
    int device = 0;
    uint64_t entries = 0, nblocks = 0, data_len = 0, index_len = 0;
    void* files = nullptr;  // open_host: data | index | blocks
    void* side = nullptr;   // counts | pos | kpos | ebase
    vbf::TableDesc desc{};
    std::vector<uint8_t> smallest, biggest;  // KeyRange's two keys, read back at open
    ~vbf_table() {
        if (hip_forked() || (!files && !side)) return;  // a forked child: the parent's allocations
        int prev = -1;
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(device);
        if (files) (void)hipFree(files);
        if (side) (void)hipFree(side);
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

namespace {

// Builds and validates the side tables on the current device; two stream synchronisations (the
// walk's entry count, then the validation's error word with the key-range positions) and one
// more for the key-range bytes.
int table_open(vbf_table& t, const uint8_t* data, uint64_t data_len, const uint8_t* index, uint64_t index_len,
               const uint32_t* blocks, uint64_t nblocks, hipStream_t s) {
    t.data_len = data_len;
    t.index_len = index_len;
    t.nblocks = nblocks;
    if (!data_len && !nblocks) {
        if (index_len)
            return fail(VBF_EINVAL, "index.db of %llu bytes for an empty data.db", (unsigned long long)index_len);
        return VBF_OK;
    }
    if (data_len > 0xFFFFFFFFull)
        return fail(VBF_EINVAL, "data.db of %llu bytes: index.db's u32 block starts cannot address it",
                    (unsigned long long)data_len);
    vbf::SstArgs w;
    uint64_t n = 0;
    int rc = sst_count_pass(data, data_len, blocks, nblocks, s, &w, &n);
    if (rc) return rc;
    if (!index) return fail(VBF_EINVAL, "index is NULL");
    size_t tmpb = 0;
    HIP_TRY(vbf::scan_u64(nullptr, &tmpb, nullptr, nullptr, nblocks + 1, s));
    const uint64_t o_pos = align256(nblocks * 4), o_kpos = o_pos + align256(nblocks * 512);
    const uint64_t o_ebase = o_kpos + align256((nblocks + 1) * 8);
    HIP_TRY(hipMalloc(&t.side, o_ebase + align256((nblocks + 1) * 8)));
    char* sb = static_cast<char*>(t.side);
    uint32_t* counts = reinterpret_cast<uint32_t*>(sb);
    uint16_t* pos = reinterpret_cast<uint16_t*>(sb + o_pos);
    uint64_t* kpos = reinterpret_cast<uint64_t*>(sb + o_kpos);
    uint64_t* ebase = reinterpret_cast<uint64_t*>(sb + o_ebase);
    const uint64_t o_err = align256((nblocks + 1) * 8), o_tmp = o_err + 256;
    void* ws = nullptr;
    if ((rc = get_workspace(s, o_tmp + tmpb, &ws, kWsTableOpen))) return rc;
    uint64_t* reclen = static_cast<uint64_t*>(ws);
    uint32_t* err = reinterpret_cast<uint32_t*>(static_cast<char*>(ws) + o_err);
    HIP_TRY(hipMemcpyAsync(counts, w.counts, nblocks * 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(ebase, w.ebase, (nblocks + 1) * 8, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemsetAsync(reclen + nblocks, 0, 8, s));
    HIP_TRY(hipMemsetAsync(err, 0, 4, s));
    HIP_TRY(hipMemsetAsync(err + 1, 0xFF, 8, s));
    const vbf::TableOpenArgs a{data, data_len, index, index_len, blocks, nblocks, counts, w.pos, w.lmin, w.lmax,
                               w.ebase, pos, reclen, kpos, err};
    vbf::phase_begin(vbf::kPhaseTableOpen, s);
    HIP_TRY(vbf::table_fill(a, s));
    HIP_TRY(vbf::scan_u64(static_cast<char*>(ws) + o_tmp, &tmpb, reclen, kpos, nblocks + 1, s));
    HIP_TRY(vbf::table_check(a, s));
    vbf::phase_end(vbf::kPhaseTableOpen, s);
    uint32_t ev[3] = {0, 0, 0}, first_len = 0;
    uint64_t last_rec = 0;
    HIP_TRY(hipMemcpyAsync(ev, err, 12, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&last_rec, kpos + nblocks - 1, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&first_len, data, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (ev[0]) {
        const char* what = (ev[0] & vbf::kTabErrBig)        ? "block longer than 4096 bytes"
                           : (ev[0] & vbf::kTabErrDense)    ? "more than 256 entries in a block"
                           : (ev[0] & vbf::kTabErrOrder)    ? "keys not strictly increasing"
                           : (ev[0] & vbf::kTabErrIndexLen) ? "index.db is not one record per block (wrong length)"
                                                            : "index.db record differs from its block's last key / start";
        return fail(VBF_EINVAL, "table rejected at block %u, entry %u: %s", ev[1], ev[2], what);
    }
    t.entries = n;
    t.desc = vbf::TableDesc{data, index, blocks, counts, pos, kpos, ebase, nblocks};
    // smallest = the first entry's key, biggest = the last index record's key (key_range/range.rs)
    t.smallest.resize(first_len);
    t.biggest.resize(index_len - last_rec - 8);
    if (first_len) HIP_TRY(hipMemcpyAsync(t.smallest.data(), data + 4, first_len, hipMemcpyDeviceToHost, s));
    if (!t.biggest.empty())
        HIP_TRY(hipMemcpyAsync(t.biggest.data(), index + last_rec + 4, t.biggest.size(), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VBF_OK;
}

// The argument checks of vbf_table_get_* that need no HIP call.
int table_get_check(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n, uint32_t nsst,
                    const vbf_table* const* tables) {
    int rc = check_keys(keys, offsets, stride, n);
    if (rc) return rc;
    if (nsst && !tables) return fail(VBF_EINVAL, "tables is NULL");
    for (uint32_t i = 0; i < nsst; ++i) {
        if (!tables[i]) return fail(VBF_EINVAL, "tables[%u] is NULL", i);
        if (tables[i]->device != tables[0]->device)
            return fail(VBF_EINVAL, "tables[%u] lives on device %d, tables[0] on %d", i, tables[i]->device,
                        tables[0]->device);
    }
    return VBF_OK;
}

// The tables' descriptors in the caller's order, uploaded to the tables' device: one stream
// synchronisation (their source is pageable).
int table_descs(uint32_t nsst, const vbf_table* const* tables, hipStream_t s, const vbf::TableDesc** out) {
    std::vector<vbf::TableDesc> tab(nsst);
    for (uint32_t i = 0; i < nsst; ++i) tab[i] = tables[i]->desc;
    void* ws = nullptr;
    int rc = get_workspace(s, nsst * sizeof(vbf::TableDesc), &ws, kWsTableDesc);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(ws, tab.data(), nsst * sizeof(vbf::TableDesc), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    *out = static_cast<const vbf::TableDesc*>(ws);
    return VBF_OK;
}

// Device pointers, on the tables' device: the descriptors go up, then the lookup is queued on `s`.
int table_lookup(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n, uint32_t nsst,
                 const vbf_table* const* tables, const uint8_t* cand, uint8_t* found, uint32_t* table_idx,
                 uint32_t* val_offsets, uint64_t* created_ms, hipStream_t s) {
    const vbf::TableDesc* tab = nullptr;
    int rc = table_descs(nsst, tables, s, &tab);
    if (rc) return rc;
    const vbf::TableGetArgs a{keys, offsets, stride, n, nsst, tab, cand, found, table_idx, val_offsets, created_ms};
    vbf::phase_begin(vbf::kPhaseTableGet, s);
    HIP_TRY(vbf::table_get(a, s));
    vbf::phase_end(vbf::kPhaseTableGet, s);
    return VBF_OK;
}

int table_no_memory() { return fail(VBF_ENOMEM, "out of host memory"); }

// The tables' own key ranges in multi_probe's layout (smallest, biggest per table): the candidate
// cut of a lookup that is given filters.
void table_bounds(uint32_t nsst, const vbf_table* const* tables, std::vector<uint8_t>* bounds,
                  std::vector<uint64_t>* boff) {
    boff->assign(1, 0);
    for (uint32_t i = 0; i < nsst; ++i) {
        bounds->insert(bounds->end(), tables[i]->smallest.begin(), tables[i]->smallest.end());
        boff->push_back(bounds->size());
        bounds->insert(bounds->end(), tables[i]->biggest.begin(), tables[i]->biggest.end());
        boff->push_back(bounds->size());
    }
    bounds->push_back(0);  // never NULL
}

}  // namespace

extern "C" {

int vbf_table_open_dev(const uint8_t* data, uint64_t data_len, const uint8_t* index, uint64_t index_len,
                       const uint32_t* blocks, uint64_t nblocks, void* stream, vbf_table** out) {
    if (!out) return fail(VBF_EINVAL, "out is NULL");
    *out = nullptr;
    if ((data_len && !data) || (index_len && !index) || (nblocks && !blocks))
        return fail(VBF_EINVAL, "NULL argument");
    FORK_GUARD();
    try {
        std::unique_ptr<vbf_table> t(new (std::nothrow) vbf_table());
        if (!t) return table_no_memory();
        HIP_TRY(hipGetDevice(&t->device));
        int rc = table_open(*t, data, data_len, index, index_len, blocks, nblocks, (hipStream_t)stream);
        if (rc) return rc;
        *out = t.release();
    } catch (const std::bad_alloc&) {
        return table_no_memory();
    }
    return ok();
}

int vbf_table_open_host(const uint8_t* data, uint64_t data_len, const uint8_t* index, uint64_t index_len, int device,
                        vbf_table** out) {
    if (!out) return fail(VBF_EINVAL, "out is NULL");
    *out = nullptr;
    if ((data_len && !data) || (index_len && !index)) return fail(VBF_EINVAL, "NULL argument");
    try {
        std::vector<uint32_t> blk;
        int rc = parse_index(index, index_len, &blk);
        if (rc) return rc;
        std::unique_ptr<vbf_table> t(new (std::nothrow) vbf_table());
        if (!t) return table_no_memory();
        HOST_CALL(call, device);
        t->device = device;
        DevImage img;  // data | index | blocks, owned by the handle
        const auto p_data = img.add<uint8_t>(data_len, data_len);
        const auto p_idx = img.add<uint8_t>(index_len, index_len);
        const auto p_blk = img.add<uint32_t>(blk.size(), !blk.empty());
        if (data_len || index_len) {
            HIP_TRY(hipMalloc(&t->files, img.bytes));
            img.base = t->files;
            if ((rc = call.up(img.ptr(p_data), data, data_len)) || (rc = call.up(img.ptr(p_idx), index, index_len)) ||
                (rc = call.up(img.ptr(p_blk), blk.data(), blk.size())) || (rc = call.sync()))  // pageable sources
                return rc;
        }
        if ((rc = table_open(*t, img.ptr(p_data), data_len, img.ptr(p_idx), index_len, img.ptr(p_blk), blk.size(),
                             call.s)))
            return rc;
        call.settled();  // table_open returned synchronised
        *out = t.release();
    } catch (const std::bad_alloc&) {
        return table_no_memory();
    }
    return ok();
}

void vbf_table_free(vbf_table* t) { delete t; }
uint64_t vbf_table_entries(const vbf_table* t) { return t ? t->entries : 0; }
uint64_t vbf_table_blocks(const vbf_table* t) { return t ? t->nblocks : 0; }
int vbf_table_device(const vbf_table* t) { return t ? t->device : VBF_DEVICE_HOST; }

int vbf_table_key_range(const vbf_table* t, uint8_t* smallest, uint64_t scap, uint64_t* slen, uint8_t* biggest,
                        uint64_t bcap, uint64_t* blen) {
    if (!t || !slen || !blen) return fail(VBF_EINVAL, "NULL argument");
    *slen = t->smallest.size();
    *blen = t->biggest.size();
    if ((smallest && scap < *slen) || (biggest && bcap < *blen))
        return fail(VBF_EINVAL, "key buffers hold %llu / %llu < %llu / %llu bytes", (unsigned long long)scap,
                    (unsigned long long)bcap, (unsigned long long)*slen, (unsigned long long)*blen);
    if (smallest && *slen) memcpy(smallest, t->smallest.data(), *slen);
    if (biggest && *blen) memcpy(biggest, t->biggest.data(), *blen);
    return ok();
}

int vbf_table_get_dev(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n, uint32_t nsst,
                      const vbf_table* const* tables, const uint8_t* cand, uint8_t* found, uint32_t* table_idx,
                      uint32_t* val_offsets, uint64_t* created_ms, void* stream) {
    int rc = table_get_check(keys, offsets, stride, n, nsst, tables);
    if (rc) return rc;
    if (!n) return ok();
    FORK_GUARD();
    hipStream_t s = (hipStream_t)stream;
    if (!nsst) {  // no table: nothing to look up, every output is zero
        if (found) HIP_TRY(hipMemsetAsync(found, 0, n, s));
        if (table_idx) HIP_TRY(hipMemsetAsync(table_idx, 0, n * 4, s));
        if (val_offsets) HIP_TRY(hipMemsetAsync(val_offsets, 0, n * 4, s));
        if (created_ms) HIP_TRY(hipMemsetAsync(created_ms, 0, n * 8, s));
        return ok();
    }
    try {
        DEVICE_SCOPE(tables[0]->device);
        if ((rc = table_lookup(keys, offsets, stride, n, nsst, tables, cand, found, table_idx, val_offsets,
                               created_ms, s)))
            return rc;
    } catch (const std::bad_alloc&) {
        return table_no_memory();
    }
    return ok();
}

int vbf_table_get_host(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n, uint32_t nsst,
                       const vbf_table* const* tables, const vbf_filter* const* filters, uint8_t* found,
                       uint32_t* table_idx, uint32_t* val_offsets, uint64_t* created_ms) {
    int rc = table_get_check(keys, offsets, stride, n, nsst, tables);
    if (rc) return rc;
    if (!n) return ok();
    if (!nsst) {
        if (found) memset(found, 0, n);
        if (table_idx) memset(table_idx, 0, n * 4);
        if (val_offsets) memset(val_offsets, 0, n * 4);
        if (created_ms) memset(created_ms, 0, n * 8);
        return ok();
    }
    const int device = tables[0]->device;
    if (filters)
        for (uint32_t i = 0; i < nsst; ++i)
            if (!filters[i]) return fail(VBF_EINVAL, "filters[%u] is NULL", i);
    try {
        // Lock order: the filters' locks and their drain (which waits for a device's worker) come
        // first, then the device's host-call lock -- as vbf_multi_probe_host and
        // vbf_filter_rebuild_from_sst_host take them.  Staging the keys before the filter locks, as
        // this call once did, would hold the device while waiting for a filter whose holder waits
        // for the device.
        MultiLock lk(filters, filters ? nsst : 0);
        if ((rc = lk.drain())) return rc;
        if (filters)
            for (uint32_t i = 0; i < nsst; ++i)
                if (filters[i]->bits->device != device)
                    return fail(VBF_EINVAL, "filters[%u] lives on device %d, the tables on %d", i,
                                filters[i]->bits->device, device);
        HOST_CALL(call, device);
        const uint64_t k0 = offsets ? offsets[0] : 0, kbytes = offsets ? offsets[n] - k0 : n * stride;
        DevImage img;  // keys | offsets | candidates | found | table_idx | val_offsets | created
        const auto p_keys = img.add<uint8_t>(kbytes);
        const auto p_off = img.add<uint64_t>(n + 1, offsets);
        const auto p_cand = img.add<uint8_t>(n * nsst, filters);
        const auto p_found = img.add<uint8_t>(n, found);
        const auto p_idx = img.add<uint32_t>(n, table_idx);
        const auto p_val = img.add<uint32_t>(n, val_offsets);
        const auto p_cr = img.add<uint64_t>(n, created_ms);
        if ((rc = img.alloc(call, kWsTableIO))) return rc;
        uint8_t* d_keys = img.ptr(p_keys);
        uint64_t* d_off = img.ptr(p_off);
        uint8_t* d_cand = img.ptr(p_cand);
        if ((rc = call.up(d_keys, kbytes ? keys + k0 : nullptr, kbytes))) return rc;
        // absolute positions in the device copy
        if (offsets && ((rc = call.up_rebased(d_off, offsets, n + 1)) || (rc = call.sync()))) return rc;
        if (filters) {  // filter_sstables_by_key_range (range.rs:91-147) with the tables' own key ranges
            std::vector<uint8_t> bounds;
            std::vector<uint64_t> boff;
            table_bounds(nsst, tables, &bounds, &boff);
            if ((rc = multi_probe(d_keys, d_off, stride, n, 1, nsst, filters, bounds.data(), boff.data(), d_cand, call.s)))
                return rc;
        }
        if ((rc = table_lookup(d_keys, d_off, stride, n, nsst, tables, d_cand, img.ptr(p_found), img.ptr(p_idx),
                               img.ptr(p_val), img.ptr(p_cr), call.s)))
            return rc;
        if ((rc = call.down(found, img.ptr(p_found), n)) || (rc = call.down(table_idx, img.ptr(p_idx), n)) ||
            (rc = call.down(val_offsets, img.ptr(p_val), n)) || (rc = call.down(created_ms, img.ptr(p_cr), n)) ||
            (rc = call.finish()))
            return rc;
    } catch (const std::bad_alloc&) {
        return table_no_memory();
    }
    return ok();
}

}  // extern "C"

// ---- batched range scans over open tables (DataStore::seek's key side) ----

namespace {

// The argument checks of vbf_table_scan_* that need no HIP call.
int table_scan_check(const uint8_t* bounds, const uint64_t* bounds_off, uint64_t nranges, uint32_t nsst,
                     const vbf_table* const* tables, uint32_t flags, uint64_t* n_out, uint64_t* key_bytes) {
    if (!n_out || !key_bytes) return fail(VBF_EINVAL, "n_out or key_bytes is NULL");
    *n_out = 0;
    *key_bytes = 0;
    if (flags & ~(uint32_t)(VBF_SCAN_KEEP_TOMBSTONES | VBF_SCAN_END_EXCLUSIVE))
        return fail(VBF_EINVAL, "unknown flag bits 0x%x", flags);
    if (nsst && !tables) return fail(VBF_EINVAL, "tables is NULL");
    for (uint32_t i = 0; i < nsst; ++i) {
        if (!tables[i]) return fail(VBF_EINVAL, "tables[%u] is NULL", i);
        if (tables[i]->device != tables[0]->device)
            return fail(VBF_EINVAL, "tables[%u] lives on device %d, tables[0] on %d", i, tables[i]->device,
                        tables[0]->device);
    }
    if (nranges && !bounds_off) return fail(VBF_EINVAL, "bounds_off is NULL");
    if (nranges && !bounds) return fail(VBF_EINVAL, "bounds is NULL");
    // the (range, table) pairs are scanned like the candidates: below 2^31 items
    if (nsst && nranges > 0x7FFFFFFEull / nsst)
        return fail(VBF_EINVAL, "too many entries: %llu ranges x %u tables", (unsigned long long)nranges, nsst);
    return VBF_OK;
}

struct ScanOut {
    uint64_t* range_off;
    uint8_t* keys;
    uint64_t* key_off;
    uint32_t* table_idx;
    uint32_t* val_offsets;
    uint64_t* created_ms;
    uint8_t* tombstones;
    bool per_entry() const { return key_off || table_idx || val_offsets || created_ms || tombstones; }
    bool any() const { return range_off || keys || per_entry(); }
};

// The capacity rule of the sizing protocol (the encoder's convention): too small is VBF_EINVAL
// with the sizes written and no output touched.
int table_scan_caps(const ScanOut& o, uint64_t entries_cap, uint64_t keys_cap, uint64_t n_out, uint64_t key_bytes) {
    if (o.per_entry() && entries_cap < n_out)
        return fail(VBF_EINVAL, "entries_cap %llu < %llu listed entries", (unsigned long long)entries_cap,
                    (unsigned long long)n_out);
    if (o.keys && keys_cap < key_bytes)
        return fail(VBF_EINVAL, "keys_cap %llu < %llu key bytes", (unsigned long long)keys_cap,
                    (unsigned long long)key_bytes);
    return VBF_OK;
}

// Bounds pass, rank pass and the two scans on the tables' device (bounds / bounds_off there):
// everything the sizes need.  Three stream synchronisations: the descriptors' upload, the candidate
// total, then *n_out and *key_bytes.  `a` comes back ready for table_scan_fill.
// Workspace: 40 bytes per candidate (slot -> table and entry start, listed flag and key length as
// u64 for scan_u64, their two scans) and 24 per (range, table) pair, plus the scans' scratch.
int table_scan_sizes(const uint8_t* bounds, const uint64_t* bounds_off, uint64_t nranges, uint32_t nsst,
                     const vbf_table* const* tables, uint32_t flags, hipStream_t s, vbf::TableScanArgs* a,
                     uint64_t* n_out, uint64_t* key_bytes) {
    *a = vbf::TableScanArgs{};
    a->bounds = bounds;
    a->bounds_off = bounds_off;
    a->nranges = nranges;
    a->nsst = nsst;
    a->flags = flags;
    int rc = table_descs(nsst, tables, s, &a->tab);
    if (rc) return rc;
    const uint64_t P = nranges * nsst;
    size_t tmpb = 0;
    HIP_TRY(vbf::scan_u64(nullptr, &tmpb, nullptr, nullptr, P + 1, s));
    const uint64_t o_cnt = align256(P * 8), o_cbase = o_cnt + align256((P + 1) * 8);
    const uint64_t o_err = o_cbase + align256((P + 1) * 8), o_tmp = o_err + 256;
    void* ws = nullptr;
    if ((rc = get_workspace(s, o_tmp + tmpb, &ws, kWsTableScanPairs))) return rc;
    char* pb = static_cast<char*>(ws);
    a->first = reinterpret_cast<uint64_t*>(pb);
    a->cnt = reinterpret_cast<uint64_t*>(pb + o_cnt);
    uint64_t* cbase = reinterpret_cast<uint64_t*>(pb + o_cbase);
    a->cbase = cbase;
    a->err = reinterpret_cast<uint32_t*>(pb + o_err);
    HIP_TRY(hipMemsetAsync(a->cnt + P, 0, 8, s));
    HIP_TRY(hipMemsetAsync(a->err, 0, 4, s));
    vbf::phase_begin(vbf::kPhaseScanRank, s);
    HIP_TRY(vbf::table_scan_bounds(*a, s));
    HIP_TRY(vbf::scan_u64(pb + o_tmp, &tmpb, a->cnt, cbase, P + 1, s));
    vbf::phase_end(vbf::kPhaseScanRank, s);
    uint64_t total = 0;
    uint32_t ev = 0;
    HIP_TRY(hipMemcpyAsync(&total, cbase + P, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&ev, a->err, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (ev & vbf::kScanErrBounds) return fail(VBF_EINVAL, "bounds_off is not nondecreasing");
    if (total > 0x7FFFFFFFull)
        return fail(VBF_EINVAL, "too many entries: %llu candidates in the ranges (limit 2^31 - 1)",
                    (unsigned long long)total);
    a->total = total;
    size_t tmpc = 0;
    HIP_TRY(vbf::scan_u64(nullptr, &tmpc, nullptr, nullptr, total + 1, s));
    const uint64_t q_pos = align256(total * 4), q_keep = q_pos + align256(total * 4);
    const uint64_t q_len = q_keep + (total + 1) * 8, q_opos = align256(q_len + (total + 1) * 8);
    const uint64_t q_kofs = q_opos + align256((total + 1) * 8), q_tmp = q_kofs + align256((total + 1) * 8);
    if ((rc = get_workspace(s, q_tmp + tmpc, &ws, kWsTableScan))) return rc;
    char* cb = static_cast<char*>(ws);
    a->m_table = reinterpret_cast<uint32_t*>(cb);
    a->m_pos = reinterpret_cast<uint32_t*>(cb + q_pos);
    a->m_keep = reinterpret_cast<uint64_t*>(cb + q_keep);
    a->m_len = reinterpret_cast<uint64_t*>(cb + q_len);
    uint64_t* opos = reinterpret_cast<uint64_t*>(cb + q_opos);
    uint64_t* kofs = reinterpret_cast<uint64_t*>(cb + q_kofs);
    a->opos = opos;
    a->kofs = kofs;
    HIP_TRY(hipMemsetAsync(a->m_keep, 0, (total + 1) * 16, s));  // m_keep | m_len
    vbf::phase_begin(vbf::kPhaseScanRank, s);
    HIP_TRY(vbf::table_scan_rank(*a, s));
    HIP_TRY(vbf::scan_u64(cb + q_tmp, &tmpc, a->m_keep, opos, total + 1, s));
    HIP_TRY(vbf::scan_u64(cb + q_tmp, &tmpc, a->m_len, kofs, total + 1, s));
    vbf::phase_end(vbf::kPhaseScanRank, s);
    HIP_TRY(hipMemcpyAsync(n_out, opos + total, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(key_bytes, kofs + total, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&ev, a->err, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (ev & vbf::kScanErrRank) {
        *n_out = *key_bytes = 0;
        return fail(VBF_EINVAL, "a merged rank fell outside its range: the tables' buffers changed since open");
    }
    return VBF_OK;
}

// The output passes, queued on `s` (device pointers; each may be NULL).
int table_scan_fill(vbf::TableScanArgs a, const ScanOut& o, hipStream_t s) {
    a.range_off = o.range_off;
    a.keys = o.keys;
    a.key_off = o.key_off;
    a.table_idx = o.table_idx;
    a.val_off = o.val_offsets;
    a.created = o.created_ms;
    a.tomb = o.tombstones;
    vbf::phase_begin(vbf::kPhaseScanEmit, s);
    HIP_TRY(vbf::table_scan_emit(a, s));
    HIP_TRY(vbf::table_scan_keys(a, s));
    vbf::phase_end(vbf::kPhaseScanEmit, s);
    return VBF_OK;
}

}  // namespace

extern "C" {

int vbf_table_scan_dev(const uint8_t* bounds, const uint64_t* bounds_off, uint64_t nranges, uint32_t nsst,
                       const vbf_table* const* tables, uint32_t flags, uint64_t* range_off, uint8_t* keys,
                       uint64_t keys_cap, uint64_t* key_off, uint32_t* table_idx, uint32_t* val_offsets,
                       uint64_t* created_ms, uint8_t* tombstones, uint64_t entries_cap, uint64_t* n_out,
                       uint64_t* key_bytes, void* stream) {
    int rc = table_scan_check(bounds, bounds_off, nranges, nsst, tables, flags, n_out, key_bytes);
    if (rc) return rc;
    if (!nranges) return ok();
    FORK_GUARD();
    hipStream_t s = (hipStream_t)stream;
    const ScanOut o{range_off, keys, key_off, table_idx, val_offsets, created_ms, tombstones};
    if (!nsst) {  // no table: every range is empty
        if (range_off) HIP_TRY(hipMemsetAsync(range_off, 0, (nranges + 1) * 8, s));
        if (key_off) HIP_TRY(hipMemsetAsync(key_off, 0, 8, s));
        return ok();
    }
    try {
        DEVICE_SCOPE(tables[0]->device);
        vbf::TableScanArgs a;
        if ((rc = table_scan_sizes(bounds, bounds_off, nranges, nsst, tables, flags, s, &a, n_out, key_bytes)))
            return rc;
        if ((rc = table_scan_caps(o, entries_cap, keys_cap, *n_out, *key_bytes))) return rc;
        if (o.any() && (rc = table_scan_fill(a, o, s))) return rc;
    } catch (const std::bad_alloc&) {
        return table_no_memory();
    }
    return ok();
}

int vbf_table_scan_host(const uint8_t* bounds, const uint64_t* bounds_off, uint64_t nranges, uint32_t nsst,
                        const vbf_table* const* tables, uint32_t flags, uint64_t* range_off, uint8_t* keys,
                        uint64_t keys_cap, uint64_t* key_off, uint32_t* table_idx, uint32_t* val_offsets,
                        uint64_t* created_ms, uint8_t* tombstones, uint64_t entries_cap, uint64_t* n_out,
                        uint64_t* key_bytes) {
    int rc = table_scan_check(bounds, bounds_off, nranges, nsst, tables, flags, n_out, key_bytes);
    if (rc) return rc;
    for (uint64_t i = 0; i < 2 * nranges; ++i)
        if (bounds_off[i] > bounds_off[i + 1])
            return fail(VBF_EINVAL, "bounds_off decreases at entry %llu", (unsigned long long)(i + 1));
    const ScanOut o{range_off, keys, key_off, table_idx, val_offsets, created_ms, tombstones};
    if (!nranges || !nsst) {  // nothing to scan: every range is empty, no device work
        if (range_off) memset(range_off, 0, (nranges + 1) * 8);
        if (key_off) key_off[0] = 0;
        return ok();
    }
    const int device = tables[0]->device;
    try {
        HOST_CALL(call, device);
        // bounds and their offsets, rebased to positions in the device copy
        const uint64_t b0 = bounds_off[0], bbytes = bounds_off[2 * nranges] - b0;
        DevImage in;
        const auto p_bounds = in.add<uint8_t>(bbytes);
        const auto p_boff = in.add<uint64_t>(2 * nranges + 1);
        if ((rc = in.alloc(call, kWsTableScanIO))) return rc;
        if ((rc = call.up(in.ptr(p_bounds), bbytes ? bounds + b0 : nullptr, bbytes)) ||
            (rc = call.up_rebased(in.ptr(p_boff), bounds_off, 2 * nranges + 1)) || (rc = call.sync()))  // pageable sources
            return rc;
        vbf::TableScanArgs a;
        if ((rc = table_scan_sizes(in.ptr(p_bounds), in.ptr(p_boff), nranges, nsst, tables, flags, call.s, &a,
                                   n_out, key_bytes)))
            return rc;
        if ((rc = table_scan_caps(o, entries_cap, keys_cap, *n_out, *key_bytes))) return rc;
        if (!o.any()) {  // the size query: table_scan_sizes returned synchronised
            call.settled();
            return ok();
        }
        // the outputs' device staging; the bounds (same slot) were consumed before the sizes came back
        const uint64_t n = *n_out, kb = *key_bytes;
        DevImage out;
        const auto p_roff = out.add<uint64_t>(nranges + 1, range_off);
        const auto p_koff = out.add<uint64_t>(n + 1, key_off);
        const auto p_cr = out.add<uint64_t>(n, created_ms);
        const auto p_idx = out.add<uint32_t>(n, table_idx);
        const auto p_val = out.add<uint32_t>(n, val_offsets);
        const auto p_tomb = out.add<uint8_t>(n, tombstones);
        const auto p_keys = out.add<uint8_t>(kb, keys);
        if ((rc = out.alloc(call, kWsTableScanIO))) return rc;
        const ScanOut d{out.ptr(p_roff), out.ptr(p_keys), out.ptr(p_koff), out.ptr(p_idx),
                        out.ptr(p_val),  out.ptr(p_cr),   out.ptr(p_tomb)};
        if ((rc = table_scan_fill(a, d, call.s))) return rc;
        if ((rc = call.down(range_off, d.range_off, nranges + 1)) || (rc = call.down(key_off, d.key_off, n + 1)) ||
            (rc = call.down(keys, d.keys, kb)) || (rc = call.down(table_idx, d.table_idx, n)) ||
            (rc = call.down(val_offsets, d.val_offsets, n)) || (rc = call.down(created_ms, d.created_ms, n)) ||
            (rc = call.down(tombstones, d.tombstones, n)) || (rc = call.finish()))
            return rc;
    } catch (const std::bad_alloc&) {
        return table_no_memory();
    }
    return ok();
}

}  // extern "C"

// ---- value-log reads and appends (ValueLog::get / ValueLog::append) ----

// A device-resident window of the value log: the file's bytes [base, base + len), borrowed from the
// caller or uploaded into `owned`.  Immutable once opened; the log has no index, so nothing is parsed.
struct vbf_vlog {
    int device = 0;
    uint64_t len = 0, base = 0;
    const uint8_t* bytes = nullptr;
    void* owned = nullptr;
    ~vbf_vlog() {
        if (!owned || hip_forked()) return;  // a forked child: the parent's allocation
        int prev = -1;
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(device);
        (void)hipFree(owned);
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

namespace {

int vlog_open_check(const uint8_t* bytes, uint64_t len, uint64_t base, vbf_vlog** out) {
    if (!out) return fail(VBF_EINVAL, "out is NULL");
    *out = nullptr;
    if (len && !bytes) return fail(VBF_EINVAL, "bytes is NULL");
    if (base + len < base)
        return fail(VBF_EINVAL, "base %llu + len %llu wraps", (unsigned long long)base, (unsigned long long)len);
    return VBF_OK;
}

// The argument checks of vbf_vlog_get_* that need no HIP call.
int vlog_get_check(const vbf_vlog* v, const uint32_t* val_offsets, uint64_t n, uint64_t* value_bytes) {
    if (!value_bytes) return fail(VBF_EINVAL, "value_bytes is NULL");
    *value_bytes = 0;
    if (!v) return fail(VBF_EINVAL, "vlog is NULL");
    if (n && !val_offsets) return fail(VBF_EINVAL, "val_offsets is NULL");
    if (n > 0x7FFFFFFEull)  // the lengths' scan runs over n + 1 items
        return fail(VBF_EINVAL, "too many items: %llu (limit 2^31 - 2)", (unsigned long long)n);
    return VBF_OK;
}

// Sizes pass and scan on the log's device (every pointer there): status, lengths and positions into
// the stream's workspace, the byte total read back (one stream synchronisation).  `a` comes back
// ready for vlog_get_fill.  Workspace: 25 bytes per item plus the scan's scratch.
int vlog_get_sizes(const vbf_vlog* v, const uint32_t* val_offsets, const uint8_t* found, uint64_t n,
                   const uint8_t* keys, const uint64_t* offsets, uint64_t stride, hipStream_t s, vbf::VlogGetArgs* a,
                   uint64_t* total) {
    *a = vbf::VlogGetArgs{};
    a->bytes = v->bytes;
    a->len = v->len;
    a->base = v->base;
    a->val_offsets = val_offsets;
    a->found = found;
    a->n = n;
    a->keys = keys;
    a->offsets = keys ? offsets : nullptr;
    a->stride = stride;
    size_t tmpb = 0;
    HIP_TRY(vbf::scan_u64(nullptr, &tmpb, nullptr, nullptr, n + 1, s));
    const uint64_t o_len = align256(n), o_voff = o_len + align256((n + 1) * 8);
    const uint64_t o_src = o_voff + align256((n + 1) * 8), o_tmp = o_src + align256(n * 8);
    void* ws = nullptr;
    int rc = get_workspace(s, o_tmp + tmpb, &ws, kWsVlog);
    if (rc) return rc;
    char* b = static_cast<char*>(ws);
    a->status = reinterpret_cast<uint8_t*>(b);
    a->vlen = reinterpret_cast<uint64_t*>(b + o_len);
    uint64_t* voff = reinterpret_cast<uint64_t*>(b + o_voff);
    a->voff = voff;
    a->src = reinterpret_cast<uint64_t*>(b + o_src);
    HIP_TRY(hipMemsetAsync(a->vlen + n, 0, 8, s));
    vbf::phase_begin(vbf::kPhaseVlogSizes, s);
    HIP_TRY(vbf::vlog_sizes(*a, s));
    HIP_TRY(vbf::scan_u64(b + o_tmp, &tmpb, a->vlen, voff, n + 1, s));
    vbf::phase_end(vbf::kPhaseVlogSizes, s);
    HIP_TRY(hipMemcpyAsync(total, voff + n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    a->total = *total;
    return VBF_OK;
}

int vlog_values_cap(const uint8_t* values, uint64_t values_cap, uint64_t total) {
    if (values && values_cap < total)
        return fail(VBF_EINVAL, "values_cap %llu < %llu value bytes", (unsigned long long)values_cap,
                    (unsigned long long)total);
    return VBF_OK;
}

// The copy pass, queued on `s` (values on the device).
int vlog_get_fill(vbf::VlogGetArgs a, uint8_t* values, hipStream_t s) {
    a.values = values;
    vbf::phase_begin(vbf::kPhaseVlogCopy, s);
    HIP_TRY(vbf::vlog_copy(a, s));
    vbf::phase_end(vbf::kPhaseVlogCopy, s);
    return VBF_OK;
}

constexpr uint64_t kVlogMaxOffset = 1ull << 32;  // data.db stores the value offset as u32

// The argument checks of vbf_vlog_encode_* that need no HIP call.
int vlog_enc_check_args(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                        const uint64_t* value_off, uint64_t base, uint64_t* out_len) {
    if (!out_len) return fail(VBF_EINVAL, "out_len is NULL");
    *out_len = 0;
    if (!n) return VBF_OK;
    if (!value_off) return fail(VBF_EINVAL, "value_off is NULL");
    if (!keys && !offsets && stride) return fail(VBF_EINVAL, "keys is NULL");
    if (!offsets && stride > 0xFFFFFFFFull)
        return fail(VBF_EINVAL, "key of %llu bytes: key_len is a u32", (unsigned long long)stride);
    // an entry is at least its 17-byte header: decidable before the lengths are known
    if (n > kVlogMaxOffset / 17 + 1 || base + 17 * (n - 1) >= kVlogMaxOffset)
        return fail(VBF_EINVAL, "entry %llu would start at or beyond 2^32: data.db's u32 value offset cannot address it",
                    (unsigned long long)(base >= kVlogMaxOffset ? 0 : (kVlogMaxOffset - base + 16) / 17));
    return VBF_OK;
}

// The append's sizes from the first, the last-but-one and the last entry of both offset arrays
// (ko / vo = {[0], [n - 1], [n]}): total bytes, the last entry's start against the 2^32 limit, the
// capacity rule (too small: VBF_EINVAL with *out_len written and nothing else).
int vlog_enc_plan(vbf::VlogEncArgs* a, const uint64_t ko[3], const uint64_t vo[3], const uint8_t* out,
                  uint64_t out_cap, uint64_t* out_len) {
    const uint64_t n = a->n;
    a->k0 = ko[0];
    a->v0 = vo[0];
    a->k_end = ko[2];
    a->v_end = vo[2];
    a->total = 17 * n + (ko[2] - ko[0]) + (vo[2] - vo[0]);
    const uint64_t last = a->base + 17 * (n - 1) + (ko[1] - ko[0]) + (vo[1] - vo[0]);
    if (last >= kVlogMaxOffset)
        return fail(VBF_EINVAL, "the last entry would start at %llu, at or beyond 2^32: data.db's u32 value offset "
                    "cannot address it", (unsigned long long)last);
    if (!a->keys && ko[2] > ko[0]) return fail(VBF_EINVAL, "keys is NULL");
    if (!a->values && vo[2] > vo[0]) return fail(VBF_EINVAL, "values is NULL");
    *out_len = a->total;
    if (out && out_cap < a->total)
        return fail(VBF_EINVAL, "out_cap %llu < %llu log bytes", (unsigned long long)out_cap,
                    (unsigned long long)a->total);
    return VBF_OK;
}

int vlog_enc_emit(const vbf::VlogEncArgs& a, hipStream_t s) {
    vbf::phase_begin(vbf::kPhaseVlogEncode, s);
    HIP_TRY(vbf::vlog_encode(a, s));
    vbf::phase_end(vbf::kPhaseVlogEncode, s);
    return VBF_OK;
}

}  // namespace

extern "C" {

int vbf_vlog_open_dev(const uint8_t* bytes, uint64_t len, uint64_t base, vbf_vlog** out) {
    int rc = vlog_open_check(bytes, len, base, out);
    if (rc) return rc;
    FORK_GUARD();
    std::unique_ptr<vbf_vlog> v(new (std::nothrow) vbf_vlog());
    if (!v) return table_no_memory();
    HIP_TRY(hipGetDevice(&v->device));
    v->len = len;
    v->base = base;
    v->bytes = len ? bytes : nullptr;
    *out = v.release();
    return ok();
}

int vbf_vlog_open_host(const uint8_t* bytes, uint64_t len, uint64_t base, int device, vbf_vlog** out) {
    int rc = vlog_open_check(bytes, len, base, out);
    if (rc) return rc;
    std::unique_ptr<vbf_vlog> v(new (std::nothrow) vbf_vlog());
    if (!v) return table_no_memory();
    HOST_CALL(call, device);
    v->device = device;
    v->len = len;
    v->base = base;
    if (len) {
        HIP_TRY(hipMalloc(&v->owned, len));
        if ((rc = call.up(static_cast<uint8_t*>(v->owned), bytes, len)) || (rc = call.sync())) return rc;  // a pageable source
        v->bytes = static_cast<const uint8_t*>(v->owned);
    }
    call.settled();
    *out = v.release();
    return ok();
}

void vbf_vlog_free(vbf_vlog* v) { delete v; }
uint64_t vbf_vlog_bytes(const vbf_vlog* v) { return v ? v->len : 0; }
uint64_t vbf_vlog_base(const vbf_vlog* v) { return v ? v->base : 0; }
int vbf_vlog_device(const vbf_vlog* v) { return v ? v->device : VBF_DEVICE_HOST; }

int vbf_vlog_get_dev(const vbf_vlog* v, const uint32_t* val_offsets, const uint8_t* found, uint64_t n,
                     const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint8_t* status, uint8_t* values,
                     uint64_t values_cap, uint64_t* value_off, uint64_t* value_bytes, void* stream) {
    int rc = vlog_get_check(v, val_offsets, n, value_bytes);
    if (rc) return rc;
    if (!n) return ok();
    FORK_GUARD();
    hipStream_t s = (hipStream_t)stream;
    int cur = -1;
    HIP_TRY(hipGetDevice(&cur));
    if (cur != v->device)
        return fail(VBF_EINVAL, "the log lives on device %d, the current device is %d", v->device, cur);
    vbf::VlogGetArgs a;
    uint64_t total = 0;
    if ((rc = vlog_get_sizes(v, val_offsets, found, n, keys, offsets, stride, s, &a, &total))) return rc;
    *value_bytes = total;
    if ((rc = vlog_values_cap(values, values_cap, total))) return rc;
    if (status) HIP_TRY(hipMemcpyAsync(status, a.status, n, hipMemcpyDeviceToDevice, s));
    if (value_off) HIP_TRY(hipMemcpyAsync(value_off, a.voff, (n + 1) * 8, hipMemcpyDeviceToDevice, s));
    if (values && (rc = vlog_get_fill(a, values, s))) return rc;
    return ok();
}

int vbf_vlog_get_host(const vbf_vlog* v, const uint32_t* val_offsets, const uint8_t* found, uint64_t n,
                      const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint8_t* status, uint8_t* values,
                      uint64_t values_cap, uint64_t* value_off, uint64_t* value_bytes) {
    int rc = vlog_get_check(v, val_offsets, n, value_bytes);
    if (rc) return rc;
    if (keys && offsets)
        for (uint64_t j = 0; j < n; ++j)
            if (offsets[j] > offsets[j + 1])
                return fail(VBF_EINVAL, "offsets descend at key %llu", (unsigned long long)j);
    if (!n) {
        if (value_off) value_off[0] = 0;
        return ok();
    }
    try {
        HOST_CALL(call, v->device);
        const uint64_t k0 = keys && offsets ? offsets[0] : 0;
        const uint64_t kb = !keys ? 0 : (offsets ? offsets[n] - k0 : n * stride);
        DevImage img;  // val_offsets | found | keys | offsets
        const auto p_vo = img.add<uint32_t>(n);
        const auto p_found = img.add<uint8_t>(n, found);
        const auto p_keys = img.add<uint8_t>(kb + 1, keys);
        const auto p_off = img.add<uint64_t>(n + 1, keys && offsets);
        if ((rc = img.alloc(call, kWsVlogIO))) return rc;
        if ((rc = call.up(img.ptr(p_vo), val_offsets, n)) || (rc = call.up(img.ptr(p_found), found, n)) ||
            (rc = call.up(img.ptr(p_keys), kb ? keys + k0 : nullptr, kb)))
            return rc;
        // positions in the device copy
        if (p_off.present && (rc = call.up_rebased(img.ptr(p_off), offsets, n + 1))) return rc;
        vbf::VlogGetArgs a;
        uint64_t total = 0;
        if ((rc = vlog_get_sizes(v, img.ptr(p_vo), img.ptr(p_found), n, img.ptr(p_keys), img.ptr(p_off), stride,
                                 call.s, &a, &total)))
            return rc;
        *value_bytes = total;
        if ((rc = vlog_values_cap(values, values_cap, total))) return rc;
        if ((rc = call.down(status, a.status, n)) || (rc = call.down(value_off, a.voff, n + 1))) return rc;
        if (values && total) {
            DevImage vals;
            const auto p_values = vals.add<uint8_t>(total);
            if ((rc = vals.alloc(call, kWsVlogOut))) return rc;
            if ((rc = vlog_get_fill(a, vals.ptr(p_values), call.s)) ||
                (rc = call.down(values, vals.ptr(p_values), total)))
                return rc;
        }
        if ((rc = call.finish())) return rc;
    } catch (const std::bad_alloc&) {
        return table_no_memory();
    }
    return ok();
}

int vbf_vlog_encode_dev(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n, const uint8_t* values,
                        const uint64_t* value_off, const int64_t* created_ms, const uint8_t* tombstones, uint64_t base,
                        uint8_t* out, uint64_t out_cap, uint64_t* out_len, uint32_t* val_offsets, void* stream) {
    int rc = vlog_enc_check_args(keys, offsets, stride, n, value_off, base, out_len);
    if (rc) return rc;
    if (!n) return ok();
    FORK_GUARD();
    hipStream_t s = (hipStream_t)stream;
    void* ws = nullptr;
    if ((rc = get_workspace(s, 256, &ws, kWsVlogEnc))) return rc;
    vbf::VlogEncArgs a{};
    a.keys = keys;
    a.offsets = offsets;
    a.stride = stride;
    a.n = n;
    a.values = values;
    a.value_off = value_off;
    a.created = created_ms;
    a.tomb = tombstones;
    a.base = base;
    a.err = static_cast<uint32_t*>(ws);
    HIP_TRY(hipMemsetAsync(a.err, 0, 4, s));
    HIP_TRY(hipMemsetAsync(a.err + 1, 0xFF, 4, s));
    vbf::phase_begin(vbf::kPhaseVlogEncode, s);
    HIP_TRY(vbf::vlog_enc_check(a, s));
    vbf::phase_end(vbf::kPhaseVlogEncode, s);
    uint64_t ko[3] = {0, (n - 1) * stride, n * stride}, vo[3] = {0, 0, 0};
    uint32_t ev[2] = {0, 0};
    if (offsets) {
        HIP_TRY(hipMemcpyAsync(&ko[0], offsets, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&ko[1], offsets + n - 1, 16, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipMemcpyAsync(&vo[0], value_off, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&vo[1], value_off + n - 1, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(ev, a.err, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (ev[0] & vbf::kVlogEncErrOrder) return fail(VBF_EINVAL, "offsets or value_off descend at entry %u", ev[1]);
    if (ev[0] & vbf::kVlogEncErrLong)
        return fail(VBF_EINVAL, "entry %u: a key or value longer than 2^32 - 1 bytes (key_len and val_len are u32)", ev[1]);
    if ((rc = vlog_enc_plan(&a, ko, vo, out, out_cap, out_len))) return rc;
    a.out = out;
    a.val_offsets = val_offsets;
    if ((out || val_offsets) && (rc = vlog_enc_emit(a, s))) return rc;
    return ok();
}

int vbf_vlog_encode_host(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n, const uint8_t* values,
                         const uint64_t* value_off, const int64_t* created_ms, const uint8_t* tombstones, uint64_t base,
                         uint8_t* out, uint64_t out_cap, uint64_t* out_len, uint32_t* val_offsets, int device) {
    int rc = vlog_enc_check_args(keys, offsets, stride, n, value_off, base, out_len);
    if (rc) return rc;
    if (!n) return ok();
    for (uint64_t j = 0; j < n; ++j) {
        if (value_off[j] > value_off[j + 1] || (offsets && offsets[j] > offsets[j + 1]))
            return fail(VBF_EINVAL, "offsets or value_off descend at entry %llu", (unsigned long long)j);
        if (value_off[j + 1] - value_off[j] > 0xFFFFFFFFull || (offsets && offsets[j + 1] - offsets[j] > 0xFFFFFFFFull))
            return fail(VBF_EINVAL, "entry %llu: a key or value longer than 2^32 - 1 bytes (key_len and val_len are u32)",
                        (unsigned long long)j);
    }
    vbf::VlogEncArgs a{};
    a.keys = keys;  // for the plan's NULL checks; the device pointers follow
    a.values = values;
    a.stride = stride;
    a.n = n;
    a.base = base;
    const uint64_t ko[3] = {offsets ? offsets[0] : 0, offsets ? offsets[n - 1] : (n - 1) * stride,
                            offsets ? offsets[n] : n * stride};
    const uint64_t vo[3] = {value_off[0], value_off[n - 1], value_off[n]};
    if ((rc = vlog_enc_plan(&a, ko, vo, out, out_cap, out_len))) return rc;
    if (!out && !val_offsets) return ok();  // the size query needs no device
    HOST_CALL(call, device);
    // device image: keys | offsets | values | value_off | created | tombstones | val_offsets | out
    const uint64_t kb = ko[2] - ko[0], vb = vo[2] - vo[0];
    DevImage img;
    const auto p_keys = img.add<uint8_t>(kb);
    const auto p_off = img.add<uint64_t>(n + 1, offsets);
    const auto p_val = img.add<uint8_t>(vb);
    const auto p_voff = img.add<uint64_t>(n + 1);
    const auto p_cr = img.add<int64_t>(n, created_ms);
    const auto p_tb = img.add<uint8_t>(n, tombstones);
    const auto p_vo = img.add<uint32_t>(n, val_offsets);
    const auto p_out = img.add<uint8_t>(a.total, out);
    if ((rc = img.alloc(call, kWsVlogEncIO))) return rc;
    if ((rc = call.up(img.ptr(p_keys), kb ? keys + ko[0] : nullptr, kb)) ||
        (rc = call.up(img.ptr(p_off), offsets, n + 1)) ||
        (rc = call.up(img.ptr(p_val), vb ? values + vo[0] : nullptr, vb)) ||
        (rc = call.up(img.ptr(p_voff), value_off, n + 1)) || (rc = call.up(img.ptr(p_cr), created_ms, n)) ||
        (rc = call.up(img.ptr(p_tb), tombstones, n)))
        return rc;
    // both offset arrays hold absolute positions: the device copies start at keys + offsets[0] and
    // values + value_off[0]
    a.keys = arena_base(img.ptr(p_keys), ko[0]);
    a.values = arena_base(img.ptr(p_val), vo[0]);
    a.offsets = img.ptr(p_off);
    a.value_off = img.ptr(p_voff);
    a.created = img.ptr(p_cr);
    a.tomb = img.ptr(p_tb);
    a.val_offsets = img.ptr(p_vo);
    a.out = img.ptr(p_out);
    if ((rc = vlog_enc_emit(a, call.s))) return rc;
    if ((rc = call.down(out, a.out, a.total)) || (rc = call.down(val_offsets, a.val_offsets, n))) return rc;
    return call.finish();
}

}  // extern "C"

// ---- the walk of the value log (ValueLog::recover, read_chunk_to_garbage_collect) ----

namespace {

// What the first sweep leaves for the second: per segment its entry position and sizes.
struct WalkSegment {
    uint64_t pos, n, kb, vb;
};
struct WalkPlan {
    vbf::WalkArgs a{};       // the workspace's parts; seg0 / ntiles / q0 / cap of the last segment walked
    void* scan_tmp = nullptr;
    size_t scan_bytes = 0;
    uint64_t s_rel = 0, lim = 0, t_end = 0;  // start, inclusion limit, the end of the tiles walked
    std::vector<WalkSegment> segs;
    uint64_t n = 0, kb = 0, vb = 0, end_rel = 0, last_entry = 0;
    int stop = VBF_WALK_END;
};

// The argument checks of vbf_vlog_walk_* that need no HIP call; the five scalars are written.
int walk_check(const vbf_vlog* v, uint64_t start, uint64_t* n_out, uint64_t* key_bytes, uint64_t* value_bytes,
               uint64_t* end_off, int* stop) {
    if (!n_out) return fail(VBF_EINVAL, "n_out is NULL");
    if (!key_bytes) return fail(VBF_EINVAL, "key_bytes is NULL");
    if (!value_bytes) return fail(VBF_EINVAL, "value_bytes is NULL");
    if (!end_off) return fail(VBF_EINVAL, "end_off is NULL");
    if (!stop) return fail(VBF_EINVAL, "stop is NULL");
    *n_out = *key_bytes = *value_bytes = 0;
    *end_off = start;
    *stop = VBF_WALK_END;
    if (!v) return fail(VBF_EINVAL, "vlog is NULL");
    if (start < v->base || start - v->base > v->len)
        return fail(VBF_EINVAL, "start %llu outside the window [%llu, %llu]", (unsigned long long)start,
                    (unsigned long long)v->base, (unsigned long long)(v->base + v->len));
    return VBF_OK;
}

// One segment's arguments: it starts at the tile of `pos` and covers at most kWalkSegment bytes.
void walk_segment_args(WalkPlan* p, uint64_t pos) {
    vbf::WalkArgs& a = p->a;
    a.seg0 = pos / vbf::kWalkTile * vbf::kWalkTile;
    const uint64_t seg_end = std::min<uint64_t>(a.seg0 + vbf::kWalkSegment, p->t_end);
    a.ntiles = (uint32_t)((seg_end - a.seg0) / vbf::kWalkTile);
    a.q0 = (uint32_t)(pos - a.seg0);
    a.cap = std::min(std::min(seg_end, a.len), p->lim);
}

// The first sweep, on the log's device: every segment from `start` until the budget is met or the
// chain stops, one stream synchronisation per segment (its result).  Workspace (slot kWsVlogWalk):
// about 4.4 bytes per byte of the largest segment walked (at most kWalkSegment) plus 32 bytes per
// possible entry of it.
int walk_sweep(const vbf_vlog* v, uint64_t start, uint64_t budget, hipStream_t s, WalkPlan* p) {
    const uint64_t len = v->len, T = vbf::kWalkTile;
    p->s_rel = start - v->base;
    // entries are included while they start below lim: the first always, the others while the bytes
    // read before them are below the budget
    const uint64_t limit = p->s_rel + budget < budget ? ~0ull : p->s_rel + budget;
    p->lim = std::max(limit, p->s_rel + 1);
    p->t_end = (std::min(len, p->lim) + T - 1) / T * T;
    const uint64_t span = p->t_end - p->s_rel / T * T;
    const uint64_t nt = std::min<uint64_t>(span, vbf::kWalkSegment) / T, ng = (nt + vbf::kWalkGroup - 1) / vbf::kWalkGroup;
    const uint64_t slots = nt * (T / 17 + 1) + 1;
    HIP_TRY(vbf::scan_u64(nullptr, &p->scan_bytes, nullptr, nullptr, nt + 1, s));
    uint64_t off = 0;
    auto part = [&off](uint64_t bytes) {
        const uint64_t o = off;
        off += align256(bytes);
        return o;
    };
    const uint64_t o_exit = part(nt * T * 4), o_gexit = part(ng * T * 4), o_tentry = part(nt * 4);
    const uint64_t o_pos = part(nt * vbf::kWalkSlots * 2), o_kpre = part(nt * vbf::kWalkSlots * 2);
    const uint64_t o_cnt = part((nt + 1) * 8), o_ksum = part((nt + 1) * 8), o_vsum = part((nt + 1) * 8);
    const uint64_t o_tend = part(nt * 8), o_ttorn = part(nt * 4);
    const uint64_t o_cbase = part((nt + 1) * 8), o_kbase = part((nt + 1) * 8), o_vbase = part((nt + 1) * 8);
    const uint64_t o_ko = part(slots * 8), o_ks = part(slots * 8), o_vo = part(slots * 8), o_vs = part(slots * 8);
    const uint64_t o_res = part(sizeof(vbf::WalkRes)), o_tmp = part(p->scan_bytes);
    void* ws = nullptr;
    int rc = get_workspace(s, off, &ws, kWsVlogWalk);
    if (rc) return rc;
    char* b = static_cast<char*>(ws);
    vbf::WalkArgs& a = p->a;
    a.bytes = v->bytes;
    a.len = len;
    a.base = v->base;
    a.lim = p->lim;
    a.exit = reinterpret_cast<uint32_t*>(b + o_exit);
    a.gexit = reinterpret_cast<uint32_t*>(b + o_gexit);
    a.tentry = reinterpret_cast<uint32_t*>(b + o_tentry);
    a.pos = reinterpret_cast<uint16_t*>(b + o_pos);
    a.kpre = reinterpret_cast<uint16_t*>(b + o_kpre);
    a.cnt = reinterpret_cast<uint64_t*>(b + o_cnt);
    a.ksum = reinterpret_cast<uint64_t*>(b + o_ksum);
    a.vsum = reinterpret_cast<uint64_t*>(b + o_vsum);
    a.tend = reinterpret_cast<uint64_t*>(b + o_tend);
    a.ttorn = reinterpret_cast<uint32_t*>(b + o_ttorn);
    a.cbase = reinterpret_cast<uint64_t*>(b + o_cbase);
    a.kbase = reinterpret_cast<uint64_t*>(b + o_kbase);
    a.vbase = reinterpret_cast<uint64_t*>(b + o_vbase);
    a.ko = reinterpret_cast<uint64_t*>(b + o_ko);
    a.ks = reinterpret_cast<uint64_t*>(b + o_ks);
    a.vo = reinterpret_cast<uint64_t*>(b + o_vo);
    a.vs = reinterpret_cast<uint64_t*>(b + o_vs);
    a.res = reinterpret_cast<vbf::WalkRes*>(b + o_res);
    p->scan_tmp = b + o_tmp;
    uint64_t pos = p->s_rel;
    for (;;) {
        walk_segment_args(p, pos);
        vbf::WalkRes r{};
        HIP_TRY(vbf::walk_passes(a, p->scan_tmp, p->scan_bytes, s));
        HIP_TRY(hipMemcpyAsync(&r, a.res, sizeof(r), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        p->segs.push_back(WalkSegment{pos, r.n, r.kbytes, r.vbytes});
        p->n += r.n;
        p->kb += r.kbytes;
        p->vb += r.vbytes;
        if (r.n) p->last_entry = r.last_entry;
        p->end_rel = r.end;
        if (r.end < pos || r.end > len || (r.end == pos && !r.torn))  // never: the walk only moves forward
            return fail(VBF_EHIP, "the walk of the segment at %llu ended at %llu", (unsigned long long)pos,
                        (unsigned long long)r.end);
        if (r.torn) {
            p->stop = VBF_WALK_TORN;
        } else if (r.end >= limit) {  // the reference tests the budget after each whole entry, before the next read
            p->stop = VBF_WALK_BUDGET;
        } else if (r.end == len) {
            p->stop = VBF_WALK_END;
        } else {
            pos = r.end;
            continue;
        }
        return VBF_OK;
    }
}

// The sizes, the limits and the capacity rule; the scalars are written before any verdict.
int walk_sizes(const vbf_vlog* v, const WalkPlan& p, const vbf::WalkOut& o, uint64_t keys_cap, uint64_t values_cap,
               uint64_t entries_cap, uint64_t* n_out, uint64_t* key_bytes, uint64_t* value_bytes, uint64_t* end_off,
               int* stop) {
    *n_out = p.n;
    *key_bytes = p.kb;
    *value_bytes = p.vb;
    *end_off = v->base + p.end_rel;
    *stop = p.stop;
    if (p.n > 0x7FFFFFFEull)
        return fail(VBF_EINVAL, "too many entries: %llu (limit 2^31 - 2)", (unsigned long long)p.n);
    if (o.val_offsets && p.n && v->base + p.last_entry >= kVlogMaxOffset)
        return fail(VBF_EINVAL, "the entry at %llu lies at or beyond 2^32: a u32 val_offset cannot address it",
                    (unsigned long long)(v->base + p.last_entry));
    const bool per_entry = o.entry_off || o.val_offsets || o.key_off || o.value_off || o.created || o.tomb;
    if (per_entry && entries_cap < p.n)
        return fail(VBF_EINVAL, "entries_cap %llu < %llu entries", (unsigned long long)entries_cap, (unsigned long long)p.n);
    if (o.keys && keys_cap < p.kb)
        return fail(VBF_EINVAL, "keys_cap %llu < %llu key bytes", (unsigned long long)keys_cap, (unsigned long long)p.kb);
    if (o.values && values_cap < p.vb)
        return fail(VBF_EINVAL, "values_cap %llu < %llu value bytes", (unsigned long long)values_cap,
                    (unsigned long long)p.vb);
    return VBF_OK;
}

inline bool walk_any(const vbf::WalkOut& o) {
    return o.entry_off || o.val_offsets || o.keys || o.key_off || o.values || o.value_off || o.created || o.tomb;
}

// The second sweep, queued on s: the outputs of every segment.  The workspace still holds the last
// segment walked; with more than one segment the passes run again per segment (no synchronisation:
// the host knows every entry position and size).
int walk_fill(WalkPlan* p, vbf::WalkOut o, hipStream_t s) {
    const size_t ns = p->segs.size();
    for (size_t k = 0; k < ns; ++k) {
        const WalkSegment& g = p->segs[k];
        if (ns > 1) {
            walk_segment_args(p, g.pos);
            HIP_TRY(vbf::walk_passes(p->a, p->scan_tmp, p->scan_bytes, s));
        }
        o.n_seg = g.n;
        o.kb_seg = g.kb;
        o.vb_seg = g.vb;
        HIP_TRY(vbf::walk_emit(p->a, o, s));
        o.j0 += g.n;
        o.k0 += g.kb;
        o.v0 += g.vb;
    }
    HIP_TRY(vbf::walk_tail(o, p->n, p->a.base + p->end_rel, p->kb, p->vb, s));
    return VBF_OK;
}

}  // namespace

extern "C" {

int vbf_vlog_walk_dev(const vbf_vlog* v, uint64_t start, uint64_t budget, uint64_t* entry_off, uint32_t* val_offsets,
                      uint8_t* keys, uint64_t keys_cap, uint64_t* key_off, uint8_t* values, uint64_t values_cap,
                      uint64_t* value_off, int64_t* created_ms, uint8_t* tombstones, uint64_t entries_cap,
                      uint64_t* n_out, uint64_t* key_bytes, uint64_t* value_bytes, uint64_t* end_off, int* stop,
                      void* stream) {
    int rc = walk_check(v, start, n_out, key_bytes, value_bytes, end_off, stop);
    if (rc) return rc;
    vbf::WalkOut o{};
    o.entry_off = entry_off;
    o.val_offsets = val_offsets;
    o.keys = keys;
    o.key_off = key_off;
    o.values = values;
    o.value_off = value_off;
    o.created = created_ms;
    o.tomb = tombstones;
    const bool empty = start - v->base == v->len;
    if (empty && !walk_any(o)) return ok();
    FORK_GUARD();
    hipStream_t s = (hipStream_t)stream;
    int cur = -1;
    HIP_TRY(hipGetDevice(&cur));
    if (cur != v->device)
        return fail(VBF_EINVAL, "the log lives on device %d, the current device is %d", v->device, cur);
    try {
        WalkPlan p;
        p.a.base = v->base;
        p.end_rel = start - v->base;
        if (!empty && (rc = walk_sweep(v, start, budget, s, &p))) return rc;
        if ((rc = walk_sizes(v, p, o, keys_cap, values_cap, entries_cap, n_out, key_bytes, value_bytes, end_off, stop)))
            return rc;
        if (walk_any(o) && (rc = walk_fill(&p, o, s))) return rc;
    } catch (const std::bad_alloc&) {
        return table_no_memory();
    }
    return ok();
}

int vbf_vlog_walk_host(const vbf_vlog* v, uint64_t start, uint64_t budget, uint64_t* entry_off, uint32_t* val_offsets,
                       uint8_t* keys, uint64_t keys_cap, uint64_t* key_off, uint8_t* values, uint64_t values_cap,
                       uint64_t* value_off, int64_t* created_ms, uint8_t* tombstones, uint64_t entries_cap,
                       uint64_t* n_out, uint64_t* key_bytes, uint64_t* value_bytes, uint64_t* end_off, int* stop) {
    int rc = walk_check(v, start, n_out, key_bytes, value_bytes, end_off, stop);
    if (rc) return rc;
    if (start - v->base == v->len) {  // nothing to walk: no device work
        if (entry_off) entry_off[0] = start;
        if (key_off) key_off[0] = 0;
        if (value_off) value_off[0] = 0;
        return ok();
    }
    try {
        HOST_CALL(call, v->device);
        WalkPlan p;
        if ((rc = walk_sweep(v, start, budget, call.s, &p))) return rc;
        vbf::WalkOut h{};  // the caller's arrays, for the capacity rule
        h.entry_off = entry_off;
        h.val_offsets = val_offsets;
        h.keys = keys;
        h.key_off = key_off;
        h.values = values;
        h.value_off = value_off;
        h.created = created_ms;
        h.tomb = tombstones;
        if ((rc = walk_sizes(v, p, h, keys_cap, values_cap, entries_cap, n_out, key_bytes, value_bytes, end_off, stop)))
            return rc;
        if (!walk_any(h)) return call.finish();
        const uint64_t n = p.n;
        DevImage img;  // entry_off | val_offsets | keys | key_off | values | value_off | created | tombstones
        const auto p_eo = img.add<uint64_t>(n + 1, entry_off);
        const auto p_vo = img.add<uint32_t>(n, val_offsets);
        const auto p_keys = img.add<uint8_t>(p.kb, keys);
        const auto p_ko = img.add<uint64_t>(n + 1, key_off);
        const auto p_vals = img.add<uint8_t>(p.vb, values);
        const auto p_vof = img.add<uint64_t>(n + 1, value_off);
        const auto p_cr = img.add<int64_t>(n, created_ms);
        const auto p_tb = img.add<uint8_t>(n, tombstones);
        if ((rc = img.alloc(call, kWsVlogWalkOut))) return rc;
        vbf::WalkOut o{};
        o.entry_off = img.ptr(p_eo);
        o.val_offsets = img.ptr(p_vo);
        o.keys = img.ptr(p_keys);
        o.key_off = img.ptr(p_ko);
        o.values = img.ptr(p_vals);
        o.value_off = img.ptr(p_vof);
        o.created = img.ptr(p_cr);
        o.tomb = img.ptr(p_tb);
        if ((rc = walk_fill(&p, o, call.s))) return rc;
        if ((rc = call.down(entry_off, o.entry_off, n + 1)) || (rc = call.down(val_offsets, o.val_offsets, n)) ||
            (rc = call.down(keys, o.keys, p.kb)) || (rc = call.down(key_off, o.key_off, n + 1)) ||
            (rc = call.down(values, o.values, p.vb)) || (rc = call.down(value_off, o.value_off, n + 1)) ||
            (rc = call.down(created_ms, o.created, n)) || (rc = call.down(tombstones, o.tomb, n)))
            return rc;
        return call.finish();
    } catch (const std::bad_alloc&) {
        return table_no_memory();
    }
}

}  // extern "C"

// ---- the garbage collector's handler over one chunk (GC::gc_handler) ----

namespace {

// The argument checks of vbf_gc_collect_host that need no HIP call and follow no handle.  A NULL
// scalar leaves everything unwritten; otherwise the six scalars are written first.
int gc_check(const vbf_vlog* v, uint64_t tail, uint64_t log_size, uint32_t nsst, const vbf_table* const* tables,
             const vbf_filter* const* filters, const uint8_t* ov_keys, const uint64_t* ov_off,
             const uint32_t* ov_val_offsets, const int64_t* ov_created_ms, const uint8_t* ov_tombstones, uint64_t ov_n,
             uint64_t* n_chunk, uint64_t* n_invalid, uint64_t* n_puts, uint64_t* append_len, uint64_t* end_off,
             int* stop) {
    if (!n_chunk) return fail(VBF_EINVAL, "n_chunk is NULL");
    if (!n_invalid) return fail(VBF_EINVAL, "n_invalid is NULL");
    if (!n_puts) return fail(VBF_EINVAL, "n_puts is NULL");
    if (!append_len) return fail(VBF_EINVAL, "append_len is NULL");
    if (!end_off) return fail(VBF_EINVAL, "end_off is NULL");
    if (!stop) return fail(VBF_EINVAL, "stop is NULL");
    *n_chunk = *n_invalid = *n_puts = *append_len = 0;
    *end_off = tail;
    *stop = VBF_WALK_END;
    if (!v) return fail(VBF_EINVAL, "vlog is NULL");
    if (nsst && !tables) return fail(VBF_EINVAL, "tables is NULL");
    for (uint32_t i = 0; i < nsst; ++i)
        if (!tables[i]) return fail(VBF_EINVAL, "tables[%u] is NULL", i);
    if (filters)
        for (uint32_t i = 0; i < nsst; ++i)
            if (!filters[i]) return fail(VBF_EINVAL, "filters[%u] is NULL", i);
    if (ov_n) {
        if (!ov_keys) return fail(VBF_EINVAL, "ov_keys is NULL");
        if (!ov_off) return fail(VBF_EINVAL, "ov_off is NULL");
        if (!ov_val_offsets) return fail(VBF_EINVAL, "ov_val_offsets is NULL");
        if (!ov_created_ms) return fail(VBF_EINVAL, "ov_created_ms is NULL");
        if (!ov_tombstones) return fail(VBF_EINVAL, "ov_tombstones is NULL");
        if (ov_n > 0x7FFFFFFEull)
            return fail(VBF_EINVAL, "too many overlay keys: %llu (limit 2^31 - 2)", (unsigned long long)ov_n);
        for (uint64_t k = 0; k < ov_n; ++k)
            if (ov_off[k] > ov_off[k + 1]) return fail(VBF_EINVAL, "ov_off descends at key %llu", (unsigned long long)k);
        for (uint64_t k = 0; k + 1 < ov_n; ++k)
            if (cmp_host(ov_keys + ov_off[k], ov_off[k + 1] - ov_off[k], ov_keys + ov_off[k + 1],
                         ov_off[k + 2] - ov_off[k + 1]) >= 0)
                return fail(VBF_EINVAL, "overlay keys not strictly ascending at key %llu", (unsigned long long)(k + 1));
    }
    // the `tail` entry is 29 bytes: from here on no entry could follow it below 2^32
    if (log_size + 25 > kVlogMaxOffset || log_size + 25 < log_size)
        return fail(VBF_EINVAL, "log_size %llu: an appended entry would start at or beyond 2^32, where data.db's u32 "
                    "value offset cannot address it", (unsigned long long)log_size);
    return VBF_OK;
}

}  // namespace

extern "C" {

int vbf_gc_collect_host(const vbf_vlog* v, uint64_t tail, uint64_t chunk_bytes, uint64_t log_size, int64_t now_ms,
                        uint32_t nsst, const vbf_table* const* tables, const vbf_filter* const* filters,
                        const uint8_t* ov_keys, const uint64_t* ov_off, const uint32_t* ov_val_offsets,
                        const int64_t* ov_created_ms, const uint8_t* ov_tombstones, uint64_t ov_n, uint8_t* verdict,
                        uint64_t entries_cap, uint8_t* append, uint64_t append_cap, uint32_t* put_ids,
                        uint32_t* put_val_offsets, uint8_t* put_tombstones, uint64_t puts_cap, uint64_t* n_chunk,
                        uint64_t* n_invalid, uint64_t* n_puts, uint64_t* append_len, uint64_t* end_off, int* stop) {
    int rc = gc_check(v, tail, log_size, nsst, tables, filters, ov_keys, ov_off, ov_val_offsets, ov_created_ms,
                      ov_tombstones, ov_n, n_chunk, n_invalid, n_puts, append_len, end_off, stop);
    if (rc) return rc;
    if (tail < v->base || tail - v->base > v->len)
        return fail(VBF_EINVAL, "tail %llu outside the window [%llu, %llu]", (unsigned long long)tail,
                    (unsigned long long)v->base, (unsigned long long)(v->base + v->len));
    const int device = v->device;
    for (uint32_t i = 0; i < nsst; ++i)
        if (tables[i]->device != device)
            return fail(VBF_EINVAL, "tables[%u] lives on device %d, the log on %d", i, tables[i]->device, device);
    if (!nsst) filters = nullptr;
    if (tail - v->base == v->len) return ok();  // nothing to walk: no device work
    try {
        // Lock order as in vbf_table_get_host: the filters' locks and their drain, then the device.
        MultiLock lk(filters, filters ? nsst : 0);
        if ((rc = lk.drain())) return rc;
        if (filters)
            for (uint32_t i = 0; i < nsst; ++i)
                if (filters[i]->bits->device != device)
                    return fail(VBF_EINVAL, "filters[%u] lives on device %d, the log on %d", i,
                                filters[i]->bits->device, device);
        HOST_CALL(call, device);
        hipStream_t s = call.s;
        WalkPlan p;
        if ((rc = walk_sweep(v, tail, chunk_bytes, s, &p))) return rc;
        const uint64_t n = p.n;
        *n_chunk = n;
        *end_off = v->base + p.end_rel;
        *stop = p.stop;
        if (n > 0x7FFFFFFEull)
            return fail(VBF_EINVAL, "too many entries: %llu (limit 2^31 - 2)", (unsigned long long)n);
        if (!n) return call.finish();  // a torn first entry: nothing to judge
        const uint64_t ok0 = ov_n ? ov_off[0] : 0, okb = ov_n ? ov_off[ov_n] - ok0 : 0;
        size_t scan_b = 0, sel_b = 0;
        HIP_TRY(vbf::scan_u64(nullptr, &scan_b, nullptr, nullptr, n + 2, s));
        HIP_TRY(vbf::select_u32(nullptr, &sel_b, nullptr, nullptr, nullptr, nullptr, n, s));
        // the chunk (entry_off | keys | key_off | created), the lookup (cand | found | val_off | wcreated),
        // the overlay, the judge's arrays: 79 bytes per chunk entry plus its key, nsst with filters
        DevImage img;
        const auto p_eo = img.add<uint64_t>(n + 1);
        const auto p_keys = img.add<uint8_t>(p.kb + 1);
        const auto p_ko = img.add<uint64_t>(n + 1);
        const auto p_cand = img.add<uint8_t>(n * nsst, filters);
        const auto p_found = img.add<uint8_t>(n);
        const auto p_val = img.add<uint32_t>(n);
        const auto p_wcr = img.add<uint64_t>(n);
        const auto p_okeys = img.add<uint8_t>(okb + 1, ov_n);
        const auto p_ooff = img.add<uint64_t>(ov_n + 1, ov_n);
        const auto p_oval = img.add<uint32_t>(ov_n, ov_n);
        const auto p_ocr = img.add<int64_t>(ov_n, ov_n);
        const auto p_otb = img.add<uint8_t>(ov_n, ov_n);
        const auto p_verdict = img.add<uint8_t>(n);
        const auto p_keep = img.add<uint8_t>(n);
        const auto p_ids = img.add<uint32_t>(n);
        const auto p_size = img.add<uint64_t>(n + 2);
        const auto p_pos = img.add<uint64_t>(n + 2);
        const auto p_ksrc = img.add<uint64_t>(n);
        const auto p_vsrc = img.add<uint64_t>(n);
        const auto p_klen = img.add<uint32_t>(n);
        const auto p_vlen = img.add<uint32_t>(n);
        const auto p_pids = img.add<uint32_t>(n + 1);
        const auto p_misc = img.add<uint64_t>(1);
        const auto p_res = img.add<vbf::GcRes>(1);
        const auto p_tmp = img.add<uint8_t>(std::max(scan_b, sel_b));
        if ((rc = img.alloc(call, kWsGc))) return rc;
        vbf::WalkOut o{};
        o.entry_off = img.ptr(p_eo);
        o.keys = img.ptr(p_keys);
        o.key_off = img.ptr(p_ko);
        if ((rc = walk_fill(&p, o, s))) return rc;
        if ((rc = call.up(img.ptr(p_okeys), ov_n && okb ? ov_keys + ok0 : nullptr, okb)) ||
            (rc = call.up_rebased(img.ptr(p_ooff), ov_off, ov_n ? ov_n + 1 : 0)) ||
            (rc = call.up(img.ptr(p_oval), ov_val_offsets, ov_n)) || (rc = call.up(img.ptr(p_ocr), ov_created_ms, ov_n)) ||
            (rc = call.up(img.ptr(p_otb), ov_tombstones, ov_n)))
            return rc;
        if (nsst) {  // step 3 of GC::get, exactly vbf_table_get_host's device side
            if (filters) {
                std::vector<uint8_t> bounds;
                std::vector<uint64_t> boff;
                table_bounds(nsst, tables, &bounds, &boff);
                if ((rc = multi_probe(o.keys, o.key_off, 0, n, 1, nsst, filters, bounds.data(), boff.data(),
                                      img.ptr(p_cand), s)))
                    return rc;
            }
            if ((rc = table_lookup(o.keys, o.key_off, 0, n, nsst, tables, img.ptr(p_cand), img.ptr(p_found), nullptr,
                                   img.ptr(p_val), img.ptr(p_wcr), s)))
                return rc;
        } else {
            HIP_TRY(hipMemsetAsync(img.ptr(p_found), 0, n, s));
        }
        vbf::GcArgs a{};
        a.bytes = v->bytes;
        a.len = v->len;
        a.base = v->base;
        a.n = n;
        a.entry_off = o.entry_off;
        a.ov_keys = img.ptr(p_okeys);
        a.ov_off = img.ptr(p_ooff);
        a.ov_val = img.ptr(p_oval);
        a.ov_created = img.ptr(p_ocr);
        a.ov_tomb = img.ptr(p_otb);
        a.ov_n = ov_n;
        a.found = img.ptr(p_found);
        a.val_off = img.ptr(p_val);
        a.wcreated = img.ptr(p_wcr);
        a.verdict = img.ptr(p_verdict);
        a.keep = img.ptr(p_keep);
        a.ids = img.ptr(p_ids);
        a.size = img.ptr(p_size);
        a.pos = img.ptr(p_pos);
        a.ksrc = img.ptr(p_ksrc);
        a.vsrc = img.ptr(p_vsrc);
        a.klen = img.ptr(p_klen);
        a.vlen = img.ptr(p_vlen);
        a.put_ids = img.ptr(p_pids);
        a.res = img.ptr(p_res);
        vbf::GcRes res{};
        uint64_t total = 0;
        HIP_TRY(hipMemsetAsync(a.res, 0, sizeof(vbf::GcRes), s));
        HIP_TRY(hipMemsetAsync(&a.res->bad, 0xFF, 8, s));
        HIP_TRY(hipMemsetAsync(img.ptr(p_pids), 0xFF, 4, s));  // put 0 comes from no chunk entry
        vbf::phase_begin(vbf::kPhaseGcJudge, s);
        HIP_TRY(vbf::gc_overlay(a, s));
        HIP_TRY(vbf::gc_judge(a, s));
        size_t tb = scan_b;
        HIP_TRY(vbf::scan_u64(img.ptr(p_tmp), &tb, a.size, img.ptr(p_pos), n + 2, s));
        tb = sel_b;
        HIP_TRY(vbf::select_u32(img.ptr(p_tmp), &tb, a.ids, a.keep, img.ptr(p_pids) + 1, img.ptr(p_misc), n, s));
        vbf::phase_end(vbf::kPhaseGcJudge, s);
        // the one readback: the invalid count, the first BAD entry, the last valid one, the byte total
        if ((rc = call.down(&res, a.res, 1)) || (rc = call.down(&total, a.pos + n + 1, 1)) || (rc = call.sync()))
            return rc;
        if (res.bad != ~0ull) {
            uint32_t at = 0;
            if ((rc = call.down(&at, a.val_off + res.bad, 1)) || (rc = call.sync())) return rc;
            return fail(VBF_EINVAL, "gc: the most recent entry of chunk entry %llu, at %u, is not a whole entry of the log",
                        (unsigned long long)res.bad, at);
        }
        *n_invalid = res.n_invalid;
        const uint64_t np = res.n_invalid ? 1 + n - res.n_invalid : 0;  // nothing to collect (:228-230): no put
        if (!np) total = 0;
        *n_puts = np;
        *append_len = total;
        if (verdict && entries_cap < n)
            return fail(VBF_EINVAL, "entries_cap %llu < %llu entries", (unsigned long long)entries_cap,
                        (unsigned long long)n);
        if (!np) {
            if ((rc = call.down(verdict, a.verdict, n))) return rc;
            return call.finish();
        }
        if (log_size + total >= kVlogMaxOffset && res.last_valid) {  // only then can an entry start at 2^32 or beyond
            uint64_t last = 0;
            if ((rc = call.down(&last, a.pos + res.last_valid, 1)) || (rc = call.sync())) return rc;
            if (log_size + last >= kVlogMaxOffset)
                return fail(VBF_EINVAL, "the last entry would start at %llu, at or beyond 2^32: data.db's u32 value offset "
                            "cannot address it", (unsigned long long)(log_size + last));
        }
        if ((put_ids || put_val_offsets || put_tombstones) && puts_cap < np)
            return fail(VBF_EINVAL, "puts_cap %llu < %llu puts", (unsigned long long)puts_cap, (unsigned long long)np);
        if (append && append_cap < total)
            return fail(VBF_EINVAL, "append_cap %llu < %llu log bytes", (unsigned long long)append_cap,
                        (unsigned long long)total);
        if ((rc = call.down(verdict, a.verdict, n)) || (rc = call.down(put_ids, a.put_ids, np))) return rc;
        if (append || put_val_offsets || put_tombstones) {
            DevImage out;  // append | put_val_offsets | put_tombstones: 1 byte per appended byte, 5 per put
            const auto p_app = out.add<uint8_t>(total, append);
            const auto p_pvo = out.add<uint32_t>(np, put_val_offsets);
            const auto p_ptb = out.add<uint8_t>(np, put_tombstones);
            if ((rc = out.alloc(call, kWsGcOut))) return rc;
            a.n_puts = np;
            a.total = total;
            a.log_size = log_size;
            a.new_tail = *end_off;
            a.now_ms = now_ms;
            a.append = out.ptr(p_app);
            a.put_val_offsets = out.ptr(p_pvo);
            a.put_tombstones = out.ptr(p_ptb);
            vbf::phase_begin(vbf::kPhaseGcEmit, s);
            HIP_TRY(vbf::gc_emit(a, s));
            vbf::phase_end(vbf::kPhaseGcEmit, s);
            if ((rc = call.down(append, a.append, total)) || (rc = call.down(put_val_offsets, a.put_val_offsets, np)) ||
                (rc = call.down(put_tombstones, a.put_tombstones, np)))
                return rc;
        }
        return call.finish();
    } catch (const std::bad_alloc&) {
        return table_no_memory();
    }
}

}  // extern "C"

// ---- device-resident memtables and the whole get (DataStore::get, src/db/store.rs:442-501) ----

// A memtable as the sort and the gather leave it: the distinct keys ascending with their offsets, the
// three per-entry arrays and the lookup's prefix table, in one allocation.  Immutable once opened.
struct vbf_memtable {
    int device = 0;
    uint64_t n = 0, key_bytes = 0;
    void* mem = nullptr;  // keys | off | pfx | val | created | tomb
    vbf::MemDesc desc{};
    ~vbf_memtable() {
        if (!mem || hip_forked()) return;  // a forked child: the parent's allocation
        int prev = -1;
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(device);
        (void)hipFree(mem);
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

namespace {

int memtable_open_check(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n, vbf_memtable** out) {
    if (!out) return fail(VBF_EINVAL, "out is NULL");
    *out = nullptr;
    if (n > 0x7FFFFFFFull) return fail(VBF_EINVAL, "too many entries (%llu > 2^31 - 1)", (unsigned long long)n);
    return check_keys(keys, offsets, stride, n);
}

// The puts (device pointers, n in [1, 2^31); ends = the first and the last offset, which may still be
// on their way from the device until the sort has synchronised) sorted and gathered into the handle on
// the current device.  Two stream synchronisations: the sort's count, the gathered key bytes.
int memtable_fill(vbf_memtable& t, const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                  const uint64_t* ends, const uint32_t* val, const int64_t* created, const uint8_t* tomb, hipStream_t s) {
    void* ws = nullptr;
    int rc = get_workspace(s, n * 4, &ws, kWsMemOpen);
    if (rc) return rc;
    uint32_t* ids = static_cast<uint32_t*>(ws);
    uint64_t nd = 0;
    const uint64_t* soff = nullptr;
    if ((rc = memtable_sort(keys, offsets, stride, n, ids, &nd, &soff, s))) return rc;
    const uint64_t kb = ends[1] - ends[0];  // read back by the sort's synchronisation; ascending: the sort passed
    DevImage img;
    const auto p_keys = img.add<uint8_t>(kb + 1);
    const auto p_off = img.add<uint64_t>(nd + 1);
    const auto p_pfx = img.add<uint64_t>(nd);
    const auto p_val = img.add<uint32_t>(nd);
    const auto p_cr = img.add<int64_t>(nd);
    const auto p_tb = img.add<uint8_t>(nd);
    HIP_TRY(hipMalloc(&t.mem, img.bytes));
    img.base = t.mem;
    // an absent per-entry array means zeros
    if (!val) HIP_TRY(hipMemsetAsync(img.ptr(p_val), 0, nd * 4, s));
    if (!created) HIP_TRY(hipMemsetAsync(img.ptr(p_cr), 0, nd * 8, s));
    if (!tomb) HIP_TRY(hipMemsetAsync(img.ptr(p_tb), 0, nd, s));
    uint64_t gkb = 0;
    if ((rc = gather_entries(keys, soff, created, tomb, val, ids, nd, img.ptr(p_keys), kb, img.ptr(p_off),
                             created ? img.ptr(p_cr) : nullptr, tomb ? img.ptr(p_tb) : nullptr,
                             val ? img.ptr(p_val) : nullptr, &gkb, s)))
        return rc;
    HIP_TRY(vbf::mem_prefixes(img.ptr(p_keys), img.ptr(p_off), nd, img.ptr(p_pfx), s));
    t.n = nd;
    t.key_bytes = gkb;
    t.desc = vbf::MemDesc{img.ptr(p_keys), img.ptr(p_off), img.ptr(p_pfx), img.ptr(p_val), img.ptr(p_cr), img.ptr(p_tb), nd};
    return VBF_OK;
}

constexpr uint64_t kGetMaxKeys = 0x7FFFFFFEull;

// The argument checks of vbf_memtable_get_* that need no HIP call; *device = the handles' device, -1
// when there is none.
int memget_check(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n, const vbf_memtable* gc,
                 const vbf_memtable* active, uint32_t nro, const vbf_memtable* const* ro, const vbf_vlog* log,
                 int* device) {
    *device = -1;
    if (n > kGetMaxKeys) return fail(VBF_EINVAL, "too many keys: %llu (limit 2^31 - 2)", (unsigned long long)n);
    int rc = check_keys(keys, offsets, stride, n);
    if (rc) return rc;
    if (nro && !ro) return fail(VBF_EINVAL, "ro is NULL");
    for (uint32_t i = 0; i < nro; ++i)
        if (!ro[i]) return fail(VBF_EINVAL, "ro[%u] is NULL", i);
    if (gc && !log) return fail(VBF_EINVAL, "a gc table needs the log: log is NULL");
    auto same = [&](const char* what, int dev) {
        if (*device < 0) *device = dev;
        return *device == dev ? VBF_OK
                              : fail(VBF_EINVAL, "%s lives on device %d, the other handles on %d", what, dev, *device);
    };
    if (gc && ((rc = same("gc", gc->device)) || (rc = same("log", log->device)))) return rc;
    if (active && (rc = same("active", active->device))) return rc;
    for (uint32_t i = 0; i < nro; ++i)
        if ((rc = same("a read-only memtable", ro[i]->device))) return rc;
    return VBF_OK;
}

bool memget_sampled() {  // VBF_MEMGET=0: the plain kernel (read per call; identical results)
    const char* e = getenv("VBF_MEMGET");
    return !(e && e[0] == '0' && !e[1]);
}

// Device pointers, on the handles' device: the layers' descriptors go up (one stream
// synchronisation, their source is pageable), then the lookup is queued on `s`.
int memget_lookup(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n, const vbf_memtable* gc,
                  const vbf_memtable* active, uint32_t nro, const vbf_memtable* const* ro, const vbf_vlog* log,
                  uint8_t* found, uint32_t* layer, uint32_t* val_offsets, uint64_t* created_ms, hipStream_t s) {
    std::vector<vbf::MemDesc> tab(2 + (size_t)nro);
    if (gc) tab[0] = gc->desc;
    if (active) tab[1] = active->desc;
    for (uint32_t i = 0; i < nro; ++i) tab[2 + i] = ro[i]->desc;
    void* ws = nullptr;
    int rc = get_workspace(s, tab.size() * sizeof(vbf::MemDesc), &ws, kWsMemGetDesc);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(ws, tab.data(), tab.size() * sizeof(vbf::MemDesc), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    vbf::MemGetArgs a{};
    a.keys = keys;
    a.offsets = offsets;
    a.stride = stride;
    a.n = n;
    a.layers = static_cast<const vbf::MemDesc*>(ws);
    a.nro = nro;
    if (gc) {
        a.log = log->bytes;
        a.log_len = log->len;
        a.log_base = log->base;
    }
    a.found = found;
    a.layer = layer;
    a.val_off = val_offsets;
    a.created = created_ms;
    vbf::phase_begin(vbf::kPhaseMemGet, s);
    HIP_TRY(vbf::mem_get(a, memget_sampled(), s));
    vbf::phase_end(vbf::kPhaseMemGet, s);
    return VBF_OK;
}

}  // namespace

extern "C" {

int vbf_memtable_open_dev(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                          const uint32_t* val_offsets, const int64_t* created_ms, const uint8_t* tombstones,
                          void* stream, vbf_memtable** out) {
    int rc = memtable_open_check(keys, offsets, stride, n, out);
    if (rc) return rc;
    FORK_GUARD();
    try {
        std::unique_ptr<vbf_memtable> t(new (std::nothrow) vbf_memtable());
        if (!t) return table_no_memory();
        HIP_TRY(hipGetDevice(&t->device));
        if (n) {
            hipStream_t s = (hipStream_t)stream;
            uint64_t ends[2] = {0, n * stride};
            if (offsets) {  // the key bytes' extent, read with the sort's count; the sort reports descending offsets
                HIP_TRY(hipMemcpyAsync(&ends[0], offsets, 8, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipMemcpyAsync(&ends[1], offsets + n, 8, hipMemcpyDeviceToHost, s));
            }
            rc = memtable_fill(*t, keys, offsets, stride, n, ends, val_offsets, created_ms, tombstones, s);
            // the copies above and the gather read the caller's arrays and write the handle: complete on return
            const hipError_t e = hipStreamSynchronize(s);
            if (rc) return rc;
            HIP_TRY(e);
        }
        *out = t.release();
    } catch (const std::bad_alloc&) {
        return table_no_memory();
    }
    return ok();
}

int vbf_memtable_open_host(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                           const uint32_t* val_offsets, const int64_t* created_ms, const uint8_t* tombstones, int device,
                           vbf_memtable** out) {
    int rc = memtable_open_check(keys, offsets, stride, n, out);
    if (rc || (rc = offsets_ascend(offsets, n))) return rc;
    const uint64_t kb = !n ? 0 : (offsets ? offsets[n] - offsets[0] : n * stride);
    if (!keys && kb) return fail(VBF_EINVAL, "keys is NULL");
    try {
        std::unique_ptr<vbf_memtable> t(new (std::nothrow) vbf_memtable());
        if (!t) return table_no_memory();
        t->device = device;
        if (n) {
            HOST_CALL(call, device);
            KeyImage m;  // keys | offsets | val | created | tombstones
            m.lay(offsets, stride, n);
            const auto p_val = m.add<uint32_t>(n, val_offsets);
            const auto p_cr = m.add<int64_t>(n, created_ms);
            const auto p_tb = m.add<uint8_t>(n, tombstones);
            if ((rc = m.alloc(call, kWsMemIO)) || (rc = m.upload(call, keys, offsets, n)) ||
                (rc = call.up(m.ptr(p_val), val_offsets, n)) || (rc = call.up(m.ptr(p_cr), created_ms, n)) ||
                (rc = call.up(m.ptr(p_tb), tombstones, n)))
                return rc;
            const uint64_t ends[2] = {0, kb};
            if ((rc = memtable_fill(*t, m.ptr(m.keys), m.ptr(m.off), stride, n, ends, m.ptr(p_val), m.ptr(p_cr),
                                    m.ptr(p_tb), call.s)))
                return rc;
            if ((rc = call.finish())) return rc;
        }
        *out = t.release();
    } catch (const std::bad_alloc&) {
        return table_no_memory();
    }
    return ok();
}

void vbf_memtable_free(vbf_memtable* t) { delete t; }
uint64_t vbf_memtable_entries(const vbf_memtable* t) { return t ? t->n : 0; }
uint64_t vbf_memtable_key_bytes(const vbf_memtable* t) { return t ? t->key_bytes : 0; }
int vbf_memtable_device(const vbf_memtable* t) { return t ? t->device : VBF_DEVICE_HOST; }

int vbf_memtable_export_host(const vbf_memtable* t, uint8_t* keys, uint64_t keys_cap, uint64_t* key_off,
                             uint32_t* val_offsets, int64_t* created_ms, uint8_t* tombstones, uint64_t entries_cap) {
    if (!t) return fail(VBF_EINVAL, "memtable is NULL");
    if (keys && keys_cap < t->key_bytes)
        return fail(VBF_EINVAL, "keys_cap %llu < %llu key bytes", (unsigned long long)keys_cap,
                    (unsigned long long)t->key_bytes);
    if ((key_off || val_offsets || created_ms || tombstones) && entries_cap < t->n)
        return fail(VBF_EINVAL, "entries_cap %llu < %llu entries", (unsigned long long)entries_cap,
                    (unsigned long long)t->n);
    if (!keys && !key_off && !val_offsets && !created_ms && !tombstones) return ok();  // sizes: the accessors
    if (!t->n) {
        if (key_off) key_off[0] = 0;
        return ok();
    }
    HOST_CALL(call, t->device);
    int rc;
    if ((rc = call.down(keys, t->desc.keys, t->key_bytes)) || (rc = call.down(key_off, t->desc.off, t->n + 1)) ||
        (rc = call.down(val_offsets, t->desc.val, t->n)) || (rc = call.down(created_ms, t->desc.created, t->n)) ||
        (rc = call.down(tombstones, t->desc.tomb, t->n)))
        return rc;
    return call.finish();
}

// Flusher::flush of an open memtable: the encoder over the handle's arrays.
int vbf_memtable_encode_host(const vbf_memtable* t, uint8_t* data, uint64_t data_cap, uint64_t* data_len, uint8_t* index,
                             uint64_t index_cap, uint64_t* index_len) {
    if (!data_len || !index_len) return fail(VBF_EINVAL, "data_len / index_len is NULL");
    *data_len = *index_len = 0;
    if (!t) return fail(VBF_EINVAL, "memtable is NULL");
    if (!t->n) return fail(VBF_EINVAL, "Cannot flush an empty table (flusher.rs:40-44, table.rs:262-264)");
    const uint64_t nd = t->n, kb = t->key_bytes;
    if (nd >= (1ull << 32) / 17 || kb >= (1ull << 32))
        return fail(VBF_EINVAL, "data.db reaches 2^32 bytes: index.db's u32 block offsets cannot address it");
    HOST_CALL(call, t->device);
    DevImage q;  // data.db | index.db; capacities that always suffice
    const auto q_data = q.add<uint8_t>(kb + 17 * nd);
    const auto q_idx = q.add<uint8_t>(kb + 8 * nd);
    int rc = q.alloc(call, kWsMemOut);
    if (rc) return rc;
    uint64_t nb = 0;
    if ((rc = sst_encode(t->desc.keys, t->desc.off, 0, nd, t->desc.val, t->desc.created, t->desc.tomb,
                         data ? q.ptr(q_data) : nullptr, kb + 17 * nd, data_len, index ? q.ptr(q_idx) : nullptr,
                         kb + 8 * nd, index_len, nullptr, 0, &nb, call.s)))
        return rc;
    if (data && data_cap < *data_len)
        return fail(VBF_EINVAL, "data holds %llu < %llu bytes", (unsigned long long)data_cap,
                    (unsigned long long)*data_len);
    if (index && index_cap < *index_len)
        return fail(VBF_EINVAL, "index holds %llu < %llu bytes", (unsigned long long)index_cap,
                    (unsigned long long)*index_len);
    if ((rc = call.down(data, q.ptr(q_data), *data_len)) || (rc = call.down(index, q.ptr(q_idx), *index_len))) return rc;
    return call.finish();
}

int vbf_memtable_get_dev(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                         const vbf_memtable* gc, const vbf_memtable* active, uint32_t nro,
                         const vbf_memtable* const* ro, const vbf_vlog* log, uint8_t* found, uint32_t* layer,
                         uint32_t* val_offsets, uint64_t* created_ms, void* stream) {
    int device = -1;
    int rc = memget_check(keys, offsets, stride, n, gc, active, nro, ro, log, &device);
    if (rc) return rc;
    if (!n) return ok();
    FORK_GUARD();
    hipStream_t s = (hipStream_t)stream;
    if (device < 0) {  // no memtable at all: nothing is found
        if (found) HIP_TRY(hipMemsetAsync(found, 0, n, s));
        if (layer) HIP_TRY(hipMemsetAsync(layer, 0xFF, n * 4, s));
        if (val_offsets) HIP_TRY(hipMemsetAsync(val_offsets, 0, n * 4, s));
        if (created_ms) HIP_TRY(hipMemsetAsync(created_ms, 0, n * 8, s));
        return ok();
    }
    try {
        DEVICE_SCOPE(device);
        if ((rc = memget_lookup(keys, offsets, stride, n, gc, active, nro, ro, log, found, layer, val_offsets, created_ms, s)))
            return rc;
    } catch (const std::bad_alloc&) {
        return table_no_memory();
    }
    return ok();
}

int vbf_memtable_get_host(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                          const vbf_memtable* gc, const vbf_memtable* active, uint32_t nro,
                          const vbf_memtable* const* ro, const vbf_vlog* log, uint8_t* found, uint32_t* layer,
                          uint32_t* val_offsets, uint64_t* created_ms) {
    int device = -1;
    int rc = memget_check(keys, offsets, stride, n, gc, active, nro, ro, log, &device);
    if (rc || (rc = offsets_ascend(offsets, n))) return rc;
    if (!n) return ok();
    if (device < 0) {
        if (found) memset(found, 0, n);
        if (layer) memset(layer, 0xFF, n * 4);
        if (val_offsets) memset(val_offsets, 0, n * 4);
        if (created_ms) memset(created_ms, 0, n * 8);
        return ok();
    }
    try {
        HOST_CALL(call, device);
        KeyImage m;  // keys | offsets | found | layer | val_offsets | created
        m.lay(offsets, stride, n);
        const auto p_found = m.add<uint8_t>(n, found);
        const auto p_layer = m.add<uint32_t>(n, layer);
        const auto p_val = m.add<uint32_t>(n, val_offsets);
        const auto p_cr = m.add<uint64_t>(n, created_ms);
        if ((rc = m.alloc(call, kWsMemGetIO)) || (rc = m.upload(call, keys, offsets, n))) return rc;
        if ((rc = memget_lookup(m.ptr(m.keys), m.ptr(m.off), stride, n, gc, active, nro, ro, log, m.ptr(p_found),
                                m.ptr(p_layer), m.ptr(p_val), m.ptr(p_cr), call.s)))
            return rc;
        if ((rc = call.down(found, m.ptr(p_found), n)) || (rc = call.down(layer, m.ptr(p_layer), n)) ||
            (rc = call.down(val_offsets, m.ptr(p_val), n)) || (rc = call.down(created_ms, m.ptr(p_cr), n)))
            return rc;
        return call.finish();
    } catch (const std::bad_alloc&) {
        return table_no_memory();
    }
}

// DataStore::get for a batch, bytes to values: the memtables, the tables for what they left open, the
// merge and the value log, all on the log's device from one upload of the keys.
int vbf_store_get_host(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                       const vbf_memtable* gc, const vbf_memtable* active, uint32_t nro, const vbf_memtable* const* ro,
                       uint32_t nsst, const vbf_table* const* tables, const vbf_filter* const* filters,
                       const vbf_vlog* log, int check_keys_flag, uint8_t* found, uint32_t* layer, uint32_t* table_idx,
                       uint32_t* val_offsets, uint64_t* created_ms, uint8_t* status, uint8_t* values,
                       uint64_t values_cap, uint64_t* value_off, uint64_t* value_bytes) {
    if (!value_bytes) return fail(VBF_EINVAL, "value_bytes is NULL");
    *value_bytes = 0;
    if (!log) return fail(VBF_EINVAL, "vlog is NULL");
    int device = -1;
    int rc = memget_check(keys, offsets, stride, n, gc, active, nro, ro, log, &device);
    if (rc || (rc = offsets_ascend(offsets, n))) return rc;
    if (nsst && !tables) return fail(VBF_EINVAL, "tables is NULL");
    for (uint32_t i = 0; i < nsst; ++i)
        if (!tables[i]) return fail(VBF_EINVAL, "tables[%u] is NULL", i);
    if (!nsst) filters = nullptr;
    if (filters)
        for (uint32_t i = 0; i < nsst; ++i)
            if (!filters[i]) return fail(VBF_EINVAL, "filters[%u] is NULL", i);
    if (device >= 0 && device != log->device)
        return fail(VBF_EINVAL, "the memtables live on device %d, the log on %d", device, log->device);
    device = log->device;
    for (uint32_t i = 0; i < nsst; ++i)
        if (tables[i]->device != device)
            return fail(VBF_EINVAL, "tables[%u] lives on device %d, the log on %d", i, tables[i]->device, device);
    if (!n) {
        if (value_off) value_off[0] = 0;
        return ok();
    }
    try {
        // Lock order as in vbf_table_get_host: the filters' locks and their drain, then the device.
        MultiLock lk(filters, filters ? nsst : 0);
        if ((rc = lk.drain())) return rc;
        if (filters)
            for (uint32_t i = 0; i < nsst; ++i)
                if (filters[i]->bits->device != device)
                    return fail(VBF_EINVAL, "filters[%u] lives on device %d, the log on %d", i,
                                filters[i]->bits->device, device);
        HOST_CALL(call, device);
        hipStream_t s = call.s;
        KeyImage m;  // keys | offsets | the merged answer | candidates | the tables' answer: 33 + nsst bytes per key
        m.lay(offsets, stride, n);
        const auto p_found = m.add<uint8_t>(n);
        const auto p_layer = m.add<uint32_t>(n);
        const auto p_val = m.add<uint32_t>(n);
        const auto p_cr = m.add<uint64_t>(n);
        const auto p_tidx = m.add<uint32_t>(n);
        const auto p_cand = m.add<uint8_t>(n * nsst, nsst);
        const auto t_found = m.add<uint8_t>(n, nsst);
        const auto t_idx = m.add<uint32_t>(n, nsst);
        const auto t_val = m.add<uint32_t>(n, nsst);
        const auto t_cr = m.add<uint64_t>(n, nsst);
        if ((rc = m.alloc(call, kWsStoreIO)) || (rc = m.upload(call, keys, offsets, n))) return rc;
        const uint8_t* d_keys = m.ptr(m.keys);
        const uint64_t* d_off = m.ptr(m.off);
        if ((rc = memget_lookup(d_keys, d_off, stride, n, gc, active, nro, ro, log, m.ptr(p_found), m.ptr(p_layer),
                                m.ptr(p_val), m.ptr(p_cr), s)))
            return rc;
        if (nsst) {
            if (filters) {  // filter_sstables_by_key_range (range.rs:91-147) with the tables' own key ranges
                std::vector<uint8_t> bounds;
                std::vector<uint64_t> boff;
                table_bounds(nsst, tables, &bounds, &boff);
                if ((rc = multi_probe(d_keys, d_off, stride, n, 1, nsst, filters, bounds.data(), boff.data(),
                                      m.ptr(p_cand), s)))
                    return rc;
            } else {
                HIP_TRY(hipMemsetAsync(m.ptr(p_cand), 1, n * nsst, s));
            }
            HIP_TRY(vbf::store_cand(m.ptr(p_found), n, nsst, m.ptr(p_cand), s));
            if ((rc = table_lookup(d_keys, d_off, stride, n, nsst, tables, m.ptr(p_cand), m.ptr(t_found), m.ptr(t_idx),
                                   m.ptr(t_val), m.ptr(t_cr), s)))
                return rc;
        }
        const vbf::StoreMergeArgs ma{n, m.ptr(p_found), m.ptr(p_layer), m.ptr(p_val), m.ptr(p_cr), m.ptr(t_found),
                                     m.ptr(t_idx), m.ptr(t_val), m.ptr(t_cr), m.ptr(p_tidx)};
        HIP_TRY(vbf::store_merge(ma, s));
        vbf::VlogGetArgs a;
        uint64_t total = 0;
        if ((rc = vlog_get_sizes(log, m.ptr(p_val), m.ptr(p_found), n, check_keys_flag ? d_keys : nullptr, d_off, stride, s, &a, &total)))
            return rc;
        *value_bytes = total;
        if ((rc = vlog_values_cap(values, values_cap, total))) return rc;
        if ((rc = call.down(found, m.ptr(p_found), n)) || (rc = call.down(layer, m.ptr(p_layer), n)) ||
            (rc = call.down(table_idx, m.ptr(p_tidx), n)) || (rc = call.down(val_offsets, m.ptr(p_val), n)) ||
            (rc = call.down(created_ms, m.ptr(p_cr), n)) || (rc = call.down(status, a.status, n)) ||
            (rc = call.down(value_off, a.voff, n + 1)))
            return rc;
        if (values && total) {
            DevImage vals;
            const auto p_values = vals.add<uint8_t>(total);
            if ((rc = vals.alloc(call, kWsVlogOut))) return rc;
            if ((rc = vlog_get_fill(a, vals.ptr(p_values), s)) || (rc = call.down(values, vals.ptr(p_values), total)))
                return rc;
        }
        return call.finish();
    } catch (const std::bad_alloc&) {
        return table_no_memory();
    }
}

}  // extern "C"

// ---- range scans over the whole store (DataStore::seek with vbf_store_get_host as the lookup) ----

namespace {

struct StoreScanOut {
    uint64_t* range_off;
    uint8_t* keys;
    uint64_t* key_off;
    uint8_t* tombstones;
    uint32_t* layer;
    uint32_t* table_idx;
    uint32_t* val_offsets;
    uint64_t* created_ms;
    uint8_t* status;
    uint8_t* values;
    uint64_t* value_off;
    bool per_entry() const {
        return key_off || tombstones || layer || table_idx || val_offsets || created_ms || status || value_off;
    }
    bool any() const { return range_off || keys || values || per_entry(); }
    void empty(uint64_t nranges) const {  // every range is empty
        if (range_off) memset(range_off, 0, (nranges + 1) * 8);
        if (key_off) key_off[0] = 0;
        if (value_off) value_off[0] = 0;
    }
};

// The bounds pass, the rank pass and the two scans on the log's device (bounds / bounds_off there).
// Three stream synchronisations: the descriptors' upload, the candidate total, then *n_out and
// *key_bytes.  `a` comes back ready for the emit passes; total == 0 ends after the second.
// Workspace: 64 bytes per layer for the descriptors at most, 24 per (range, layer) pair, 61 per
// candidate (listed flag and key length as u64 for scan_u64, their two scans, the key's address, the
// get's answer: time, layer, table, offset, found), plus the scans' scratch.
int store_scan_sizes(const uint8_t* bounds, const uint64_t* bounds_off, uint64_t nranges, const vbf_memtable* gc,
                     const vbf_memtable* active, uint32_t nro, const vbf_memtable* const* ro, uint32_t nsst,
                     const vbf_table* const* tables, const vbf_vlog* log, uint32_t flags, hipStream_t s,
                     vbf::StoreScanArgs* a, uint64_t* n_out, uint64_t* key_bytes) {
    *a = vbf::StoreScanArgs{};
    a->bounds = bounds;
    a->bounds_off = bounds_off;
    a->nranges = nranges;
    a->nmem = 2 + nro;
    a->nsst = nsst;
    a->flags = flags;
    a->log = log->bytes;
    a->log_len = log->len;
    a->log_base = log->base;
    std::vector<vbf::MemDesc> mem(a->nmem);
    if (gc) mem[0] = gc->desc;
    if (active) mem[1] = active->desc;
    for (uint32_t i = 0; i < nro; ++i) mem[2 + i] = ro[i]->desc;
    std::vector<vbf::TableDesc> tab(nsst);
    for (uint32_t i = 0; i < nsst; ++i) tab[i] = tables[i]->desc;
    const uint64_t mb = mem.size() * sizeof(vbf::MemDesc), tb = tab.size() * sizeof(vbf::TableDesc);
    void* ws = nullptr;
    int rc = get_workspace(s, align256(mb) + tb, &ws, kWsStoreScanDesc);
    if (rc) return rc;
    char* db = static_cast<char*>(ws);
    HIP_TRY(hipMemcpyAsync(db, mem.data(), mb, hipMemcpyHostToDevice, s));
    if (tb) HIP_TRY(hipMemcpyAsync(db + align256(mb), tab.data(), tb, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // pageable sources
    a->mem = reinterpret_cast<const vbf::MemDesc*>(db);
    a->tab = reinterpret_cast<const vbf::TableDesc*>(db + align256(mb));
    const uint64_t P = nranges * (a->nmem + nsst);
    size_t tmpb = 0;
    HIP_TRY(vbf::scan_u64(nullptr, &tmpb, nullptr, nullptr, P + 1, s));
    const uint64_t o_cnt = align256(P * 8), o_cbase = o_cnt + align256((P + 1) * 8);
    const uint64_t o_err = o_cbase + align256((P + 1) * 8), o_tmp = o_err + 256;
    if ((rc = get_workspace(s, o_tmp + tmpb, &ws, kWsStoreScanPairs))) return rc;
    char* pb = static_cast<char*>(ws);
    a->first = reinterpret_cast<uint64_t*>(pb);
    a->cnt = reinterpret_cast<uint64_t*>(pb + o_cnt);
    uint64_t* cbase = reinterpret_cast<uint64_t*>(pb + o_cbase);
    a->cbase = cbase;
    a->err = reinterpret_cast<uint32_t*>(pb + o_err);
    HIP_TRY(hipMemsetAsync(a->cnt + P, 0, 8, s));
    HIP_TRY(hipMemsetAsync(a->err, 0, 4, s));
    vbf::phase_begin(vbf::kPhaseScanRank, s);
    HIP_TRY(vbf::store_scan_bounds(*a, s));
    HIP_TRY(vbf::scan_u64(pb + o_tmp, &tmpb, a->cnt, cbase, P + 1, s));
    vbf::phase_end(vbf::kPhaseScanRank, s);
    uint64_t total = 0;
    uint32_t ev = 0;
    HIP_TRY(hipMemcpyAsync(&total, cbase + P, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&ev, a->err, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (ev & vbf::kScanErrBounds) return fail(VBF_EINVAL, "bounds_off is not nondecreasing");
    if (total > 0x7FFFFFFFull)
        return fail(VBF_EINVAL, "too many entries: %llu candidates in the ranges (limit 2^31 - 1)",
                    (unsigned long long)total);
    a->total = total;
    *n_out = *key_bytes = 0;
    if (!total) return VBF_OK;
    size_t tmpc = 0;
    HIP_TRY(vbf::scan_u64(nullptr, &tmpc, nullptr, nullptr, total + 1, s));
    const uint64_t q_len = (total + 1) * 8, q_opos = align256(q_len + (total + 1) * 8);
    const uint64_t q_kofs = q_opos + align256((total + 1) * 8), q_src = q_kofs + align256((total + 1) * 8);
    const uint64_t q_cr = q_src + align256(total * 8), q_layer = q_cr + align256(total * 8);
    const uint64_t q_tidx = q_layer + align256(total * 4), q_val = q_tidx + align256(total * 4);
    const uint64_t q_found = q_val + align256(total * 4), q_tmp = q_found + align256(total);
    if ((rc = get_workspace(s, q_tmp + tmpc, &ws, kWsStoreScan))) return rc;
    char* cb = static_cast<char*>(ws);
    a->m_keep = reinterpret_cast<uint64_t*>(cb);
    a->m_len = reinterpret_cast<uint64_t*>(cb + q_len);
    uint64_t* opos = reinterpret_cast<uint64_t*>(cb + q_opos);
    uint64_t* kofs = reinterpret_cast<uint64_t*>(cb + q_kofs);
    a->opos = opos;
    a->kofs = kofs;
    a->m_src = reinterpret_cast<const uint8_t**>(cb + q_src);
    a->m_created = reinterpret_cast<uint64_t*>(cb + q_cr);
    a->m_layer = reinterpret_cast<uint32_t*>(cb + q_layer);
    a->m_tidx = reinterpret_cast<uint32_t*>(cb + q_tidx);
    a->m_val = reinterpret_cast<uint32_t*>(cb + q_val);
    a->m_found = reinterpret_cast<uint8_t*>(cb + q_found);
    HIP_TRY(hipMemsetAsync(a->m_keep, 0, (total + 1) * 16, s));  // m_keep | m_len
    vbf::phase_begin(vbf::kPhaseScanRank, s);
    HIP_TRY(vbf::store_scan_rank(*a, s));
    HIP_TRY(vbf::scan_u64(cb + q_tmp, &tmpc, a->m_keep, opos, total + 1, s));
    HIP_TRY(vbf::scan_u64(cb + q_tmp, &tmpc, a->m_len, kofs, total + 1, s));
    vbf::phase_end(vbf::kPhaseScanRank, s);
    HIP_TRY(hipMemcpyAsync(n_out, opos + total, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(key_bytes, kofs + total, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&ev, a->err, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (ev & vbf::kScanErrRank) {
        *n_out = *key_bytes = 0;
        return fail(VBF_EINVAL, "a merged rank fell outside its range: a layer's buffers changed since open");
    }
    return VBF_OK;
}

}  // namespace

extern "C" {

int vbf_store_scan_host(const uint8_t* bounds, const uint64_t* bounds_off, uint64_t nranges, const vbf_memtable* gc,
                        const vbf_memtable* active, uint32_t nro, const vbf_memtable* const* ro, uint32_t nsst,
                        const vbf_table* const* tables, const vbf_vlog* log, uint32_t flags, int check_keys_flag,
                        uint64_t* range_off, uint8_t* keys, uint64_t keys_cap, uint64_t* key_off, uint8_t* tombstones,
                        uint32_t* layer, uint32_t* table_idx, uint32_t* val_offsets, uint64_t* created_ms,
                        uint8_t* status, uint64_t entries_cap, uint8_t* values, uint64_t values_cap,
                        uint64_t* value_off, uint64_t* n_out, uint64_t* key_bytes, uint64_t* value_bytes) {
    if (!n_out || !key_bytes || !value_bytes) return fail(VBF_EINVAL, "n_out / key_bytes / value_bytes is NULL");
    *n_out = *key_bytes = *value_bytes = 0;
    int device = -1;
    int rc = memget_check(nullptr, nullptr, 0, 0, gc, active, nro, ro, log, &device);  // the handles: no key batch here
    if (rc) return rc;
    if (!log) return fail(VBF_EINVAL, "vlog is NULL");
    if (flags & ~(uint32_t)(VBF_SCAN_KEEP_TOMBSTONES | VBF_SCAN_END_EXCLUSIVE))
        return fail(VBF_EINVAL, "unknown flags 0x%x", flags);
    if (nsst && !tables) return fail(VBF_EINVAL, "tables is NULL");
    for (uint32_t i = 0; i < nsst; ++i)
        if (!tables[i]) return fail(VBF_EINVAL, "tables[%u] is NULL", i);
    if (nranges && !bounds_off) return fail(VBF_EINVAL, "bounds_off is NULL");
    if (nranges && !bounds) return fail(VBF_EINVAL, "bounds is NULL");
    // the (range, layer) pairs are scanned like the candidates: below 2^31 items
    const uint64_t nl = 2 + (uint64_t)nro + nsst;
    if (nranges > 0x7FFFFFFEull / nl)
        return fail(VBF_EINVAL, "too many entries: %llu ranges x %llu layers", (unsigned long long)nranges,
                    (unsigned long long)nl);
    for (uint64_t i = 0; i < 2 * nranges; ++i)
        if (bounds_off[i] > bounds_off[i + 1])
            return fail(VBF_EINVAL, "bounds_off decreases at entry %llu", (unsigned long long)(i + 1));
    const StoreScanOut o{range_off, keys, key_off, tombstones, layer, table_idx, val_offsets, created_ms, status,
                         values, value_off};
    const bool layers = gc || active || nro || nsst;
    if (layers) {  // everything on the log's device
        if (device >= 0 && device != log->device)
            return fail(VBF_EINVAL, "the memtables live on device %d, the log on %d", device, log->device);
        for (uint32_t i = 0; i < nsst; ++i)
            if (tables[i]->device != log->device)
                return fail(VBF_EINVAL, "tables[%u] lives on device %d, the log on %d", i, tables[i]->device,
                            log->device);
    }
    if (!nranges || !layers) {  // nothing to scan: every range is empty, no device work
        o.empty(nranges);
        return ok();
    }
    try {
        HOST_CALL(call, log->device);
        hipStream_t s = call.s;
        // bounds and their offsets, rebased to positions in the device copy
        const uint64_t b0 = bounds_off[0], bbytes = bounds_off[2 * nranges] - b0;
        DevImage in;
        const auto p_bounds = in.add<uint8_t>(bbytes + 1);
        const auto p_boff = in.add<uint64_t>(2 * nranges + 1);
        if ((rc = in.alloc(call, kWsStoreScanIn))) return rc;
        if ((rc = call.up(in.ptr(p_bounds), bbytes ? bounds + b0 : nullptr, bbytes)) ||
            (rc = call.up_rebased(in.ptr(p_boff), bounds_off, 2 * nranges + 1)))
            return rc;  // pageable sources: store_scan_sizes synchronises before it launches
        vbf::StoreScanArgs a;
        if ((rc = store_scan_sizes(in.ptr(p_bounds), in.ptr(p_boff), nranges, gc, active, nro, ro, nsst, tables, log,
                                   flags, s, &a, n_out, key_bytes)))
            return rc;
        const uint64_t n = *n_out, kb = *key_bytes;
        if (!n) {  // nothing listed: store_scan_sizes returned synchronised
            call.settled();
            o.empty(nranges);
            return ok();
        }
        if (n > kGetMaxKeys)  // the value lengths' scan runs over n + 1 items
            return fail(VBF_EINVAL, "too many entries: %llu listed (limit 2^31 - 2)", (unsigned long long)n);
        // The listed entries on the device: the emit passes fill them, the value fetch reads them, the
        // capacity rule is applied once all three sizes are known, and only then anything goes down.
        DevImage out;
        const auto p_roff = out.add<uint64_t>(nranges + 1);
        const auto p_koff = out.add<uint64_t>(n + 1);
        const auto p_cr = out.add<uint64_t>(n);
        const auto p_layer = out.add<uint32_t>(n);
        const auto p_idx = out.add<uint32_t>(n);
        const auto p_val = out.add<uint32_t>(n);
        const auto p_tomb = out.add<uint8_t>(n);
        const auto p_found = out.add<uint8_t>(n);
        const auto p_keys = out.add<uint8_t>(kb + 1, keys || check_keys_flag);
        if ((rc = out.alloc(call, kWsStoreScanOut))) return rc;
        a.range_off = out.ptr(p_roff);
        a.keys = out.ptr(p_keys);
        a.key_off = out.ptr(p_koff);
        a.tomb = out.ptr(p_tomb);
        a.layer = out.ptr(p_layer);
        a.table_idx = out.ptr(p_idx);
        a.val_off = out.ptr(p_val);
        a.created = out.ptr(p_cr);
        a.found = out.ptr(p_found);
        vbf::phase_begin(vbf::kPhaseScanEmit, s);
        HIP_TRY(vbf::store_scan_emit(a, s));
        HIP_TRY(vbf::store_scan_keys(a, s));
        vbf::phase_end(vbf::kPhaseScanEmit, s);
        vbf::VlogGetArgs va;
        uint64_t total = 0;
        if ((rc = vlog_get_sizes(log, a.val_off, a.found, n, check_keys_flag ? a.keys : nullptr, a.key_off, 0, s, &va,
                                 &total)))
            return rc;
        *value_bytes = total;
        if (o.per_entry() && entries_cap < n)
            return fail(VBF_EINVAL, "entries_cap %llu < %llu listed entries", (unsigned long long)entries_cap,
                        (unsigned long long)n);
        if (keys && keys_cap < kb)
            return fail(VBF_EINVAL, "keys_cap %llu < %llu key bytes", (unsigned long long)keys_cap,
                        (unsigned long long)kb);
        if ((rc = vlog_values_cap(values, values_cap, total))) return rc;
        if (!o.any()) {  // the size query: vlog_get_sizes returned synchronised
            call.settled();
            return ok();
        }
        if ((rc = call.down(range_off, a.range_off, nranges + 1)) || (rc = call.down(key_off, a.key_off, n + 1)) ||
            (rc = call.down(keys, a.keys, kb)) || (rc = call.down(tombstones, a.tomb, n)) ||
            (rc = call.down(layer, a.layer, n)) || (rc = call.down(table_idx, a.table_idx, n)) ||
            (rc = call.down(val_offsets, a.val_off, n)) || (rc = call.down(created_ms, a.created, n)) ||
            (rc = call.down(status, va.status, n)) || (rc = call.down(value_off, va.voff, n + 1)))
            return rc;
        if (values && total) {
            DevImage vals;
            const auto p_values = vals.add<uint8_t>(total);
            if ((rc = vals.alloc(call, kWsVlogOut))) return rc;
            if ((rc = vlog_get_fill(va, vals.ptr(p_values), s)) || (rc = call.down(values, vals.ptr(p_values), total)))
                return rc;
        }
        return call.finish();
    } catch (const std::bad_alloc&) {
        return table_no_memory();
    }
}

}  // extern "C"
