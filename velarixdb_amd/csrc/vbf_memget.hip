// Batched memtable lookups on gfx950: steps 0-2 of DataStore::get (src/db/store.rs:442-472) before
// the SSTs get their turn, and the small passes that join them with vbf_table.hip's answers.
//
// A vbf_memtable is what vbf_memtable_sort_* + the gather leave on the device: E distinct keys in
// ascending `Ord for [u8]` order (off[E + 1] into keys), the three per-entry arrays, and pfx[E], each
// key's first 8 bytes as a big-endian word, zero-padded (k_mem_prefix, at open).  Key order implies
// pfx order, but not strictly: "ab" and "ab\0" share a prefix, and so does every key of a family with
// a common 8-byte stem.
//
//   k_mem_get<false> : the plain version (VBF_MEMGET=0).  One lane per key, the fold of store.rs in
//                      registers; per layer a binary search with cmp_keys over off / keys, as
//                      k_gc_overlay does.
//   k_mem_get<true>  : the default.  A lookup is a chain of dependent reads, so the chain is cut
//                      twice.  A step compares pfx[mid], one 8-byte load from a dense array, and reads
//                      off[mid], off[mid + 1] and key bytes only on a prefix tie (the tie is what
//                      makes the search exact: the comparator is (pfx, key), the sort's own).  And the
//                      top of every search runs in LDS: per layer the workgroup stages an evenly
//                      strided sample of pfx (at most kMemSample = 4096 words, 32 KiB; all of pfx
//                      for E <= 4096), each lane takes the sample's lower and upper bound of its
//                      prefix, and only the log2(E / samples) steps inside those bounds go to memory.
//                      A workgroup looks up kMemKeys = 1024 keys, four per lane, so a staged sample is
//                      read by 1024 searches.
//
// Precedence (per key, the same in both): gc_stands / fold_hit / fold_close of vbf_store_fold.hpp,
// shared with the whole-store range scan.
//
//   k_store_cand  : rows of the SST candidate matrix of the keys a memtable decided are zeroed.
//   k_store_merge : a memtable's answer stands, otherwise the tables' with layer = 2^31 | table.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vbf_kernels.hpp"
#include "vbf_keycmp.hpp"
#include "vbf_store_fold.hpp"

namespace vbf {

namespace {

constexpr uint32_t kMemSample = 4096;  // pfx words staged per layer: 32 KiB of LDS
constexpr uint32_t kMemPer = 4;        // keys per lane
constexpr uint32_t kMemKeys = 256 * kMemPer;

__global__ __launch_bounds__(256) void k_mem_prefix(const uint8_t* keys, const uint64_t* off, uint64_t n,
                                                    uint64_t* pfx) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const uint64_t b = off[e];
    pfx[e] = key_prefix8(keys + b, off[e + 1] - b);
}

struct Query {
    const uint8_t* k;
    uint64_t len, pfx;
};

// The entry of `d` that holds q, d.n when none does: a binary search over [lo, hi) by full keys.
__device__ __forceinline__ uint64_t find_plain(const MemDesc& d, const Query& q) {
    uint64_t lo = 0, hi = d.n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        const uint64_t k0 = d.off[mid], k1 = d.off[mid + 1];
        const int c = cmp_keys(d.keys + k0, k1 - k0, q.k, q.len);
        if (c == 0) return mid;
        if (c < 0) lo = mid + 1;
        else hi = mid;
    }
    return d.n;
}

// The same by (pfx, key) inside [lo, hi): every entry before lo is smaller, every one from hi on greater.
__device__ __forceinline__ uint64_t find_pfx(const MemDesc& d, const Query& q, uint64_t lo, uint64_t hi) {
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        const uint64_t p = d.pfx[mid];
        int c;
        if (p != q.pfx) {
            c = p < q.pfx ? -1 : 1;
        } else {
            const uint64_t k0 = d.off[mid], k1 = d.off[mid + 1];
            c = cmp_keys(d.keys + k0, k1 - k0, q.k, q.len);
            if (c == 0) return mid;
        }
        if (c < 0) lo = mid + 1;
        else hi = mid;
    }
    return d.n;
}

__device__ __forceinline__ void store(const MemGetArgs& a, uint64_t j, const Fold& f) {
    const bool hit = f.found != 0;
    if (a.found) a.found[j] = f.found;
    if (a.layer) a.layer[j] = hit ? f.layer : 0xFFFFFFFFu;
    if (a.val_off) a.val_off[j] = hit ? f.val : 0;
    if (a.created) a.created[j] = hit ? (uint64_t)f.time : 0;
}

template <bool kSampled>
__global__ __launch_bounds__(256) void k_mem_get(MemGetArgs a) {
    __shared__ uint64_t smp[kSampled ? kMemSample : 1];
    const uint64_t base = (uint64_t)blockIdx.x * kMemKeys + threadIdx.x;
    Query q[kMemPer];
    Fold f[kMemPer];
#pragma unroll
    for (uint32_t r = 0; r < kMemPer; ++r) {
        const uint64_t j = base + (uint64_t)r * 256;
        f[r] = Fold{0, j >= a.n, 0, 0, 0};
        q[r] = Query{a.keys, 0, 0};
        if (j < a.n) {
            const uint64_t b = a.offsets ? a.offsets[j] : j * a.stride;
            q[r].k = a.keys + b;
            q[r].len = a.offsets ? a.offsets[j + 1] - b : a.stride;
            q[r].pfx = key_prefix8(q[r].k, q[r].len);
        }
    }
    const uint32_t nl = 2 + a.nro;
    for (uint32_t L = 0; L < nl; ++L) {  // uniform over the workgroup: the barriers below are safe
        const MemDesc d = a.layers[L];
        if (d.n == 0) continue;
        if constexpr (kSampled) {
            // sample i = pfx[i * step], i < S: step = ceil(E / 4096), S = ceil(E / step) <= 4096
            const uint64_t step = (d.n + kMemSample - 1) / kMemSample;
            const uint32_t S = (uint32_t)((d.n + step - 1) / step);
            __syncthreads();  // the previous layer's searches are done with smp
            for (uint32_t i = threadIdx.x; i < S; i += 256) smp[i] = d.pfx[(uint64_t)i * step];
            __syncthreads();
#pragma unroll
            for (uint32_t r = 0; r < kMemPer; ++r) {
                if (f[r].decided) continue;
                const uint64_t p = q[r].pfx;
                uint32_t lo = 0, hi = S;  // sl: the first sample >= p
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (smp[mid] < p) lo = mid + 1;
                    else hi = mid;
                }
                const uint32_t sl = lo;
                hi = S;  // su: the first sample > p
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (smp[mid] <= p) lo = mid + 1;
                    else hi = mid;
                }
                const uint32_t su = lo;
                // pfx[(sl - 1) * step] < p: a match lies behind it; pfx[su * step] > p: before it
                const uint64_t b0 = sl ? (uint64_t)(sl - 1) * step + 1 : 0;
                const uint64_t b1 = su < S ? (uint64_t)su * step : d.n;
                const uint64_t e = find_pfx(d, q[r], b0, b1);
                if (e < d.n) fold_hit(a, d, L, e, f[r]);
            }
        } else {
#pragma unroll
            for (uint32_t r = 0; r < kMemPer; ++r) {
                if (f[r].decided) continue;
                const uint64_t e = find_plain(d, q[r]);
                if (e < d.n) fold_hit(a, d, L, e, f[r]);
            }
        }
    }
#pragma unroll
    for (uint32_t r = 0; r < kMemPer; ++r) {
        const uint64_t j = base + (uint64_t)r * 256;
        if (j >= a.n) continue;
        fold_close(f[r]);
        store(a, j, f[r]);
    }
}

__global__ __launch_bounds__(256) void k_store_cand(const uint8_t* found, uint64_t n, uint32_t nsst, uint8_t* cand) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;  // one lane per matrix byte
    if (i >= n * nsst) return;
    if (found[i / nsst]) cand[i] = 0;
}

__global__ __launch_bounds__(256) void k_store_merge(StoreMergeArgs a) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= a.n) return;
    uint32_t who = 0xFFFFFFFFu;
    if (a.found[j] == 0 && a.t_found && a.t_found[j] != 0) {
        who = a.t_idx[j];
        a.found[j] = a.t_found[j];
        a.layer[j] = 0x80000000u | who;
        a.val_off[j] = a.t_val[j];
        a.created[j] = a.t_created[j];
    }
    a.table_idx[j] = who;
}

}  // namespace

hipError_t mem_prefixes(const uint8_t* keys, const uint64_t* off, uint64_t n, uint64_t* pfx, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_mem_prefix, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, keys, off, n, pfx);
    return hipGetLastError();
}

hipError_t mem_get(const MemGetArgs& a, bool sampled, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    const dim3 grid((uint32_t)((a.n + kMemKeys - 1) / kMemKeys));  // n < 2^31
    if (sampled) hipLaunchKernelGGL(k_mem_get<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_mem_get<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t store_cand(const uint8_t* found, uint64_t n, uint32_t nsst, uint8_t* cand, hipStream_t s) {
    const uint64_t cells = n * nsst;
    if (cells == 0) return hipSuccess;
    const uint64_t nb = (cells + 255) / 256;
    if (nb > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_store_cand, dim3((uint32_t)nb), dim3(256), 0, s, found, n, nsst, cand);
    return hipGetLastError();
}

hipError_t store_merge(const StoreMergeArgs& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_store_merge, dim3((uint32_t)((a.n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace vbf
