// Memtable flush on gfx950: a batch of puts in arrival order -> SkipMap order, and the memtable's
// filter step over the batch.
//
// MemTable::insert (memtable/mem.rs:207-221) is `if !contains(key) { set(key) }` on the filter and
// SkipMap::insert on the entries; crossbeam-skiplist removes an entry of the same key before it
// inserts, so the last put of a key wins.  Flusher::flush hands the map to Table::write_to_file
// (flush/flusher.rs:37-64, sst/table.rs:258-326) in ascending `Ord for [u8]` order.
//
// The sort:
//   1. k_mt_check / k_mt_prefix: the offsets are checked (descending offsets would make key
//      lengths wrap) and copied -- or generated from the stride -- into an array the later passes
//      index; on a bad batch every key of the copy is empty, so nothing reads out of bounds and
//      the entry point reports the error.  (id, big-endian 8-byte prefix) pairs for every entry.
//   2. k_mt_tile_sort: one workgroup sorts one tile of kMtTile pairs in LDS (bitonic network) by
//      (prefix, full key, id).  The id as the last tie-break makes the order total, so the network
//      sorts equal keys by arrival.  The key bytes are read only on a prefix tie.
//   3. the compaction merge's levels (merge_levels_from) over the tile boundaries: stable, the
//      earlier tile first on equal keys, so every group of equal keys stays in arrival order.
//   4. k_mt_keep: position i survives when position i + 1 holds another key -- the group's last
//      put; then the select.
//
// The filter step (filter_insert_*): `first[b]` per filter bit holds 0 where the bit was set
// before the batch, else the smallest j + 1 among the keys j that hash to b (atomicMin).  Key j
// was not contained at its turn iff it owns one of its bits: a contained key has every bit owned
// by an earlier key or the prior contents, and a skipped set never owns a bit, so skips do not
// change the minima.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "keyhash.hpp"
#include "sip13.hpp"
#include "vbf_keycmp.hpp"
#include "vbf_kernels.hpp"

namespace vbf {

constexpr uint32_t kMtTile = 2048;  // the merge's tile (compact_tile()): 24 KB of LDS
constexpr uint32_t kMtNone = 0xFFFFFFFFu;

// err[0] = the first e with offsets[e + 1] < offsets[e]; stays 0xFFFFFFFF on a good batch.
__global__ __launch_bounds__(256) void k_mt_check(const uint64_t* offsets, uint64_t n, uint32_t* err) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n && offsets[e + 1] < offsets[e]) atomicMin(err, (uint32_t)e);  // n < 2^31
}

__global__ __launch_bounds__(256) void k_mt_prefix(const uint8_t* keys, const uint64_t* offsets, uint64_t stride,
                                                   uint64_t n, const uint32_t* err, uint64_t* soff, uint32_t* ids,
                                                   uint64_t* pfx) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e > n) return;
    uint64_t b, end;
    if (offsets) {
        const bool bad = *err != kMtNone;
        b = bad ? 0 : offsets[e];
        end = bad ? 0 : offsets[e < n ? e + 1 : e];
    } else {
        b = e * stride;
        end = b + stride;
    }
    soff[e] = b;
    if (e == n) return;
    ids[e] = (uint32_t)e;
    pfx[e] = key_prefix8(keys + b, end - b);
}

// x after y in (prefix, full key, id) order; a padding slot (id kMtNone) after every entry.
__device__ __forceinline__ bool mt_after(const CompactArgs& a, uint64_t px, uint32_t x, uint64_t py, uint32_t y) {
    if (x == kMtNone || y == kMtNone) return x == kMtNone && y != kMtNone;
    if (px != py) return px > py;
    const int c = cmp_ids(a, x, y);
    return c ? c > 0 : x > y;
}

// One workgroup per tile of kMtTile (id, prefix) pairs, sorted in place.  The last tile is padded
// in LDS with slots that sort last and are never stored.
__global__ __launch_bounds__(256) void k_mt_tile_sort(CompactArgs a, uint64_t n, uint32_t* ids, uint64_t* pfx) {
    __shared__ uint64_t sp[kMtTile];
    __shared__ uint32_t si[kMtTile];
    const uint64_t base = (uint64_t)blockIdx.x * kMtTile;
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(kMtTile, n - base);
    for (uint32_t x = threadIdx.x; x < kMtTile; x += 256) {
        si[x] = x < cnt ? ids[base + x] : kMtNone;
        sp[x] = x < cnt ? pfx[base + x] : ~0ull;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= kMtTile; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < kMtTile / 2; t += 256) {
                const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;  // lo < kMtTile - j
                const bool up = (lo & k) == 0;
                const uint64_t pl = sp[lo], ph = sp[hi];
                const uint32_t il = si[lo], ih = si[hi];
                // ascending blocks swap when lo is after hi, descending ones when it is not
                if (mt_after(a, pl, il, ph, ih) == up) {
                    sp[lo] = ph;
                    sp[hi] = pl;
                    si[lo] = ih;
                    si[hi] = il;
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t x = threadIdx.x; x < cnt; x += 256) {
        ids[base + x] = si[x];
        pfx[base + x] = sp[x];
    }
}

__global__ __launch_bounds__(256) void k_mt_keep(CompactArgs a, const uint32_t* order, const uint64_t* opfx,
                                                 uint64_t n, uint8_t* keep) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    keep[p] = p + 1 == n || cmp_pid(a, opfx[p], order[p], opfx[p + 1], order[p + 1]) != 0;
}

uint32_t memtable_tile() { return kMtTile; }

hipError_t memtable_prefixes(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n, uint32_t* err,
                             uint64_t* soff, uint32_t* ids, uint64_t* pfx, hipStream_t s) {
    if (offsets) hipLaunchKernelGGL(k_mt_check, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, offsets, n, err);
    hipLaunchKernelGGL(k_mt_prefix, dim3((uint32_t)((n + 1 + 255) / 256)), dim3(256), 0, s, keys, offsets, stride, n,
                       err, soff, ids, pfx);
    return hipGetLastError();
}

hipError_t memtable_tile_sort(const CompactArgs& a, uint64_t n, uint32_t* ids, uint64_t* pfx, hipStream_t s) {
    hipLaunchKernelGGL(k_mt_tile_sort, dim3((uint32_t)((n + kMtTile - 1) / kMtTile)), dim3(256), 0, s, a, n, ids, pfx);
    return hipGetLastError();
}

hipError_t memtable_keep(const CompactArgs& a, const uint32_t* order, const uint64_t* opfx, uint64_t n, uint8_t* keep,
                         hipStream_t s) {
    hipLaunchKernelGGL(k_mt_keep, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, a, order, opfx, n, keep);
    return hipGetLastError();
}

// ---- the filter step ----

__global__ __launch_bounds__(256) void k_fi_init(const uint32_t* words, uint32_t m, uint32_t* first) {
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (b < m) first[b] = ((words[b >> 5] >> (b & 31)) & 1u) ? 0u : kMtNone;
}

template <bool LP>
__device__ __forceinline__ Prefix fi_prefix(const KeyBatch& kb, uint64_t j) {
    const uint64_t b = kb.offsets ? kb.offsets[j] - kb.off_base : j * kb.stride;
    const uint64_t len = kb.offsets ? kb.offsets[j + 1] - kb.offsets[j] : kb.stride;
    return key_prefix_at<LP>(kb.keys, b, len);
}

template <bool LP>
__global__ __launch_bounds__(256) void k_fi_claim(KeyBatch kb, uint32_t m, uint64_t mu, uint32_t k, uint32_t* first) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= kb.n) return;
    const Prefix p = fi_prefix<LP>(kb, j);
    for (uint32_t i = 0; i < k; ++i) atomicMin(first + fast_mod(prefix_hash(p, i), m, mu), (uint32_t)(j + 1));
}

// partial[block] = the block's keys that own one of their bits.
template <bool LP>
__global__ __launch_bounds__(256) void k_fi_count(KeyBatch kb, uint32_t m, uint64_t mu, uint32_t k,
                                                  const uint32_t* first, uint32_t* partial) {
    __shared__ uint32_t wsum[4];
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool fresh = false;
    if (j < kb.n) {
        const Prefix p = fi_prefix<LP>(kb, j);
        for (uint32_t i = 0; i < k && !fresh; ++i)
            fresh = first[fast_mod(prefix_hash(p, i), m, mu)] == (uint32_t)(j + 1);
    }
    const unsigned long long mask = __ballot(fresh);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

uint64_t filter_insert_partials(uint64_t n) { return (n + 255) / 256; }

// Queues init, claim and count; the number of new keys is added to *count.  m > 0, k > 0, n > 0.
hipError_t filter_insert_count(const KeyBatch& kb, uint32_t m, uint32_t k, const uint32_t* words, uint32_t* first,
                               uint32_t* partial, unsigned long long* count, hipStream_t s) {
    const uint64_t mu = ~0ull / m;
    const uint32_t blocks = (uint32_t)filter_insert_partials(kb.n);
    hipLaunchKernelGGL(k_fi_init, dim3((uint32_t)(((uint64_t)m + 255) / 256)), dim3(256), 0, s, words, m, first);
    if (kb.len_prefix) {
        hipLaunchKernelGGL(k_fi_claim<true>, dim3(blocks), dim3(256), 0, s, kb, m, mu, k, first);
        hipLaunchKernelGGL(k_fi_count<true>, dim3(blocks), dim3(256), 0, s, kb, m, mu, k, first, partial);
    } else {
        hipLaunchKernelGGL(k_fi_claim<false>, dim3(blocks), dim3(256), 0, s, kb, m, mu, k, first);
        hipLaunchKernelGGL(k_fi_count<false>, dim3(blocks), dim3(256), 0, s, kb, m, mu, k, first, partial);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_count_finish(partial, blocks, count, s);
}

}  // namespace vbf
