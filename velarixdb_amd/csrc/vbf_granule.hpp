// vbf_granule.hpp -- the pieces of the copies that divide their work by OUTPUT bytes, shared by the
// value-log reads and appends (vbf_vlog.hip) and the GC's emit (vbf_gc.hip): the slice of the
// destination a workgroup owns, the masked 16-byte loads, the one store per granule and the searches
// that find the items overlapping a slice.  See vbf_vlog.hip's head for the scheme.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vbf_kernels.hpp"

namespace vbf {

constexpr uint32_t kHdr = 17;
constexpr uint32_t kGran = 16;
constexpr uint32_t kVlogWindow = 1024;  // items (entries) of a slice whose positions are staged in LDS
using u128 = unsigned __int128;

// The slice of workgroup b in the destination's address space.  `head` = the bytes of the first
// granule in front of out[0]; positions x count from that granule's start, so x % 16 == 0 is a
// granule's start whatever the alignment of `out`, and stream position p = x - head.
struct Slice {
    uint64_t head, x0, x1, end;
};
__device__ __forceinline__ Slice slice_of(const uint8_t* out, uint64_t total) {
    Slice s;
    s.head = reinterpret_cast<uintptr_t>(out) & (kGran - 1);
    s.end = s.head + total;
    s.x0 = (uint64_t)blockIdx.x * kVlogSlice;
    s.x1 = s.x0 + kVlogSlice < s.end ? s.x0 + kVlogSlice : s.end;
    return s;
}

// n (1..16) source bytes at p as the low bytes of a word, the bytes above them zero.  whole: all of
// p[0..16) may be read (one 16-byte load at p's own alignment); otherwise only the n bytes are.
__device__ __forceinline__ u128 ld_piece(const uint8_t* p, uint32_t n, bool whole) {
    u128 v;
    if (whole) {
        __builtin_memcpy(&v, p, 16);
    } else {
        v = 0;
        for (uint32_t b = 0; b < n; ++b) v |= (u128)p[b] << (8 * b);
    }
    if (n < kGran) v &= ((u128)1 << (8 * n)) - 1;
    return v;
}

// One granule's store: g = the 16 bytes of positions [x, x + 16), of which [lo, hi) are inside the
// stream.  A whole granule is one aligned 16-byte store; a ragged one stores its bytes singly.
__device__ __forceinline__ void store_gran(uint8_t* out, const Slice& s, uint64_t x, uint64_t lo, uint64_t hi, u128 g) {
    uint8_t* dst = out + x - s.head;  // (out - head) is 16-byte aligned; never dereferenced below out
    if (hi - lo == kGran) {
        const uint64_t w0 = (uint64_t)g, w1 = (uint64_t)(g >> 64);
        *reinterpret_cast<uint4*>(dst) =
            make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
        return;
    }
    for (uint64_t y = lo; y < hi; ++y) dst[y - x] = (uint8_t)(g >> (8 * (uint32_t)(y - x)));
}

// The largest i in [lo, hi] with f(i) <= p, for nondecreasing f with f(lo) <= p.
template <class F>
__device__ __forceinline__ uint64_t last_le(uint64_t lo, uint64_t hi, uint64_t p, F&& f) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (f(mid) <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// The first and the last item (entry) that overlap the slice, found once per workgroup by two lanes:
// the largest i in [0, n - 1] with start(i) <= the slice's first / last stream position.
template <class F>
__device__ __forceinline__ void slice_items(const Slice& s, uint64_t n, F&& start, uint64_t* sh) {
    if (threadIdx.x == 0 || threadIdx.x == 64) {
        const uint64_t x = threadIdx.x == 0 ? (s.x0 > s.head ? s.x0 : s.head) : s.x1 - 1;
        sh[threadIdx.x / 64] = last_le(0, n - 1, x - s.head, start);
    }
    __syncthreads();
}

// Workgroups of the balanced copies: one per kVlogSlice bytes of the granule-aligned range that
// holds out[0..total).
inline uint64_t slices_of(const uint8_t* out, uint64_t total) {
    const uint64_t head = reinterpret_cast<uintptr_t>(out) & (kGran - 1);
    return (head + total + kVlogSlice - 1) / kVlogSlice;
}

}  // namespace vbf
