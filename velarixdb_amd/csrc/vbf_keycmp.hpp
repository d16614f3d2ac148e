// vbf_keycmp.hpp -- Rust `Ord for [u8]` over the entries of an arena, shared by the compaction
// merge (vbf_compact.hip) and the memtable sort (vbf_memtable.hip): both order (8-byte big-endian
// prefix, entry id) pairs and read the key bytes only on a prefix tie.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vbf_kernels.hpp"
#include "vbf_keyprefix.hpp"

namespace vbf {

// 8 bytes at a time as big-endian words, then the tail byte by byte.
__device__ __forceinline__ int cmp_keys(const uint8_t* ka, uint64_t la, const uint8_t* kb, uint64_t lb) {
    const uint64_t n = la < lb ? la : lb;
    uint64_t i = 0;
    for (; i + 8 <= n; i += 8) {
        const uint64_t x = ld_be64(ka + i), y = ld_be64(kb + i);
        if (x != y) return x < y ? -1 : 1;
    }
    for (; i < n; ++i) {
        const uint32_t x = ka[i], y = kb[i];
        if (x != y) return x < y ? -1 : 1;
    }
    return la < lb ? -1 : (la > lb ? 1 : 0);
}

__device__ __forceinline__ int cmp_ids(const CompactArgs& a, uint32_t x, uint32_t y) {
    const uint64_t bx = a.offsets[x], by = a.offsets[y];
    return cmp_keys(a.keys + bx, a.offsets[x + 1] - bx, a.keys + by, a.offsets[y + 1] - by);
}

// (prefix, id) order: prefixes first, the full keys only on a prefix tie.
__device__ __forceinline__ int cmp_pid(const CompactArgs& a, uint64_t px, uint32_t x, uint64_t py, uint32_t y) {
    if (px != py) return px < py ? -1 : 1;
    return cmp_ids(a, x, y);
}

}  // namespace vbf
