// vbf_keyprefix.hpp -- a key's first 8 bytes as a big-endian word: the first half of the (prefix,
// key) comparator of the memtable sort, the compaction merge (vbf_keycmp.hpp) and the memtable
// searches (vbf_memget.hip, vbf_store_scan.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vbf {

// 8 bytes at a time as big-endian words (global memory takes unaligned 8-byte loads).
__device__ __forceinline__ uint64_t ld_be64(const uint8_t* p) {
    uint64_t w;
    __builtin_memcpy(&w, p, 8);
    return __builtin_bswap64(w);
}

// Big-endian 8-byte prefix of a key (zero-padded): prefixes order keys except on ties.
__device__ __forceinline__ uint64_t key_prefix8(const uint8_t* k, uint64_t len) {
    if (len >= 8) return ld_be64(k);
    uint64_t w = 0;
    for (uint64_t i = 0; i < len; ++i) w |= (uint64_t)k[i] << (56 - 8 * i);
    return w;
}

}  // namespace vbf
