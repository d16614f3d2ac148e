// vbf_store_fold.hpp -- DataStore::get's precedence over the memtable layers (src/db/store.rs:
// 442-472), stated once for the point lookups (k_mem_get, vbf_memget.hip) and the whole-store range
// scan (k_sscan_rank, vbf_store_scan.hip).  Layer 0 is the gc table, 1 the active memtable, 2 + r
// read-only memtable r.
//
// The gc layer decides only with a live entry whose log header (vbf_vlog.hip's window tests) is a
// live value or BAD; the active memtable decides whatever it holds; the read-only tables fold by
// strictly greater signed time from 0, the earlier table on a tie; what is left at time <= 0 is not
// found.  `A` is the kernel's argument struct: its log / log_len / log_base are the log window, read
// only for hits in layer 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vbf_kernels.hpp"

namespace vbf {

constexpr uint64_t kLogHdr = 17;

// vbf_vlog_get_*'s window tests on the header at `off`: true when the gc entry's hit stands (a live
// value, or BAD, which the value fetch reports), false for NONE and TOMBSTONE (search_gc_entries'
// Ok(None): the lookup falls through).
template <class A>
__device__ __forceinline__ bool gc_stands(const A& a, uint64_t off) {
    const uint64_t end = a.log_base + a.log_len;
    if (off >= end) return false;
    if (off < a.log_base || off + kLogHdr > end) return true;
    const uint8_t* e = a.log + (off - a.log_base);
    uint32_t kl, vl;
    __builtin_memcpy(&kl, e, 4);
    __builtin_memcpy(&vl, e + 4, 4);
    if (off + kLogHdr + kl + vl > end) return true;  // at most 2^32 + 2^33: no wrap in 64 bits
    return e[16] != 1;
}

struct Fold {
    uint8_t found;
    bool decided;  // by the gc layer or the active memtable: no later layer is asked
    uint32_t layer, val;
    int64_t time;
};

// Layer L's entry e (a hit) folded into f, by the rules of store.rs:445-472.  The caller asks the
// layers in order and stops asking once f.decided.
template <class A>
__device__ __forceinline__ void fold_hit(const A& a, const MemDesc& d, uint32_t L, uint64_t e, Fold& f) {
    const bool tomb = d.tomb[e] != 0;  // as the encoder writes it
    const uint32_t val = d.val[e];
    const int64_t t = d.created[e];
    if (L == 0) {
        if (tomb || !gc_stands(a, val)) return;
        f = Fold{1, true, 0, val, t};
    } else if (L == 1) {
        f = Fold{(uint8_t)(tomb ? 2 : 1), true, 1, val, t};
    } else if (t > f.time) {
        f = Fold{(uint8_t)(tomb ? 2 : 1), false, L, val, t};
    }
}

// After the last memtable layer: found_in_table, only a time above 0 counts.
__device__ __forceinline__ void fold_close(Fold& f) {
    if (!f.decided && f.time <= 0) f.found = 0;
}

}  // namespace vbf
