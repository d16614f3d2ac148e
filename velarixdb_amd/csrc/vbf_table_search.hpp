// vbf_table_search.hpp -- the key comparison and the two searches over an open table (TableDesc),
// shared by the point lookups (vbf_table.hip) and the range scans (vbf_table_scan.hip).  On a table
// that passed k_table_check the index keys and every block's keys are strictly increasing, so both
// of the reference's file scans are binary searches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vbf_kernels.hpp"

namespace vbf {

constexpr uint32_t kTabMaxEnt = 256;   // pos slots per block (vbf_sst.hip's kMaxEnt)

__device__ __forceinline__ uint64_t ld8(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
__device__ __forceinline__ uint32_t ld4(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// Rust `Ord for [u8]` (cmp_bytes of keyhash.hpp is the bytewise statement): -1 / 0 / 1.  Whole
// 8-byte words are read at the keys' own byte offsets, only while both keys have 8 bytes left; the
// last 0..7 bytes go bytewise.  No byte outside [a, a + la) or [b, b + lb) is read.
__device__ __forceinline__ int cmp_keys(const uint8_t* a, uint64_t la, const uint8_t* b, uint64_t lb) {
    const uint64_t n = la < lb ? la : lb;
    uint64_t i = 0;
    for (; i + 8 <= n; i += 8) {
        const uint64_t x = ld8(a + i), y = ld8(b + i);
        if (x != y) return __builtin_bswap64(x) < __builtin_bswap64(y) ? -1 : 1;
    }
    uint64_t x = 0, y = 0;
    for (; i < n; ++i) {
        x = (x << 8) | a[i];
        y = (y << 8) | b[i];
    }
    if (x != y) return x < y ? -1 : 1;
    return la < lb ? -1 : (la > lb ? 1 : 0);
}

// Index step (IndexFileNode::get_from_index): the first block whose index record's key (the block's
// last key) is >= q; d.nblocks when every index key is smaller.
__device__ __forceinline__ uint64_t index_lower(const TableDesc& d, const uint8_t* q, uint64_t ql) {
    uint64_t lo = 0, hi = d.nblocks;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        const uint64_t r0 = d.kpos[mid], r1 = d.kpos[mid + 1];
        if (cmp_keys(d.index + r0 + 4, r1 - r0 - 8, q, ql) < 0) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Block step: at = the first entry of block b whose key is >= q (counts[b] when none is); hit = that
// entry when its key equals q (DataFileNode::find_entry's answer), else nullptr; hit_len its key
// length; eq = (hit != nullptr), carried apart for callers that want only the yes/no (ROCm 7.2's
// clang crashes in simplifycfg on a kernel that only null-tests `hit`).
struct BlockPos {
    uint32_t at;
    uint32_t hit_len;
    const uint8_t* hit;
    bool eq;
};
__device__ __forceinline__ BlockPos block_lower(const TableDesc& d, uint64_t b, const uint8_t* q, uint64_t ql) {
    const uint8_t* blk = d.data + d.blocks[b];
    const uint16_t* ps = d.pos + b * kTabMaxEnt;
    uint32_t el = 0, eh = d.counts[b];
    const uint8_t* found = nullptr;
    uint32_t fl = 0;
    bool eq = false;
    while (el < eh) {
        const uint32_t mid = (el + eh) >> 1;
        const uint8_t* ent = blk + ps[mid];
        const uint32_t L = ld4(ent);
        const int c = cmp_keys(ent + 4, L, q, ql);
        if (c == 0) {
            found = ent;
            fl = L;
            el = mid;
            eq = true;
            break;
        }
        if (c < 0) el = mid + 1;
        else eh = mid;
    }
    return BlockPos{el, fl, found, eq};
}

// The fold of DataStore::search_key_in_sstables (src/db/store.rs:579-612) over the tables in the
// caller's order: the winner starts at default_datetime() (0) and only a strictly newer entry
// replaces it, so a tie goes to the earlier table and created_at == 0 never wins.  found: 0 no
// winner, 1 live, 2 tombstone.  Starts as TabFold{0, 0, 0xFFFFFFFFu, 0}.
struct TabFold {
    uint64_t best;
    uint32_t val, idx, found;
};
__device__ __forceinline__ void fold_table_hit(TabFold& f, uint32_t t, const uint8_t* hit, uint32_t hl) {
    const uint64_t created = ld8(hit + 8 + hl);
    if (created > f.best) {
        f.best = created;
        f.val = ld4(hit + 4 + hl);
        f.idx = t;
        f.found = hit[16 + hl] == 1 ? 2u : 1u;
    }
}

// The rank of the first entry of `d` with key >= q: the index step, the block step, then ebase.
// No index record >= q (or an empty table): every entry is smaller, the rank is the entry count.
// eq: the table holds q, at `hit` (the first entry > q then has rank + 1); else hit = nullptr.
struct RankPos {
    uint64_t rank;
    const uint8_t* hit;
    uint32_t hit_len;
    bool eq;
};
__device__ __forceinline__ RankPos rank_lower(const TableDesc& d, const uint8_t* q, uint64_t ql) {
    RankPos r{0, nullptr, 0, false};
    if (d.nblocks != 0) {
        const uint64_t b = index_lower(d, q, ql);
        r.rank = d.ebase[b];
        if (b != d.nblocks) {
            const BlockPos at = block_lower(d, b, q, ql);
            r.rank += at.at;
            r.hit = at.hit;
            r.hit_len = at.hit_len;
            r.eq = at.eq;
        }
    }
    return r;
}

// The largest i in [0, n) with a[i] <= v, for nondecreasing a with a[0] <= v < a[n].
__device__ __forceinline__ uint64_t last_le(const uint64_t* a, uint64_t n, uint64_t v) {
    uint64_t lo = 0, hi = n;  // a[lo] <= v < a[hi]
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace vbf
