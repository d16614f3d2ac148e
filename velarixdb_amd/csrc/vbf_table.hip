// Batched point lookups in SST tables on gfx950: the read path after the
// filters.  velarixdb answers a get per candidate SST with two linear file scans -- index.db for the
// first record whose key is >= the searched key (IndexFileNode::get_from_index, src/fs/mod.rs:
// 667-710), then data.db from that block's offset for an equal key (DataFileNode::find_entry,
// src/fs/mod.rs:334-389) -- and keeps the strictly newest hit over the SSTs
// (DataStore::search_key_in_sstables, src/db/store.rs:579-612).
//
// A table handle holds, next to the borrowed data.db / index.db / block starts, four side tables
// built once at open:
//   counts[nblocks]        entries per block           (k_sst_walk, vbf_sst.hip)
//   ebase[nblocks + 1] u64 entries before block b      (exclusive scan of counts; the range scans'
//                                                       entry ranks, vbf_table_scan.hip)
//   pos[nblocks][256] u16  entry starts in each block  (k_sst_walk; k_table_fill expands the blocks
//                                                       of one key length, which the walk leaves out)
//   kpos[nblocks + 1] u64  start of index record b     (exclusive scan of the blocks' last-key
//                                                       lengths + 8; kpos[nblocks] = index_len)
// and is validated once (k_table_check): keys strictly increasing over the whole file, index record
// b = (last key of block b, start of block b), index.db consumed exactly, no block over 4096 bytes
// or 256 entries.  On such a table both scans are searches over strictly increasing sequences.
//
//   k_table_get : one lane per key.  The lane loops over its candidate tables in order with the
//                 fold in registers (no atomics: ties go to the earlier table by construction); per
//                 table a binary search over the index keys, then one over the chosen block's entry
//                 starts (vbf_table_search.hpp, shared with the range scans).  Keys are compared
//                 as Rust's `Ord for [u8]` in byte-swapped 8-byte words read at their own byte
//                 offsets (never past a key's end), the tail bytewise.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "vbf_kernels.hpp"
#include "vbf_table_search.hpp"

namespace vbf {

namespace {

constexpr uint32_t kTabWaves = 4;      // waves per workgroup of the open passes; one block per wave
constexpr uint32_t kTabMaxBlock = 4096;
constexpr uint32_t kTabFixed = 17;     // key_len + value offset + created_at + tombstone

__device__ __forceinline__ void tab_error(uint32_t* err, uint32_t bits, uint64_t block, uint64_t entry) {
    atomicOr(err, bits);
    atomicMin(err + 1, (uint32_t)std::min<uint64_t>(block, 0xFFFFFFFFu));
    atomicMin(err + 2, (uint32_t)std::min<uint64_t>(entry, 0xFFFFFFFFu));
}

// Open pass 1 (after k_sst_walk): the handle's own entry starts for every block, the size of every
// block's index record, and the two limits the reference's writer guarantees.
__global__ __launch_bounds__(64 * kTabWaves) void k_table_fill(TableOpenArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t b = (uint64_t)blockIdx.x * kTabWaves + (threadIdx.x >> 6);
    if (b >= a.nblocks) return;
    const uint64_t s = a.blocks[b];
    const uint64_t e = b + 1 < a.nblocks ? a.blocks[b + 1] : a.len;
    const uint32_t n = a.counts[b];
    if (lane == 0) a.reclen[b] = 8;  // keeps the scan defined when the block is rejected
    if (e - s > kTabMaxBlock) {
        if (lane == 0) tab_error(a.err, kTabErrBig, b, a.ebase[b]);
        return;
    }
    if (n > kTabMaxEnt || n == 0) {
        if (lane == 0) tab_error(a.err, kTabErrDense, b, a.ebase[b]);
        return;
    }
    const uint32_t L0 = a.lmin[b];
    const bool uni = a.lmax[b] == L0;  // the walk stores no starts for a block of one key length
    const uint16_t* pin = a.pos_walk + b * kTabMaxEnt;
    uint16_t* pout = a.pos + b * kTabMaxEnt;
    for (uint32_t i = lane; i < n; i += 64) pout[i] = uni ? (uint16_t)(i * (L0 + kTabFixed)) : pin[i];
    if (lane == 0) {
        const uint32_t last = uni ? (n - 1) * (L0 + kTabFixed) : (uint32_t)pin[n - 1];
        a.reclen[b] = (uint64_t)ld4(a.data + s + last) + 8;  // u32 key_len | key | u32 block start
    }
}

// Open pass 2: every entry's key against its predecessor's (over block boundaries too), and index
// record b against block b.  Blocks k_table_fill rejected are skipped (the error is recorded).
__global__ __launch_bounds__(64 * kTabWaves) void k_table_check(TableOpenArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t b = (uint64_t)blockIdx.x * kTabWaves + (threadIdx.x >> 6);
    if (b >= a.nblocks) return;
    const uint64_t s = a.blocks[b];
    const uint64_t e = b + 1 < a.nblocks ? a.blocks[b + 1] : a.len;
    const uint32_t n = a.counts[b];
    if (e - s > kTabMaxBlock || n > kTabMaxEnt || n == 0) return;
    const uint16_t* ps = a.pos + b * kTabMaxEnt;
    for (uint32_t i = lane; i < n; i += 64) {
        const uint8_t* cur = a.data + s + ps[i];
        const uint8_t* prev = nullptr;
        if (i > 0) {
            prev = a.data + s + ps[i - 1];
        } else if (b > 0) {
            const uint64_t s0 = a.blocks[b - 1];
            const uint32_t n0 = a.counts[b - 1];
            if (s - s0 <= kTabMaxBlock && n0 > 0 && n0 <= kTabMaxEnt)
                prev = a.data + s0 + a.pos[(b - 1) * kTabMaxEnt + n0 - 1];
        }
        if (prev && cmp_keys(prev + 4, ld4(prev), cur + 4, ld4(cur)) >= 0)
            tab_error(a.err, kTabErrOrder, b, a.ebase[b] + i);
    }
    // index record b: u32 key_len | the block's last key | u32 block start
    const uint64_t r0 = a.kpos[b], r1 = a.kpos[b + 1];
    if (r1 > a.index_len || (b + 1 == a.nblocks && r1 != a.index_len)) {
        if (lane == 0) tab_error(a.err, kTabErrIndexLen, b, a.ebase[b]);
        return;
    }
    const uint8_t* lastk = a.data + s + ps[n - 1];
    const uint32_t L = ld4(lastk);  // r1 - r0 == L + 8 by construction
    bool bad = false;
    if (lane == 0) bad = ld4(a.index + r0) != L || ld4(a.index + r0 + 4 + L) != (uint32_t)s;
    for (uint32_t t = lane; t < L; t += 64) bad |= a.index[r0 + 4 + t] != lastk[4 + t];
    if (__ballot(bad) && lane == 0) tab_error(a.err, kTabErrIndexRec, b, a.ebase[b] + n - 1);
}

// One lane per key; see the file comment.
__global__ __launch_bounds__(256) void k_table_get(TableGetArgs a) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= a.n) return;
    const uint64_t qb = a.offsets ? a.offsets[j] : j * a.stride;
    const uint64_t ql = a.offsets ? a.offsets[j + 1] - qb : a.stride;
    const uint8_t* q = a.keys + qb;
    TabFold f{0, 0, 0xFFFFFFFFu, 0};  // default_datetime(): only a strictly newer entry replaces the winner
    for (uint32_t t = 0; t < a.nsst; ++t) {
        if (a.cand && !a.cand[j * a.nsst + t]) continue;
        const TableDesc& d = a.tab[t];
        // index step: the first record with key >= q; none -> the table is skipped
        const uint64_t lo = index_lower(d, q, ql);
        if (lo == d.nblocks) continue;
        // block step: equality inside that block
        const BlockPos at = block_lower(d, lo, q, ql);
        if (!at.hit) continue;
        fold_table_hit(f, t, at.hit, at.hit_len);
    }
    if (a.found) a.found[j] = (uint8_t)f.found;
    if (a.table_idx) a.table_idx[j] = f.idx;
    if (a.val_off) a.val_off[j] = f.val;
    if (a.created) a.created[j] = f.best;
}

}  // namespace

hipError_t table_fill(const TableOpenArgs& a, hipStream_t s) {
    if (a.nblocks == 0) return hipSuccess;
    const uint64_t grid = (a.nblocks + kTabWaves - 1) / kTabWaves;
    hipLaunchKernelGGL(k_table_fill, dim3((uint32_t)grid), dim3(64 * kTabWaves), 0, s, a);
    return hipGetLastError();
}

hipError_t table_check(const TableOpenArgs& a, hipStream_t s) {
    if (a.nblocks == 0) return hipSuccess;
    const uint64_t grid = (a.nblocks + kTabWaves - 1) / kTabWaves;
    hipLaunchKernelGGL(k_table_check, dim3((uint32_t)grid), dim3(64 * kTabWaves), 0, s, a);
    return hipGetLastError();
}

hipError_t table_get(const TableGetArgs& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_table_get, dim3((uint32_t)((a.n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace vbf
