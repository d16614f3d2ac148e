// Batched range scans over open SST tables on gfx950: the key side of DataStore::seek
// (src/range/range_iterator.rs:47-60, a stub in the reference).  For a range [lo, hi] and the tables
// in the caller's order the scan lists, in ascending key order, every key inside the bounds for
// which the point lookup (k_table_get, vbf_table.hip) finds a winner, with that winner's fields: the
// fold of DataStore::search_key_in_sstables (src/db/store.rs:579-612) decides, nothing else.
//
// Every table is strictly increasing (checked at open), so an entry's place in the merged order of a
// range follows from searches alone -- no merge pass:
//
//   k_scan_bounds : one lane per (range, table).  Rank (entry index in the table: ebase[block] +
//                   index in the block) of the first entry >= lo and of the first entry > hi (>= hi
//                   when the end is exclusive): first[r][t], cnt[r][t].  An exclusive scan of cnt in
//                   range-major order numbers the candidates; the total is read back.
//   k_scan_rank   : one lane per candidate (r, t, i).  The lane searches its own key in every other
//                   table t': the lower-bound rank lb_t' and, where t' holds the key, that copy's
//                   created_at.  The candidate is listed iff it is the fold's winner (created != 0,
//                   no greater created_at anywhere, no equal one in an earlier table) and, without
//                   KEEP_TOMBSTONES, no tombstone.  Its merged slot in range r is
//                       sum over t' of (lb_t' - first[r][t'])  +  #{t' < t holding the key},
//                   the number of the range's candidates before it in (key, table) order: unique.
//                   The lane writes (table, entry start, listed, key length) to that slot.
//                   Consecutive lanes hold consecutive keys of one table, so their searches in t'
//                   walk the same index records and blocks.
//   (scans)       : exclusive scans of the listed flags and of the listed key lengths over the
//                   slots give every output's position and key offset; n_out and key_bytes are read
//                   back together.
//   k_scan_emit   : one lane per slot: the listed entry's fields and key offset; range_off.
//   k_scan_keys   : eight lanes per slot copy the key in 8-byte words read and written at the key's
//                   own byte offsets, the last 0..7 bytes bytewise.  No byte outside a key is read.
//
// Work: O(candidates x nsst x (log nblocks + log 256)) key comparisons -- a choice for short and
// medium ranges over a handful of tables; it is not a merge-path scan.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vbf_kernels.hpp"
#include "vbf_table_search.hpp"

namespace vbf {

namespace {

constexpr uint32_t kScanKeyLanes = 8;  // lanes per key in k_scan_keys

// rank_lower and last_le: vbf_table_search.hpp (shared with the whole-store scan).

__global__ __launch_bounds__(256) void k_scan_bounds(TableScanArgs a) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.nranges * a.nsst) return;
    const uint64_t r = p / a.nsst;
    const TableDesc& d = a.tab[p % a.nsst];
    const uint64_t o0 = a.bounds_off[2 * r], o1 = a.bounds_off[2 * r + 1], o2 = a.bounds_off[2 * r + 2];
    a.first[p] = 0;
    a.cnt[p] = 0;
    if (o0 > o1 || o1 > o2) {  // lengths would wrap: nothing is read
        atomicOr(a.err, kScanErrBounds);
        return;
    }
    // one search body for both ends (w = 0: lo_r, w = 1: hi_r), kept a loop
    uint64_t rk[2];
#pragma clang loop unroll(disable)
    for (uint32_t w = 0; w < 2; ++w) {
        const uint64_t qb = w ? o1 : o0, qe = w ? o2 : o1;
        const RankPos at = rank_lower(d, a.bounds + qb, qe - qb);
        // hi_r itself is inside an inclusive range: the end is the first entry > hi_r
        rk[w] = at.rank + (w && at.eq && !(a.flags & kScanEndExclusive) ? 1 : 0);
    }
    a.first[p] = rk[0];
    a.cnt[p] = rk[1] > rk[0] ? rk[1] - rk[0] : 0;  // lo_r > hi_r: an empty range
}

__global__ __launch_bounds__(256) void k_scan_rank(TableScanArgs a) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.total) return;
    const uint64_t P = a.nranges * a.nsst;
    const uint64_t p = last_le(a.cbase, P, c);  // cbase[p] <= c < cbase[p + 1]
    const uint64_t r = p / a.nsst;
    const uint32_t t = (uint32_t)(p % a.nsst);
    const TableDesc& d = a.tab[t];
    const uint64_t i = a.first[p] + (c - a.cbase[p]);
    const uint64_t b = last_le(d.ebase, d.nblocks, i);
    const uint32_t start = d.blocks[b] + d.pos[b * kTabMaxEnt + (i - d.ebase[b])];
    const uint8_t* ent = d.data + start;
    const uint32_t L = ld4(ent);
    const uint8_t* key = ent + 4;
    const uint64_t created = ld8(ent + 8 + L);
    bool win = created != 0;
    uint64_t rank = i - a.first[p];
    const uint64_t* first_r = a.first + r * a.nsst;
    for (uint32_t u = 0; u < a.nsst; ++u) {
        if (u == t) continue;
        const RankPos at = rank_lower(a.tab[u], key, L);
        rank += at.rank - first_r[u];
        if (!at.eq) continue;
        const uint64_t other = ld8(at.hit + 8 + at.hit_len);
        if (u < t) {
            ++rank;
            win &= other < created;  // a tie goes to the earlier table
        } else {
            win &= other <= created;
        }
    }
    if (!(a.flags & kScanKeepTombstones) && ent[16 + L] == 1) win = false;
    const uint64_t slot = a.cbase[r * a.nsst] + rank;
    if (slot >= a.cbase[(r + 1) * a.nsst]) {  // cannot happen on tables that passed the open check
        atomicOr(a.err, kScanErrRank);
        return;
    }
    a.m_table[slot] = t;
    a.m_pos[slot] = start;
    a.m_keep[slot] = win ? 1 : 0;
    a.m_len[slot] = win ? L : 0;
}

// Slots 0 .. total - 1 write their entry (when listed); slot `total` closes key_off; the first
// nranges + 1 lanes write range_off.
__global__ __launch_bounds__(256) void k_scan_emit(TableScanArgs a) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (a.range_off && s <= a.nranges) a.range_off[s] = a.opos[a.cbase[s * a.nsst]];
    if (s > a.total) return;
    const uint64_t o = a.opos[s];
    if (s == a.total) {
        if (a.key_off) a.key_off[o] = a.kofs[s];
        return;
    }
    if (!a.m_keep[s]) return;
    const uint32_t t = a.m_table[s];
    const uint8_t* ent = a.tab[t].data + a.m_pos[s];
    const uint32_t L = ld4(ent);
    if (a.key_off) a.key_off[o] = a.kofs[s];
    if (a.table_idx) a.table_idx[o] = t;
    if (a.val_off) a.val_off[o] = ld4(ent + 4 + L);
    if (a.created) a.created[o] = ld8(ent + 8 + L);
    if (a.tomb) a.tomb[o] = ent[16 + L] == 1;
}

__global__ __launch_bounds__(256) void k_scan_keys(TableScanArgs a) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t s = g / kScanKeyLanes;
    const uint32_t lane = (uint32_t)(g % kScanKeyLanes);
    if (s >= a.total || !a.m_keep[s]) return;
    const uint8_t* ent = a.tab[a.m_table[s]].data + a.m_pos[s];
    const uint32_t L = ld4(ent);
    const uint8_t* src = ent + 4;
    uint8_t* dst = a.keys + a.kofs[s];
    const uint32_t words = L / 8;
    for (uint32_t w = lane; w < words; w += kScanKeyLanes) {
        const uint64_t v = ld8(src + 8 * w);
        __builtin_memcpy(dst + 8 * w, &v, 8);
    }
    for (uint32_t j = words * 8 + lane; j < L; j += kScanKeyLanes) dst[j] = src[j];
}

inline dim3 grid256(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

}  // namespace

hipError_t table_scan_bounds(const TableScanArgs& a, hipStream_t s) {
    const uint64_t P = a.nranges * a.nsst;
    if (P == 0) return hipSuccess;
    hipLaunchKernelGGL(k_scan_bounds, grid256(P), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t table_scan_rank(const TableScanArgs& a, hipStream_t s) {
    if (a.total == 0) return hipSuccess;
    hipLaunchKernelGGL(k_scan_rank, grid256(a.total), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t table_scan_emit(const TableScanArgs& a, hipStream_t s) {
    const uint64_t n = (a.total > a.nranges ? a.total : a.nranges) + 1;
    hipLaunchKernelGGL(k_scan_emit, grid256(n), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t table_scan_keys(const TableScanArgs& a, hipStream_t s) {
    if (a.total == 0 || !a.keys) return hipSuccess;
    hipLaunchKernelGGL(k_scan_keys, grid256(a.total * kScanKeyLanes), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace vbf
