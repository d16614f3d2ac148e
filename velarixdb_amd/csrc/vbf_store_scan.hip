// Batched range scans over the whole store on gfx950: DataStore::seek (src/range/range_iterator.rs:
// 47-60, a stub in the reference) over the gc table, the active memtable, the read-only memtables
// and the SSTs.  The scan has no semantics of its own: for a range [lo, hi] it lists, in ascending key
// order, every key inside the bounds that any layer holds and for which the whole get
// (vbf_store_get_host: k_mem_get, k_table_get, k_store_merge) finds a winner, with that winner's
// fields.  The precedence is not restated here: the memtable layers fold through vbf_store_fold.hpp
// (k_mem_get's own code), the tables through fold_table_hit (k_table_get's), and a memtable's answer
// stands before the tables' as in k_store_merge.
//
// The pipeline is vbf_table_scan.hip's, which needs only that every layer is strictly increasing: a
// memtable handle holds distinct ascending keys, a table passed its open check.  A layer is searched
// by kind -- a memtable by the (pfx, key) comparator of k_mem_get (pfx[mid] first, the key bytes only
// on a prefix tie), a table by the index and block searches of vbf_table_search.hpp.
//
//   k_sscan_bounds : one lane per (range, layer).  Rank of the first entry >= lo and of the first
//                    entry > hi (>= hi when the end is exclusive): first[r][L], cnt[r][L].  An
//                    exclusive scan of cnt in range-major order numbers the candidates.
//   k_sscan_rank   : one lane per candidate (r, L, i).  The lane searches its own key in every other
//                    layer L': the lower-bound rank lb_L' and, where L' holds the key, the entry.
//                    Its merged slot in range r is
//                        sum over L' of (lb_L' - first[r][L'])  +  #{L' < L holding the key}.
//                    The candidate of the first layer that holds the key is the key's
//                    representative; a lane that finds its key in an earlier layer stops there.  The
//                    representative folds the copies it has just located (its own, then the later
//                    layers' in order) and writes listed / key length / key bytes / layer / table /
//                    offset / time to its slot.
//                    A lane's search is a chain of dependent loads; a step in a memtable reads
//                    pfx[mid], one 8-byte load from a dense array, and off / key bytes only on a
//                    prefix tie.  Consecutive lanes hold consecutive keys of one layer, so their
//                    searches walk the same top of every other layer and end next to each other.
//                    Every search starts from the whole layer: starting a memtable search from the
//                    range's own ranks (first[r][L'], + cnt[r][L']) was measured and changed nothing
//                    (whole-store range scan), so it is not here.
//   (scans)        : exclusive scans of the listed flags and of the listed key lengths over the
//                    slots give every output's position and key offset.
//   k_sscan_emit   : one lane per slot: the listed entry's fields and key offset; range_off.
//   k_sscan_keys   : eight lanes per slot copy the key as k_scan_keys does.
//
// Work: O(candidates x layers x log) key comparisons -- a choice for short and medium ranges; it is
// not a merge-path scan.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vbf_kernels.hpp"
#include "vbf_keyprefix.hpp"
#include "vbf_store_fold.hpp"
#include "vbf_table_search.hpp"

namespace vbf {

namespace {

constexpr uint32_t kSscanKeyLanes = 8;  // lanes per key in k_sscan_keys

// The rank of the first entry of memtable `d` with key >= q, by (pfx, key), inside [lo, hi]: every
// entry before lo is smaller than q, every one from hi on greater.  eq: entry `rank` holds q.
struct MemPos {
    uint64_t rank;
    bool eq;
};
__device__ __forceinline__ MemPos mem_lower(const MemDesc& d, const uint8_t* q, uint64_t ql, uint64_t qp,
                                            uint64_t lo, uint64_t hi) {
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        const uint64_t p = d.pfx[mid];
        int c;
        if (p != qp) {
            c = p < qp ? -1 : 1;
        } else {
            const uint64_t k0 = d.off[mid], k1 = d.off[mid + 1];
            c = cmp_keys(d.keys + k0, k1 - k0, q, ql);
            if (c == 0) return MemPos{mid, true};  // distinct keys: the lower bound itself
        }
        if (c < 0) lo = mid + 1;
        else hi = mid;
    }
    return MemPos{lo, false};
}

__global__ __launch_bounds__(256) void k_sscan_bounds(StoreScanArgs a) {
    const uint32_t nl = a.nmem + a.nsst;
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.nranges * nl) return;
    const uint64_t r = p / nl;
    const uint32_t L = (uint32_t)(p % nl);
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
        const uint64_t qb = w ? o1 : o0, ql = (w ? o2 : o1) - qb;
        const uint8_t* q = a.bounds + qb;
        uint64_t rank;
        bool eq;
        if (L < a.nmem) {
            const MemDesc& d = a.mem[L];
            const MemPos at = mem_lower(d, q, ql, key_prefix8(q, ql), 0, d.n);
            rank = at.rank;
            eq = at.eq;
        } else {
            const RankPos at = rank_lower(a.tab[L - a.nmem], q, ql);
            rank = at.rank;
            eq = at.eq;
        }
        // hi_r itself is inside an inclusive range: the end is the first entry > hi_r
        rk[w] = rank + (w && eq && !(a.flags & kScanEndExclusive) ? 1 : 0);
    }
    a.first[p] = rk[0];
    a.cnt[p] = rk[1] > rk[0] ? rk[1] - rk[0] : 0;  // lo_r > hi_r: an empty range
}

__global__ __launch_bounds__(256) void k_sscan_rank(StoreScanArgs a) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.total) return;
    const uint32_t nl = a.nmem + a.nsst;
    const uint64_t p = last_le(a.cbase, a.nranges * nl, c);  // cbase[p] <= c < cbase[p + 1]
    const uint64_t r = p / nl;
    const uint32_t L = (uint32_t)(p % nl);
    const uint64_t* first_r = a.first + r * nl;
    const uint64_t i = first_r[L] + (c - a.cbase[p]);
    // the candidate's key, and its entry when a table holds it
    const uint8_t* key;
    const uint8_t* ent = nullptr;
    uint64_t kl, kp;
    if (L < a.nmem) {
        const MemDesc& d = a.mem[L];
        const uint64_t b = d.off[i];
        key = d.keys + b;
        kl = d.off[i + 1] - b;
        kp = d.pfx[i];
    } else {
        const TableDesc& d = a.tab[L - a.nmem];
        const uint64_t b = last_le(d.ebase, d.nblocks, i);
        ent = d.data + d.blocks[b] + d.pos[b * kTabMaxEnt + (i - d.ebase[b])];
        kl = ld4(ent);
        key = ent + 4;
        kp = key_prefix8(key, kl);
    }
    uint64_t rank = i - first_r[L];
    Fold f{0, false, 0, 0, 0};
    TabFold tf{0, 0, 0xFFFFFFFFu, 0};
    if (L < a.nmem) fold_hit(a, a.mem[L], L, i, f);
    else fold_table_hit(tf, L - a.nmem, ent, (uint32_t)kl);
    for (uint32_t u = 0; u < nl; ++u) {
        if (u == L) continue;
        uint64_t lb;
        bool eq;
        const uint8_t* hit = nullptr;
        uint32_t hl = 0;
        if (u < a.nmem) {
            const MemDesc& d = a.mem[u];
            const MemPos at = mem_lower(d, key, kl, kp, 0, d.n);
            lb = at.rank;
            eq = at.eq;
        } else {
            const RankPos at = rank_lower(a.tab[u - a.nmem], key, kl);
            lb = at.rank;
            eq = at.eq;
            hit = at.hit;
            hl = at.hit_len;
        }
        if (eq && u < L) return;  // an earlier layer holds the key: its candidate is the representative
        rank += lb - first_r[u];
        if (!eq) continue;
        if (u < a.nmem) {
            if (!f.decided) fold_hit(a, a.mem[u], u, lb, f);
        } else {
            fold_table_hit(tf, u - a.nmem, hit, hl);
        }
    }
    fold_close(f);
    // a memtable's answer stands, otherwise the tables' (k_store_merge)
    uint32_t found = f.found, layer = f.layer, tidx = 0xFFFFFFFFu, val = f.val;
    uint64_t created = (uint64_t)f.time;
    if (found == 0 && tf.found != 0) {
        found = tf.found;
        layer = 0x80000000u | tf.idx;
        tidx = tf.idx;
        val = tf.val;
        created = tf.best;
    }
    const bool listed = found == 1 || (found == 2 && (a.flags & kScanKeepTombstones));
    const uint64_t slot = a.cbase[r * nl] + rank;
    if (slot >= a.cbase[(r + 1) * nl]) {  // cannot happen on layers that are strictly increasing
        atomicOr(a.err, kScanErrRank);
        return;
    }
    if (!listed) return;  // the slots were zeroed
    a.m_keep[slot] = 1;
    a.m_len[slot] = kl;
    a.m_src[slot] = key;
    a.m_created[slot] = created;
    a.m_layer[slot] = layer;
    a.m_tidx[slot] = tidx;
    a.m_val[slot] = val;
    a.m_found[slot] = (uint8_t)found;
}

// Slots 0 .. total - 1 write their entry (when listed); slot `total` closes key_off; the first
// nranges + 1 lanes write range_off.
__global__ __launch_bounds__(256) void k_sscan_emit(StoreScanArgs a) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t nl = a.nmem + a.nsst;
    if (a.range_off && s <= a.nranges) a.range_off[s] = a.opos[a.cbase[s * nl]];
    if (s > a.total) return;
    const uint64_t o = a.opos[s];
    if (s == a.total) {
        if (a.key_off) a.key_off[o] = a.kofs[s];
        return;
    }
    if (!a.m_keep[s]) return;
    const uint8_t found = a.m_found[s];
    if (a.key_off) a.key_off[o] = a.kofs[s];
    if (a.tomb) a.tomb[o] = found == 2;
    if (a.layer) a.layer[o] = a.m_layer[s];
    if (a.table_idx) a.table_idx[o] = a.m_tidx[s];
    if (a.val_off) a.val_off[o] = a.m_val[s];
    if (a.created) a.created[o] = a.m_created[s];
    if (a.found) a.found[o] = found;
}

__global__ __launch_bounds__(256) void k_sscan_keys(StoreScanArgs a) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t s = g / kSscanKeyLanes;
    const uint32_t lane = (uint32_t)(g % kSscanKeyLanes);
    if (s >= a.total || !a.m_keep[s]) return;
    const uint8_t* src = a.m_src[s];
    const uint64_t L = a.m_len[s];
    uint8_t* dst = a.keys + a.kofs[s];
    const uint64_t words = L / 8;
    for (uint64_t w = lane; w < words; w += kSscanKeyLanes) {
        const uint64_t v = ld8(src + 8 * w);
        __builtin_memcpy(dst + 8 * w, &v, 8);
    }
    for (uint64_t j = words * 8 + lane; j < L; j += kSscanKeyLanes) dst[j] = src[j];
}

inline dim3 grid256(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

}  // namespace

hipError_t store_scan_bounds(const StoreScanArgs& a, hipStream_t s) {
    const uint64_t P = a.nranges * (a.nmem + a.nsst);
    if (P == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sscan_bounds, grid256(P), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t store_scan_rank(const StoreScanArgs& a, hipStream_t s) {
    if (a.total == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sscan_rank, grid256(a.total), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t store_scan_emit(const StoreScanArgs& a, hipStream_t s) {
    const uint64_t n = (a.total > a.nranges ? a.total : a.nranges) + 1;
    hipLaunchKernelGGL(k_sscan_emit, grid256(n), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t store_scan_keys(const StoreScanArgs& a, hipStream_t s) {
    if (a.total == 0 || !a.keys) return hipSuccess;
    hipLaunchKernelGGL(k_sscan_keys, grid256(a.total * kSscanKeyLanes), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace vbf
