// The walk of the value log on gfx950: ValueLog::recover (VLogFileNode::recover, fs/mod.rs:520-577)
// and the GC's chunk read (read_chunk_to_garbage_collect, fs/mod.rs:579-651).
//
// The log has no index: entry p's successor is p + 17 + key_len(p) + val_len(p), so one lane that
// follows the chain pays one dependent memory round trip per entry.  Here the window is cut into
// tiles of kWalkTile bytes and every BYTE position is treated as a possible entry start; all
// positions are OUT or relative to the segment's first byte (u32: a segment is far below 4 GiB).
//
//   k_walk_hop   : one workgroup per tile.  The tile (plus the 8 bytes of header lengths that may lie
//                  beyond it) is staged in LDS, nxt(p) computed for each of its positions in 64 bits
//                  and clamped to OUT where the header or the body crosses the end of the window or
//                  the successor lies at or beyond `cap` (the end of the segment, of the window or of
//                  the budget).  Every hop advances by at least 17 bytes, so kWalkRounds rounds of
//                  pointer doubling in LDS resolve exit(p): the first position of p's chain outside
//                  the tile.  The exit table goes to the workspace.
//   k_walk_group : tiles are grouped by kWalkGroup.  For every position of a group's first tile,
//                  follow exit[] until the position leaves the group: at most kWalkGroup dependent
//                  loads, all groups and positions in parallel.
//   k_walk_entry : one workgroup.  Lane 0 follows the group exits from the segment's entry position
//                  (one step per group; a group entered past its first tile -- behind a value that
//                  spans tiles -- is crossed by its tile exits); then one lane per entered group
//                  follows the tile exits and writes each entered tile's entry position.
//   k_walk_mark  : one wave per entered tile.  The tile is staged again and walked from its entry
//                  position, wave-uniform, at most 241 dependent LDS reads: the entry starts, the
//                  key bytes in front of each entry, the tile's count and byte sums, and where and
//                  why the walk left the tile (torn entry, budget or the tile's end).
//   scan_u64     : over the tiles' counts and byte sums.
//   k_walk_emit  : one lane per entry: the per-entry outputs and, for the copies, each key's and
//                  value's place in the output and in the log.  The bytes themselves are moved by
//                  vlog_copy, the balanced slice copy of vbf_vlog.hip, once for keys, once for values.
//
// Every length read from the log is untrusted (positions that are no entry starts hold arbitrary
// bytes): successors are computed in 64 bits and compared with the window's end before any use as an
// index; no byte outside bytes[0..len) is read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vbf_kernels.hpp"
#include "vbf_table_search.hpp"

namespace vbf {

namespace {

constexpr uint32_t kHdr = 17;
constexpr uint32_t kOut = kWalkOut;
constexpr uint32_t kImgDwords = (15 + kWalkTile + 8 + 15) / 16 * 4 + 4;  // 16-byte chunks + one dword of slack

constexpr uint32_t ceil_log2(uint32_t x) { return x <= 1 ? 0 : 1 + ceil_log2((x + 1) / 2); }
// A chain has at most kWalkTile / 17 + 1 positions inside a tile (0, 17, ...), so that many hops
// leave it; round r of the doubling covers 2^r hops.
constexpr uint32_t kWalkRounds = ceil_log2(kWalkTile / kHdr + 1);
static_assert((1u << kWalkRounds) >= kWalkTile / kHdr + 1 && kWalkRounds == 8, "doubling rounds for a 4096-byte tile");
static_assert(kWalkTile % 256 == 0 && kWalkTile <= 4096, "kpre and pos are u16 below kWalkTile; 16 positions per lane");
static_assert(kWalkTile / kHdr + 1 <= kWalkSlots, "entry slots per tile");

// Stage the window's bytes [t0, t0 + kWalkTile + 8) as a 16-byte aligned image: byte t0 + x at image
// byte sh + x.  Chunks inside bytes[0..len) are one aligned 16-byte load; the chunks that straddle
// either end of the window are read bytewise, bytes outside it are zero.  -> sh
__device__ __forceinline__ uint32_t stage_tile(const uint8_t* bytes, uint64_t len, uint64_t t0, uint32_t* img,
                                               uint32_t lane, uint32_t lanes) {
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(bytes + t0) & 15);
    const int64_t a0 = (int64_t)t0 - sh;
    const uint32_t nc = (sh + kWalkTile + 8 + 15) / 16;
    for (uint32_t c = lane; c < nc; c += lanes) {
        const int64_t g = a0 + 16 * (int64_t)c;
        uint4 v;
        if (g >= 0 && (uint64_t)g + 16 <= len) {
            v = *reinterpret_cast<const uint4*>(bytes + g);
        } else {
            uint32_t w[4] = {0, 0, 0, 0};
            for (uint32_t b = 0; b < 16; ++b)
                if (g + b >= 0 && (uint64_t)(g + b) < len) w[b >> 2] |= (uint32_t)bytes[g + b] << (8 * (b & 3));
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4*>(img + 4 * c) = v;
    }
    if (lane == 0) img[4 * nc] = 0;  // img_u32 of the last bytes reads one dword past them
    return sh;
}

__device__ __forceinline__ uint32_t img_u32(const uint32_t* img, uint32_t o) {
    return __builtin_amdgcn_alignbyte(img[(o >> 2) + 1], img[o >> 2], o & 3);
}

// The successor of the entry at window position p, whose two lengths are kl and vl; false when the
// header or the body crosses the end of the window.  At most 2^64 - 1 is far away: p < len.
__device__ __forceinline__ bool successor(uint64_t p, uint64_t len, uint32_t kl, uint32_t vl, uint64_t* nx) {
    if (len - p < kHdr) return false;
    const uint64_t body = (uint64_t)kl + vl;  // < 2^33
    if (len - p - kHdr < body) return false;
    *nx = p + kHdr + body;
    return true;
}

__global__ __launch_bounds__(256) void k_walk_hop(WalkArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t img[kImgDwords];
    __shared__ uint32_t tab[kWalkTile];
    const uint32_t t = blockIdx.x, tid = threadIdx.x;
    const uint64_t t0 = a.seg0 + (uint64_t)t * kWalkTile;
    const uint32_t t0r = t * kWalkTile, t1r = t0r + kWalkTile;
    const uint32_t sh = stage_tile(a.bytes, a.len, t0, img, tid, 256);
    __syncthreads();
    for (uint32_t k = 0; k < kWalkTile / 256; ++k) {
        const uint32_t l = tid + 256 * k;
        const uint64_t p = t0 + l;
        uint32_t e = kOut;
        uint64_t nx;
        if (p < a.len && successor(p, a.len, img_u32(img, sh + l), img_u32(img, sh + l + 4), &nx) && nx < a.cap)
            e = (uint32_t)(nx - a.seg0);  // cap <= seg0 + ntiles * kWalkTile
        tab[l] = e;
    }
    __syncthreads();
    for (uint32_t r = 0; r < kWalkRounds; ++r) {
        uint32_t v[kWalkTile / 256];
#pragma unroll
        for (uint32_t k = 0; k < kWalkTile / 256; ++k) {
            v[k] = tab[tid + 256 * k];
            if (v[k] < t1r) v[k] = tab[v[k] - t0r];  // still inside the tile (kOut is above every t1r)
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < kWalkTile / 256; ++k) tab[tid + 256 * k] = v[k];
        __syncthreads();
    }
    for (uint32_t k = 0; k < kWalkTile / 256; ++k) {
        const uint32_t l = tid + 256 * k;
        a.exit[(uint64_t)t0r + l] = tab[l] < t1r ? kOut : tab[l];  // never: kWalkRounds rounds leave the tile
    }
}

__global__ __launch_bounds__(256) void k_walk_group(WalkArgs a) {
    const uint32_t g = blockIdx.x / (kWalkTile / 256);
    const uint32_t l = (blockIdx.x % (kWalkTile / 256)) * 256 + threadIdx.x;
    const uint32_t g0 = g * kWalkGroup;
    const uint32_t gt = g0 + kWalkGroup < a.ntiles ? g0 + kWalkGroup : a.ntiles;
    const uint32_t gend = gt * kWalkTile;
    uint32_t q = a.exit[(uint64_t)g0 * kWalkTile + l];
    for (uint32_t i = 0; i < kWalkGroup && q < gend; ++i) q = a.exit[q];  // every exit advances by a tile or more
    a.gexit[(uint64_t)g * kWalkTile + l] = q;
}

__global__ __launch_bounds__(256) void k_walk_entry(WalkArgs a) {
    __shared__ uint32_t gentry[kWalkSegment / kWalkTile / kWalkGroup];
    const uint32_t ng = (a.ntiles + kWalkGroup - 1) / kWalkGroup;
    const uint32_t nend = a.ntiles * kWalkTile;
    for (uint32_t g = threadIdx.x; g < ng; g += 256) gentry[g] = kOut;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t q = a.q0;
        while (q < nend) {  // one step per group entered
            const uint32_t g = q / (kWalkGroup * kWalkTile), l = q - g * (kWalkGroup * kWalkTile);
            gentry[g] = q;
            if (l < kWalkTile) {
                q = a.gexit[(uint64_t)g * kWalkTile + l];
            } else {  // entered behind a value that spans tiles: cross the group by its tile exits
                const uint32_t gt = (g + 1) * kWalkGroup < a.ntiles ? (g + 1) * kWalkGroup : a.ntiles;
                for (uint32_t i = 0; i < kWalkGroup && q < gt * kWalkTile; ++i) q = a.exit[q];
            }
            if (q != kOut && q / (kWalkGroup * kWalkTile) <= g) break;  // never: exits only move forward
        }
    }
    __syncthreads();
    for (uint32_t g = threadIdx.x; g < ng; g += 256) {
        uint32_t q = gentry[g];
        const uint32_t gt = (g + 1) * kWalkGroup < a.ntiles ? (g + 1) * kWalkGroup : a.ntiles;
        uint32_t last = kOut;
        for (uint32_t i = 0; i < kWalkGroup && q < gt * kWalkTile; ++i) {
            last = q / kWalkTile;
            a.tentry[last] = q;
            q = a.exit[q];
        }
        if (last != kOut) atomicMax(&a.res->last_tile, last);
    }
}

__global__ __launch_bounds__(256) void k_walk_mark(WalkArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t img[4][kImgDwords];
    __shared__ uint16_t spos[4][kWalkSlots], skpre[4][kWalkSlots];
    const uint32_t wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const uint32_t t = blockIdx.x * 4 + wave;
    if (t >= a.ntiles) return;  // nothing below synchronises across waves
    const uint32_t qe = a.tentry[t];
    if (qe == kOut || qe / kWalkTile != t) {  // the second: never
        if (lane == 0) {
            a.cnt[t] = 0;
            a.ksum[t] = 0;
            a.vsum[t] = 0;
        }
        return;
    }
    const uint64_t t0 = a.seg0 + (uint64_t)t * kWalkTile;
    const uint32_t sh = stage_tile(a.bytes, a.len, t0, img[wave], lane, 64);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // entries start below the tile's end, the window's end and the inclusion limit
    uint64_t stop = t0 + kWalkTile;
    if (a.len < stop) stop = a.len;
    if (a.lim < stop) stop = a.lim;
    uint64_t p = a.seg0 + qe, ks = 0, vs = 0, lastp = 0;
    uint32_t i = 0, torn = 0;
    while (p < stop && i < kWalkSlots) {  // wave-uniform: every lane walks the same chain
        const uint32_t o = sh + (uint32_t)(p - t0);
        const uint32_t kl = img_u32(img[wave], o), vl = img_u32(img[wave], o + 4);
        uint64_t nx;
        if (!successor(p, a.len, kl, vl, &nx)) {
            torn = 1;
            break;
        }
        if (lane == (i & 63)) {
            spos[wave][i] = (uint16_t)(p - t0);
            skpre[wave][i] = (uint16_t)ks;  // the entries before this one lie inside the tile
        }
        ks += kl;
        vs += vl;
        lastp = p;
        p = nx;
        ++i;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (uint32_t k = lane; k < i; k += 64) {
        a.pos[(uint64_t)t * kWalkSlots + k] = spos[wave][k];
        a.kpre[(uint64_t)t * kWalkSlots + k] = skpre[wave][k];
    }
    if (lane == 0) {
        a.cnt[t] = i;
        a.ksum[t] = ks;
        a.vsum[t] = vs;
        a.tend[t] = p;
        a.ttorn[t] = torn;
        if (i) atomicMax(reinterpret_cast<unsigned long long*>(&a.res->last_entry), (unsigned long long)lastp);
    }
}

// The segment's result: the scans' totals and how the walk left the last tile it entered.
__global__ void k_walk_fin(WalkArgs a) {
    const uint32_t lt = a.res->last_tile < a.ntiles ? a.res->last_tile : 0;
    a.res->n = a.cbase[a.ntiles];
    a.res->kbytes = a.kbase[a.ntiles];
    a.res->vbytes = a.vbase[a.ntiles];
    a.res->end = a.tend[lt];
    a.res->torn = a.ttorn[lt];
}

__global__ __launch_bounds__(256) void k_walk_emit(WalkArgs a, WalkOut o) {
    const uint32_t t = blockIdx.x, i = threadIdx.x;
    if (t == 0 && i == 255) {  // the copies' sentinels
        a.ko[o.n_seg] = o.kb_seg;
        a.vo[o.n_seg] = o.vb_seg;
    }
    const uint64_t c = a.cbase[t + 1] - a.cbase[t];
    if (i >= c || i >= kWalkSlots) return;
    const uint64_t js = a.cbase[t] + i;
    if (js >= o.n_seg) return;  // never: n_seg is cbase[ntiles]
    const uint64_t j = o.j0 + js;
    const uint32_t lp = a.pos[(uint64_t)t * kWalkSlots + i], l0 = a.pos[(uint64_t)t * kWalkSlots];
    const uint32_t kp = a.kpre[(uint64_t)t * kWalkSlots + i];
    const uint64_t p = a.seg0 + (uint64_t)t * kWalkTile + lp;
    const uint8_t* e = a.bytes + p;  // a whole entry: the mark pass checked it against the window
    const uint64_t kl = ld4(e);
    const uint64_t kofs = a.kbase[t] + kp, vofs = a.vbase[t] + (lp - l0 - kHdr * i - kp);
    a.ko[js] = kofs;
    a.ks[js] = p + kHdr;
    a.vo[js] = vofs;
    a.vs[js] = p + kHdr + kl;
    if (o.entry_off) o.entry_off[j] = a.base + p;
    if (o.val_offsets) o.val_offsets[j] = (uint32_t)(a.base + p);
    if (o.key_off) o.key_off[j] = o.k0 + kofs;
    if (o.value_off) o.value_off[j] = o.v0 + vofs;
    if (o.created) o.created[j] = (int64_t)ld8(e + 8);
    if (o.tomb) o.tomb[j] = e[16] == 1;
}

// Element n of the three n + 1 arrays.
__global__ void k_walk_tail(WalkOut o, uint64_t n, uint64_t end_off, uint64_t kb, uint64_t vb) {
    if (o.entry_off) o.entry_off[n] = end_off;
    if (o.key_off) o.key_off[n] = kb;
    if (o.value_off) o.value_off[n] = vb;
}

}  // namespace

hipError_t walk_passes(const WalkArgs& a, void* scan_tmp, size_t scan_bytes, hipStream_t s) {
    const uint32_t nt = a.ntiles, ng = (nt + kWalkGroup - 1) / kWalkGroup;
    if (nt == 0 || nt > kWalkSegment / kWalkTile) return hipErrorInvalidValue;
    hipError_t e;
    if ((e = hipMemsetAsync(a.tentry, 0xFF, (size_t)nt * 4, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(a.res, 0, sizeof(WalkRes), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(a.cnt + nt, 0, 8, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(a.ksum + nt, 0, 8, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(a.vsum + nt, 0, 8, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_walk_hop, dim3(nt), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_walk_group, dim3(ng * (kWalkTile / 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_walk_entry, dim3(1), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_walk_mark, dim3((nt + 3) / 4), dim3(256), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t b = scan_bytes;
    if ((e = scan_u64(scan_tmp, &b, a.cnt, a.cbase, (uint64_t)nt + 1, s)) != hipSuccess) return e;
    b = scan_bytes;
    if ((e = scan_u64(scan_tmp, &b, a.ksum, a.kbase, (uint64_t)nt + 1, s)) != hipSuccess) return e;
    b = scan_bytes;
    if ((e = scan_u64(scan_tmp, &b, a.vsum, a.vbase, (uint64_t)nt + 1, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_walk_fin, dim3(1), dim3(1), 0, s, a);
    return hipGetLastError();
}

hipError_t walk_emit(const WalkArgs& a, const WalkOut& o, hipStream_t s) {
    if (o.n_seg == 0) return hipSuccess;
    hipLaunchKernelGGL(k_walk_emit, dim3(a.ntiles), dim3(256), 0, s, a, o);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    VlogGetArgs c{};
    c.bytes = a.bytes;
    c.len = a.len;
    c.n = o.n_seg;
    if (o.keys) {
        c.voff = a.ko;
        c.src = a.ks;
        c.total = o.kb_seg;
        c.values = o.keys + o.k0;
        if ((e = vlog_copy(c, s)) != hipSuccess) return e;
    }
    if (o.values) {
        c.voff = a.vo;
        c.src = a.vs;
        c.total = o.vb_seg;
        c.values = o.values + o.v0;
        if ((e = vlog_copy(c, s)) != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t walk_tail(const WalkOut& o, uint64_t n, uint64_t end_off, uint64_t kb, uint64_t vb, hipStream_t s) {
    if (!o.entry_off && !o.key_off && !o.value_off) return hipSuccess;
    hipLaunchKernelGGL(k_walk_tail, dim3(1), dim3(1), 0, s, o, n, end_off, kb, vb);
    return hipGetLastError();
}

}  // namespace vbf
