// SST data.db / index.db encoder on gfx950: the step after the merge on the
// compaction path, the inverse of vbf_sst.hip.  Table::write_to_file (src/sst/table.rs:287-324)
// lays the entries back to back in data.db, entry = u32 key_len | key | u32 value offset | i64
// created_at ms | u8 tombstone (Block::serialize, block/block_manager.rs:176-193), cuts them into
// blocks greedily -- a block takes the next entry unless size + (L + 17) > 4096 (is_full, :159-161)
// -- and writes one index.db record per block, u32 key_len | key | u32 block_start with the block's
// LAST key (write_block, table.rs:333-340; Index::serialize_entry, index/indexer.rs:151-170).
//
// data.db needs no scan: entry j starts at (offsets[j] - offsets[0]) + 17 j.  The blocks do: where
// block b + 1 starts depends on where block b started, and walks from different entries need never
// meet (equal entry sizes), so the cut has to be carried exactly.  A block holds at most 240
// entries (4096 / 17), hence a block sequence enters a tile of 1024 entries at one of its first 240
// and the tile is a function {0..239} -> {0..239}: entry point in, entry point into the next tile
// out.  Those tables compose associatively.
//
//   k_enc_tile  : tile positions in LDS; next(e) = first entry of the block after the one starting
//                 at e (binary search, one lane per entry), kept as the u8 delta next(e) - e; the
//                 tile's table by pointer doubling over next (10 rounds in LDS); lengths checked.
//   k_enc_group : 128 tile tables staged in LDS, composed by 240 lanes -> one table per group.
//   k_enc_top   : one workgroup walks the group tables (at most 1928: data.db stays below 2^32
//                 bytes) -> every group's entry point.
//   k_enc_apply : one workgroup per group walks its 128 tables from that point -> every tile's.
//   k_enc_walk<false> : each tile follows its deltas from its entry point and counts its blocks and
//                 their index.db bytes; an exclusive scan of the pairs places the records.
//   k_enc_walk<true>  : the same walk, recorded in LDS; lanes write the block offsets and, one lane
//                 per index.db byte, the records.
//   k_enc_data  : one lane per aligned dword of data.db, the entry found by a binary search over
//                 the tile's positions in LDS; bytes composed from the four input arrays.
// Separate launches throughout: no workgroup waits on another.  A fixed stride needs none of the
// segmentation (4096 / (stride + 17) entries per block): k_enc_index_fixed and k_enc_data<true>.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>

#include "vbf_kernels.hpp"

namespace vbf {

constexpr uint32_t kEncThreads = 256;
constexpr uint32_t kEncBlock = 4096;                    // consts/mod.rs:107
constexpr uint32_t kEncFixed = 17;                      // key_len + value offset + created_at + tombstone
constexpr uint32_t kEncMaxKey = kEncBlock - kEncFixed;  // a longer key fails the flush (BlockIsFull)
constexpr uint32_t kEncPos = kEncTile + kEncReach + 1;  // positions a tile needs: its own and its reach
static_assert(kEncTile % kEncThreads == 0 && kEncTile >= kEncReach && (1u << 10) >= kEncTile, "tile shape");
static_assert((kEncGroup * kEncReach) % 16 == 0, "group tables are staged with 16-byte loads");

// pos[i] = data.db bytes between entry t0 and entry t0 + i, i <= avail.
__device__ __forceinline__ void enc_load_pos(const SstEncArgs& a, uint64_t t0, uint32_t avail, uint64_t off0,
                                             uint32_t* pos) {
    for (uint32_t i = threadIdx.x; i <= avail; i += kEncThreads)
        pos[i] = (uint32_t)(a.offsets[t0 + i] - off0) + kEncFixed * i;
}

__global__ __launch_bounds__(kEncThreads) void k_enc_tile(SstEncArgs a) {
    __shared__ uint32_t pos[kEncPos];
    __shared__ uint16_t nxt[kEncTile];
    const uint32_t tid = threadIdx.x;
    const uint64_t t = blockIdx.x, t0 = t * kEncTile;
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(kEncTile, a.n - t0);
    const uint32_t avail = (uint32_t)std::min<uint64_t>(kEncTile + kEncReach, a.n - t0);
    const uint64_t off0 = a.offsets[t0];
    uint32_t bits = 0, bad = 0xFFFFFFFFu;
    for (uint32_t i = tid; i <= avail; i += kEncThreads) {
        const uint64_t o = a.offsets[t0 + i];
        pos[i] = (uint32_t)(o - off0) + kEncFixed * i;
        if (i < cnt) {  // this tile's entry: its length, in full width
            const uint64_t o1 = a.offsets[t0 + i + 1];
            const uint32_t b = o1 < o ? kEncErrOrder : o1 - o > kEncMaxKey ? kEncErrBig : 0;
            if (b && bad == 0xFFFFFFFFu) bad = i;
            bits |= b;
        }
    }
    if (bits) {
        atomicOr(a.err, bits);
        atomicMin(a.err + 1, (uint32_t)std::min<uint64_t>(t0 + bad, 0xFFFFFFFEu));
    }
    __syncthreads();
    // every index below stays inside the tile's arrays whatever the offsets hold: a malformed
    // input is reported by the host after this pass, not trusted by it
    for (uint32_t e = tid; e < kEncTile; e += kEncThreads) {
        uint32_t f = kEncTile;  // past the last entry: the walk is over
        if (e < cnt) {
            uint32_t lo = e + 1, hi = std::min(e + kEncReach, avail);
            const uint32_t base = pos[e];
            while (lo < hi) {  // the last f with entries e .. f-1 within one block
                const uint32_t mid = (lo + hi + 1) >> 1;
                if (pos[mid] - base <= kEncBlock) lo = mid;
                else hi = mid - 1;
            }
            f = lo;
            a.delta[t0 + e] = (uint8_t)(f - e);
        }
        nxt[e] = (uint16_t)f;
    }
    __syncthreads();
    // nxt[e] -> where the walk from e leaves the tile: 2^10 >= kEncTile steps by doubling
    for (uint32_t r = 0; r < 10; ++r) {
        uint32_t v[kEncTile / kEncThreads];
#pragma unroll
        for (uint32_t q = 0; q < kEncTile / kEncThreads; ++q) {
            v[q] = nxt[tid + kEncThreads * q];
            if (v[q] < kEncTile) v[q] = nxt[v[q]];
        }
        __syncthreads();
#pragma unroll
        for (uint32_t q = 0; q < kEncTile / kEncThreads; ++q) nxt[tid + kEncThreads * q] = (uint16_t)v[q];
        __syncthreads();
    }
    if (tid < kEncReach) a.tab[t * kEncReach + tid] = (uint8_t)(nxt[tid] - kEncTile);
}

// Stage `count` tables of kEncReach bytes (count <= kEncGroup; src 16-byte aligned, readable up to
// the next multiple of 16 bytes).
__device__ __forceinline__ void enc_stage_tables(const uint8_t* src, uint32_t count, uint8_t* tabs) {
    const uint32_t chunks = (count * kEncReach + 15) / 16;
    for (uint32_t i = threadIdx.x; i < chunks; i += kEncThreads)
        reinterpret_cast<uint4*>(tabs)[i] = reinterpret_cast<const uint4*>(src)[i];
    __syncthreads();
}

__global__ __launch_bounds__(kEncThreads) void k_enc_group(SstEncArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t tabs[kEncGroup * kEncReach];
    const uint64_t g = blockIdx.x;
    const uint32_t nt = (uint32_t)std::min<uint64_t>(kEncGroup, a.ntiles - g * kEncGroup);
    enc_stage_tables(a.tab + g * kEncGroup * kEncReach, nt, tabs);
    if (threadIdx.x >= kEncReach) return;
    uint32_t v = threadIdx.x;
    for (uint32_t k = 0; k < nt; ++k) v = tabs[k * kEncReach + v];
    a.gtab[g * kEncReach + threadIdx.x] = (uint8_t)v;
}

__global__ __launch_bounds__(kEncThreads) void k_enc_top(SstEncArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t tabs[kEncGroup * kEncReach];
    uint32_t v = 0;  // the first block starts at entry 0
    for (uint64_t g0 = 0; g0 < a.ngroups; g0 += kEncGroup) {
        const uint32_t ng = (uint32_t)std::min<uint64_t>(kEncGroup, a.ngroups - g0);
        __syncthreads();
        enc_stage_tables(a.gtab + g0 * kEncReach, ng, tabs);
        if (threadIdx.x == 0)
            for (uint32_t k = 0; k < ng; ++k) {
                a.gep[g0 + k] = (uint8_t)v;
                v = tabs[k * kEncReach + v];
            }
    }
}

__global__ __launch_bounds__(kEncThreads) void k_enc_apply(SstEncArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t tabs[kEncGroup * kEncReach];
    const uint64_t g = blockIdx.x;
    const uint32_t nt = (uint32_t)std::min<uint64_t>(kEncGroup, a.ntiles - g * kEncGroup);
    enc_stage_tables(a.tab + g * kEncGroup * kEncReach, nt, tabs);
    if (threadIdx.x != 0) return;
    uint32_t v = a.gep[g];
    for (uint32_t k = 0; k < nt; ++k) {
        a.ep[g * kEncGroup + k] = (uint8_t)v;
        v = tabs[k * kEncReach + v];
    }
}

// The tile's blocks, from its true entry point.  A block belongs to the tile that holds its first
// entry; its last entry (the index key) may lie in the next tile, inside the loaded reach.
template <bool EMIT>
__global__ __launch_bounds__(kEncThreads) void k_enc_walk(SstEncArgs a) {
    __shared__ uint32_t pos[kEncPos];
    __shared__ uint8_t dl[kEncTile];
    __shared__ uint16_t bs[EMIT ? kEncTile : 1], be[EMIT ? kEncTile : 1];  // first / last entry of block k
    __shared__ uint32_t irel[EMIT ? kEncTile + 1 : 1];                     // index bytes before its record
    __shared__ uint32_t s_nb;
    const uint32_t tid = threadIdx.x;
    const uint64_t t = blockIdx.x, t0 = t * kEncTile;
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(kEncTile, a.n - t0);
    const uint32_t avail = (uint32_t)std::min<uint64_t>(kEncTile + kEncReach, a.n - t0);
    const uint64_t off0 = a.offsets[t0];
    enc_load_pos(a, t0, avail, off0, pos);
    for (uint32_t i = tid; i < cnt; i += kEncThreads) dl[i] = a.delta[t0 + i];
    __syncthreads();
    if (tid == 0) {
        uint32_t e = a.ep[t], nb = 0, ib = 0;
        while (e < cnt) {
            const uint32_t f = e + dl[e];  // <= avail: k_enc_tile searched no further
            if constexpr (EMIT) {
                bs[nb] = (uint16_t)e;
                be[nb] = (uint16_t)(f - 1);
                irel[nb] = ib;
            }
            ib += pos[f] - pos[f - 1] - kEncFixed + 8;
            ++nb;
            e = f;
        }
        if constexpr (EMIT) {
            irel[nb] = ib;
            s_nb = nb;
        } else {
            a.tsum[t] = ((uint64_t)nb << 40) | ib;
        }
    }
    if constexpr (EMIT) {
        __syncthreads();
        const uint32_t nb = s_nb;
        if (nb == 0) return;
        const uint64_t tb = a.tbase[t], B = tb >> 40, I = tb & ((1ull << 40) - 1);
        const uint64_t d0 = (off0 - a.offsets[0]) + (uint64_t)kEncFixed * t0;  // data.db bytes before the tile
        if (a.blocks)
            for (uint32_t k = tid; k < nb; k += kEncThreads) a.blocks[B + k] = (uint32_t)(d0 + pos[bs[k]]);
        if (!a.index) return;
        const uint32_t total = irel[nb];
        uint32_t hint = 0;  // a lane moves forward through the records
        for (uint32_t y = tid; y < total; y += kEncThreads) {
            uint32_t lo = hint, hi = nb - 1;
            while (lo < hi) {
                const uint32_t mid = (lo + hi + 1) >> 1;
                if (irel[mid] <= y) lo = mid;
                else hi = mid - 1;
            }
            hint = lo;
            const uint32_t r = y - irel[lo], last = be[lo], L = pos[last + 1] - pos[last] - kEncFixed;
            uint32_t byte;
            if (r < 4) byte = L >> (8 * r);
            else if (r < 4 + L) byte = a.keys[off0 + (pos[last] - kEncFixed * last) + (r - 4)];
            else byte = (uint32_t)(d0 + pos[bs[lo]]) >> (8 * (r - 4 - L));
            a.index[I + y] = (uint8_t)byte;
        }
    }
}

// Fixed stride: block b = entries b * per .. , record b = the stride, the block's last key, b * per * es.
__global__ __launch_bounds__(kEncThreads) void k_enc_index_fixed(SstEncArgs a, uint32_t per, uint64_t nblocks) {
    const uint64_t rs = a.stride + 8, es = a.stride + kEncFixed;
    const uint64_t y = (uint64_t)blockIdx.x * kEncThreads + threadIdx.x;
    if (y >= nblocks * rs) return;
    const uint64_t b = y / rs, start = b * per * es;
    const uint32_t r = (uint32_t)(y - b * rs);
    if (r == 0 && a.blocks) a.blocks[b] = (uint32_t)start;
    if (!a.index) return;
    const uint64_t last = std::min<uint64_t>((b + 1) * per, a.n) - 1;
    uint32_t byte;
    if (r < 4) byte = (uint32_t)a.stride >> (8 * r);
    else if (r < 4 + a.stride) byte = a.keys[last * a.stride + (r - 4)];
    else byte = (uint32_t)start >> (8 * (r - 4 - (uint32_t)a.stride));
    a.index[y] = (uint8_t)byte;
}

// One tile's entries as data.db bytes.
template <bool STRIDE>
struct EncTileView {
    const SstEncArgs& a;
    const uint32_t* pos;
    uint64_t t0, off0;
    uint32_t es;
    __device__ __forceinline__ uint32_t P(uint32_t i) const { return STRIDE ? i * es : pos[i]; }
    __device__ __forceinline__ const uint8_t* key(uint32_t i) const {
        return a.keys + (STRIDE ? (t0 + i) * a.stride : off0 + (pos[i] - kEncFixed * i));
    }
    // Bytes r .. r+3 of entry i, little-endian; those past the entry's end are unspecified.
    __device__ __forceinline__ uint32_t bytes4(uint32_t i, uint32_t r) const {
        const uint32_t L = P(i + 1) - P(i) - kEncFixed;
        const bool tail = r + 4 > 4 + L;  // the dword reaches the 13 bytes behind the key
        uint64_t lo = 0, hi = 0;          // those bytes: value offset | created_at | tombstone
        if (L >= 4) {
            // One key dword, read where the key has four bytes for it, and the fixed fields when
            // the dword reaches them: every load of the lane is issued before the first is used,
            // and the bytes are placed by shifts, not branches (lanes of a wave sit at every
            // position of their entries, so each branch would be taken by some lane).
            const uint32_t kq = r < 4 ? 0u : std::min(r - 4, L - 4);
            uint32_t kd;
            __builtin_memcpy(&kd, key(i) + kq, 4);
            if (tail) {
                const uint64_t e = t0 + i;
                const uint64_t cr = a.created ? (uint64_t)a.created[e] : 0;
                lo = (uint64_t)(a.val_off ? a.val_off[e] : 0u) | (cr << 32);
                hi = (cr >> 32) | ((uint64_t)(a.tomb && a.tomb[e] != 0) << 32);
            }
            const int s = (int)r - 4 - (int)kq;  // output byte t is byte t + s of kd
            uint32_t v = r < 4 ? L >> (8 * r) : 0u;  // L < 2^16: the bytes behind the length are 0
            v |= (s <= -4 || s >= 4) ? 0u : s >= 0 ? kd >> (8 * s) : kd << (8 * -s);
            if (tail) {
                const int q = (int)r - 4 - (int)L;  // -3 .. 12: output byte t is fixed byte t + q
                v |= q < 0    ? (uint32_t)lo << (8 * -q)
                     : q >= 8 ? (uint32_t)(hi >> (8 * (q - 8)))
                              : (uint32_t)(lo >> (8 * q)) | (q > 4 ? (uint32_t)(hi << (8 * (8 - q))) : 0u);
            }
            return v;
        }
        // keys under four bytes: field by field
        if (r == 0) return L;
        if (tail) {
            const uint64_t e = t0 + i;
            const uint64_t cr = a.created ? (uint64_t)a.created[e] : 0;
            lo = (uint64_t)(a.val_off ? a.val_off[e] : 0u) | (cr << 32);
            hi = (cr >> 32) | ((uint64_t)(a.tomb && a.tomb[e] != 0) << 32);
        }
        if (r >= 4 + L) {
            const uint32_t q = r - 4 - L;  // 0 .. 12
            if (q >= 8) return (uint32_t)(hi >> (8 * (q - 8)));
            return (uint32_t)(lo >> (8 * q)) | (q > 4 ? (uint32_t)(hi << (8 * (8 - q))) : 0u);
        }
        const uint8_t* k = key(i);  // a field boundary inside the dword: byte by byte
        uint32_t v = 0;
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t) {
            const uint32_t rr = r + t;
            uint32_t b;
            if (rr < 4) b = L >> (8 * rr);
            else if (rr < 4 + L) b = k[rr - 4];
            else {
                const uint32_t q = rr - 4 - L;
                b = q < 8 ? (uint32_t)(lo >> (8 * q)) : q < 13 ? (uint32_t)(hi >> (8 * (q - 8))) : 0u;
            }
            v |= (b & 0xFFu) << (8 * t);
        }
        return v;
    }
};

template <bool STRIDE>
__global__ __launch_bounds__(kEncThreads) void k_enc_data(SstEncArgs a) {
    __shared__ uint32_t pos[STRIDE ? 1 : kEncTile + 1];
    const uint32_t tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * kEncTile;
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(kEncTile, a.n - t0);
    uint64_t off0 = 0, d0;
    uint32_t es = 0, total;
    if constexpr (STRIDE) {
        es = (uint32_t)a.stride + kEncFixed;
        d0 = t0 * es;
        total = cnt * es;
    } else {
        off0 = a.offsets[t0];
        enc_load_pos(a, t0, cnt, off0, pos);
        __syncthreads();
        d0 = (off0 - a.offsets[0]) + (uint64_t)kEncFixed * t0;
        total = pos[cnt];
    }
    const EncTileView<STRIDE> v{a, pos, t0, off0, es};
    uint8_t* out = a.data + d0;
    // aligned dword w of the output covers tile bytes 4w - sh .. 4w - sh + 3
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(out) & 3), nw = (sh + total + 3) >> 2;
    uint32_t hint = 0;  // a lane moves forward through the entries
    for (uint32_t w = tid; w < nw; w += kEncThreads) {
        const uint32_t xlo = std::max(4 * w, sh) - sh, xhi = std::min(4 * w + 4, sh + total) - sh;
        uint32_t i;
        if constexpr (STRIDE) {
            i = xlo / es;
        } else {
            // a lane's next dword is 1024 bytes on: at most 60 entries of >= 17 bytes further
            uint32_t lo = hint, hi = w == tid ? cnt - 1 : std::min(cnt - 1, hint + 4 * kEncThreads / kEncFixed + 1);
            while (lo < hi) {  // the entry that holds byte xlo
                const uint32_t mid = (lo + hi + 1) >> 1;
                if (pos[mid] <= xlo) lo = mid;
                else hi = mid - 1;
            }
            i = hint = lo;
        }
        if (xhi - xlo == 4) {
            const uint32_t r = xlo - v.P(i), E = v.P(i + 1) - v.P(i);
            uint32_t val = v.bytes4(i, r);
            if (r + 4 > E) {  // the dword runs into the next entry's length field (entries >= 17 bytes)
                const uint32_t k = E - r, L2 = v.P(i + 2) - v.P(i + 1) - kEncFixed;
                val = (val & ((1u << (8 * k)) - 1)) | (L2 << (8 * k));
            }
            *reinterpret_cast<uint32_t*>(out + xlo) = val;
        } else {  // the tile's first / last bytes share their dword with a neighbour tile
            for (uint32_t x = xlo; x < xhi; ++x) {
                if (x >= v.P(i + 1)) ++i;
                out[x] = (uint8_t)v.bytes4(i, x - v.P(i));
            }
        }
    }
}

hipError_t sst_enc_segment(const SstEncArgs& a, hipStream_t s) {
    phase_begin(kPhaseEncTile, s);
    hipLaunchKernelGGL(k_enc_tile, dim3((uint32_t)a.ntiles), dim3(kEncThreads), 0, s, a);
    phase_end(kPhaseEncTile, s);
    phase_begin(kPhaseEncScan, s);
    hipLaunchKernelGGL(k_enc_group, dim3((uint32_t)a.ngroups), dim3(kEncThreads), 0, s, a);
    hipLaunchKernelGGL(k_enc_top, dim3(1), dim3(kEncThreads), 0, s, a);
    hipLaunchKernelGGL(k_enc_apply, dim3((uint32_t)a.ngroups), dim3(kEncThreads), 0, s, a);
    hipLaunchKernelGGL(k_enc_walk<false>, dim3((uint32_t)a.ntiles), dim3(kEncThreads), 0, s, a);
    return hipGetLastError();  // the caller scans tsum and closes the phase
}

hipError_t sst_enc_emit(const SstEncArgs& a, hipStream_t s) {
    const uint32_t ntiles = (uint32_t)((a.n + kEncTile - 1) / kEncTile);
    if (a.index || a.blocks) {
        phase_begin(kPhaseEncIndex, s);
        if (a.offsets) {
            hipLaunchKernelGGL(k_enc_walk<true>, dim3(ntiles), dim3(kEncThreads), 0, s, a);
        } else {
            const uint32_t per = kEncBlock / ((uint32_t)a.stride + kEncFixed);
            const uint64_t nblocks = (a.n + per - 1) / per, bytes = nblocks * (a.stride + 8);
            hipLaunchKernelGGL(k_enc_index_fixed, dim3((uint32_t)((bytes + kEncThreads - 1) / kEncThreads)),
                               dim3(kEncThreads), 0, s, a, per, nblocks);
        }
        phase_end(kPhaseEncIndex, s);
    }
    if (a.data) {
        phase_begin(kPhaseEncData, s);
        if (a.offsets) hipLaunchKernelGGL(k_enc_data<false>, dim3(ntiles), dim3(kEncThreads), 0, s, a);
        else hipLaunchKernelGGL(k_enc_data<true>, dim3(ntiles), dim3(kEncThreads), 0, s, a);
        phase_end(kPhaseEncData, s);
    }
    return hipGetLastError();
}

}  // namespace vbf
