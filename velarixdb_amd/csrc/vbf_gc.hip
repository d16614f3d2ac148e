// The garbage collector's data step on gfx950: GC::gc_handler (src/gc/garbage_collector.rs:168-262)
// after the chunk has been walked (vbf_vlog_walk.hip) and its keys looked up (vbf_table.hip).
//
// The handler sorts the chunk's entries into valid and invalid (:203-214) and, when any is invalid,
// appends a `tail` entry (write_tail_to_disk, :265-275) and the valid entries with their MOST RECENT
// values (write_valid_entries_to_vlog, :304-317) to the log.  Both the key and the value of every
// appended entry already lie in the window on the device, so the bytes to append are written straight
// from it: no key or value buffer in between.
//
//   k_gc_overlay : one lane per chunk entry.  Steps 1 and 2 of GC::get (:440-463), folded by the
//                  caller into one sorted map: a binary search of the entry's key (read in the
//                  window) with cmp_keys; a hit overrides the tables' answer whatever its time.
//   k_gc_judge   : one lane per chunk entry.  The first test that applies gives the verdict: the key
//                  is nowhere, the winner is a tombstone, then k_vlog_sizes' window checks on the
//                  most recent entry (at or past the end: none; before the base or cut by the end:
//                  BAD, the first such entry by an atomic min), its tombstone byte, the signed time
//                  compare (:205) and the one-byte "*" test (:206).  A valid entry gets the size of
//                  its appended entry, 17 + own key + most recent value, and the two places in the
//                  window they are copied from.  An exclusive scan over the sizes, the `tail` put as
//                  item 0, places the entries; a select of the valid entries' indices gives put_ids.
//   k_gc_emit    : the hot path, the balanced copy of vbf_vlog.hip over the bytes to append.  Values
//                  run from 0 bytes to megabytes, so the work is divided by OUTPUT bytes: workgroup b
//                  owns slice b of the destination, finds the puts that overlap it by binary search
//                  in the scanned positions (staged in LDS when at most kVlogWindow apart), and each
//                  lane stores whole aligned 16-byte granules gathered piece by piece: header bytes
//                  from registers, key bytes and value bytes from their two places in the log, each
//                  piece one 16-byte load at the source's own alignment (bytewise only where 16 bytes
//                  would run past the window).  Put 0's key and value come from registers.  Nothing
//                  outside bytes[0..len) is read, nothing outside append[0..total) is written.  Also
//                  writes put_val_offsets and put_tombstones.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vbf_granule.hpp"
#include "vbf_kernels.hpp"
#include "vbf_keycmp.hpp"

namespace vbf {

namespace {

__device__ __forceinline__ uint32_t rd4(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

__global__ __launch_bounds__(256) void k_gc_overlay(GcArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const uint8_t* e = a.bytes + (a.entry_off[i] - a.base);  // a whole entry: the walk checked it
    const uint8_t* key = e + kHdr;
    const uint64_t kl = rd4(e);
    uint64_t lo = 0, hi = a.ov_n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        const uint64_t k0 = a.ov_off[mid], k1 = a.ov_off[mid + 1];
        const int c = cmp_keys(a.ov_keys + k0, k1 - k0, key, kl);
        if (c == 0) {
            a.found[i] = a.ov_tomb[mid] ? 2 : 1;
            a.val_off[i] = a.ov_val[mid];
            a.wcreated[i] = (uint64_t)a.ov_created[mid];
            return;
        }
        if (c < 0) lo = mid + 1;
        else hi = mid;
    }
}

__global__ __launch_bounds__(256) void k_gc_judge(GcArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        a.size[0] = kGcTailSize;
        a.size[a.n + 1] = 0;
    }
    if (i >= a.n) return;
    const uint64_t p = a.entry_off[i] - a.base;
    const uint8_t* own = a.bytes + p;
    const uint8_t fd = a.found[i];
    uint8_t vd = kGcValid;
    uint64_t kl = 0, vl = 0, vsrc = 0;
    if (fd == 0) {
        vd = kGcAbsent;
    } else if (fd != 1) {
        vd = kGcDeleted;
    } else {
        const uint64_t off = a.val_off[i], end = a.base + a.len;
        if (off >= end) {
            vd = kGcLogNone;
        } else if (off < a.base || off + kHdr > end) {
            vd = kGcBad;
        } else {
            const uint8_t* e = a.bytes + (off - a.base);
            const uint64_t wkl = rd4(e), wvl = rd4(e + 4);
            if (off + kHdr + wkl + wvl > end) {  // at most 2^32 + 2^33: no wrap in 64 bits
                vd = kGcBad;
            } else if (e[16] == 1) {
                vd = kGcLogTombstone;
            } else {
                int64_t created;
                __builtin_memcpy(&created, own + 8, 8);
                if (created < (int64_t)a.wcreated[i]) {
                    vd = kGcOlder;
                } else if (wvl == 1 && e[kHdr + wkl] == '*') {
                    vd = kGcStar;
                } else {
                    kl = rd4(own);
                    vl = wvl;
                    vsrc = (off - a.base) + kHdr + wkl;
                }
            }
        }
    }
    const bool valid = vd == kGcValid;
    a.verdict[i] = vd;
    a.keep[i] = valid;
    a.ids[i] = (uint32_t)i;
    a.size[i + 1] = valid ? kHdr + kl + vl : 0;
    a.ksrc[i] = p + kHdr;
    a.vsrc[i] = vsrc;
    a.klen[i] = (uint32_t)kl;
    a.vlen[i] = (uint32_t)vl;
    if (vd == kGcBad) atomicMin(reinterpret_cast<unsigned long long*>(&a.res->bad), (unsigned long long)i);
    if (!valid) atomicAdd(reinterpret_cast<unsigned long long*>(&a.res->n_invalid), 1ull);
    else atomicMax(reinterpret_cast<unsigned long long*>(&a.res->last_valid), (unsigned long long)(i + 1));
}

// Put j as the copy reads it: its lengths, where its key and value start in the window, the header
// (bytes 0..15 as one word; byte 16, the tombstone, is always 0) and, for put 0, the 12 bytes of key
// and value as one word.
struct GcPut {
    uint64_t kl, vl, ksrc, vsrc;
    u128 hdr, lit;
    bool reg;
};
__device__ __forceinline__ GcPut gc_put(const GcArgs& a, uint64_t j) {
    GcPut e;
    e.reg = j == 0;
    if (e.reg) {
        e.kl = 4;
        e.vl = 8;
        e.ksrc = e.vsrc = 0;
        e.lit = (u128)0x6C696174u | ((u128)a.new_tail << 32);  // "tail", LE64(new tail)
    } else {
        const uint32_t id = a.put_ids[j];
        e.kl = a.klen[id];
        e.vl = a.vlen[id];
        e.ksrc = a.ksrc[id];
        e.vsrc = a.vsrc[id];
        e.lit = 0;
    }
    e.hdr = (u128)(e.kl | (e.vl << 32)) | ((u128)(uint64_t)a.now_ms << 64);
    return e;
}

// Put j's first byte in the bytes to append.
__device__ __forceinline__ uint64_t gc_start(const GcArgs& a, uint64_t j) {
    return j == 0 ? 0 : a.pos[(uint64_t)a.put_ids[j] + 1];
}

// start(j): put j's first byte in the output, for first <= j <= last.
template <class St>
__device__ __forceinline__ void gc_granules(const GcArgs& a, const Slice& s, uint64_t first, uint64_t last, St&& start) {
    for (uint64_t x = s.x0 + (uint64_t)threadIdx.x * kGran; x < s.x1; x += 256 * kGran) {
        const uint64_t lo = x > s.head ? x : s.head, hi = x + kGran < s.end ? x + kGran : s.end;
        uint64_t p = lo - s.head;
        const uint64_t pe = hi - s.head;
        uint64_t j = last_le(first, last, p, start);  // puts are at least 17 bytes: start(j) <= p < start(j + 1)
        GcPut e = gc_put(a, j);
        uint64_t q = p - start(j);                    // byte q of put j
        uint32_t at = (uint32_t)(lo - x);
        u128 g = 0;
        while (p < pe) {
            if (q >= kHdr + e.kl + e.vl) {  // the next put starts here (none is empty)
                e = gc_put(a, ++j);
                q = 0;
            }
            const uint64_t room = pe - p;
            uint64_t n;
            u128 v;
            if (q < kHdr) {  // header bytes q .. q + n - 1: bytes 0..15 from hdr, byte 16 is 0
                n = kHdr - q < room ? kHdr - q : room;
                v = q < 16 ? e.hdr >> (8 * (uint32_t)q) : 0;
                if (n < kGran) v &= ((u128)1 << (8 * (uint32_t)n)) - 1;
            } else if (e.reg) {  // put 0: key and value from registers
                n = kHdr + 12 - q < room ? kHdr + 12 - q : room;
                v = e.lit >> (8 * (uint32_t)(q - kHdr));
                if (n < kGran) v &= ((u128)1 << (8 * (uint32_t)n)) - 1;
            } else if (q < kHdr + e.kl) {
                n = kHdr + e.kl - q < room ? kHdr + e.kl - q : room;
                const uint64_t kp = e.ksrc + (q - kHdr);
                v = ld_piece(a.bytes + kp, (uint32_t)n, kp + kGran <= a.len);
            } else {
                n = kHdr + e.kl + e.vl - q < room ? kHdr + e.kl + e.vl - q : room;
                const uint64_t vp = e.vsrc + (q - kHdr - e.kl);
                v = ld_piece(a.bytes + vp, (uint32_t)n, vp + kGran <= a.len);
            }
            g |= v << (8 * at);
            at += (uint32_t)n;
            p += n;
            q += n;
        }
        store_gran(a.append, s, x, lo, hi, g);
    }
}

__global__ __launch_bounds__(256) void k_gc_emit(GcArgs a) {
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < a.n_puts; j += (uint64_t)gridDim.x * 256) {
        if (a.put_val_offsets) a.put_val_offsets[j] = (uint32_t)(a.log_size + gc_start(a, j));
        if (a.put_tombstones) a.put_tombstones[j] = j != 0 && a.vlen[a.put_ids[j]] == 0;
    }
    if (!a.append) return;
    const Slice s = slice_of(a.append, a.total);
    if (s.x0 >= s.end) return;
    __shared__ uint64_t sh[2];
    __shared__ uint64_t lst[kVlogWindow];
    slice_items(s, a.n_puts, [&a](uint64_t j) { return gc_start(a, j); }, sh);
    const uint64_t first = sh[0], last = sh[1], cnt = last - first + 1;
    if (cnt <= kVlogWindow) {  // the same in every lane of the workgroup
        for (uint32_t k = threadIdx.x; k < cnt; k += 256) lst[k] = gc_start(a, first + k);
        __syncthreads();
        gc_granules(a, s, first, last, [&](uint64_t j) { return lst[j - first]; });
    } else {
        gc_granules(a, s, first, last, [&a](uint64_t j) { return gc_start(a, j); });
    }
}

}  // namespace

hipError_t gc_overlay(const GcArgs& a, hipStream_t s) {
    if (a.n == 0 || a.ov_n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_gc_overlay, dim3((uint32_t)((a.n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t gc_judge(const GcArgs& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_gc_judge, dim3((uint32_t)((a.n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t gc_emit(const GcArgs& a, hipStream_t s) {
    if (a.n_puts == 0 || (!a.append && !a.put_val_offsets && !a.put_tombstones)) return hipSuccess;
    uint64_t nb = a.append ? slices_of(a.append, a.total) : (a.n_puts + 255) / 256;
    if (nb > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (nb == 0) nb = 1;
    hipLaunchKernelGGL(k_gc_emit, dim3((uint32_t)nb), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace vbf
