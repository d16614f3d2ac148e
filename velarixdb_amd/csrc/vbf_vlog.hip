// Batched value-log reads and appends on gfx950: the last step of a get and the first of a put.
//
// The log (src/vlog/v_log.rs) is a file of entries laid back to back, little-endian, no padding and
// no index (ValueLogEntry::serialize, v_log.rs:291-309):
//
//     u32 key_len | u32 val_len | u64 created_at ms | u8 tombstone | key | value
//
// An entry is addressed by the file position of its first byte; data.db stores that as a u32.
// ValueLog::get (v_log.rs:205-207) -> VLogFileNode::get (fs/mod.rs:470-518) seeks there, reads the
// 17-byte header, skips the key and returns the value; DataStore::get_value_from_vlog
// (db/store.rs:628-641) turns a tombstone (byte == 1) into None.  ValueLog::append (v_log.rs:173-196)
// writes an entry at the file's size and returns that position.
//
//   k_vlog_sizes  : one lane per item.  Mask, window checks (in 64 bits: key_len = val_len =
//                   0xFFFFFFFF must not wrap), the header read at the entry's own byte offset, the
//                   optional key compare in 8-byte words; writes status, value length and the
//                   value's position in the log.  An exclusive scan of the lengths (scan_u64)
//                   places the values; the total is read back.
//   k_vlog_copy   : the hot path.  Values run from 0 bytes to megabytes, so the work is divided by
//                   OUTPUT bytes, not by item: workgroup b owns the destination granules (16-byte
//                   words aligned on the destination ADDRESS) of slice b, kVlogSlice bytes of the
//                   address range that holds `values`.  It finds the first and last item that
//                   overlap its slice by binary search in value_off and, when they are at most
//                   kVlogWindow apart, stages their value_off and source positions in LDS.  Lane t
//                   then takes granules t, t + 256, ... of the slice, so a wave stores 1 KiB
//                   contiguous per instruction.  Per granule a lane finds its item by binary search
//                   between those two items (no steps inside a large value, a handful over a run of
//                   short ones -- never one lane for a whole run) and gathers the granule piece by
//                   piece: one piece per value that overlaps it, each one 16-byte load at the
//                   source's own alignment, masked to the piece and shifted to its place (bytewise
//                   only where 16 bytes would run past the end of the log).  A granule inside one
//                   value is one piece.  The granule is stored once, as one aligned 16-byte word; the
//                   two ragged granules at values[0] and values[total) store their bytes singly.
//                   Every granule is written by exactly one lane; nothing outside bytes[0..len) is
//                   read and nothing outside values[0..total) is written.
//   k_vlog_encode : the same balanced copy over the output of an append: per entry three segments,
//                   the 17 header bytes (from registers), the key, the value.  Entry j starts at
//                   17 j + (key bytes before j) + (value bytes before j): a closed form of the two
//                   offset arrays, so the search needs no scan.  Also writes val_offsets.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vbf_granule.hpp"
#include "vbf_kernels.hpp"
#include "vbf_table_search.hpp"

namespace vbf {

namespace {

// a[0..la) == b[0..la) in 8-byte words read at the keys' own byte offsets, the last 0..7 bytes
// bytewise.  No byte outside either key is read.
__device__ __forceinline__ bool same_bytes(const uint8_t* a, const uint8_t* b, uint64_t n) {
    uint64_t i = 0;
    for (; i + 8 <= n; i += 8)
        if (ld8(a + i) != ld8(b + i)) return false;
    for (; i < n; ++i)
        if (a[i] != b[i]) return false;
    return true;
}

__global__ __launch_bounds__(256) void k_vlog_sizes(VlogGetArgs a) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= a.n) return;
    uint8_t st = kVlogSkipped;
    uint64_t vl = 0, src = 0;
    if (!a.found || a.found[j] == 1) {
        const uint64_t off = a.val_offsets[j], end = a.base + a.len;
        if (off >= end) {
            st = kVlogNone;
        } else if (off < a.base || off + kHdr > end) {
            st = kVlogBad;
        } else {
            const uint8_t* e = a.bytes + (off - a.base);
            const uint64_t kl = ld4(e), v = ld4(e + 4);
            if (off + kHdr + kl + v > end) {  // at most 2^32 + 2^33: no wrap in 64 bits
                st = kVlogBad;
            } else {
                bool same = true;
                if (a.keys) {
                    const uint64_t k0 = a.offsets ? a.offsets[j] : j * a.stride;
                    const uint64_t k1 = a.offsets ? a.offsets[j + 1] : k0 + a.stride;
                    same = k1 - k0 == kl && k0 <= k1 && same_bytes(e + kHdr, a.keys + k0, kl);
                }
                if (!same) {
                    st = kVlogKeyMismatch;
                } else if (e[16] == 1) {
                    st = kVlogTombstone;
                } else {
                    st = kVlogValue;
                    vl = v;
                    src = (off - a.base) + kHdr + kl;
                }
            }
        }
    }
    a.status[j] = st;
    a.vlen[j] = vl;
    a.src[j] = src;
}

// The granules of the slice, lane t taking t, t + 256, ...  voff(i) / src(i): item i's place in the
// output stream and its value's position in the log, for first <= i <= last (voff also for last + 1).
template <class V, class S>
__device__ __forceinline__ void copy_granules(const VlogGetArgs& a, const Slice& s, uint64_t first, uint64_t last,
                                              V&& voff, S&& src) {
    for (uint64_t x = s.x0 + (uint64_t)threadIdx.x * kGran; x < s.x1; x += 256 * kGran) {
        const uint64_t lo = x > s.head ? x : s.head, hi = x + kGran < s.end ? x + kGran : s.end;
        uint64_t p = lo - s.head;
        const uint64_t pe = hi - s.head;
        uint64_t i = last_le(first, last, p, voff);  // voff(i) <= p < voff(i + 1): item i holds byte p
        uint32_t at = (uint32_t)(lo - x);            // the granule's byte the next piece starts at
        u128 g = 0;
        while (p < pe) {
            uint64_t nxt = voff(i + 1);
            while (p >= nxt) {  // the next item with a byte (zero-length values in between)
                ++i;
                nxt = voff(i + 1);
            }
            const uint64_t e = nxt < pe ? nxt : pe;
            const uint32_t n = (uint32_t)(e - p);
            const uint64_t pos = src(i) + (p - voff(i));
            g |= ld_piece(a.bytes + pos, n, pos + kGran <= a.len) << (8 * at);
            at += n;
            p = e;
        }
        store_gran(a.values, s, x, lo, hi, g);
    }
}

__global__ __launch_bounds__(256) void k_vlog_copy(VlogGetArgs a) {
    const Slice s = slice_of(a.values, a.total);
    if (s.x0 >= s.end) return;
    __shared__ uint64_t sh[2];
    __shared__ uint64_t lv[kVlogWindow + 1], ls[kVlogWindow];
    const uint64_t* gv = a.voff;
    const uint64_t* gs = a.src;
    slice_items(s, a.n, [gv](uint64_t i) { return gv[i]; }, sh);
    const uint64_t first = sh[0], last = sh[1], cnt = last - first + 1;
    if (cnt <= kVlogWindow) {  // the same in every lane of the workgroup
        for (uint32_t k = threadIdx.x; k <= cnt; k += 256) lv[k] = gv[first + k];
        for (uint32_t k = threadIdx.x; k < cnt; k += 256) ls[k] = gs[first + k];
        __syncthreads();
        copy_granules(a, s, first, last, [&](uint64_t i) { return lv[i - first]; },
                      [&](uint64_t i) { return ls[i - first]; });
    } else {
        copy_granules(a, s, first, last, [gv](uint64_t i) { return gv[i]; }, [gs](uint64_t i) { return gs[i]; });
    }
}

// ---- append ----

// Key / value bytes in front of entry j (positions in the caller's arrays) and the entry's place in
// the output: 17 j + key bytes before j + value bytes before j.
struct EncPos {
    const VlogEncArgs& a;
    __device__ __forceinline__ uint64_t kpos(uint64_t j) const { return a.offsets ? a.offsets[j] : j * a.stride; }
    __device__ __forceinline__ uint64_t vpos(uint64_t j) const { return a.value_off[j]; }
    __device__ __forceinline__ uint64_t start(uint64_t j) const {
        return kHdr * j + (kpos(j) - a.k0) + (vpos(j) - a.v0);
    }
};

// One lane per entry: both offset arrays nondecreasing, key and value lengths within u32.
__global__ __launch_bounds__(256) void k_vlog_enc_check(VlogEncArgs a) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= a.n) return;
    uint32_t bits = 0;
    const uint64_t v0 = a.value_off[j], v1 = a.value_off[j + 1];
    if (v0 > v1) bits |= kVlogEncErrOrder;
    else if (v1 - v0 > 0xFFFFFFFFull) bits |= kVlogEncErrLong;
    if (a.offsets) {
        const uint64_t k0 = a.offsets[j], k1 = a.offsets[j + 1];
        if (k0 > k1) bits |= kVlogEncErrOrder;
        else if (k1 - k0 > 0xFFFFFFFFull) bits |= kVlogEncErrLong;
    }
    if (bits) {
        atomicOr(a.err, bits);
        atomicMin(a.err + 1, (uint32_t)(j > 0xFFFFFFFEull ? 0xFFFFFFFEull : j));
    }
}

// Entry j as the copy reads it: its lengths, where its key and value start in the caller's arrays,
// and the header: bytes 0..15 as one word, byte 16 apart.
struct EncEntry {
    uint64_t kl, vl, kabs, vabs;
    u128 hdr;
    uint8_t tomb;
};
__device__ __forceinline__ EncEntry enc_entry(const VlogEncArgs& a, const EncPos& f, uint64_t j) {
    EncEntry e;
    e.kabs = f.kpos(j);
    e.vabs = f.vpos(j);
    e.kl = f.kpos(j + 1) - e.kabs;
    e.vl = f.vpos(j + 1) - e.vabs;
    e.hdr = (u128)((e.kl & 0xFFFFFFFFull) | (e.vl << 32)) | ((u128)(a.created ? (uint64_t)a.created[j] : 0) << 64);
    e.tomb = a.tomb ? (a.tomb[j] != 0) : 0;
    return e;
}

// start(j): entry j's first byte in the output, for first <= j <= last.
template <class St>
__device__ __forceinline__ void encode_granules(const VlogEncArgs& a, const EncPos& f, const Slice& s, uint64_t first,
                                                uint64_t last, St&& start) {
    for (uint64_t x = s.x0 + (uint64_t)threadIdx.x * kGran; x < s.x1; x += 256 * kGran) {
        const uint64_t lo = x > s.head ? x : s.head, hi = x + kGran < s.end ? x + kGran : s.end;
        uint64_t p = lo - s.head;
        const uint64_t pe = hi - s.head;
        uint64_t j = last_le(first, last, p, start);  // entries are at least 17 bytes: start(j) <= p < start(j + 1)
        EncEntry e = enc_entry(a, f, j);
        uint64_t q = p - start(j);                    // byte q of entry j
        uint32_t at = (uint32_t)(lo - x);
        u128 g = 0;
        while (p < pe) {
            if (q >= kHdr + e.kl + e.vl) {  // the next entry starts here (none is empty)
                e = enc_entry(a, f, ++j);
                q = 0;
            }
            const uint64_t room = pe - p;
            uint64_t n;
            u128 v;
            if (q < kHdr) {  // header bytes q .. q + n - 1: bytes 0..15 from hdr, byte 16 the tombstone
                n = kHdr - q < room ? kHdr - q : room;
                v = q < 16 ? e.hdr >> (8 * (uint32_t)q) : 0;
                if (q != 0) v |= (u128)e.tomb << (8 * (uint32_t)(16 - q));
                if (n < kGran) v &= ((u128)1 << (8 * (uint32_t)n)) - 1;
            } else if (q < kHdr + e.kl) {
                n = kHdr + e.kl - q < room ? kHdr + e.kl - q : room;
                const uint64_t kp = e.kabs + (q - kHdr);
                v = ld_piece(a.keys + kp, (uint32_t)n, kp + kGran <= a.k_end);
            } else {
                n = kHdr + e.kl + e.vl - q < room ? kHdr + e.kl + e.vl - q : room;
                const uint64_t vp = e.vabs + (q - kHdr - e.kl);
                v = ld_piece(a.values + vp, (uint32_t)n, vp + kGran <= a.v_end);
            }
            g |= v << (8 * at);
            at += (uint32_t)n;
            p += n;
            q += n;
        }
        store_gran(a.out, s, x, lo, hi, g);
    }
}

__global__ __launch_bounds__(256) void k_vlog_encode(VlogEncArgs a) {
    const EncPos f{a};
    if (a.val_offsets)
        for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < a.n; j += (uint64_t)gridDim.x * 256)
            a.val_offsets[j] = (uint32_t)(a.base + f.start(j));
    if (!a.out) return;
    const Slice s = slice_of(a.out, a.total);
    if (s.x0 >= s.end) return;
    __shared__ uint64_t sh[2];
    __shared__ uint64_t lst[kVlogWindow];
    slice_items(s, a.n, [&f](uint64_t j) { return f.start(j); }, sh);
    const uint64_t first = sh[0], last = sh[1], cnt = last - first + 1;
    if (cnt <= kVlogWindow) {  // the same in every lane of the workgroup
        for (uint32_t k = threadIdx.x; k < cnt; k += 256) lst[k] = f.start(first + k);
        __syncthreads();
        encode_granules(a, f, s, first, last, [&](uint64_t j) { return lst[j - first]; });
    } else {
        encode_granules(a, f, s, first, last, [&f](uint64_t j) { return f.start(j); });
    }
}

}  // namespace

hipError_t vlog_sizes(const VlogGetArgs& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_vlog_sizes, dim3((uint32_t)((a.n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t vlog_copy(const VlogGetArgs& a, hipStream_t s) {
    if (a.total == 0 || a.n == 0 || !a.values) return hipSuccess;
    const uint64_t nb = slices_of(a.values, a.total);
    if (nb > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_vlog_copy, dim3((uint32_t)nb), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t vlog_enc_check(const VlogEncArgs& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_vlog_enc_check, dim3((uint32_t)((a.n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t vlog_encode(const VlogEncArgs& a, hipStream_t s) {
    if (a.n == 0 || (!a.out && !a.val_offsets)) return hipSuccess;
    uint64_t nb = a.out ? slices_of(a.out, a.total) : (a.n + 255) / 256;
    if (nb > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (nb == 0) nb = 1;
    hipLaunchKernelGGL(k_vlog_encode, dim3((uint32_t)nb), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace vbf
