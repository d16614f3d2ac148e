// vlog_walk_serial.hip -- the obvious walk of a value log, for tools/vlog_walk_bench.py only: ONE lane
// follows p -> p + 17 + key_len(p) + val_len(p) and writes every entry's position.  One dependent
// memory round trip per entry; the library's tiled walk (velarixdb_amd/csrc/vbf_vlog_walk.hip) is
// measured against it.  Not part of libvbf.so.
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++20 -shared -fPIC -o tools/libvlog_walk_serial.so tools/vlog_walk_serial.hip
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__global__ void k_walk_serial(const uint8_t* bytes, uint64_t len, uint64_t* entry_off, uint64_t cap, uint64_t* out) {
    uint64_t p = 0, n = 0;
    while (p < len) {
        if (len - p < 17) break;
        uint32_t kl, vl;
        __builtin_memcpy(&kl, bytes + p, 4);
        __builtin_memcpy(&vl, bytes + p + 4, 4);
        const uint64_t body = (uint64_t)kl + vl;
        if (len - p - 17 < body) break;
        if (n < cap) entry_off[n] = p;
        ++n;
        p += 17 + body;
    }
    out[0] = n;  // entries
    out[1] = p;  // where the walk stopped
}

}  // namespace

// entry_off: cap slots; out: two u64 (entries, end).  Queued on `stream`.
extern "C" int vlog_walk_serial(const uint8_t* bytes, uint64_t len, uint64_t* entry_off, uint64_t cap, uint64_t* out,
                                void* stream) {
    hipLaunchKernelGGL(k_walk_serial, dim3(1), dim3(1), 0, (hipStream_t)stream, bytes, len, entry_off, cap, out);
    return (int)hipGetLastError();
}
