"""Value-log walk timing, beside tools/vlog_get_bench.py and with its conventions: a clock settle, W
untimed warm-up steps, then K steps timed with device events around each call.

  python tools/vlog_walk_bench.py [--cases meta,full26,full1k] [--steps 10] [--warmup 2] [--scale 1.0]

One process, everything device-resident, one JSON line per case.  The log is written by
vbf_vlog_encode_dev and walked from its first byte to its end (budget UINT64_MAX: recover):
  meta    10M entries of 26 bytes (5-byte key, 4-byte value: the fixture's entry size), every
          per-entry array but no key or value bytes
  full26  the same log, every array
  full1k  256K entries with 16-byte keys and 1 KiB values, every array
Per case:
  walk        vbf_vlog_walk_dev with the outputs sized by a size query: entries/s and GB/s of log
              walked (the call synchronises the stream once per 8 MiB segment; that is in the time)
  sizes       the size query alone (no output array)
  memcpy      a device-to-device hipMemcpyAsync of the log's bytes: the ceiling
  serial      tools/vlog_walk_serial.hip, one lane following the chain and writing entry_off, over
              the first --serial-mib MiB of the log (its time is linear in the entries)
The entry positions of both walks are compared with the encoder's val_offsets once per case.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import torch  # noqa: E402

import velarixdb_amd as vbf  # noqa: E402
from velarixdb_amd._lib import call, lib  # noqa: E402

from sst_write_bench import timed, vp  # noqa: E402
from vlog_get_bench import hip_runtime  # noqa: E402

T0 = 1720785462000
U64MAX = 2**64 - 1
SERIAL_LIB = os.path.join(HERE, "libvlog_walk_serial.so")
CASES = {"meta": (10_000_000, 5, 4, False), "full26": (10_000_000, 5, 4, True), "full1k": (262_144, 16, 1024, True)}


def serial_lib():
    src = os.path.join(HERE, "vlog_walk_serial.hip")
    if not os.path.exists(SERIAL_LIB) or os.path.getmtime(SERIAL_LIB) < os.path.getmtime(src):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call([hipcc, "--offload-arch=" + os.environ.get("VBF_OFFLOAD_ARCH", "gfx950"), "-O3",
                               "-std=c++20", "-shared", "-fPIC", "-o", SERIAL_LIB, src])
    so = ctypes.CDLL(SERIAL_LIB)
    so.vlog_walk_serial.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                    ctypes.c_void_p]
    so.vlog_walk_serial.restype = ctypes.c_int
    return so


def run(case, args, dev, sp, rt, so):
    n0, klen, vlen, full = CASES[case]
    N = max(int(n0 * args.scale), 1)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    keys = torch.randint(0, 256, (N * klen,), dtype=torch.uint8, device=dev, generator=g)
    values = torch.randint(0, 256, (N * vlen,), dtype=torch.uint8, device=dev, generator=g)
    voff = torch.arange(N + 1, device=dev, dtype=torch.int64) * vlen
    cr = T0 + torch.arange(N, device=dev, dtype=torch.int64)
    ln = ctypes.c_uint64()
    head = (vp(keys), None, klen, N, vp(values), vp(voff), vp(cr), None, 0)
    call("vbf_vlog_encode_dev", *head, None, 0, ctypes.byref(ln), None, sp)
    log = torch.empty(ln.value, dtype=torch.uint8, device=dev)
    vo = torch.empty(N, dtype=torch.int32, device=dev)
    call("vbf_vlog_encode_dev", *head, vp(log), ln.value, ctypes.byref(ln), vp(vo), sp)
    torch.cuda.synchronize()
    del values, voff
    L = ln.value
    hv = ctypes.c_void_p()
    call("vbf_vlog_open_dev", vp(log), L, 0, ctypes.byref(hv))
    res = {"case": case, "entries": N, "entry_bytes": 17 + klen + vlen, "log_bytes": L, "steps": args.steps,
           "warmup": args.warmup}

    sc = [ctypes.c_uint64() for _ in range(4)]
    stop = ctypes.c_int()
    tail = [ctypes.byref(x) for x in sc] + [ctypes.byref(stop), sp]

    def sizes():
        call("vbf_vlog_walk_dev", hv, 0, U64MAX, None, None, None, 0, None, None, 0, None, None, None, 0, *tail)

    sizes()
    n, kb, vb = sc[0].value, sc[1].value, sc[2].value
    assert (n, kb, vb, sc[3].value, stop.value) == (N, N * klen, N * vlen, L, 0)
    eo = torch.empty(n + 1, dtype=torch.int64, device=dev)
    wvo = torch.empty(n, dtype=torch.int32, device=dev)
    ko = torch.empty(n + 1, dtype=torch.int64, device=dev)
    vof = torch.empty(n + 1, dtype=torch.int64, device=dev)
    wcr = torch.empty(n, dtype=torch.int64, device=dev)
    wtb = torch.empty(n, dtype=torch.uint8, device=dev)
    kout = torch.empty(kb, dtype=torch.uint8, device=dev) if full else None
    vout = torch.empty(vb, dtype=torch.uint8, device=dev) if full else None

    def walk():
        call("vbf_vlog_walk_dev", hv, 0, U64MAX, vp(eo), vp(wvo), vp(kout), kb, vp(ko), vp(vout), vb, vp(vof), vp(wcr),
             vp(wtb), n, *tail)

    for name, fn in (("sizes", sizes), ("walk", walk)):
        r = timed(fn, args.steps, args.warmup)
        r["entries_per_s"] = round(N / r["ms_per_step"] * 1e3)
        r["log_GB_per_s"] = round(L / r["ms_per_step"] / 1e6, 2)
        res[name] = r
    torch.cuda.synchronize()
    assert torch.equal(wvo, vo) and torch.equal(eo[:-1], vo.to(torch.int64) & 0xFFFFFFFF) and int(eo[-1]) == L
    assert torch.equal(wcr, cr) and not bool(wtb.any()) and int(ko[-1]) == kb and int(vof[-1]) == vb
    if full:
        assert torch.equal(kout, keys), "walked key bytes differ from the keys"

    scratch = torch.empty(L, dtype=torch.uint8, device=dev)

    def memcpy():
        rc = rt.hipMemcpyAsync(scratch.data_ptr(), log.data_ptr(), L, 3, sp)  # hipMemcpyDeviceToDevice
        assert rc == 0

    r = timed(memcpy, args.steps, args.warmup)
    r["GB_per_s"] = round(L / r["ms_per_step"] / 1e6, 1)
    res["memcpy_d2d"] = r
    del scratch

    # the one-lane walk over a prefix of whole entries
    entry = 17 + klen + vlen
    sn = max(min(N, (args.serial_mib << 20) // entry), 1)
    s_out = torch.zeros(2, dtype=torch.int64, device=dev)
    s_eo = torch.empty(sn, dtype=torch.int64, device=dev)

    def serial():
        rc = so.vlog_walk_serial(log.data_ptr(), sn * entry, s_eo.data_ptr(), sn, s_out.data_ptr(), sp)
        assert rc == 0

    r = timed(serial, max(args.steps // 3, 2), 1)
    torch.cuda.synchronize()
    assert s_out.tolist() == [sn, sn * entry] and torch.equal(s_eo, eo[:sn])
    r["entries"] = sn
    r["entries_per_s"] = round(sn / r["ms_per_step"] * 1e3)
    r["log_GB_per_s"] = round(sn * entry / r["ms_per_step"] / 1e6, 3)
    res["serial_one_lane"] = r
    res["walk_over_serial"] = round(res["walk"]["entries_per_s"] / r["entries_per_s"], 2)
    res["walk_over_memcpy"] = round(res["walk"]["log_GB_per_s"] / res["memcpy_d2d"]["GB_per_s"], 4)
    lib.vbf_vlog_free(hv)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="meta,full26,full1k")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="scales every entry count (a quick run)")
    ap.add_argument("--serial-mib", type=int, default=32, help="MiB of the log the one-lane kernel walks")
    args = ap.parse_args()
    assert torch.cuda.is_available() and vbf.device_count() > 0, "needs an MI355X: there is no CPU path"
    dev = torch.device("cuda:0")
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rt = hip_runtime()
    so = serial_lib()
    for case in args.cases.split(","):
        run(case, args, dev, sp, rt, so)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
