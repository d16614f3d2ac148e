"""Value-log fetch and append timing, beside tools/table_get_bench.py and with its conventions: a
clock settle, W untimed warm-up steps, then K steps timed with device events around each call.

  python tools/vlog_get_bench.py [--shapes small,page,huge,mix] [--steps 10] [--warmup 2] [--scale 1.0]

One process, everything device-resident, one JSON line per shape:
  small  10M fetches of 100 B values      (a log of 10M entries)
  page   1M fetches of 4 KiB values       (a log of 256K entries, offsets drawn with repeats: 1M
                                           distinct 4 KiB entries would pass 2^32 bytes)
  huge   4 096 fetches of 1 MiB values    (a log of 1 024 entries)
  mix    64K fetches, value lengths log-uniform in [16 B, 256 KiB] (a log of 32K entries)
Keys are 16 bytes (a counter big-endian, twice: sorted by construction).  Per shape:
  encode      vbf_vlog_encode_dev of the log's entries: entries/s and GB/s of log written
  table_get   vbf_table_get_dev alone on the fetched keys (one table, encoded from the append's
              val_offsets and opened on those buffers)
  fetch       vbf_vlog_get_dev fed with the lookup's found / val_offsets: fetches/s and GB/s of
              value bytes delivered
  get+fetch   the two in a row: what the fetch adds to a get
  memcpy      a device-to-device hipMemcpyAsync of the same value_bytes: the ceiling
The fetched bytes are compared with the values once per shape (torch gather on the device).
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import velarixdb_amd as vbf  # noqa: E402
from velarixdb_amd._lib import call, lib  # noqa: E402

from sst_write_bench import timed, vp  # noqa: E402
from table_get_bench import be16  # noqa: E402

T0 = 1720785462000


def hip_runtime():
    """The HIP runtime this process already runs on (the copy torch loaded)."""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert paths, "no HIP runtime is mapped"
    rt = ctypes.CDLL(sorted(paths)[0])
    rt.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    rt.hipMemcpyAsync.restype = ctypes.c_int
    return rt


def lengths(shape, scale, dev):
    """-> (value lengths of the log's entries, number of fetches)"""
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    if shape == "small":
        n = int(10_000_000 * scale)
        return torch.full((n,), 100, dtype=torch.int64, device=dev), n
    if shape == "page":
        return torch.full((int(262_144 * scale),), 4096, dtype=torch.int64, device=dev), int(1_000_000 * scale)
    if shape == "huge":
        return torch.full((max(int(1024 * scale), 1),), 1 << 20, dtype=torch.int64, device=dev), max(int(4096 * scale), 1)
    n = int(32_768 * scale)
    u = torch.rand(n, device=dev, generator=g, dtype=torch.float64)
    return torch.exp2(4 + 14 * u).to(torch.int64), 2 * n  # 2^4 .. 2^18


def run(shape, args, dev, sp, rt):
    lens, Q = lengths(shape, args.scale, dev)
    N = lens.numel()
    voff = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    voff[1:] = torch.cumsum(lens, 0)
    vbytes = int(voff[-1])
    g = torch.Generator(device=dev)
    g.manual_seed(13)
    values = torch.randint(0, 256, (vbytes,), dtype=torch.uint8, device=dev, generator=g)
    j = torch.arange(N, device=dev, dtype=torch.int64)
    keys = be16(2 * j).reshape(-1)
    cr = T0 + j
    res = {"shape": shape, "entries": N, "fetches": Q, "log_value_bytes": vbytes, "steps": args.steps,
           "warmup": args.warmup}

    # the append
    ln = ctypes.c_uint64()
    head = (vp(keys), None, 16, N, vp(values), vp(voff), vp(cr), None, 0)
    call("vbf_vlog_encode_dev", *head, None, 0, ctypes.byref(ln), None, sp)
    log = torch.empty(ln.value, dtype=torch.uint8, device=dev)
    vo = torch.empty(N, dtype=torch.int32, device=dev)
    r = timed(lambda: call("vbf_vlog_encode_dev", *head, vp(log), ln.value, ctypes.byref(ln), vp(vo), sp),
              args.steps, args.warmup)
    r["entries_per_s"] = round(N / r["ms_per_step"] * 1e3)
    r["log_GB_per_s"] = round(ln.value / r["ms_per_step"] / 1e6, 1)
    res["log_bytes"] = ln.value
    res["encode"] = r

    # the table that points into it, and the log's handle
    dl, il, nb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    S = (ctypes.byref(dl), ctypes.byref(il), ctypes.byref(nb))
    a = (vp(keys), None, 16, N, vp(vo), vp(cr), None)
    call("vbf_sst_encode_dev", *a, None, 0, S[0], None, 0, S[1], None, 0, S[2], sp)
    data = torch.empty(dl.value, dtype=torch.uint8, device=dev)
    index = torch.empty(il.value, dtype=torch.uint8, device=dev)
    blocks = torch.empty(nb.value, dtype=torch.int32, device=dev)
    call("vbf_sst_encode_dev", *a, vp(data), dl.value, S[0], vp(index), il.value, S[1], vp(blocks), nb.value, S[2], sp)
    ht, hv = ctypes.c_void_p(), ctypes.c_void_p()
    call("vbf_table_open_dev", vp(data), dl.value, vp(index), il.value, vp(blocks), nb.value, sp, ctypes.byref(ht))
    call("vbf_vlog_open_dev", vp(log), ln.value, 0, ctypes.byref(hv))
    handles = (ctypes.c_void_p * 1)(ht.value)

    # the batch: Q entries drawn with repeats (every entry once, in a random order, when Q == N)
    pick = torch.randperm(N, device=dev, generator=g) if Q == N else torch.randint(0, N, (Q,), device=dev, generator=g)
    qk = be16(2 * pick).reshape(-1)
    found = torch.empty(Q, dtype=torch.uint8, device=dev)
    val = torch.empty(Q, dtype=torch.int32, device=dev)
    status = torch.empty(Q, dtype=torch.uint8, device=dev)
    out_off = torch.empty(Q + 1, dtype=torch.int64, device=dev)
    tot = ctypes.c_uint64()

    def get():
        call("vbf_table_get_dev", vp(qk), None, 16, Q, 1, handles, None, vp(found), None, vp(val), None, sp)

    get()
    call("vbf_vlog_get_dev", hv, vp(val), vp(found), Q, None, None, 0, None, None, 0, None, ctypes.byref(tot), sp)
    out = torch.empty(tot.value, dtype=torch.uint8, device=dev)
    res["value_bytes"] = tot.value

    def fetch():
        call("vbf_vlog_get_dev", hv, vp(val), vp(found), Q, None, None, 0, vp(status), vp(out), tot.value, vp(out_off),
             ctypes.byref(tot), sp)

    def both():
        get()
        fetch()

    for name, fn in (("table_get", get), ("fetch", fetch), ("get_then_fetch", both)):
        r = timed(fn, args.steps, args.warmup)
        r["per_s"] = round(Q / r["ms_per_step"] * 1e3)
        if name != "table_get":
            r["value_GB_per_s"] = round(tot.value / r["ms_per_step"] / 1e6, 1)
        res[name] = r
    torch.cuda.synchronize()
    assert bool((status == 1).all()) and int(out_off[-1]) == tot.value == int(lens[pick].sum())
    # the fetched bytes against the values: the items of about the first and the last 64 MiB of the output
    first = max(int(torch.searchsorted(out_off, 64 << 20, right=True)) - 1, 1)
    last = min(int(torch.searchsorted(out_off, max(tot.value - (64 << 20), 0))), Q - 1)
    for i0, i1 in ((0, first), (last, Q)):
        items = pick[i0:i1]
        delta = torch.repeat_interleave(voff[:-1][items] - out_off[i0:i1], lens[items])  # source - destination
        lo, hi = int(out_off[i0]), int(out_off[i1])
        at = torch.arange(lo, hi, device=dev)
        assert torch.equal(out[lo:hi], values[at + delta]), "fetched bytes differ from the values"

    scratch = torch.empty(tot.value, dtype=torch.uint8, device=dev)

    def memcpy():
        rc = rt.hipMemcpyAsync(scratch.data_ptr(), out.data_ptr(), tot.value, 3, sp)  # hipMemcpyDeviceToDevice
        assert rc == 0

    r = timed(memcpy, args.steps, args.warmup)
    r["GB_per_s"] = round(tot.value / r["ms_per_step"] / 1e6, 1)
    res["memcpy_d2d"] = r
    res["fetch_over_memcpy"] = round(res["fetch"]["value_GB_per_s"] / r["GB_per_s"], 3)
    lib.vbf_table_free(ht)
    lib.vbf_vlog_free(hv)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="small,page,huge,mix")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="scales every entry and fetch count (a quick run)")
    args = ap.parse_args()
    assert torch.cuda.is_available() and vbf.device_count() > 0, "needs an MI355X: there is no CPU path"
    dev = torch.device("cuda:0")
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rt = hip_runtime()
    for shape in args.shapes.split(","):
        run(shape, args, dev, sp, rt)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
