"""Range scan timing (vbf_table_scan_dev), beside tools/table_get_bench.py and with its conventions:
a clock settle, W untimed warm-up steps, then K steps timed with device events around each call
(a call synchronises its stream three times; that wait is inside the time).

  python tools/table_scan_bench.py [--tables 8] [--entries 1000000] [--ranges 10000] [--span 100] [--steps 10] [--warmup 2]

One process, everything device-resident, one JSON line:
  T tables of N sorted 16-byte keys as in table_get_bench (table t holds the even values
  2 (j T + t): disjoint tables, every 97th entry a tombstone), encoded with vbf_sst_encode_dev and
  opened with vbf_table_open_dev;
  (a) one range over everything, filled call (sizes known), entries/s; beside it the route the
      library offered before for the same question: vbf_sst_decode_dev of every table into one arena,
      then vbf_compact_merge_dev (ids only -- no gather of keys and fields, which the scan includes);
  (b) R ranges of about S entries each at random places, ranges/s and entries/s, the size query and
      the filled call timed apart;
  (c) for orientation, vbf_table_get_dev over as many present keys as (b) lists: the only route to
      those entries before, and only for a caller who already knows the keys.
The answers of (a) and (b) are checked against the construction.
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
from table_get_bench import DevTable, be16  # noqa: E402


class Scan:
    """One batch of ranges on the device with outputs sized by a first call."""

    def __init__(self, lo, hi, handles, T, flags, dev, sp):
        self.nr = lo.numel()
        self.bounds = torch.stack([be16(lo), be16(hi)], dim=1).reshape(-1).contiguous()  # lo_0 hi_0 lo_1 ...
        self.boff = torch.arange(2 * self.nr + 1, device=dev, dtype=torch.int64) * 16
        self.head = (vp(self.bounds), vp(self.boff), self.nr, T, handles, flags)
        self.n, self.kb, self.sp = ctypes.c_uint64(), ctypes.c_uint64(), sp
        self.size()
        n, kb = self.n.value, self.kb.value
        self.range_off = torch.empty(self.nr + 1, dtype=torch.int64, device=dev)
        self.keys = torch.empty(max(kb, 1), dtype=torch.uint8, device=dev)
        self.key_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        self.table = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        self.val = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        self.cr = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        self.tomb = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)

    def size(self):
        call("vbf_table_scan_dev", *self.head, None, None, 0, None, None, None, None, None, 0, ctypes.byref(self.n),
             ctypes.byref(self.kb), self.sp)

    def fill(self):
        call("vbf_table_scan_dev", *self.head, vp(self.range_off), vp(self.keys), self.keys.numel(), vp(self.key_off),
             vp(self.table), vp(self.val), vp(self.cr), vp(self.tomb), self.table.numel(), ctypes.byref(self.n),
             ctypes.byref(self.kb), self.sp)


def rate(r, items, name):
    r[name] = round(items / r["ms_per_step"] * 1e3)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, default=8)
    ap.add_argument("--entries", type=int, default=1_000_000)
    ap.add_argument("--ranges", type=int, default=10_000)
    ap.add_argument("--span", type=int, default=100)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available() and vbf.device_count() > 0, "needs an MI355X: there is no CPU path"
    dev = torch.device("cuda:0")
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    T, N, R, S = args.tables, args.entries, args.ranges, args.span
    tabs = [DevTable(t, T, N, dev, sp) for t in range(T)]
    for tb in tabs:
        tb.h = tb.open()
    handles = (ctypes.c_void_p * T)(*[tb.h.value for tb in tabs])
    res = {"workload": "%d tables x %d x 16B keys; %d ranges of ~%d entries" % (T, N, R, S), "steps": args.steps,
           "warmup": args.warmup}
    live = lambda v: ((v // 2) // T) % 97 != 0  # entry j = (v / 2) / T of its table; every 97th is a tombstone

    # (a) everything in one range
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    full = Scan(zero, zero - 1, handles, T, 0, dev, sp)  # hi = ff..ff
    assert full.n.value == T * N - T * ((N + 96) // 97) and full.kb.value == 16 * full.n.value
    res["full_range"] = rate(timed(full.fill, args.steps, args.warmup), full.n.value, "entries_per_s")
    res["full_range"]["entries"] = full.n.value
    res["full_range_size_query"] = timed(full.size, args.steps, args.warmup)
    torch.cuda.synchronize()
    v = torch.arange(T * N, device=dev, dtype=torch.int64) * 2
    v = v[live(v)]
    assert torch.equal(full.keys.view(-1, 16), be16(v)) and torch.equal(full.table.long(), (v // 2) % T)
    assert torch.equal(full.cr, 1720785462000 + v // 2) and not bool(full.tomb.any())
    assert full.range_off.tolist() == [0, full.n.value]
    del full, v

    # the same question before this entry point: decode every table into one arena, compaction merge
    E = T * N
    a_keys = torch.empty(E * 16, dtype=torch.uint8, device=dev)
    a_off = torch.arange(E + 1, device=dev, dtype=torch.int64) * 16
    a_cr = torch.empty(E, dtype=torch.int64, device=dev)
    a_tb = torch.empty(E, dtype=torch.uint8, device=dev)
    ids = torch.empty(E, dtype=torch.int32, device=dev)
    run_off = (ctypes.c_uint64 * (T + 1))(*[t * N for t in range(T + 1)])
    n1, n2 = ctypes.c_uint64(), ctypes.c_uint64()

    def decode_merge():
        for t, tb in enumerate(tabs):
            call("vbf_sst_decode_dev", vp(tb.data), tb.data.numel(), vp(tb.blocks), tb.blocks.numel(),
                 ctypes.c_void_p(a_keys.data_ptr() + t * N * 16), N * 16, None, None,
                 ctypes.c_void_p(a_cr.data_ptr() + t * N * 8), ctypes.c_void_p(a_tb.data_ptr() + t * N), N,
                 ctypes.byref(n1), sp)
        call("vbf_compact_merge_dev", vp(a_keys), vp(a_off), vp(a_cr), vp(a_tb), run_off, T, None, None, None, 0, 0,
             0, 0, 0, vp(ids), ctypes.byref(n1), None, None, ctypes.byref(n2), sp)

    res["decode_then_compaction_merge"] = rate(timed(decode_merge, args.steps, args.warmup), E, "entries_per_s")
    res["decode_then_compaction_merge"]["merged_entries"] = n1.value
    del a_keys, a_off, a_cr, a_tb, ids

    # (b) R ranges of about S entries: S consecutive even values from a random even start
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    lo = torch.randint(0, T * N - S, (R,), device=dev, generator=g) * 2
    many = Scan(lo, lo + 2 * S - 1, handles, T, 0, dev, sp)
    r = timed(many.fill, args.steps, args.warmup)
    rate(r, many.n.value, "entries_per_s")
    rate(r, R, "ranges_per_s")
    r["entries"] = many.n.value
    res["many_ranges"] = r
    res["many_ranges_size_query"] = timed(many.size, args.steps, args.warmup)
    torch.cuda.synchronize()
    v = (lo.view(-1, 1) + 2 * torch.arange(S, device=dev)).reshape(-1)
    keep = live(v)
    assert torch.equal(many.keys.view(-1, 16), be16(v[keep])) and torch.equal(many.table.long(), (v[keep] // 2) % T)
    want_off = torch.cat([zero, keep.view(R, S).sum(1).cumsum(0)])
    assert torch.equal(many.range_off, want_off) and many.n.value == int(keep.sum())

    # (c) point lookups of as many present keys
    Q = many.n.value
    qk = many.keys.clone()
    found = torch.empty(Q, dtype=torch.uint8, device=dev)
    idx = torch.empty(Q, dtype=torch.int32, device=dev)
    val = torch.empty(Q, dtype=torch.int32, device=dev)
    cr = torch.empty(Q, dtype=torch.int64, device=dev)

    def get():
        call("vbf_table_get_dev", vp(qk), None, 16, Q, T, handles, None, vp(found), vp(idx), vp(val), vp(cr), sp)

    res["get_same_keys"] = rate(timed(get, args.steps, args.warmup), Q, "gets_per_s")
    torch.cuda.synchronize()
    assert bool((found == 1).all()) and torch.equal(idx, many.table) and torch.equal(val, many.val)
    assert torch.equal(cr, many.cr)
    for tb in tabs:
        lib.vbf_table_free(tb.h)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
