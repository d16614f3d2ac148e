"""Memtable flush timing: the sort alone and the flush end to end, beside what the host and the
compaction merge do with the same batch.

  python tools/memtable_flush_bench.py [--sizes 65536,1048576,16777216] [--sets rand16,var,user16]
                                       [--steps 5] [--warmup 2] [--py-max-n 16777216]

One process, one JSON line per (key set, n).  Key sets, each with about 10 % of the puts repeating
an earlier key:
  rand16  16-byte keys of vbf_gen_fixed_dev (8 random bytes, then the counter): no prefix ties
  var     config 3's variable-length keys (8..128 B, mean ~26 B, vbf_gen_var_dev)
  user16  b"user%012d": every compare past the shared 8-byte prefix reads the key bytes
Per line:
  sort_dev      vbf_memtable_sort_dev on device-resident keys, device events around the call (it
                ends in its own stream synchronisation): entries/s, and the library's phases
                mem_sort (prefix pass + tile sort) and mem_merge (merge levels + keep + select)
  flush_host    vbf_flush_write_host from host arrays to host files, host clock (the call is
                synchronous): upload, sort, gather, encode, download
  py_sorted     the host's way for arbitrary keys: a dict for "last put wins", then sorted() on bytes
  np_lexsort    16-byte sets only: numpy's stable lexsort over the keys viewed as two big-endian
                u64 columns, then the last of every run of equal keys
  merge_host    the nearest route without this feature: the batch cut into 2048-entry runs that
                the HOST sorts and deduplicates (prep_s, Python), then vbf_compact_merge_host over
                those runs with created_ms = the put's index, so the newest put wins (call_s)
The device sort's ids are compared with py_sorted's once per line.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import velarixdb_amd as vbf  # noqa: E402
from velarixdb_amd import workloads as wl  # noqa: E402
from velarixdb_amd._lib import call  # noqa: E402

from sst_write_bench import timed, vp  # noqa: E402

RUN = 2048


def key_set(name, n, dev, sp):
    """-> (device keys, device offsets or None, stride): n puts, ~10 % repeating an earlier put's key"""
    g = torch.Generator(device=dev)
    g.manual_seed(0x3E37)
    src = torch.arange(n, device=dev)
    dup = torch.rand(n, device=dev, generator=g) < 0.1
    earlier = (torch.rand(n, device=dev, generator=g, dtype=torch.float64) * src).to(torch.int64)
    src = torch.where(dup, earlier, src)  # put j carries the key of put src[j] <= j
    if name == "var":
        off_h = wl.var_offsets(wl.SEED_CFG3, 0, n)
        soff = torch.from_numpy(off_h.view(np.int64)).to(dev)
        base = torch.empty(int(off_h[-1]), dtype=torch.uint8, device=dev)
        call("vbf_gen_var_dev", wl.SEED_CFG3, 0, n, vp(soff), vp(base), sp)
        lens = (soff[1:] - soff[:-1])[src]
        off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(lens, 0)
        at = torch.repeat_interleave(soff[:-1][src] - off[:-1], lens) + torch.arange(int(off[-1]), device=dev)
        return base[at], off, 0
    if name == "rand16":
        base = torch.empty(n * 16, dtype=torch.uint8, device=dev)
        call("vbf_gen_fixed_dev", wl.SEED_CFG2, 0, n, 16, vp(base), sp)
        return base.view(n, 16)[src].reshape(-1).contiguous(), None, 16
    assert name == "user16", name
    ids = torch.randint(0, 10 ** 12, (n,), device=dev, generator=g)[src]
    digits = (ids[:, None] // (10 ** torch.arange(11, -1, -1, device=dev))[None, :]) % 10 + 48
    rows = torch.cat([torch.tensor(list(b"user"), device=dev).expand(n, 4), digits], 1).to(torch.uint8)
    return rows.reshape(-1).contiguous(), None, 16


def host_clock(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"s_per_call": round(sum(ts) / len(ts), 6), "s_min": round(min(ts), 6), "s_max": round(max(ts), 6)}


def py_last_sorted(keys):
    last = {}
    for j, k in enumerate(keys):
        last[k] = j
    return [last[k] for k in sorted(last)]


def run(name, n, args, dev, sp):
    keys_d, off_d, stride = key_set(name, n, dev, sp)
    torch.cuda.synchronize()
    keys_h = keys_d.cpu().numpy()
    off_h = None if off_d is None else off_d.cpu().numpy().view(np.uint64)
    kb = keys_h.size
    res = {"set": name, "n": n, "key_bytes": kb, "steps": args.steps, "warmup": args.warmup}

    # the sort alone, device-resident
    ids_d = torch.empty(n, dtype=torch.int32, device=dev)
    c = ctypes.c_uint64()

    def sort_dev():
        call("vbf_memtable_sort_dev", vp(keys_d), vp(off_d), stride, n, vp(ids_d), ctypes.byref(c), sp)

    r = timed(sort_dev, args.steps, args.warmup)
    r["entries_per_s"] = round(n / r["ms_per_step"] * 1e3)
    res["distinct"] = c.value
    res["sort_dev"] = r
    ids = ids_d.cpu().numpy().view(np.uint32)[:c.value]

    # the flush end to end, host to host
    val = np.arange(n, dtype=np.uint32)
    cr = np.arange(1, n + 1, dtype=np.int64)
    tb = np.zeros(n, np.uint8)
    data, index = np.empty(kb + 17 * n, np.uint8), np.empty(kb + 8 * n, np.uint8)
    out_ids = np.empty(n, np.uint32)
    dl, il, no = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    op = None if off_h is None else off_h.ctypes.data

    def flush():
        call("vbf_flush_write_host", keys_h.ctypes.data, op, stride, n, val.ctypes.data, cr.ctypes.data, tb.ctypes.data,
             None, data.ctypes.data, data.size, ctypes.byref(dl), index.ctypes.data, index.size, ctypes.byref(il),
             out_ids.ctypes.data, ctypes.byref(no), 0)

    r = host_clock(flush, args.steps, args.warmup)
    r["entries_per_s"] = round(n / r["s_per_call"])
    r["data_bytes"], r["index_bytes"] = dl.value, il.value
    res["flush_host"] = r
    assert no.value == c.value and np.array_equal(out_ids[:no.value], ids)

    # host baselines
    if stride:
        def lexsort():
            cols = keys_h.view(">u8").reshape(n, 2)
            order = np.lexsort((cols[:, 1], cols[:, 0]))  # stable: equal keys stay in arrival order
            s = cols[order]
            lastof = np.ones(n, bool)
            lastof[:-1] = (s[1:] != s[:-1]).any(1)
            return order[lastof]

        r = host_clock(lexsort, max(1, min(args.steps, 3)), 0)
        r["entries_per_s"] = round(n / r["s_per_call"])
        res["np_lexsort"] = r
        assert np.array_equal(lexsort().astype(np.uint32), ids)
    if n <= args.py_max_n:
        raw = keys_h.tobytes()
        bounds = off_h.tolist() if off_h is not None else list(range(0, kb + 1, stride))
        t0 = time.perf_counter()
        pk = [raw[bounds[j]:bounds[j + 1]] for j in range(n)]
        res["py_make_bytes_s"] = round(time.perf_counter() - t0, 4)
        t0 = time.perf_counter()
        want = py_last_sorted(pk)
        dt = time.perf_counter() - t0
        res["py_sorted"] = {"s_per_call": round(dt, 4), "entries_per_s": round(n / dt)}
        assert np.array_equal(np.asarray(want, np.uint32), ids), "device sort differs from the host's"

        # the compaction merge fed host-sorted runs: arena = the runs' surviving puts
        t0 = time.perf_counter()
        pick = []
        for lo in range(0, n, RUN):
            pick.append([lo + j for j in py_last_sorted(pk[lo:lo + RUN])])
        prep = time.perf_counter() - t0
        run_off = np.concatenate([[0], np.cumsum([len(p) for p in pick])]).astype(np.uint64)
        pick = np.concatenate(pick).astype(np.int64)
        lens = np.asarray([bounds[j + 1] - bounds[j] for j in pick.tolist()], np.uint64)
        aoff = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        akeys = np.frombuffer(b"".join(pk[j] for j in pick.tolist()), np.uint8)
        acr, atb = (pick + 1).astype(np.int64), np.zeros(pick.size, np.uint8)
        mids = np.empty(pick.size, np.uint32)
        mn, mu = ctypes.c_uint64(), ctypes.c_uint64()

        def merge():
            call("vbf_compact_merge_host", akeys.ctypes.data, aoff.ctypes.data, acr.ctypes.data, atb.ctypes.data,
                 run_off.ctypes.data, run_off.size - 1, None, None, None, 0, 0, 0, 0, 0, mids.ctypes.data,
                 ctypes.byref(mn), None, None, ctypes.byref(mu), 0)

        r = host_clock(merge, max(1, min(args.steps, 3)), 1)
        r["prep_s"] = round(prep, 4)
        r["entries_per_s_call"] = round(n / r["s_per_call"])
        r["entries_per_s_with_prep"] = round(n / (r["s_per_call"] + prep))
        res["merge_host"] = r
        assert np.array_equal(pick[mids[:mn.value].astype(np.int64)].astype(np.uint32), ids)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,1048576,16777216")
    ap.add_argument("--sets", default="rand16,var,user16")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--py-max-n", type=int, default=1 << 24, help="largest n the Python baselines run at")
    args = ap.parse_args()
    assert torch.cuda.is_available() and vbf.device_count() > 0, "needs an MI355X: there is no CPU path"
    dev = torch.device("cuda:0")
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for n in (int(x) for x in args.sizes.split(",")):
        for name in args.sets.split(","):
            run(name, n, args, dev, sp)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
