"""gc.collect_device beside gc.collect: one run of the GC's handler over a chunk of the value log, as
one fused device pass (vbf_gc_collect_host) and as the chain of four host calls it replaces.

  python tools/gc_collect_bench.py [--chunks 1,64,512] [--values 100,4096] [--repeats 5] [--warmup 1]

One process, one JSON line per shape.  A shape is a chunk of --chunks MiB of a log whose entries have
16-byte keys and values of --values bytes; half of the chunk's entries are overwritten by a later put
that lies behind the chunk (so the window is 1.5 chunks long); the keys are spread over 4 tables, read
with and without their filters.  Both routes get the same handles and the same arguments.  Per shape:
the two results are first compared byte for byte; then the routes alternate, --warmup untimed rounds
and --repeats timed ones, a host clock around each call (both are synchronous: they return with the
device drained).  Reported: the median, the fastest and the slowest call of each route in ms, and
host_over_device = median(collect) / median(collect_device), above 1 where the fused route is faster.
Also the bytes each route moves between host and device, computed from the shape (handles excluded:
the log window and the tables are on the device before either route starts).

What the numbers hold.  The times are whole Python calls, so they include the Python side of both
routes (both build the list of the puts' keys; collect also slices every value it re-appends).
collect_device makes two calls of vbf_gc_collect_host, a size query and the filling call, and each
runs the walk, the lookup, the judge and the scan: the device work before the emit is done twice, and
that is inside its time.  The byte counts are the arrays that cross the bus; the size query moves
only its scalars, so the fused route's bytes are those of one pass although its device work is two.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import velarixdb_amd as vbf  # noqa: E402
from velarixdb_amd import BloomFilter, Table, ValueLog, gc, memtable  # noqa: E402
from velarixdb_amd.keys import pack_fixed  # noqa: E402

T0 = 1720785462000
KLEN, NTABLES = 16, 4


def make_log(n, vlen):
    """n chunk entries and n // 2 later puts of every second key -> (log bytes, entry size, keys [n, 16])"""
    entry = np.dtype([("kl", "<u4"), ("vl", "<u4"), ("cr", "<u8"), ("tb", "u1"), ("key", "u1", KLEN), ("val", "u1", vlen)])
    assert entry.itemsize == 17 + KLEN + vlen and vlen >= 8
    rng = np.random.default_rng(0x6C0)
    pattern = rng.integers(0, 256, vlen, dtype=np.uint8)
    m = n + n // 2
    log = np.zeros(m, entry)
    log["kl"], log["vl"] = KLEN, vlen
    ids = np.concatenate([np.arange(n), np.arange(1, n, 2)[:n // 2]]).astype(np.uint64)
    log["cr"] = T0 + np.arange(m, dtype=np.uint64)
    keys = np.empty((m, KLEN), np.uint8)
    keys[:, :8] = np.frombuffer(b"userkey-", np.uint8)
    keys[:, 8:] = ids.astype(">u8").view(np.uint8).reshape(m, 8)  # big-endian: key order is id order
    log["key"] = keys
    log["val"] = pattern
    log["val"][:, :8] = np.arange(m, dtype="<u8").view(np.uint8).reshape(m, 8)  # no two values alike
    return log.tobytes(), entry.itemsize, keys[:n]


def make_tables(n, esize, keys):
    """Key i lives in table i % 4 and points at its most recent entry -> ([Table], [BloomFilter])"""
    i = np.arange(n, dtype=np.int64)
    recent = np.where(i % 2 == 1, n + (i - 1) // 2, i)  # odd keys were put again behind the chunk
    tables, filters = [], []
    for t in range(NTABLES):
        sel = i[t::NTABLES]
        f = BloomFilter(0.01, max(sel.size, 1))
        res = memtable.flush(pack_fixed(keys[sel]), (recent[sel] * esize).astype(np.uint32), T0 + recent[sel],
                             np.zeros(sel.size, np.uint8), filter=f)
        tables.append(Table.open(res.data, res.index))
        filters.append(f)
    return tables, filters


def traffic(n, vlen, n_puts, append_len):
    """Host<->device bytes of the two routes for n chunk entries (every one found live in a table).
    collect_device's size query runs the device pass a second time but moves no array: see the docstring."""
    kb, vb = n * KLEN, n * vlen
    walk = 8 * (n + 1) * 3 + kb + vb + 8 * n + n                             # down: every array of the walk
    get = (kb + 8 * (n + 1)) + (n + 4 * n + 4 * n + 8 * n)                   # up keys, down the answers
    fetch = (4 * n + n) + (n + 8 * (n + 1) + vb)                             # up offsets, down the most recent values
    pk, pv = 4 + (n_puts - 1) * KLEN, 8 + (n_puts - 1) * vlen                # the puts' keys and values
    assert append_len == 17 * n_puts + pk + pv
    enc = (pk + 8 * (n_puts + 1) * 2 + pv + 8 * n_puts) + (append_len + 4 * n_puts)
    return {"collect": walk + get + fetch + enc, "collect_device": n + append_len + 9 * n_puts}


def same(a, b):
    assert (a is None) == (b is None)
    if a is None:
        return
    assert a.append == b.append and a.put_keys == b.put_keys and (a.total_bytes_read, a.new_tail) == (b.total_bytes_read, b.new_tail)
    for name in ("invalid", "put_val_offsets", "put_created_ms", "put_tombstones"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


def run(chunk_mib, vlen, args):
    esize = 17 + KLEN + vlen
    n = max((chunk_mib << 20) // esize, 2)
    log, esize, keys = make_log(n, vlen)
    tables, filters = make_tables(n, esize, keys)
    chunk, log_size, now = n * esize, len(log), T0 + 10**9
    with ValueLog.open(log) as vl:
        del log
        for use_filters in (False, True):
            fl = filters if use_filters else None
            routes = {"collect": lambda: gc.collect(vl, tables, 0, chunk, log_size, now, filters=fl),
                      "collect_device": lambda: gc.collect_device(vl, tables, 0, chunk, log_size, now, filters=fl)}
            a, b = routes["collect"](), routes["collect_device"]()
            same(b, a)  # byte-identical at the timed size, before any clock runs
            assert a is not None and a.invalid.size == n // 2 and a.total_bytes_read == chunk
            times = {name: [] for name in routes}
            for r in range(args.warmup + args.repeats):
                for name, fn in routes.items():
                    t = time.perf_counter()
                    fn()
                    dt = (time.perf_counter() - t) * 1e3
                    if r >= args.warmup:
                        times[name].append(dt)
            res = {"chunk_mib": chunk_mib, "value_bytes": vlen, "entries": n, "invalid": int(a.invalid.size),
                   "append_bytes": len(a.append), "tables": NTABLES, "filters": use_filters, "repeats": args.repeats,
                   "warmup": args.warmup, "host_device_bytes": traffic(n, vlen, len(a.put_keys), len(a.append))}
            for name, ts in times.items():
                res[name] = {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3),
                             "max_ms": round(max(ts), 3)}
            res["host_over_device"] = round(res["collect"]["median_ms"] / res["collect_device"]["median_ms"], 3)
            print(json.dumps(res), flush=True)
            del a, b
    for t in tables:
        t.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", default="1,64,512", help="chunk sizes in MiB")
    ap.add_argument("--values", default="100,4096", help="value sizes in bytes")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    assert vbf.device_count() > 0, "needs an MI355X: there is no CPU path"
    for chunk_mib in (int(x) for x in args.chunks.split(",")):
        for vlen in (int(x) for x in args.values.split(",")):
            run(chunk_mib, vlen, args)


if __name__ == "__main__":
    main()
