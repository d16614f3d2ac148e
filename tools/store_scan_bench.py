"""store.scan_many beside the two routes a caller had before it.

  python tools/store_scan_bench.py [--entries 262144] [--cands 10,1000,100000] [--ranges 4096,256,8]
                                   [--repeats 3] [--warmup 1] [--stem]

One process, one JSON line per shape.  The store: an active memtable and two read-only ones of
--entries distinct 16-byte keys each, one SST of --entries keys below them, a log of 32-byte values.
The keys of the four layers interleave in key order and every eighth key has an older copy in the
next layer down, so a range of C candidates holds about C / 4 entries of every layer and C / 9
duplicates; the clocks grow from the SST up to the active memtable.  A shape is --ranges[i] ranges of
about --cands[i] candidates each, at random places.  Keys are 8 random bytes and a counter; with --stem
they share their first 8 bytes, so every prefix compare ties and reads key bytes.

Routes, on the same data:
  new      store.scan_many over the three MemTable handles, the table and the log
           (vbf_store_scan_host).  "new" is the call as a caller makes it: when the
           answer outgrows the first guess ("two_calls") the device pass runs twice.  "new_exact" is
           one call with capacities = the answer's sizes: the pass alone.
  flushed  (a) the route that existed before: MemTable.flush() of every memtable, Table.open of the
           files, table.scan_values over [active, read-only 0, read-only 1, SST].  The time includes the
           flushes and the opens, which a caller pays once per memtable state; "flushed_scan" is the
           scan alone over tables already open.  A cost comparison only: that route answers with the
           tables' fold, which agrees with the get's precedence here because the clocks grow with the
           layers (the outputs are compared first).
  get      (b) store.get_many over exactly the listed keys, packed beforehand: the floor for a caller
           that already knew the keys.
--warmup untimed and --repeats timed rounds alternate, a host clock around each synchronous Python
call.  Reported: median ms, listed entries/s and ranges/s from the median, the ratios flushed / new
and new / get, and the bytes each route moves between host and device per call, computed from the
shape and the answer's sizes.
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
from velarixdb_amd import MemTable, Table, ValueLog, memtable, store, table  # noqa: E402
from velarixdb_amd.keys import HostBatch, pack_offsets  # noqa: E402

T0 = 1720785462000
KLEN, VLEN, LOG_ENTRIES = 16, 32, 65536


def batch(rows):
    rows = np.ascontiguousarray(rows, np.uint8)
    return HostBatch(rows.reshape(-1), None, KLEN, rows.shape[0], 1)


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=262144)
    ap.add_argument("--cands", default="10,1000,100000")
    ap.add_argument("--ranges", default="4096,256,8")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--stem", action="store_true")
    a = ap.parse_args()
    ints = lambda s: [int(x) for x in s.split(",")]
    rng = np.random.default_rng(0x5CA9)
    E = a.entries
    N = 4 * E
    # the universe, ascending: 8 random bytes (sorted; or the stem) and a running big-endian counter
    uni = np.empty((N, KLEN), np.uint8)
    head = np.sort(rng.integers(0, 2**63, N, dtype=np.uint64))
    uni[:, :8] = np.frombuffer(b"user0000", np.uint8) if a.stem else head.astype(">u8").view(np.uint8).reshape(N, 8)
    uni[:, 8:] = np.arange(N, dtype=np.uint64).astype(">u8").view(np.uint8).reshape(N, 8)
    lk = uni[rng.integers(0, N, LOG_ENTRIES)]
    vals = rng.integers(0, 256, (LOG_ENTRIES, VLEN), dtype=np.uint8)
    log, lvo = ValueLog.encode(batch(lk), [v.tobytes() for v in vals], created_ms=np.full(LOG_ENTRIES, T0, np.int64))
    vlog = ValueLog.open(log)
    # layer L (0 active, 1 and 2 read-only, 3 the SST) holds the keys j with j % 4 == L, and an older copy
    # of every eighth key of the layer above
    own = [np.arange(L, N, 4) for L in range(4)]
    ids = [own[0]] + [np.sort(np.concatenate([own[L], own[L - 1][::8]])) for L in (1, 2, 3)]
    puts = [(batch(uni[i]), lvo[rng.integers(0, LOG_ENTRIES, i.size)], np.full(i.size, T0 + 3000 - 1000 * L, np.int64))
            for L, i in enumerate(ids)]
    sst = memtable.flush(*puts[3])
    tab = Table.open(sst.data, sst.index)
    mems = [MemTable.open(*p) for p in puts[:3]]
    total_cands = sum(i.size for i in ids)

    def prepare():
        files = [m.flush() for m in mems]
        return files, [Table.open(f.data, f.index) for f in files]
    files, flushed = prepare()
    # a flush brings the two files and the export of the entries down; the open sends the files up again
    prep_bytes = sum(2 * (f.data.size + f.index.size) for f in files) + sum(m.key_bytes + 21 * m.entries + 8 for m in mems)
    for C, R in zip(ints(a.cands), ints(a.ranges)):
        span = max(1, round(C * N / total_cands))  # universe keys per range
        starts = rng.integers(0, N - span, R)
        ranges = [(uni[s].tobytes(), uni[s + span - 1].tobytes()) for s in starts.tolist()]
        new = lambda: store.scan_many(ranges, [tab], vlog, active=mems[0], read_only=mems[1:])
        old_scan = lambda ts: table.scan_values(ranges, ts + [tab], vlog)

        def old():
            _, ts = prepare()
            r = old_scan(ts)
            for t in ts:
                t.close()
            return r
        r, (g, v) = new(), old_scan(flushed)
        assert np.array_equal(r.range_off, g.range_off) and np.array_equal(r.keys, g.keys)
        assert np.array_equal(r.val_offsets, g.val_offsets) and np.array_equal(r.values.values, v.values)
        listed = pack_offsets(r.keys, r.key_off)
        get = lambda: store.get_many(listed, [tab], vlog, active=mems[0], read_only=mems[1:])
        k = get()
        assert (k.found == 1).all() and np.array_equal(k.layer, r.layer) and np.array_equal(k.values.values, r.values.values)
        n, kb, vb = int(r.layer.size), int(r.keys.size), int(r.values.values.size)
        exact = lambda: store.scan_many(ranges, [tab], vlog, active=mems[0], read_only=mems[1:], capacities=(n, kb, vb))
        assert np.array_equal(exact().values.values, r.values.values)
        tn, to, ts_, tg, te = [], [], [], [], []
        for i in range(a.warmup + a.repeats):  # the routes alternate
            for acc, fn in ((tn, new), (to, old), (ts_, lambda: old_scan(flushed)), (tg, get), (te, exact)):
                t = time.perf_counter()
                fn()
                if i >= a.warmup:
                    acc.append((time.perf_counter() - t) * 1e3)
        med = statistics.median
        bb = sum(len(lo) + len(hi) for lo, hi in ranges) + 8 * (2 * R + 1)
        out = {"entries": E, "stem": a.stem, "ranges": R, "cands_per_range": round(span * total_cands / N, 1),
               "listed": n, "key_bytes": kb, "value_bytes": vb, "two_calls": bool(n > max(256, store.ENTRY_GUESS * R)),
               "new": stats(tn), "flushed": stats(to), "flushed_scan": stats(ts_), "get": stats(tg),
               "new_exact": stats(te), "exact_over_get": round(med(te) / med(tg), 2),
               "flushed_over_exact": round(med(to) / med(te), 2),
               "new_entries_per_s": round(n / med(tn) * 1e3), "new_ranges_per_s": round(R / med(tn) * 1e3),
               "flushed_entries_per_s": round(n / med(to) * 1e3), "get_entries_per_s": round(n / med(tg) * 1e3),
               "flushed_over_new": round(med(to) / med(tn), 2), "flushed_scan_over_new": round(med(ts_) / med(tn), 2),
               "new_over_get": round(med(tn) / med(tg), 2),
               # new: the bounds up (twice when the first guess was too small); per listed entry key_off 8 + tombstone 1
               # + layer 4 + table 4 + val_offset 4 + created 8 + status 1 + value_off 8, the keys and the values down
               "new_bytes": {"up": bb * (2 if n > max(256, store.ENTRY_GUESS * R) else 1), "down": 8 * (R + 1) + 38 * n + 16 + kb + vb},
               # flushed: the flushes and opens; the bounds up twice (size query, filling call), key_off 8 + table 4 +
               # val_offset 4 + created 8 + tombstone 1 and the keys down; val_offsets 4 + found 1 up twice, status 1 +
               # value_off 8 and the values down
               "flushed_bytes": {"prepare": prep_bytes, "up": 2 * bb + 2 * 5 * n, "down": 8 * (R + 1) + 25 * n + 8 + kb + 9 * n + 8 + vb},
               # get: the keys and their offsets up; found 1 + layer 4 + table 4 + val_offset 4 + created 8 + status 1 +
               # value_off 8 and the values down
               "get_bytes": {"up": kb + 8 * (n + 1), "down": 30 * n + 8 + vb}}
        print(json.dumps(out), flush=True)
    for t in mems + flushed + [tab]:
        t.close()
    vlog.close()


if __name__ == "__main__":
    assert vbf.device_count() > 0
    main()
