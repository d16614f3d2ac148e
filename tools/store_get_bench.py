"""store.get_many beside the route that answers the same question without memtable handles.

  python tools/store_get_bench.py [--entries 512,65536,4194304] [--batches 1024,65536,1048576,16777216]
                                  [--hits 0,50,100] [--repeats 3] [--warmup 1] [--stem] [--value-guess 48]

One process, one JSON line per shape.  A shape: an active memtable and two read-only ones of --entries
distinct 16-byte keys each, one SST of 65 536 entries below them, a log of 32-byte values; a batch of
--batches keys of which --hits per cent lie in the memtables (a third in each) and the rest half in
the SST and half nowhere.  Keys are 16 random bytes (distinct 8-byte prefixes); with --stem they share
their first 8 bytes, so every prefix compare of the lookup ties and reads key bytes.

Routes, on the same data:
  new      store.get_many over the three MemTable handles, the table and the log (vbf_store_get_host),
           with the default kernel and with VBF_MEMGET=0 (the plain kernel)
  flushed  what the library offered before the handles: memtable.flush of each memtable's puts, Table.open
           of the results, table.get_values over [active, read-only 0, read-only 1, SST].  Its answer is
           the same here because the clocks grow from the SST up to the active memtable (the fold by
           time then agrees with the precedence by layer).  Timed twice: the lookup alone with the
           tables already open ("flushed_get"), and the three flushes + opens that a caller pays once
           per memtable state ("flushed_prepare"); the new route's counterpart, MemTable.open of the
           three batches of puts, is "open".
Per shape the two routes' found / val_offsets / values are compared first; then --warmup untimed and
--repeats timed rounds alternate, a host clock around each synchronous Python call.  Reported: median
(fastest - slowest) ms, gets/s from the median, and the bytes each route moves between host and
device per call, computed from the shape (the handles are on the device before either route starts).
mem_get_ms is the library's own phase time of the lookup kernel alone (vbf_profile_*), default and
plain, from one extra profiled call each.
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
from velarixdb_amd._lib import call, profile_read  # noqa: E402
from velarixdb_amd.keys import HostBatch  # noqa: E402

T0 = 1720785462000
KLEN, VLEN, SST_ENTRIES, LOG_ENTRIES = 16, 32, 65536, 65536


def batch(rows):
    rows = np.ascontiguousarray(rows, np.uint8)
    return HostBatch(rows.reshape(-1), None, KLEN, rows.shape[0], 1)


_COUNT = [0]


def make_keys(rng, n, stem):
    """n distinct keys: 8 random bytes (or the stem) and a running big-endian counter."""
    k = np.empty((n, KLEN), np.uint8)
    k[:, :8] = np.frombuffer(b"user0000", np.uint8) if stem else rng.integers(0, 256, (n, 8), dtype=np.uint8)
    k[:, 8:] = (np.arange(n, dtype=np.uint64) + np.uint64(_COUNT[0])).astype(">u8").view(np.uint8).reshape(n, 8)
    _COUNT[0] += n
    return k


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return ts


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def with_knob(value, fn):
    os.environ["VBF_MEMGET"] = value
    try:
        return fn()
    finally:
        del os.environ["VBF_MEMGET"]


def phase_ms(fn):
    call("vbf_profile_enable", 1)
    profile_read()
    fn()
    ms = profile_read()["mem_get"][0]
    call("vbf_profile_enable", 0)
    return round(ms, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", default="512,65536,4194304")
    ap.add_argument("--batches", default="1024,65536,1048576,16777216")
    ap.add_argument("--hits", default="0,50,100")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--stem", action="store_true")
    ap.add_argument("--value-guess", type=int, default=store.VALUE_GUESS,
                    help="store.VALUE_GUESS: the value bytes per key store.get_many makes room for in its first call")
    a = ap.parse_args()
    store.VALUE_GUESS = a.value_guess
    ints = lambda s: [int(x) for x in s.split(",")]
    rng = np.random.default_rng(0x57067)
    # the log: LOG_ENTRIES live entries the memtables' and the table's entries point into
    lk = make_keys(rng, LOG_ENTRIES, a.stem)
    vals = rng.integers(0, 256, (LOG_ENTRIES, VLEN), dtype=np.uint8)
    log, lvo = ValueLog.encode(batch(lk), [v.tobytes() for v in vals], created_ms=np.full(LOG_ENTRIES, T0, np.int64))
    vlog = ValueLog.open(log)
    for E in ints(a.entries):
        universe = make_keys(rng, 3 * E + 2 * SST_ENTRIES, a.stem)
        layers = [universe[i * E:(i + 1) * E] for i in range(3)]          # active, read-only 0, read-only 1
        sst_keys, absent = universe[3 * E:3 * E + SST_ENTRIES], universe[3 * E + SST_ENTRIES:]
        vo = lambda n: lvo[rng.integers(0, LOG_ENTRIES, n)]
        puts = [(batch(k), vo(E), np.full(E, T0 + 3000 - 1000 * i, np.int64)) for i, k in enumerate(layers)]
        sst = memtable.flush(batch(sst_keys), vo(SST_ENTRIES), np.full(SST_ENTRIES, T0, np.int64))
        tab = Table.open(sst.data, sst.index)
        t_open = timed(lambda: [m.close() for m in [MemTable.open(*p) for p in puts]], 0, 1)
        mems = [MemTable.open(*p) for p in puts]

        def prepare():
            return [Table.open(f.data, f.index) for f in (memtable.flush(*p) for p in puts)]
        t_prep = timed(lambda: [t.close() for t in prepare()], 0, 1)
        flushed = prepare()
        prep_files = sum(f.data.size + f.index.size for f in (memtable.flush(*p) for p in puts))
        for B in ints(a.batches):
            for hit in ints(a.hits):
                nh = B * hit // 100
                parts = [layers[i][rng.integers(0, E, nh // 3 + (i < nh % 3))] for i in range(3)]
                rest = B - nh
                parts += [sst_keys[rng.integers(0, SST_ENTRIES, rest // 2)], absent[rng.integers(0, SST_ENTRIES, rest - rest // 2)]]
                q = np.concatenate(parts)
                q = batch(q[rng.permutation(B)])
                new = lambda: store.get_many(q, [tab], vlog, active=mems[0], read_only=mems[1:])
                old = lambda: table.get_values(q, flushed + [tab], vlog)
                r, (g, v) = new(), old()
                p = with_knob("0", new)
                assert np.array_equal(r.found, g.found) and np.array_equal(r.val_offsets, g.val_offsets)
                assert np.array_equal(r.values.values, v.values) and np.array_equal(r.values.status, v.status)
                assert np.array_equal(p.layer, r.layer) and np.array_equal(p.values.values, r.values.values)
                assert int((r.layer <= 3).sum()) == nh
                tn, tp, to = [], [], []
                for i in range(a.warmup + a.repeats):  # the routes alternate
                    for ts, fn in ((tn, new), (tp, lambda: with_knob("0", new)), (to, old)):
                        t = time.perf_counter()
                        fn()
                        if i >= a.warmup:
                            ts.append((time.perf_counter() - t) * 1e3)
                vb = int(r.values.values.size)
                out = {"entries": E, "batch": B, "hit_pct": hit, "stem": a.stem, "value_guess": a.value_guess, "value_bytes": vb,
                       "new": stats(tn), "new_plain": stats(tp), "flushed_get": stats(to),
                       "new_gets_per_s": round(B / statistics.median(tn) * 1e3), "plain_gets_per_s": round(B / statistics.median(tp) * 1e3),
                       "flushed_gets_per_s": round(B / statistics.median(to) * 1e3),
                       "flushed_over_new": round(statistics.median(to) / statistics.median(tn), 2),
                       "plain_over_default": round(statistics.median(tp) / statistics.median(tn), 2),
                       "mem_get_ms": {"default": phase_ms(new), "plain": phase_ms(lambda: with_knob("0", new))},
                       "open_ms": round(t_open[0], 2), "flushed_prepare_ms": round(t_prep[0], 2),
                       # new: keys up; found 1 + layer 4 + table 4 + val_offset 4 + created 8 + status 1 + value_off 8, values down
                       "new_bytes": {"up": B * KLEN, "down": B * 30 + 8 + vb},
                       # flushed: keys up, found 1 + table 4 + val_offset 4 + created 8 down; then val_offsets 4 + found 1 up
                       # twice (size query, filling call), status 1 + value_off 8 and the values down
                       "flushed_bytes": {"up": B * KLEN + 2 * B * 5, "down": B * 17 + B * 9 + 8 + vb},
                       # per memtable state: the puts up and the two files down, the files up again; against the puts up
                       "flushed_prepare_bytes": 3 * E * (KLEN + 12) + 2 * prep_files, "open_bytes": 3 * E * (KLEN + 12)}
                print(json.dumps(out), flush=True)
        for t in mems + flushed + [tab]:
            t.close()
    vlog.close()


if __name__ == "__main__":
    assert vbf.device_count() > 0
    main()
