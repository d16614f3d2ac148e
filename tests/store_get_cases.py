"""Worlds for the get tests: a log window, a gc table, an active memtable, read-only memtables and
one SST, holding every row of a hand-written truth table of DataStore::get's precedence rules plus
filler keys.  tests/test_store_get_ref.py pins the checker (tests/store_get_ref.py) on the table;
the GPU tests compare the library with the checker over the same worlds.  Generators only.
"""
import functools

import numpy as np

import key_torture as kt
import store_get_ref as sg
import vlog_ref as vr

BASE = 1000                 # the log window's first file position
T = 1_720_785_462_309       # a real clock (ms)
NEG = 2**63 + 977           # a created_at that is negative as an i64
STEM = b"user0000-0000000/"  # 17 bytes: every row's compare goes past the 8-byte prefix
GC, ACTIVE, RO, NONE, TABLE = sg.LAYER_GC, sg.LAYER_ACTIVE, sg.LAYER_RO, sg.LAYER_NONE, sg.LAYER_TABLE
SST_INDEX = 2               # the worlds' own table comes after the two fixture SSTs

# name: (gc, active, {r: read-only r}, sst, (found, layer, status)) -- an entry is (log, created_at, tombstone)
# with log = "live" / "tomb" (its own log entry, live or a tombstone), "none" (an offset past the end),
# "bad_lo" (before the window) or "bad_hi" (its header crosses the end).  One row per sentence of the rules.
ROWS = {
    # the gc layer decides with a live entry and a live value in the log, whatever lies below
    "gc_live": (("live", T + 5, 0), ("live", T + 9, 0), {0: ("live", T + 9, 0)}, ("live", T + 1, 0), (1, GC, vr.VALUE)),
    # a tombstone gc entry returns Ok(None): the active memtable answers
    "gc_tomb_entry": (("live", T + 5, 1), ("live", T + 1, 0), {}, None, (1, ACTIVE, vr.VALUE)),
    # log status NONE: falls through
    "gc_log_none": (("none", T + 5, 0), ("live", T + 1, 0), {}, None, (1, ACTIVE, vr.VALUE)),
    # log status TOMBSTONE: falls through, here to a read-only table
    "gc_log_tomb": (("tomb", T + 5, 0), None, {1: ("live", T + 2, 0)}, None, (1, RO + 1, vr.VALUE)),
    # a BAD offset keeps the gc hit; the fetch reports BAD
    "gc_log_bad_lo": (("bad_lo", T + 5, 0), ("live", T + 9, 0), {}, None, (1, GC, vr.BAD)),
    "gc_log_bad_hi": (("bad_hi", T + 5, 0), None, {}, None, (1, GC, vr.BAD)),
    # a tombstone gc entry and nothing below: not found
    "gc_tomb_only": (("live", T + 5, 1), None, {}, None, (0, NONE, vr.SKIPPED)),
    # a fall-through can reach the SSTs
    "gc_none_to_sst": (("none", T + 5, 0), None, {}, ("live", T + 1, 0), (1, TABLE | SST_INDEX, vr.VALUE)),
    # the active memtable decides whatever its time: no fall-through
    "active_live": (None, ("live", T + 1, 0), {0: ("live", T + 50, 0)}, ("live", T + 60, 0), (1, ACTIVE, vr.VALUE)),
    "active_tomb_hides": (None, ("live", T + 1, 1), {0: ("live", T + 50, 0)}, ("live", T + 60, 0), (2, ACTIVE, vr.SKIPPED)),
    "active_time_zero": (None, ("live", 0, 0), {0: ("live", T + 50, 0)}, None, (1, ACTIVE, vr.VALUE)),
    "active_time_neg": (None, ("live", NEG, 1), {}, ("live", T + 1, 0), (2, ACTIVE, vr.SKIPPED)),
    # found with a live entry whose offset lies past the end of the log: the fetch reports NONE
    "active_log_none": (None, ("none", T + 1, 0), {}, None, (1, ACTIVE, vr.NONE)),
    # read-only: the strictly newest wins, in whichever table it lies
    "ro_newest": (None, None, {0: ("live", T + 1, 0), 1: ("live", T + 3, 0), 2: ("live", T + 2, 0)}, ("live", T + 99, 0),
                  (1, RO + 1, vr.VALUE)),
    # a tie: the earlier table
    "ro_tie": (None, None, {0: ("live", T + 7, 0), 2: ("live", T + 7, 1)}, None, (1, RO + 0, vr.VALUE)),
    "ro_tomb_newest": (None, None, {0: ("live", T + 1, 0), 1: ("live", T + 2, 1)}, ("live", T + 99, 0), (2, RO + 1, vr.SKIPPED)),
    # a live entry whose log entry is a tombstone: found, the fetch reports TOMBSTONE
    "ro_log_tomb": (None, None, {0: ("tomb", T + 1, 0)}, None, (1, RO + 0, vr.TOMBSTONE)),
    # an entry at time <= 0 never wins, and the SSTs get their turn
    "ro_time_zero_sst": (None, None, {0: ("live", 0, 0)}, ("live", T + 1, 0), (1, TABLE | SST_INDEX, vr.VALUE)),
    "ro_time_neg_sst": (None, None, {1: ("live", NEG, 0)}, ("live", T + 1, 1), (2, TABLE | SST_INDEX, vr.SKIPPED)),
    "ro_time_neg_only": (None, None, {0: ("live", 2**64 - 1, 0)}, None, (0, NONE, vr.SKIPPED)),
    "ro_neg_then_pos": (None, None, {0: ("live", 2**64 - 1, 0), 1: ("live", 5, 0)}, None, (1, RO + 1, vr.VALUE)),
    # past 2^63 as u64 is negative: the older positive entry wins
    "ro_pos_then_neg": (None, None, {0: ("live", 5, 0), 2: ("live", NEG, 0)}, None, (1, RO + 0, vr.VALUE)),
    "sst_only": (None, None, {}, ("live", T + 1, 0), (1, TABLE | SST_INDEX, vr.VALUE)),
    "sst_tomb": (None, None, {}, ("live", T + 1, 1), (2, TABLE | SST_INDEX, vr.SKIPPED)),
    "nowhere": (None, None, {}, None, (0, NONE, vr.SKIPPED)),
}
ROW_KEYS = {name: STEM + name.encode() for name in ROWS}
ROW_KEYS["ro_newest"] = b""          # the zero-length key is an ordinary key
ROW_KEYS["active_live"] = b"k\0\0"   # between "k\0" and "k\0\0\0" of the ordering universe


@functools.lru_cache(maxsize=1)
def _pool():
    """Filler keys, none a row key: the ordering universe (families past 8 equal bytes, pairs that
    differ by trailing zeros), the torture keys up to 300 bytes, numbered keys behind one stem."""
    rows = set(ROW_KEYS.values())
    keys = list(kt.ordered_universe()) + [k for k in kt.torture_keys(3) if len(k) <= 300]
    keys += [b"user0000-0000000#%06d" % i + b"\0" * (i % 3) for i in range(12000)]
    seen, out = set(rows), []
    for k in keys:
        if k not in seen:
            seen.add(k)
            out.append(k)
    return out


class World:
    """layers: puts (keys, val_offsets, created u64, tombs) for "gc", "active" and ("ro", r); the
    checker's Store over the same puts; the SST's items; queries."""


@functools.lru_cache(maxsize=None)
def world(gc_size, active_size, ro_sizes, seed=0x6E7):
    """A world whose layers hold about the given numbers of distinct keys (0 = the layer is absent;
    a present layer holds its truth-table rows beside the filler).  Rows naming a read-only table
    beyond len(ro_sizes) lose that entry."""
    rng = np.random.default_rng([seed, gc_size, active_size, *ro_sizes])
    pool = _pool()
    nro = len(ro_sizes)
    names = ["gc", "active"] + [("ro", r) for r in range(nro)] + ["sst"]
    sizes = dict(zip(names, (gc_size, active_size, *ro_sizes, 600)))
    want = {n: [] for n in names}     # (key, log kind, created, tomb)
    for row, (g, a, ros, sst, _) in ROWS.items():
        k = ROW_KEYS[row]
        for n, e in [("gc", g), ("active", a), ("sst", sst)] + [(("ro", r), e) for r, e in ros.items()]:
            if e is not None and sizes.get(n, 0) > 0:
                want[n].append((k, *e))
    for n in names:                    # a layer smaller than its rows holds the first of them
        want[n] = want[n][:sizes[n]]
    for n in names:                    # filler: random keys of the pool, real and odd times, one in six deleted
        extra = max(0, sizes[n] - len(want[n]))
        for i in rng.choice(len(pool), min(extra, len(pool)), replace=False):
            t = int(rng.choice([T + int(rng.integers(1, 1000)), 0, NEG, 1])) if rng.integers(0, 8) == 0 else T + int(rng.integers(1, 1000))
            want[n].append((pool[int(i)], "live" if rng.integers(0, 10) else "tomb", t, int(rng.integers(0, 6) == 0)))
    # the log: one entry per (layer, key) that names "live" or "tomb"
    entries, at = [], {}
    for n in names:
        for k, kind, t, tomb in want[n]:
            if kind in ("live", "tomb"):
                at[(n, k)] = len(entries)
                entries.append((k, b"" if len(entries) % 7 == 3 else b"v:%s:" % repr(n).encode() + k[:20], t, kind == "tomb"))
    log, offs = vr.encode(entries, BASE)
    end = BASE + len(log)
    where = {"none": end + 7, "bad_lo": BASE - 1, "bad_hi": end - 5}
    w = World()
    w.log, w.base, w.nro = log, BASE, nro
    w.layers = {}
    for n in names:
        items = [(k, offs[at[(n, k)]] if (n, k) in at else where[kind], t, tomb) for k, kind, t, tomb in want[n]]
        if n == "sst":
            w.sst_items = sorted((k, vo, t if t else 1, tomb) for k, vo, t, tomb in items)
            continue
        order = rng.permutation(len(items))
        puts = [items[int(i)] for i in order]
        if len(puts) > 4:              # a few earlier puts of keys that are put again: the last put wins
            puts = [(k, vo ^ 1, (t + 1) & (2**64 - 1), 1 - tomb) for k, vo, t, tomb in puts[-3:]] + puts
        w.layers[n] = ([p[0] for p in puts], np.array([p[1] for p in puts], np.uint32),
                       np.array([p[2] for p in puts], np.uint64), np.array([p[3] for p in puts], np.uint8))
    present = sorted({k for n in names for k, *_ in want[n]})
    pick = [present[int(i)] for i in rng.choice(len(present), min(len(present), 2500), replace=False)]
    around = []
    for k in pick:                     # absent keys around every present one
        around += [k + b"\0", k[:-1], k[:-1] + bytes([(k[-1] + 1) & 0xFF]) if k else b"\x01", k + b"\xff"]
    q = list(ROW_KEYS.values()) + pick + around + [b"", b""] + pick[:200]
    w.queries = [q[int(i)] for i in rng.permutation(len(q))]
    return w


def mem(w, n):
    """The checker's dict for layer n, None when the world has no such layer."""
    if n not in w.layers or not w.layers[n][0]:
        return None
    return sg.memtable(*w.layers[n])


def store(w, tables=()):
    return sg.Store(w.log, w.base, mem(w, "gc"), mem(w, "active"), [mem(w, ("ro", r)) or {} for r in range(w.nro)], tables)
