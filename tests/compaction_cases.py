"""Buckets for the compaction merge (sized.rs:170-320) on the three axes the random buckets of
test_gpu_compaction.py leave alone: run geometry (empty, uneven and tile-edge tables), times (real
epoch milliseconds, the i64 limits, u64 TTLs) and the shape of the tombstone map.

Generators only, seeded and deterministic.  Every case is a function without arguments that returns
(runs, start_map, use_ttl, entry_ttl, tomb_ttl, now): runs as _arena of test_gpu_compaction.py takes
them, [(keys, created i64, tombstones u8)] per table, and start_map a dict key -> time.  CASES maps
a case's name to its function; GEOMETRY, TIMES and MAPS list the names by family.

test_compaction_cases.py checks on the CPU that every case does something (keeps entries, drops
entries, changes the map) and pins the oracle on the time and map cases with an independent
model; test_gpu_compaction_shapes.py runs them on the device.

The time cases reach `created + ttl` sums past 2^64 and negative `created` values.  The oracle and
the kernel both compute has_expired (mem.rs:149-153) in wrapping u64 there, and these cases compare
the two with each other: they claim nothing about what the Rust reference does at such times."""
import numpy as np

T0 = 1720785462000  # a real created_at (ms since the epoch), above bit 40
I64_MIN, I64_MAX = -2**63, 2**63 - 1
U64_MAX = 2**64 - 1
TILE = 2048  # the merge tile (kTile, csrc/vbf_compact.hip)


def _key(i):
    return b"%08d" % i


def _tables(rng, universe, sizes, tomb_p, times):
    """One table per size: that many keys of `universe` (sorted), times(rng, n) -> created."""
    runs = []
    for n in sizes:
        pick = np.sort(rng.choice(len(universe), size=n, replace=False))
        runs.append(([universe[i] for i in pick], np.asarray(times(rng, n), np.int64),
                     (rng.random(n) < tomb_p).astype(np.uint8)))
    return runs


def _epoch(rng, n):
    return T0 + rng.integers(0, 30, size=n)  # many ties, real magnitude


def _epoch_map(rng, universe, n):
    return {universe[i]: T0 + int(rng.integers(-5, 35)) for i in rng.choice(len(universe), size=n, replace=False)}


# ---- run geometry -------------------------------------------------------------------------------

GEOMETRY_SIZES = [
    (0, 5, 0, 7, 0),
    (0, 0, 0),                    # no entries at all: n_out = 0 and no error
    (0, 0, 300),
    (300, 0, 0),
    (TILE - 1, TILE + 1),         # the pair is exactly two tiles
    (TILE, TILE, 1),
    (2 * TILE, 0, 2 * TILE + 1),
    (6000, 1, 1, 1, 3),
    (1,) * 33,                    # six levels, an odd segment count at five of them
    (255, 257, 256, TILE, 1, 0, TILE - 1),
]


def _geometry(seed, sizes):
    def case():
        rng = np.random.default_rng(seed)
        uni = [_key(i) for i in range(8000)]
        runs = _tables(rng, uni, sizes, 0.25, _epoch)
        return runs, _epoch_map(rng, uni, 1000), True, 20, 25, T0 + 40
    return case


def _every_key_in_every_table():
    """9 tables x the same 600 keys: every fold group has 9 entries, so groups straddle every
    8-output lane range, every tile edge and every 256-lane block of k_fold."""
    rng = np.random.default_rng(7100)
    uni = [_key(i) for i in range(600)]
    runs = _tables(rng, uni, (600,) * 9, 0.25, _epoch)
    return runs, _epoch_map(rng, uni, 75), True, 20, 25, T0 + 40


def _empty_key_tables():
    """Five tables that each hold only the empty key: no key bytes at all (keys may be NULL).
    By hand: table 1's tombstone is recorded, the newer values of tables 2..4 replace it and the
    last one stays (created + 20 >= now)."""
    cr = [T0 + 21, T0 + 22, T0 + 23, T0 + 23, T0 + 25]
    tb = [0, 1, 0, 0, 0]
    runs = [([b""], np.asarray([c], np.int64), np.asarray([t], np.uint8)) for c, t in zip(cr, tb)]
    return runs, {}, True, 20, 25, T0 + 40


# ---- times --------------------------------------------------------------------------------------

TIME_VALUES = [I64_MIN, I64_MIN + 1, -1, 0, 1, T0, T0 + 1, T0 + 2**32, T0 - 2**32, I64_MAX - 1, I64_MAX]
TIME_SETTINGS = [  # (now, entry_ttl, tomb_ttl)
    (T0 + 40, 20, 25),
    (0, 0, 0),
    (U64_MAX, U64_MAX, 1),
    (T0, 2**63, 2**63 + 5),
    (2**63 + 7, 5, U64_MAX - 2),
]


def _times(seed, now, entry_ttl, tomb_ttl):
    def case():
        rng = np.random.default_rng(seed)
        uni = [_key(i) for i in range(400)]
        vals = np.asarray(TIME_VALUES, np.int64)
        runs = _tables(rng, uni, (300,) * 5, 0.4, lambda r, n: vals[r.integers(0, vals.size, size=n)])
        start = {uni[i]: int(vals[rng.integers(0, vals.size)]) for i in rng.choice(len(uni), size=100, replace=False)}
        return runs, start, True, entry_ttl, tomb_ttl, now
    return case


def _high_word_times():
    """Times T0 + k * 2^32: the low 32 bits are all equal, only the high word orders them."""
    rng = np.random.default_rng(7300)
    uni = [_key(i) for i in range(400)]
    runs = _tables(rng, uni, (300,) * 5, 0.4, lambda r, n: T0 + r.integers(0, 6, size=n) * 2**32)
    start = {uni[i]: T0 + int(rng.integers(-1, 7)) * 2**32 for i in rng.choice(len(uni), size=100, replace=False)}
    return runs, start, True, 2 * 2**32, 3 * 2**32, T0 + 6 * 2**32


# ---- the tombstone map, on one medium bucket ----------------------------------------------------

def _map_bucket():
    rng = np.random.default_rng(7400)
    uni = [_key(1000 + i) for i in range(1500)]
    return rng, uni, _tables(rng, uni, (500, 700, 300, 600), 0.25, _epoch)


def _in_bucket(runs):
    return sorted({k for ks, _, _ in runs for k in ks})


def _map_one_key():
    rng, uni, runs = _map_bucket()
    held = _in_bucket(runs)
    return runs, {held[len(held) // 2]: T0 + 10}, True, 20, 25, T0 + 40


def _map_all_below():
    rng, uni, runs = _map_bucket()
    start = {b"00000%03d" % i: T0 + int(rng.integers(-5, 35)) for i in range(200)}  # < b"00001000"
    return runs, start, True, 20, 25, T0 + 40


def _map_all_above():
    rng, uni, runs = _map_bucket()
    start = {b"9%07d" % i: T0 + int(rng.integers(-5, 35)) for i in range(200)}
    return runs, start, True, 20, 25, T0 + 40


def _map_every_key():
    rng, uni, runs = _map_bucket()
    return runs, {k: T0 + int(rng.integers(-5, 35)) for k in _in_bucket(runs)}, True, 20, 25, T0 + 40


def newest_created(runs):
    """key -> the largest created of its entries"""
    out = {}
    for ks, cr, _ in runs:
        for k, c in zip(ks, cr.tolist()):
            out[k] = max(out.get(k, c), c)
    return out


def _map_time_equals_created():
    """For 300 keys the map's time is exactly the `created` of the key's newest entry: tombstone_check
    keeps an entry only when created > time, so every entry of these keys is dropped."""
    rng, uni, runs = _map_bucket()
    newest = newest_created(runs)
    held = sorted(newest)
    start = {held[i]: newest[held[i]] for i in rng.choice(len(held), size=300, replace=False)}
    for i in rng.choice(len(held), size=200, replace=False):
        start.setdefault(held[i], T0 + int(rng.integers(-5, 35)))
    return runs, start, True, 20, 25, T0 + 40


def _name(sizes):
    return "sizes_" + ("1x%d" % len(sizes) if len(sizes) > 8 else "_".join(str(n) for n in sizes))


CASES = {_name(s): _geometry(7000 + i, s) for i, s in enumerate(GEOMETRY_SIZES)}
CASES["every_key_in_every_table"] = _every_key_in_every_table
CASES["empty_key_tables"] = _empty_key_tables
GEOMETRY = list(CASES)
TIMES = []
for _i, (_now, _e, _t) in enumerate(TIME_SETTINGS):
    CASES["times_%d" % _i] = _times(7200 + _i, _now, _e, _t)
    TIMES.append("times_%d" % _i)
CASES["times_high_word"] = _high_word_times
TIMES.append("times_high_word")
MAPS = ["map_one_key", "map_all_below", "map_all_above", "map_every_key", "map_time_equals_created"]
CASES.update(zip(MAPS, (_map_one_key, _map_all_below, _map_all_above, _map_every_key, _map_time_equals_created)))

NO_ENTRIES = _name((0, 0, 0))  # the one degenerate case: nothing to keep, drop or record
# the cases carried through to files (merge_bucket_sst)
TO_FILES = [_name((TILE - 1, TILE + 1)), _name((2 * TILE, 0, 2 * TILE + 1)), "every_key_in_every_table",
            "times_0", "times_1"]
