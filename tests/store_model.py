"""A dictionary model of the whole store, and the same store as files composed from the checkers.

ModelStore holds two things side by side:

  the dictionary   key -> (value, created_at ms as u64, tombstone), last put wins: what a user of the
                   store expects to read back
  the files        the value log (vlog_ref.encode), one table per flush (memtable_ref.sort_ids, then
                   the oracle's Table::write_to_file) with its memtable filter
                   (memtable_ref.insert_model), read with sst_get_ref.search + vlog_ref.get, scanned
                   with sst_scan_ref.scan_many, merged with the oracle's fold (oracle.compact_merge
                   with an oracle.TombstoneMap), walked with vlog_walk_ref.walk and collected with
                   vlog_walk_ref.gc_handler

Nothing here restates an operation a second time: every step is one of the existing checkers, fed
the bytes the previous checker produced.  tests/test_store_model.py holds the two halves against
each other on the CPU; tests/test_gpu_store_lifecycle.py drives the library through the same
histories and compares it with the files step by step.

The scenario generator lives here too, so both tests run the same histories (see SCENARIOS).  The
product never imports this module.
"""
import functools
import struct
from dataclasses import dataclass

import numpy as np

import memtable_ref as mref
import sst_get_ref as gref
import sst_scan_ref as sref
import vlog_ref as vr
import vlog_walk_ref as wr

T0 = 1_720_785_462_309             # a real clock (ms)
P = 1e-4                           # every filter's false positive rate (consts/mod.rs:17)
ENTRY_TTL_MS = 365 * 86400000      # consts/mod.rs:63
TOMBSTONE_TTL_MS = 120 * 86400000  # consts/mod.rs:67
COMPACT_NOW = T0 + 10**7           # the compactions' clock: later than no tombstone's created + ttl
GC_NOW = T0 + 10**8                # the GC's clock: after every put below 2^63
STEM = b"user0000-0000000"         # 16 bytes: every compare goes past the 8-byte prefix
LONGEST = STEM + b"L" * (4079 - len(STEM))  # the longest key the encoder takes
FULL = (b"", b"\xff" * 40)         # every generated key lies inside
KEEP_TOMBSTONES, END_EXCLUSIVE = sref.KEEP_TOMBSTONES, sref.END_EXCLUSIVE
HIGH_CLOCK = 2**63 + 977           # a created_at that is negative as an i64
SEAM_KEY = STEM + b"seam"          # put twice, see Scenario.seam_gen; no generation draws it


@dataclass(frozen=True)
class Scenario:
    name: str
    seed: int
    sizes: tuple            # puts per generation (one memtable each), cut at the 2048-entry tile's edges
    universe: int           # distinct keys, at most 4000
    base: int = 0           # the log window's first file position
    ties: bool = False      # whole runs of puts share a millisecond inside a batch
    big_values: bool = False  # a 70 000-byte value and six of 1.5 MiB: the log passes 8 MiB
    high_clock_gen: int = -1  # from this generation on created_at >= 2^63 (never inside the GC's chunk)
    seam_gen: int = -1      # the memtable fills mid-millisecond: this generation's last put and the next
                            # one's first are SEAM_KEY, same millisecond, same value -- the one tie that
                            # crosses tables; the two copies differ in their val_offset alone


# Generations 0-2 and 3-5 are the two buckets of the partial compaction; the GC's chunk ends inside
# generation 1; every scenario has a generation outside both buckets.
SCENARIOS = {s.name: s for s in (
    Scenario("plain", 0x51A1, (300, 300, 1, 300, 300, 1, 300), 1200),
    Scenario("tiles", 0x711E5, (2047, 2049, 4097, 6145, 2049, 2047, 300), 4000, ties=True),
    Scenario("big", 0xB16, (300, 2049, 300, 1, 300, 300, 300), 1000, base=12_345, big_values=True, high_clock_gen=6),
    Scenario("partial", 0x9A27, (2049, 300, 4097, 2047, 300, 2049, 300), 3000, seam_gen=3),
)}
LARGEST, SMALLEST = "tiles", "plain"


@dataclass
class Generation:
    keys: list            # bytes, in arrival order
    values: list          # bytes
    created: np.ndarray   # uint64
    tombs: np.ndarray     # uint8


@dataclass
class History:
    scenario: Scenario
    universe: list        # sorted
    absent: list          # 200 keys no generation puts
    gens: list
    ranges: list          # 50 (lo, hi) between universe keys, one empty range last


def _universe(rng, n):
    special = [b"", b"a", b"ab", b"abc", b"abcd", b"abcde", b"abcdef", b"abcdefg", LONGEST, STEM, STEM + b"\0",
               b"abc\0", STEM + b"pair", STEM + b"pair\0", STEM + b"pair\0\0", b"abcdefg\0"]
    if n < len(special) + 8:
        raise ValueError("universe too small")
    keys = set(special)
    i = 0
    while len(keys) < n:
        if i % 10 == 9:
            keys.add(rng.bytes(int(rng.integers(8, 25))))  # one key in ten without the stem
        else:
            keys.add(STEM + b"%06d" % i + b"x" * (i % 5))
        i += 1
    return special, sorted(keys)


def _absent(universe):
    have = set(universe)
    cand = [STEM[:-1], b"abcdefgh", LONGEST[:-1], b"\xff", b"\0", STEM + b"pai", b"b"]
    cand += [STEM + b"%06d" % i + b"!" for i in range(0, 4000, 20)]
    out = [k for k in cand if k not in have and k != wr.TAIL_ENTRY_KEY][:200]
    assert len(out) == 200
    return out


@functools.lru_cache(maxsize=None)
def history(name):
    """The scenario's puts, generation by generation, from its seed alone."""
    scn = SCENARIOS[name]
    rng = np.random.default_rng(scn.seed)
    special, universe = _universe(rng, scn.universe)
    regular = sorted(set(universe) - set(special))
    if scn.seam_gen >= 0:
        universe = sorted(universe + [SEAM_KEY])
    t = T0
    gens = []
    for g, n in enumerate(scn.sizes):
        if g == scn.high_clock_gen:
            t = HIGH_CLOCK
        keys = [regular[i] for i in rng.integers(0, len(regular), n)]
        if n > 1:  # one put in twenty goes to a special key: each occurs in every larger generation
            for j in np.flatnonzero(rng.integers(0, 20, n) == 0):
                keys[j] = special[int(rng.integers(0, len(special)))]
        kind = rng.integers(0, 100, n)
        values = [b"*" if c < 5 else b"" if c < 10 else rng.bytes(int(L)) for c, L in zip(kind, rng.integers(0, 201, n))]
        tombs = (rng.integers(0, 6, n) == 0).astype(np.uint8)
        values = [b"*" if d else v for v, d in zip(values, tombs)]  # a delete writes the marker
        if scn.big_values and g < 2 and n >= 300:
            sizes = ([70_000] if g == 0 else []) + [1536 * 1024] * 3
            for j, size in zip(rng.choice(n, len(sizes), replace=False), sizes):
                values[j], tombs[j] = rng.bytes(size), 0
        created = np.zeros(n, np.uint64)
        run = 0
        for j in range(n):
            if run == 0:
                t += int(rng.integers(1, 4))
                run = int(rng.integers(1, 41)) if scn.ties else 1
            created[j] = t
            run -= 1
        if g > 0 and g - 1 == scn.seam_gen:
            last = gens[-1]
            last.keys[-1] = keys[0] = SEAM_KEY
            last.values[-1] = values[0] = b"the same value on both sides of the seam"
            last.tombs[-1] = tombs[0] = 0
            created[:np.searchsorted(created, created[0], "right")] = last.created[-1]
        else:
            assert not gens or int(gens[-1].created[-1]) < int(created[0])
        t += 1000  # every batch has a millisecond range of its own: no tie crosses tables but the seam
        gens.append(Generation(keys, values, created, tombs))
    at = rng.integers(0, len(universe) - 1, 50)
    ranges = [(universe[a], universe[min(a + int(w), len(universe) - 1)]) for a, w in zip(at, rng.integers(0, 60, 50))]
    ranges.append((b"zz", b"aa"))  # lo > hi: empty
    return History(scn, universe, _absent(universe), gens, ranges)


class Batch:
    """Keys packed as the oracle reads them (data, absolute offsets, a length prefix in the hash)."""

    def __init__(self, keys):
        self.data = np.frombuffer(b"".join(keys), np.uint8).copy()
        self.offsets = np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.uint64)
        self.stride, self.n, self.len_prefix = 0, len(keys), 1


@dataclass
class ModelTable:
    data: bytes           # data.db
    index: bytes          # index.db
    sst: gref.Sst
    entries: int
    ids: np.ndarray       # the entries as indices into the flushed batch (None for a merged table)
    m: int                # the filter beside the table: bits, hash functions, words, no_of_elements
    k: int
    words: np.ndarray
    num_elements: int


def _table(ora, keys, val_offsets, created, tombs):
    """Table::write_to_file over sorted keys -> (data bytes, index bytes)."""
    b = Batch(keys)
    data, index = ora.sst_write(b.data if b.data.size else np.zeros(1, np.uint8), b.offsets,
                                np.asarray(val_offsets, np.uint32), np.asarray(created, np.uint64),
                                np.asarray(tombs, np.uint8))
    return data.tobytes(), index.tobytes()


class ModelStore:
    def __init__(self, ora, base=0):
        self.ora, self.base = ora, base
        self.dict = {}
        self.log = bytearray()
        self._bytes = None
        self.tables = []

    def clone(self):
        """A store that can go its own way: same files so far, own dictionary, log and table list."""
        c = ModelStore(self.ora, self.base)
        c.dict, c.log, c.tables = dict(self.dict), bytearray(self.log), list(self.tables)
        return c

    # ---- the log ----
    @property
    def log_size(self):
        return self.base + len(self.log)

    def log_bytes(self):
        if self._bytes is None or len(self._bytes) != len(self.log):
            self._bytes = bytes(self.log)
        return self._bytes

    # ---- writes ----
    def flush(self, keys, val_offsets, created, tombs):
        """Flusher::flush of the puts in arrival order, and the memtable's filter step over them,
        in a filter sized BloomFilter::new(P, number of puts) -> ModelTable (appended)."""
        ora = self.ora
        vo, cr, tb = np.asarray(val_offsets, np.uint32), np.asarray(created, np.uint64), np.asarray(tombs, np.uint8)
        ids = mref.sort_ids(keys)
        i64 = ids.astype(np.int64)
        data, index = _table(ora, [keys[i] for i in ids.tolist()], vo[i64], cr[i64], tb[i64])
        n = len(keys)
        m = ora.num_bits(n, P)
        k = ora.num_hash(m, n)
        f, _ = mref.insert_model(ora, Batch(keys), m, k)
        tab = ModelTable(data, index, gref.Sst(data, index), ids.size, ids, m, k, f.words(), f.num_elements)
        self.tables.append(tab)
        return tab

    def put_batch(self, keys, values, created, tombs):
        """DataStore::put for a batch that fills one memtable, then its flush
        -> (the bytes appended, every put's val_offset, ModelTable)."""
        entries = [(k, v, int(c), int(t)) for k, v, c, t in zip(keys, values, created, tombs)]
        blob, offs = vr.encode(entries, self.log_size)
        self.log += blob
        for k, v, c, t in entries:
            self.dict[k] = (v, c, 1 if t else 0)
        return blob, offs, self.flush(keys, offs, created, tombs)

    # ---- reads ----
    def ssts(self):
        return [t.sst for t in self.tables]

    def get(self, key):
        """-> (found, table, val_offset, created_ms, value or None): DataStore::get over the files."""
        found, who, vo, created = gref.search(key, self.ssts())
        value = None
        if found == 1:
            st, value = vr.get(self.log_bytes(), vo, self.base, key)
            assert st == vr.VALUE, "the table's entry of %r does not lead to its value (status %d)" % (key, st)
        return found, who, vo, created, value

    def scan(self, lo, hi, flags=0):
        """-> [(key, table, val_offset, created_ms, tombstone)] in key order."""
        return sref.scan(lo, hi, self.ssts(), flags)

    def scan_many(self, ranges, flags=0):
        return sref.scan_many(ranges, self.ssts(), flags)

    def expect(self, key):
        """What the dictionary says a get returns: the value, or None when absent or deleted."""
        hit = self.dict.get(key)
        return None if hit is None or hit[2] else hit[0]

    def expect_slice(self, lo, hi, flags=0):
        """The sorted dictionary slice a scan lists: [(key, value)] of the live keys inside the bounds."""
        return [(k, self.dict[k][0]) for k in sorted(self.dict)
                if lo <= k and (k < hi if flags & END_EXCLUSIVE else k <= hi) and not self.dict[k][2]]

    # ---- compaction ----
    def compact(self, table_indices, tmap, now=COMPACT_NOW):
        """merge_ssts_in_buckets for the bucket `table_indices` (in that order) with the runner's
        tombstone map `tmap` -> ModelTable with the filter BloomFilter::new(P, n) built over the
        merged keys.  The store is unchanged; see replace()."""
        ora = self.ora
        parts = [ora.sst_decode(np.frombuffer(self.tables[i].data, np.uint8)) for i in table_indices]
        keys = [p[0][int(p[1][j]):int(p[1][j + 1])].tobytes() for p in parts for j in range(p[1].size - 1)]
        b = Batch(keys)
        val = np.concatenate([p[2] for p in parts])
        created = np.concatenate([p[3] for p in parts]).view(np.int64)
        tomb = np.concatenate([p[4] for p in parts])
        run_off = np.concatenate([[0], np.cumsum([p[1].size - 1 for p in parts])]).astype(np.uint64)
        ids = ora.compact_merge(b.data, b.offsets, created, tomb, run_off, False, ENTRY_TTL_MS, TOMBSTONE_TTL_MS, now,
                                tmap).astype(np.int64)
        mk = [keys[i] for i in ids.tolist()]
        data, index = _table(ora, mk, val[ids], created[ids].view(np.uint64), tomb[ids])
        n = ids.size
        m = ora.num_bits(n, P)
        k = ora.num_hash(m, n)
        return ModelTable(data, index, gref.Sst(data, index), n, None, m, k, ora.build_words(Batch(mk), m, k), n)

    def replace(self, table_indices, merged):
        """The bucket's tables leave, the merged one takes the place of the first."""
        first = min(table_indices)
        self.tables = [merged if i == first else t for i, t in enumerate(self.tables)
                       if i == first or i not in table_indices]

    # ---- recovery ----
    def recover(self, head, cut=0):
        """recover_memtable's puts (recovery.rs:245-286): the log's entries from `head` on without
        the first (:261-264) -> [(offset, key, value, created as i64, tombstone)]; `cut` bytes are
        missing at the end of the file."""
        log = self.log_bytes()
        entries, _, stop = wr.walk(log[:len(log) - cut], head, base=self.base)
        assert stop == (wr.TORN if cut else wr.END)
        return entries[1:]

    # ---- GC ----
    def lookup(self, key):
        """GC::get: (most recent value, its creation time as the signed DateTime the reference
        compares), or None for NotFoundInDB."""
        found, _, vo, created = gref.search(key, self.ssts())
        if found != 1:
            return None
        st, v = vr.get(self.log_bytes(), int(vo), self.base)
        assert st not in (vr.BAD, vr.KEY_MISMATCH)
        return (v, created - 2**64 if created >= 2**63 else created) if st == vr.VALUE else None

    def gc(self, tail, chunk_bytes, now=GC_NOW):
        return wr.gc_handler(self.log_bytes(), self.base, tail, chunk_bytes, self.log_size, now, self.lookup)

    def apply_gc(self, res):
        """Appends the GC's entries to the log and flushes its puts into a new table; the dictionary
        gains the `tail` key, whose value is the new tail."""
        blob, offs = vr.encode(res["append"], self.log_size)
        assert offs == [p[1] for p in res["puts"]]
        self.log += blob
        k, v, c, _ = res["append"][0]
        assert k == wr.TAIL_ENTRY_KEY and v == struct.pack("<Q", res["new_tail"])
        self.dict[k] = (v, c, 0)
        return self.flush([p[0] for p in res["puts"]], offs, [p[2] for p in res["puts"]], [p[3] for p in res["puts"]])


def gc_chunk(offsets_by_gen, base):
    """(tail, chunk_bytes) for the lifecycle's GC run: from the start of the log to the middle of
    generation 1, so the chunk holds overwritten, deleted, "*", empty and valid entries."""
    offs = offsets_by_gen[1]
    return base, int(offs[len(offs) // 2]) - base


def build(ora, name, upto=None):
    """A ModelStore after the scenario's first `upto` generations (all by default)
    -> (store, [(blob, val_offsets, ModelTable)] per generation)."""
    h = history(name)
    store = ModelStore(ora, h.scenario.base)
    steps = [store.put_batch(g.keys, g.values, g.created, g.tombs) for g in h.gens[:upto]]
    return store, steps
