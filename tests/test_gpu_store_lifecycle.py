"""The whole store on the GPU against the dictionary model (tests/store_model.py): puts, flushes,
reads, scans, recovery, partial and full compaction and a GC run, several generations deep, through
the library's Python API.  Each step's inputs are the bytes the previous GPU step produced, never
the checker's; every comparison is exact equality.

`Life` is the GPU side alone: it knows the scenario's puts and nothing of the checkers, and records
every artefact it produces.  The tests compare what it returns with the store composed from the
checkers, and with the dictionary wherever tests/test_store_model.py kept that claim (its docstring
lists the claims dropped, and why).  One step leaves the Python API: the recovery also asks
vbf_vlog_walk_host for its val_offsets output, which no Python caller requests (Walk.val_offsets is
derived from entry_off), so that output is checked against a log whose base is not zero."""
import ctypes
import hashlib
import struct
import time

import numpy as np
import pytest

import sst_get_ref as gref
import sst_scan_ref as sref
import store_model as sm
from test_gpu_vlog_recover_gc import same_gc

pytestmark = pytest.mark.gpu
NAMES = list(sm.SCENARIOS)
BUCKETS = ((0, 1, 2), (3, 4, 5))  # the partial compaction's two rounds, as generations


def _bytes(x):
    if isinstance(x, np.ndarray):
        return x.dtype.str.encode() + np.ascontiguousarray(x).tobytes()
    if isinstance(x, (bytes, bytearray)):
        return bytes(x)
    return repr(x).encode()


class Life:
    """One scenario driven through the library, phase by phase; `art` collects (label, bytes) of
    every artefact in the order produced."""

    def __init__(self, vbf, name):
        self.vbf, self.h = vbf, sm.history(name)
        self.base = self.h.scenario.base
        self.keys = self.h.universe + self.h.absent
        self.ranges = [sm.FULL] + self.h.ranges
        self.ranges_excl = self.h.ranges[:8]
        self.art = []
        self.gens = None

    def rec(self, label, *parts):
        self.art += [(label, _bytes(p)) for p in parts]

    def digest(self):
        d = hashlib.sha256()
        for label, b in self.art:
            d.update(label.encode() + struct.pack("<Q", len(b)) + b)
        return d.hexdigest()

    def close(self):
        self.gens = None  # drops the device-resident filters

    # ---- puts ----
    def generations(self):
        """Every generation through put_many into a filter of its own -> [dict] per generation."""
        if self.gens is not None:
            return self.gens
        from velarixdb_amd import BloomFilter, ValueLog, memtable
        from velarixdb_amd.keys import pack
        out, size = [], self.base
        for g in self.h.gens:
            b, cr = pack(g.keys), g.created.view(np.int64)
            f = BloomFilter(sm.P, len(g.keys))
            log, res = memtable.put_many(b, g.values, cr, g.tombs, base=size, filter=f)
            again, vo = ValueLog.encode(b, g.values, created_ms=cr, tombstones=g.tombs, base=size)
            assert again == log  # put_many keeps the offsets to itself
            d = dict(log=log, vo=vo, res=res, filter=f, words=f.words().copy(), num_elements=f.num_elements(),
                     m=f.num_bits(), k=f.no_of_hash_func)
            self.rec("gen", log, vo, res.data, res.index, res.ids, res.smallest, res.biggest, d["words"], d["num_elements"])
            out.append(d)
            size += len(log)
        self.gens = out
        return out

    def log(self, upto=None):
        return b"".join(d["log"] for d in self.generations()[:upto])

    # ---- reads ----
    def read(self, label, files, log, filters=None, keys=None):
        """get_values over the tables opened from `files` (oldest first), with and without the
        filters, and newest first -> ((GetResult, Values), the same newest first)."""
        from velarixdb_amd import Table, ValueLog, get_values
        from velarixdb_amd.keys import pack
        b = pack(self.keys if keys is None else keys)
        tables = []
        try:
            tables = [Table.open(d, i) for d, i in files]
            with ValueLog.open(log, base=self.base) as vl:
                r, v = get_values(b, tables, vl, check_keys=True)
                if filters is not None:
                    rf, vf = get_values(b, tables, vl, filters=filters, check_keys=True)
                    for x, y in zip(_get_arrays(r, v), _get_arrays(rf, vf)):
                        assert np.array_equal(x, y), "the filters changed an answer"
                rr, vv = get_values(b, tables[::-1], vl, check_keys=True)
        finally:
            for t in tables:
                t.close()
        self.rec(label, *_get_arrays(r, v), rr.table, rr.val_offsets)
        return (r, v), (rr, vv)

    def scan(self, label, files, log):
        """scan_values: the full range, 50 ranges between universe keys and an empty one; eight of
        them end-exclusive; the full range with its tombstones -> [(flags, ranges, ScanResult, Values)]."""
        from velarixdb_amd import Table, ValueLog, scan_values
        tables, out = [], []
        try:
            tables = [Table.open(d, i) for d, i in files]
            with ValueLog.open(log, base=self.base) as vl:
                for flags, ranges in ((0, self.ranges), (sm.END_EXCLUSIVE, self.ranges_excl), (sm.KEEP_TOMBSTONES, [sm.FULL])):
                    s, v = scan_values(ranges, tables, vl, keep_tombstones=bool(flags & sm.KEEP_TOMBSTONES),
                                       end_exclusive=bool(flags & sm.END_EXCLUSIVE), check_keys=True)
                    self.rec(label, *_scan_arrays(s), v.status, v.values, v.value_off)
                    out.append((flags, ranges, s, v))
        finally:
            for t in tables:
                t.close()
        return out

    def files(self, upto=None):
        return [(d["res"].data, d["res"].index) for d in self.generations()[:upto]]

    def reads_after(self, g):
        gens = self.generations()
        files, log, filters = self.files(g + 1), self.log(g + 1), [d["filter"] for d in gens[:g + 1]]
        return self.read("read%d" % g, files, log, filters), self.scan("scan%d" % g, files, log)

    # ---- recovery ----
    def recovery(self):
        """recover_puts from the head after each generation, then a flush of what it returned, cut at
        the generation boundaries -> [(head, (keys, vo, cr, tb), [FlushResult per later generation],
        val_offsets as vbf_vlog_walk_host writes them)], and the same from a log cut 3 bytes short."""
        from velarixdb_amd import ValueLog, memtable
        from velarixdb_amd.keys import HostBatch
        gens = self.generations()
        sizes = [len(g.keys) for g in self.h.gens]
        log, out = self.log(), []
        with ValueLog.open(log, base=self.base) as vl:
            for g in range(len(gens)):
                head = int(gens[g]["vo"][-1])
                keys, vo, cr, tb = memtable.recover_puts(vl, head)
                flushed, at = [], 0
                if keys.n == sum(sizes[g + 1:]):
                    for n in sizes[g + 1:]:
                        cut = HostBatch(keys.data, keys.offsets[at:at + n + 1].copy(), 0, n, keys.len_prefix)
                        flushed.append(memtable.flush(cut, vo[at:at + n], cr[at:at + n], tb[at:at + n]))
                        at += n
                raw = _walk_val_offsets(vl, head)
                self.rec("recover%d" % g, keys.data[int(keys.offsets[0]):int(keys.offsets[-1])], keys.offsets - keys.offsets[0],
                         vo, cr, tb, raw, *[x for f in flushed for x in (f.data, f.index)])
                out.append((head, (keys, vo, cr, tb), flushed, raw))
        with ValueLog.open(log[:-3], base=self.base) as vl:
            torn = memtable.recover_puts(vl, int(gens[0]["vo"][-1]))
            self.rec("torn", torn[1], torn[2], torn[3])
        return out, torn

    # ---- compaction ----
    def merge(self, merger, files):
        from velarixdb_amd import sst
        data, index, bf, n = merger.merge_bucket_sst([sst.load_entries(d, i) for d, i in files], now_ms=sm.COMPACT_NOW)
        out = dict(data=data, index=index, n=n, words=bf.words().copy(), m=bf.num_bits(), k=bf.no_of_hash_func,
                   map=dict(merger.tombstones))
        del bf
        self.rec("merge", data, index, n, out["words"], sorted(out["map"].items()))
        return out

    def merger(self):
        from velarixdb_amd.compaction import CompactionConfig, SizedTierMerger
        return SizedTierMerger(CompactionConfig(filter_false_positive=sm.P))

    def partial(self):
        """Two rounds with one merger: generations 0-2, then 3-5 -> (rounds, files afterwards, reads, scans)."""
        files, merger, rounds = self.files(), self.merger(), []
        for r, bucket in enumerate(BUCKETS):
            rounds.append(self.merge(merger, [files[i] for i in bucket]))
        after = [(rounds[0]["data"], rounds[0]["index"]), (rounds[1]["data"], rounds[1]["index"])] + files[6:]
        return rounds, after, self.read("partial", after, self.log()), self.scan("partial", after, self.log())

    def full(self):
        """A fresh merger over every table -> (round, reads, scans over the one table)."""
        m = self.merge(self.merger(), self.files())
        after = [(m["data"], m["index"])]
        return m, self.read("full", after, self.log()), self.scan("full", after, self.log())

    # ---- GC ----
    def gc(self):
        """gc.collect over the chunk that ends inside generation 1, its bytes appended, its puts
        flushed into a table of their own, and every key and `tail` read again."""
        from velarixdb_amd import BloomFilter, Table, ValueLog, gc, memtable
        gens = self.generations()
        log = self.log()
        tail, chunk = sm.gc_chunk([d["vo"] for d in gens], self.base)
        tables = []
        try:
            tables = [Table.open(d, i) for d, i in self.files()]
            with ValueLog.open(log, base=self.base) as vl:
                got = gc.collect(vl, tables, tail, chunk, self.base + len(log), sm.GC_NOW, filters=[d["filter"] for d in gens])
        finally:
            for t in tables:
                t.close()
        if got is None:
            return tail, chunk, None, None, None
        f = BloomFilter(sm.P, len(got.put_keys))
        res = memtable.flush(got.put_keys, got.put_val_offsets, got.put_created_ms, got.put_tombstones, filter=f)
        self.rec("gc", got.invalid, got.total_bytes_read, got.new_tail, got.append, got.put_val_offsets, got.put_created_ms,
                 got.put_tombstones, res.data, res.index, f.words())
        reads = self.read("gc", self.files() + [(res.data, res.index)], log + got.append,
                          [d["filter"] for d in gens] + [f], keys=self.keys + [b"tail"])
        return tail, chunk, got, res, reads

    def everything(self):
        for g in range(len(self.generations())):
            self.reads_after(g)
        self.recovery()
        self.partial()
        self.full()
        self.gc()
        return self.digest()


def _get_arrays(r, v):
    return r.found, r.table, r.val_offsets, r.created_ms, v.status, v.values, v.value_off


def _scan_arrays(s):
    return s.range_off, s.keys, s.key_off, s.table, s.val_offsets, s.created_ms, s.tombstones


def _walk_val_offsets(vl, start):
    """The val_offsets output of vbf_vlog_walk_host, which ValueLog.walk leaves NULL."""
    from velarixdb_amd._lib import call
    sc = [ctypes.c_uint64() for _ in range(4)]
    stop = ctypes.c_int()
    tail = [ctypes.byref(x) for x in sc] + [ctypes.byref(stop)]
    none = (None, None, None, 0, None, None, 0, None, None, None)
    call("vbf_vlog_walk_host", vl._h, start, 2**64 - 1, *none, 0, *tail)
    n = sc[0].value
    vo = np.zeros(max(n, 1), np.uint32)
    call("vbf_vlog_walk_host", vl._h, start, 2**64 - 1, None, vo.ctypes.data, *none[2:], n, *tail)
    return vo[:n]


# ---- the model's side ----

_models, _lives = {}, {}


def model(ora, name):
    """-> ([the composed store after each generation], [(blob, val_offsets, ModelTable)])"""
    if name not in _models:
        h = sm.history(name)
        store, stores, steps = sm.ModelStore(ora, h.scenario.base), [], []
        for g in h.gens:
            steps.append(store.put_batch(g.keys, g.values, g.created, g.tombs))
            stores.append(store.clone())
        _models[name] = (stores, steps)
    return _models[name]


@pytest.fixture(scope="module")
def lives(vbf):
    def get(name):
        if name not in _lives:
            _lives[name] = Life(vbf, name)
        return _lives[name]
    yield get
    for life in _lives.values():
        life.close()
    _lives.clear()


def check_reads(got, store, keys, expect=None, loose=()):
    """The GPU's answers against sst_get_ref over the composed store's tables in the same order, the
    values against the composed store's get and, with `expect`, against the dictionary."""
    (r, v), (rr, vv) = got
    for (res, order) in ((r, 1), (rr, -1)):
        want = gref.search_many(keys, store.ssts()[::order])
        for name, a, w in zip(("found", "table", "val_offsets", "created_ms"),
                              (res.found, res.table, res.val_offsets, res.created_ms), want):
            assert np.array_equal(a, w), "%s differs (table order %d)" % (name, order)
    # no tie in created_at crosses tables but the seam's, whose two copies hold one value: the
    # order of the tables changes no value
    assert np.array_equal(r.found, rr.found) and np.array_equal(r.created_ms, rr.created_ms)
    for a, b in zip((v.status, v.values, v.value_off), (vv.status, vv.values, vv.value_off)):
        assert np.array_equal(a, b)
    for j, k in enumerate(keys):
        value = v.value(j)
        assert value == store.get(k)[4], k
        if expect is not None and k not in loose:
            assert value == expect(k), k


def check_scans(got, store, dictionary=True):
    for flags, ranges, s, v in got:
        want = store.scan_many(ranges, flags)
        for name, a, w in zip(("range_off", "keys", "key_off", "table", "val_offsets", "created_ms", "tombstones"),
                              _scan_arrays(s), want):
            assert np.array_equal(a, w), "%s differs (flags %d)" % (name, flags)
        for r, (lo, hi) in enumerate(ranges):
            rows = list(s.range(r))
            listed = [(row[0], v.value(i)) for i, row in zip(range(int(s.range_off[r]), int(s.range_off[r + 1])), rows)]
            assert [(k, val) for k, val in listed if val is not None] == \
                [(k, store.get(k)[4]) for k, *_ in rows if store.get(k)[0] == 1]
            if dictionary and not flags & sm.KEEP_TOMBSTONES:
                assert listed == store.expect_slice(lo, hi, flags), (lo, hi, flags)


# ---- the phases ----

@pytest.mark.parametrize("name", NAMES)
def test_generations(lives, ora, name):
    """The log, the offsets, the table's files and the memtable's filter of every generation."""
    _, steps = model(ora, name)
    for g, (d, (blob, offs, tab)) in enumerate(zip(lives(name).generations(), steps)):
        res = d["res"]
        assert d["log"] == blob and d["vo"].tolist() == offs, g
        assert res.data.tobytes() == tab.data and res.index.tobytes() == tab.index, g
        assert np.array_equal(res.ids, tab.ids) and res.ids.dtype == np.uint32
        keys = sm.history(name).gens[g].keys
        assert (res.smallest, res.biggest) == (min(keys), max(keys))
        assert (d["m"], d["k"], d["num_elements"]) == (tab.m, tab.k, tab.num_elements), g
        assert np.array_equal(d["words"], tab.words), g


@pytest.mark.parametrize("name", NAMES)
def test_reads_and_scans_after_every_generation(lives, ora, name):
    stores, _ = model(ora, name)
    life = lives(name)
    for g, store in enumerate(stores):
        reads, scans = life.reads_after(g)
        check_reads(reads, store, life.keys, store.expect)
        check_scans(scans, store)


@pytest.mark.parametrize("name", NAMES)
def test_recovery(lives, ora, name):
    stores, steps = model(ora, name)
    life = lives(name)
    gens = life.generations()
    out, torn = life.recovery()
    h = sm.history(name)
    for g, (head, (keys, vo, cr, tb), flushed, raw) in enumerate(out):
        want = stores[-1].recover(head)
        assert head == steps[g][1][-1] and keys.n == len(want) == sum(len(x.keys) for x in h.gens[g + 1:])
        assert keys.n == 0 or int(keys.offsets[0]) > 0  # the first offset is not zero: the head's key lies before it
        assert [keys.data[int(keys.offsets[j]):int(keys.offsets[j + 1])].tobytes() for j in range(keys.n)] == [e[1] for e in want]
        assert vo.tolist() == [e[0] for e in want] and cr.tolist() == [e[3] for e in want]
        assert tb.tolist() == [e[4] for e in want]
        assert raw.tolist() == [head] + vo.tolist()  # vbf_vlog_walk_host's own val_offsets, head entry included
        assert len(flushed) == len(gens) - g - 1
        for f, d, (_, _, tab) in zip(flushed, gens[g + 1:], steps[g + 1:]):  # the bytes the original flush wrote
            assert np.array_equal(f.data, d["res"].data) and np.array_equal(f.index, d["res"].index)
            assert f.data.tobytes() == tab.data and np.array_equal(f.ids, tab.ids)
    # a crash mid-append: the torn last put is absent, everything before it unchanged
    want = stores[-1].recover(out[0][0], cut=3)
    assert len(want) == out[0][1][0].n - 1
    assert torn[0].n == len(want) and torn[1].tolist() == [e[0] for e in want] == out[0][1][1][:-1].tolist()
    assert np.array_equal(torn[2], out[0][1][2][:-1]) and np.array_equal(torn[3], out[0][1][3][:-1])


def check_merge(got, tab, tmap, ora):
    assert got["n"] == tab.entries and got["data"].tobytes() == tab.data and got["index"].tobytes() == tab.index
    assert (got["m"], got["k"]) == (tab.m, tab.k) and np.array_equal(got["words"], tab.words)
    assert got["map"] == tmap.items()


@pytest.mark.parametrize("name", NAMES)
def test_partial_compaction(lives, ora, name):
    """The composed store is the expectation: it does not read back the dictionary (sized.rs:286-320)."""
    stores, _ = model(ora, name)
    rounds, after, reads, scans = lives(name).partial()
    s, tmap = stores[-1].clone(), ora.TombstoneMap()
    for r, bucket in enumerate(((0, 1, 2), (1, 2, 3))):  # generations 3-5 are tables 1-3 after the first round
        tab = s.compact(bucket, tmap)
        check_merge(rounds[r], tab, tmap, ora)
        s.replace(bucket, tab)
    assert [(bytes(d), bytes(i)) for d, i in after] == [(t.data, t.index) for t in s.tables]
    check_reads(reads, s, lives(name).keys)
    check_scans(scans, s, dictionary=False)


@pytest.mark.parametrize("name", NAMES)
def test_full_compaction(lives, ora, name):
    stores, _ = model(ora, name)
    life = lives(name)
    got, reads, scans = life.full()
    s, tmap = stores[-1].clone(), ora.TombstoneMap()
    every = tuple(range(len(s.tables)))
    tab = s.compact(every, tmap)
    check_merge(got, tab, tmap, ora)
    s.replace(every, tab)
    dictionary = sm.history(name).scenario.high_clock_gen < 0  # see tests/test_store_model.py
    check_reads(reads, s, life.keys, s.expect if dictionary else None)
    check_scans(scans, s, dictionary=dictionary)


@pytest.mark.parametrize("name", NAMES)
def test_gc(lives, ora, name):
    stores, _ = model(ora, name)
    life = lives(name)
    s = stores[-1].clone()
    tail, chunk, got, res, reads = life.gc()
    want = s.gc(tail, chunk)
    same_gc(got, want, s.log_size, sm.GC_NOW)
    # GC::put writes an empty value as a tombstone (garbage_collector.rs:404-419): such a key reads as
    # deleted afterwards, unless a put at 2^63 or later still wins the get
    loose = {k for k, v, *_ in want["append"][1:] if v == b"" and s.dict[k][1] < sm.GC_NOW}
    tab = s.apply_gc(want)
    assert res.data.tobytes() == tab.data and res.index.tobytes() == tab.index and np.array_equal(res.ids, tab.ids)
    keys = life.keys + [b"tail"]
    check_reads(reads, s, keys, s.expect, loose)
    (r, v), _ = reads
    assert v.value(len(keys) - 1) == struct.pack("<Q", got.new_tail)
    assert all(r.found[keys.index(k)] == 2 for k in loose)
    # no live answer points into the collected chunk, but for a live "*" (garbage_collector.rs:205-208)
    inside = np.flatnonzero((r.found == 1) & (r.val_offsets >= tail) & (r.val_offsets < got.new_tail))
    assert all(s.expect(keys[j]) == b"*" for j in inside)


def test_state_between_calls(vbf):
    """The largest scenario, the smallest, the largest again, and once more after the workspaces were
    released: every artefact of the three large runs is the same, whatever an earlier call left behind."""
    digests = []
    for name in (sm.LARGEST, sm.SMALLEST, sm.LARGEST, None, sm.LARGEST):
        if name is None:
            vbf.lib.vbf_release_workspaces()
            continue
        life = Life(vbf, name)
        try:
            t = time.perf_counter()
            digests.append((name, life.everything(), len(life.art)))
            print("%s: the whole lifecycle on the GPU in %.2f s" % (name, time.perf_counter() - t))
        finally:
            life.close()
    large = [d for d in digests if d[0] == sm.LARGEST]
    assert len(large) == 3 and large[0][2] > 100 and len({d[1:] for d in large}) == 1, digests
