"""The checker for the whole get: DataStore::get restated over Python dicts, line for line.

A memtable is a dict key -> Entry(val_offset, created_at, is_tombstone); created_at is the signed
64-bit value the reference's DateTime holds (millis).  The SSTs and the value log are the existing
checkers' (sst_get_ref.search, vlog_ref.get) over file bytes.

  memtable_get        MemTable::get, src/memtable/mem.rs:223-230: the Bloom filter is asked first and
                      the map only when it says yes.  The filter holds every key that was inserted
                      (mem.rs:209-211) and has no false negatives, so the filter test is `key in dict`
                      or a false positive, and either way the answer is the map's.
  search_gc_entries   src/db/store.rs:489-501.
  get                 src/db/store.rs:442-481.

Two readings, as include/vbf.h states them: get_value_from_vlog's error on an entry that is not a whole
entry of the log (BAD) is carried as status BAD of a found key, not as a failed call -- so a gc entry
with such an offset keeps its hit; and validate_size (:443) stays with the caller, a zero-length key is
an ordinary key.  The product never imports this module.
"""
from collections import namedtuple

import numpy as np

import sst_get_ref as gref
import vlog_ref as vr

Entry = namedtuple("Entry", "val_offset created_at is_tombstone")
LAYER_GC, LAYER_ACTIVE, LAYER_RO, LAYER_NONE, LAYER_TABLE = 0, 1, 2, 0xFFFFFFFF, 0x80000000
NO_TABLE = gref.NO_TABLE
VLOG_START_OFFSET = 0
DEFAULT_DATETIME = 0  # util::default_datetime(): the epoch

Got = namedtuple("Got", "found layer table val_offset created_ms status value")


def i64(x):
    x = int(x) & 0xFFFFFFFFFFFFFFFF
    return x - 2**64 if x >= 2**63 else x


def memtable(keys, val_offsets=None, created=None, tombs=None):
    """SkipMap::insert for the puts in order (the last put of a key wins) -> dict key -> Entry."""
    m = {}
    for j, k in enumerate(keys):
        m[bytes(k)] = Entry(0 if val_offsets is None else int(val_offsets[j]), 0 if created is None else i64(created[j]),
                            False if tombs is None else bool(tombs[j]))
    return m


def memtable_get(table, key):
    if key in table:  # bloom_filter.contains(key): no false negatives
        return table.get(key)
    return table.get(key)  # a false positive, or "no": the map has no such key either way


class Store:
    """What DataStore::get reads: gc_updated_entries, active_memtable, read_only_memtables (in
    iteration order), the SSTs (sst_get_ref.Sst or (data, index)) and the log's bytes [base, ...)."""

    def __init__(self, log=b"", base=0, gc=None, active=None, read_only=(), tables=()):
        self.log, self.base = bytes(log), base
        self.gc, self.active, self.read_only = gc, active, list(read_only)
        self.tables = [t if isinstance(t, gref.Sst) else gref.Sst(*t) for t in tables]

    def get_value_from_vlog(self, offset, key, check_key):
        """-> (status, value): store.rs:628-641 over vlog_ref.get."""
        return vr.get(self.log, int(offset), self.base, key if check_key else None)

    def search_gc_entries(self, key):
        """-> Entry when the gc entries decide the get, else None (Ok(None): the get goes on)."""
        gc_entries = self.gc or {}
        if gc_entries:  # !gc_entries.is_empty()
            e = gc_entries.get(key)
            if e is not None:
                if e.is_tombstone:
                    return None
                st, _ = vr.get(self.log, e.val_offset, self.base)
                if st in (vr.NONE, vr.TOMBSTONE):  # get_value_from_vlog returned Ok(None)
                    return None
                return e  # a value -- or BAD, where the reference's `?` fails the get
        return None

    def get(self, key, allowed=None, check_key=False):
        key = bytes(key)

        def answer(found, layer, table, offset, time):
            st, value = vr.SKIPPED, None
            if found == 1:
                st, value = self.get_value_from_vlog(offset, key, check_key)
            return Got(found, layer, table, offset, time & 0xFFFFFFFFFFFFFFFF, st, value)

        val = self.search_gc_entries(key)
        if val is not None:
            return answer(1, LAYER_GC, NO_TABLE, val.val_offset, val.created_at)
        offset = VLOG_START_OFFSET
        insert_time = DEFAULT_DATETIME
        lowest_insert_time = DEFAULT_DATETIME
        val = memtable_get(self.active, key) if self.active is not None else None
        if val is not None:
            return answer(2 if val.is_tombstone else 1, LAYER_ACTIVE, NO_TABLE, val.val_offset, val.created_at)
        is_deleted = False
        who = LAYER_NONE
        for r, table in enumerate(self.read_only):
            val = memtable_get(table, key)
            if val is not None:
                if val.created_at > insert_time:
                    offset = val.val_offset
                    insert_time = val.created_at
                    is_deleted = val.is_tombstone
                    who = LAYER_RO + r
        if insert_time > lowest_insert_time:  # found_in_table
            return answer(2 if is_deleted else 1, who, NO_TABLE, offset, insert_time)
        found, t, vo, created = gref.search(key, self.tables, allowed)
        if found == 0:
            return answer(0, LAYER_NONE, NO_TABLE, 0, 0)
        return answer(found, LAYER_TABLE | t, t, vo, created)

    def memtable_step(self, key):
        """Steps 0-2 alone -> (found, layer, val_offset, created_ms) as vbf_memtable_get_* reports them."""
        saved, self.tables = self.tables, []
        try:
            g = self.get(key)
        finally:
            self.tables = saved
        return g.found, g.layer, g.val_offset, g.created_ms

    def get_many(self, keys, allowed=None, check_keys=False):
        """-> dict of numpy arrays as vbf_store_get_host fills them."""
        got = [self.get(k, None if allowed is None else allowed[j], check_keys) for j, k in enumerate(keys)]
        lens = [len(g.value) if g.status == vr.VALUE else 0 for g in got]
        return {
            "found": np.array([g.found for g in got], np.uint8),
            "layer": np.array([g.layer for g in got], np.uint32),
            "table": np.array([g.table for g in got], np.uint32),
            "val_offsets": np.array([g.val_offset for g in got], np.uint32),
            "created_ms": np.array([g.created_ms for g in got], np.uint64),
            "status": np.array([g.status for g in got], np.uint8),
            "values": np.frombuffer(b"".join(g.value for g in got if g.status == vr.VALUE), np.uint8).copy(),
            "value_off": np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64),
        }

    def memtable_many(self, keys):
        rows = [self.memtable_step(k) for k in keys]
        cols = list(zip(*rows)) if rows else [(), (), (), ()]
        return (np.array(cols[0], np.uint8), np.array(cols[1], np.uint32), np.array(cols[2], np.uint32),
                np.array(cols[3], np.uint64))
