"""Batched point lookups in SST tables on the GPU: the read path after the
filters.

velarixdb answers a get per candidate SST with two file scans -- index.db for the first record whose
key is >= the searched key (IndexFileNode::get_from_index, src/fs/mod.rs:667-710), then data.db from
that block for an equal key (DataFileNode::find_entry, src/fs/mod.rs:334-389) -- and keeps the
strictly newest hit (DataStore::search_key_in_sstables, src/db/store.rs:579-612).  Here a table is
opened once on the device (C ABI vbf_table_open_*, validated there) and a batch of keys is looked up
in every table in one launch (vbf_table_get_host, velarixdb_amd/csrc/vbf_table.hip).

  Table.open(data, index)     -> Table       data.db / index.db bytes, uploaded and validated
  Table.open_dir(sst_dir)     -> Table       the same from an SST directory
  get_many(keys, tables, filters=None) -> GetResult(found, table, val_offsets, created_ms)
      found 0 = nowhere, 1 = live, 2 = tombstone; table = index into `tables` (0xFFFFFFFF when
      found == 0).  filters (one BloomFilter per table) only prune work: the answers are the same.
  scan_many(ranges, tables, keep_tombstones=False, end_exclusive=False)
      -> ScanResult(range_off, keys, key_off, table, val_offsets, created_ms, tombstones)
      the key side of DataStore::seek (src/range/range_iterator.rs:47-60) for a batch of (lo, hi)
      ranges: per range, in key order, every key inside the bounds that get_many would find, with
      get_many's answer for it (C ABI vbf_table_scan_host, velarixdb_amd/csrc/vbf_table_scan.hip).
  get_values(keys, tables, vlog, filters=None, check_keys=False) -> (GetResult, Values)
  scan_values(ranges, tables, vlog, ...)                         -> (ScanResult, Values)
      the same two, followed by the value-log read of every live answer (velarixdb_amd/vlog.py).
"""
import ctypes
from dataclasses import dataclass

import numpy as np

from ._lib import VBF_SCAN_END_EXCLUSIVE, VBF_SCAN_KEEP_TOMBSTONES, VbfError, call, lib
from .filter import _raise
from .keys import HostBatch, pack
from .sst import _buf, read_sst_files

FOUND_NONE, FOUND_LIVE, FOUND_TOMBSTONE = 0, 1, 2
NO_TABLE = 0xFFFFFFFF


class Table:
    """An SST resident on `device`: data.db, index.db and the lookup side tables."""

    def __init__(self, _handle):
        self._h = _handle

    @classmethod
    def open(cls, data, index, device=0):
        """Uploads and validates the two files; AssertionError for a file the reference's writer
        cannot have produced (unsorted keys, an index that does not match its blocks, ...)."""
        a, pa = _buf(data)
        b, pb = _buf(index)
        h = ctypes.c_void_p()
        try:
            call("vbf_table_open_host", pa, a.size, pb, b.size, int(device), ctypes.byref(h))
        except VbfError as e:
            _raise("table_open", e)
        return cls(h)

    @classmethod
    def open_dir(cls, sst_dir, device=0):
        return cls.open(*read_sst_files(sst_dir), device=device)

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            lib.vbf_table_free(h)
        self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def entries(self):
        return lib.vbf_table_entries(self._h)

    @property
    def blocks(self):
        return lib.vbf_table_blocks(self._h)

    @property
    def device(self):
        return lib.vbf_table_device(self._h)

    def key_range(self):
        """(smallest_key, biggest_key) as KeyRange stores them (key_range/range.rs)."""
        sl, bl = ctypes.c_uint64(), ctypes.c_uint64()
        call("vbf_table_key_range", self._h, None, 0, ctypes.byref(sl), None, 0, ctypes.byref(bl))
        s, b = np.zeros(sl.value + 1, np.uint8), np.zeros(bl.value + 1, np.uint8)
        call("vbf_table_key_range", self._h, s.ctypes.data, sl.value, ctypes.byref(sl), b.ctypes.data, bl.value,
             ctypes.byref(bl))
        return s[:sl.value].tobytes(), b[:bl.value].tobytes()


@dataclass
class GetResult:
    found: np.ndarray        # uint8: 0 nowhere, 1 live, 2 tombstone
    table: np.ndarray        # uint32 index into `tables`, NO_TABLE when found == 0
    val_offsets: np.ndarray  # uint32
    created_ms: np.ndarray   # uint64


def get_many(keys, tables, filters=None):
    """DataStore::search_key_in_sstables for every key over `tables` in the given order."""
    b = keys if isinstance(keys, HostBatch) else pack(keys)
    tables = list(tables)
    nsst = len(tables)
    if filters is not None:
        filters = list(filters)
        if len(filters) != nsst:
            raise ValueError("one filter per table")
    res = GetResult(np.zeros(b.n, np.uint8), np.zeros(b.n, np.uint32), np.zeros(b.n, np.uint32),
                    np.zeros(b.n, np.uint64))
    th = (ctypes.c_void_p * max(nsst, 1))(*[t._h.value for t in tables])
    fh = (ctypes.c_void_p * max(nsst, 1))(*[f._h.value for f in filters]) if filters is not None else None
    d, o = b.ptrs()
    vp = lambda x: x.ctypes.data if x.size else None
    try:
        call("vbf_table_get_host", d, o, b.stride, b.n, nsst, th, fh, vp(res.found), vp(res.table),
             vp(res.val_offsets), vp(res.created_ms))
    except VbfError as e:
        _raise("table_get", e)
    return res


@dataclass
class ScanResult:
    range_off: np.ndarray    # uint64 [nranges + 1]: range r lists outputs range_off[r] .. range_off[r+1]
    keys: np.ndarray         # uint8: the listed keys back to back
    key_off: np.ndarray      # uint64 [n + 1]: key i = keys[key_off[i] .. key_off[i+1])
    table: np.ndarray        # uint32 index into `tables` of the winning entry
    val_offsets: np.ndarray  # uint32
    created_ms: np.ndarray   # uint64
    tombstones: np.ndarray   # uint8: 1 only with keep_tombstones

    def range(self, r):
        """(key bytes, table, val_offset, created_ms, tombstone) for every entry of range r, in key order."""
        kb = self.keys.tobytes()
        for i in range(int(self.range_off[r]), int(self.range_off[r + 1])):
            yield (kb[int(self.key_off[i]):int(self.key_off[i + 1])], int(self.table[i]), int(self.val_offsets[i]),
                   int(self.created_ms[i]), int(self.tombstones[i]))


def scan_many(ranges, tables, keep_tombstones=False, end_exclusive=False):
    """For every (lo, hi) of `ranges` (bytes, both ends inclusive unless end_exclusive) the keys of
    `tables` inside it that get_many over the same tables finds, ascending, with its answers.  One
    size query, then one filling call."""
    ranges = [(bytes(lo), bytes(hi)) for lo, hi in ranges]
    tables = list(tables)
    nr, nsst = len(ranges), len(tables)
    flat = [b for pair in ranges for b in pair]
    bounds = np.frombuffer(b"".join(flat) + b"\0", np.uint8)  # never NULL
    boff = np.concatenate([[0], np.cumsum([len(b) for b in flat], dtype=np.uint64)]).astype(np.uint64)
    th = (ctypes.c_void_p * max(nsst, 1))(*[t._h.value for t in tables])
    flags = (VBF_SCAN_KEEP_TOMBSTONES if keep_tombstones else 0) | (VBF_SCAN_END_EXCLUSIVE if end_exclusive else 0)
    n, kb = ctypes.c_uint64(), ctypes.c_uint64()
    head = (bounds.ctypes.data, boff.ctypes.data, nr, nsst, th, flags)
    try:
        call("vbf_table_scan_host", *head, None, None, 0, None, None, None, None, None, 0, ctypes.byref(n),
             ctypes.byref(kb))
        res = ScanResult(np.zeros(nr + 1, np.uint64), np.zeros(kb.value, np.uint8), np.zeros(n.value + 1, np.uint64),
                         np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint64),
                         np.zeros(n.value, np.uint8))
        vp = lambda x: x.ctypes.data if x.size else None
        call("vbf_table_scan_host", *head, res.range_off.ctypes.data, vp(res.keys), kb.value, res.key_off.ctypes.data,
             vp(res.table), vp(res.val_offsets), vp(res.created_ms), vp(res.tombstones), n.value, ctypes.byref(n),
             ctypes.byref(kb))
    except VbfError as e:
        _raise("table_scan", e)
    return res


def get_values(keys, tables, vlog, filters=None, check_keys=False):
    """A batched get that ends in values: get_many, then the value-log read of every live winner
    (DataStore::get_value_from_vlog, src/db/store.rs:628-641) -> (GetResult, vlog.Values).  Items
    that were not found, or whose winner is a tombstone, are SKIPPED in the Values.  check_keys makes
    every fetch check that the log's entry holds the searched key (the reference does not)."""
    b = keys if isinstance(keys, HostBatch) else pack(keys)
    res = get_many(b, tables, filters)
    return res, vlog.get_many(res.val_offsets, found=res.found, keys=b if check_keys else None)


def scan_values(ranges, tables, vlog, keep_tombstones=False, end_exclusive=False, check_keys=False):
    """scan_many, then the value-log read of every listed live entry -> (ScanResult, vlog.Values);
    a listed tombstone (keep_tombstones) is SKIPPED in the Values."""
    from .keys import pack_offsets
    res = scan_many(ranges, tables, keep_tombstones=keep_tombstones, end_exclusive=end_exclusive)
    found = np.where(res.tombstones != 0, FOUND_TOMBSTONE, FOUND_LIVE).astype(np.uint8)
    keys = pack_offsets(res.keys, res.key_off) if check_keys else None
    return res, vlog.get_many(res.val_offsets, found=found, keys=keys)
