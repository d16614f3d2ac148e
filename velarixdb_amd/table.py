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
"""
import ctypes
from dataclasses import dataclass

import numpy as np

from ._lib import VbfError, call, lib
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
