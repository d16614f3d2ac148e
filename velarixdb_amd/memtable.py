"""Memtable flush on the GPU: a batch of puts in arrival order -> an SST's files.

DataStore::put appends to the value log and calls MemTable::insert (src/db/store.rs:215-243,
src/memtable/mem.rs:207-221); Flusher::flush hands the memtable's SkipMap to Table::write_to_file
(src/flush/flusher.rs:37-64, src/sst/table.rs:258-326).  For a whole batch -- a bulk load, or the
replay of a recovered value log (src/db/recovery.rs:245-286) -- that is a sort with "last insert
wins" (crossbeam-skiplist removes an entry of the same key before it inserts), the gather of the
survivors and the encode, all on the device (C ABI vbf_memtable_sort_host / vbf_flush_write_host,
velarixdb_amd/csrc/vbf_memtable.hip).

  sort_ids(keys)                       -> uint32 ids: the distinct keys ascending, each by its last put
  flush(keys, val_offsets, created_ms=None, tombstones=None, filter=None)
      -> FlushResult(data, index, ids, smallest, biggest)   data.db / index.db bytes of the table
  put_many(keys, values, created_ms, tombstones=None, base=0, filter=None)
      -> (log bytes, FlushResult)      ValueLog.encode, then flush with its val_offsets
  flush_to_dir(sst_dir, keys, val_offsets, ...)             flush into sst_dir/data.db and index.db
  recover_puts(vlog, head_offset)      -> (keys, val_offsets, created_ms, tombstones): the recovered
                                       log's entries after the head entry, ready for sort_ids / flush
  BloomFilter.insert_many(keys)        the memtable's filter step, see filter.py
  MemTable.open(keys, val_offsets, created_ms=None, tombstones=None)   -> MemTable: the puts sorted and
                                       kept on the device (C ABI vbf_memtable_open_host), immutable
  mt.export()                          -> MemEntries(keys, val_offsets, created_ms, tombstones), sorted
  mt.flush()                           -> FlushResult: Flusher::flush of the open table
  MemTable.get_many(keys, active=None, read_only=(), gc=None, vlog=None)
      -> MemGet(found, layer, val_offsets, created_ms): steps 0-2 of DataStore::get (store.rs:442-472)
      for a batch -- the gc table, the active memtable, the read-only ones -- on the device
      (vbf_memtable_get_host, velarixdb_amd/csrc/vbf_memget.hip); store.get_many goes on to the values

`filter` (a device-resident BloomFilter on `device`) takes MemTable::insert's filter step over
every put in order.  Cutting a put stream into memtables by capacity (is_full, mem.rs:277-279),
the `head` entry of migrate_memtable_to_read_only (store.rs:250-263) and summary.db stay with
the caller.
"""
import ctypes
import os
from dataclasses import dataclass

import numpy as np

from ._lib import VbfError, call, lib
from .filter import _raise
from .keys import HostBatch, pack, pack_offsets
from .sst import DATA_FILE_NAME, INDEX_FILE_NAME
from .vlog import ValueLog


@dataclass
class FlushResult:
    data: np.ndarray    # uint8: data.db
    index: np.ndarray   # uint8: index.db
    ids: np.ndarray     # uint32: the table's entries as indices into the batch, in key order
    smallest: bytes     # the summary's two keys (table.rs:270-274)
    biggest: bytes


def _batch(keys):
    return keys if isinstance(keys, HostBatch) else pack(keys)


def _key(b, j):
    if b.offsets is not None:
        return b.data[int(b.offsets[j]):int(b.offsets[j + 1])].tobytes()
    return b.data[j * b.stride:(j + 1) * b.stride].tobytes()


def sort_ids(keys, device=0):
    """SkipMap order of the puts `keys` (bytes, or a HostBatch): the distinct keys ascending, each
    represented by the index of its last put."""
    b = _batch(keys)
    ids = np.zeros(b.n, np.uint32)
    n_out = ctypes.c_uint64()
    d, o = b.ptrs()
    try:
        call("vbf_memtable_sort_host", d, o, b.stride, b.n, ids.ctypes.data if b.n else None, ctypes.byref(n_out),
             int(device))
    except VbfError as e:
        _raise("memtable_sort", e)
    return ids[:n_out.value]


def flush(keys, val_offsets, created_ms=None, tombstones=None, filter=None, device=0):
    """Flusher::flush for the puts `keys` in arrival order.  An empty batch raises AssertionError
    ("Cannot flush an empty table", flusher.rs:40-44), and so does a key over 4079 bytes (where the
    reference fails with BlockIsFull)."""
    b = _batch(keys)
    n = b.n
    arr = lambda x, t: None if x is None else np.ascontiguousarray(x, dtype=t)
    vo, cr, tb = arr(val_offsets, np.uint32), arr(created_ms, np.int64), arr(tombstones, np.uint8)
    if any(x is not None and x.size != n for x in (vo, cr, tb)):
        raise ValueError("one val_offset / created_ms / tombstone per key")
    kb = int(b.offsets[-1] - b.offsets[0]) if b.offsets is not None else n * b.stride
    data, index = np.zeros(kb + 17 * n + 1, np.uint8), np.zeros(kb + 8 * n + 1, np.uint8)
    ids = np.zeros(max(n, 1), np.uint32)
    dl, il, n_out = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    vp = lambda x: x.ctypes.data if x is not None and x.size else None
    d, o = b.ptrs()
    try:
        call("vbf_flush_write_host", d, o, b.stride, n, vp(vo), vp(cr), vp(tb), filter._h if filter is not None else None,
             data.ctypes.data, data.size, ctypes.byref(dl), index.ctypes.data, index.size, ctypes.byref(il),
             ids.ctypes.data, ctypes.byref(n_out), int(device))
    except VbfError as e:
        _raise("flush_write", e)
    ids = ids[:n_out.value]
    return FlushResult(data[:dl.value].copy(), index[:il.value].copy(), ids, _key(b, int(ids[0])), _key(b, int(ids[-1])))


def put_many(keys, values, created_ms, tombstones=None, base=0, filter=None, device=0):
    """DataStore::put for a batch, through to the flushed table: ValueLog.encode (the log's bytes
    when the file's size is `base`, and every put's val_offset), then flush -> (log bytes,
    FlushResult)."""
    b = _batch(keys)
    log, vo = ValueLog.encode(b, values, created_ms=created_ms, tombstones=tombstones, base=base, device=device)
    return log, flush(b, vo, created_ms=created_ms, tombstones=tombstones, filter=filter, device=device)


def recover_puts(vlog, head_offset):
    """The data side of recover_memtable (src/db/recovery.rs:245-286): the value log's entries from
    `head_offset` on (ValueLog::recover, a ValueLog.walk on the device) without the first one, which
    is the most recent entry already in an SST (recovery.rs:261-264), as the puts that rebuild the
    memtables -> (keys HostBatch, val_offsets u32, created_ms i64, tombstones u8), in log order,
    ready for sort_ids / flush.  A torn last entry (a crash mid-append) is left out.  Cutting the
    stream into memtables by capacity stays with the caller."""
    w = vlog.walk(start=head_offset, values=False)
    if w.n == 0:
        return HostBatch(np.zeros(0, np.uint8), np.zeros(1, np.uint64), 0, 0, 1), np.zeros(0, np.uint32), \
            np.zeros(0, np.int64), np.zeros(0, np.uint8)
    keys = HostBatch(w.keys.data, w.keys.offsets[1:].copy(), 0, w.n - 1, w.keys.len_prefix)
    return keys, w.val_offsets[1:].copy(), w.created_ms[1:].copy(), w.tombstones[1:].copy()


def flush_to_dir(sst_dir, keys, val_offsets, created_ms=None, tombstones=None, filter=None, device=0):
    """flush, with data.db and index.db written into `sst_dir` (created when missing), as
    sst.write_sst_files writes them."""
    res = flush(keys, val_offsets, created_ms=created_ms, tombstones=tombstones, filter=filter, device=device)
    os.makedirs(sst_dir, exist_ok=True)
    with open(os.path.join(sst_dir, DATA_FILE_NAME + ".db"), "wb") as f:
        f.write(res.data.tobytes())
    with open(os.path.join(sst_dir, INDEX_FILE_NAME + ".db"), "wb") as f:
        f.write(res.index.tobytes())
    return res


LAYER_GC, LAYER_ACTIVE, LAYER_READ_ONLY, LAYER_NONE = 0, 1, 2, 0xFFFFFFFF
LAYER_TABLE = 0x80000000  # store.get_many: layer = LAYER_TABLE | index into `tables`


@dataclass
class MemEntries:
    keys: HostBatch          # the distinct keys ascending (offsets from 0)
    val_offsets: np.ndarray  # uint32
    created_ms: np.ndarray   # int64
    tombstones: np.ndarray   # uint8


@dataclass
class MemGet:
    found: np.ndarray        # uint8: 0 in no memtable, 1 live, 2 tombstone
    layer: np.ndarray        # uint32: LAYER_GC, LAYER_ACTIVE, LAYER_READ_ONLY + r, LAYER_NONE
    val_offsets: np.ndarray  # uint32
    created_ms: np.ndarray   # uint64: the winner's created_at bits


def _handles(tabs):
    tabs = list(tabs)
    return tabs, (ctypes.c_void_p * max(len(tabs), 1))(*[t._h.value for t in tabs])


class MemTable:
    """An immutable memtable resident on `device`: the puts it was opened from, sorted, last put wins."""

    def __init__(self, _handle):
        self._h = _handle

    @classmethod
    def open(cls, keys, val_offsets, created_ms=None, tombstones=None, device=0):
        """MemTable::insert (mem.rs:207-221) for the puts `keys` in arrival order."""
        b = _batch(keys)
        n = b.n
        arr = lambda x, t: None if x is None else np.ascontiguousarray(x, dtype=t)
        vo, cr, tb = arr(val_offsets, np.uint32), arr(created_ms, np.int64), arr(tombstones, np.uint8)
        if any(x is not None and x.size != n for x in (vo, cr, tb)):
            raise ValueError("one val_offset / created_ms / tombstone per key")
        vp = lambda x: x.ctypes.data if x is not None and x.size else None
        d, o = b.ptrs()
        h = ctypes.c_void_p()
        try:
            call("vbf_memtable_open_host", d, o, b.stride, n, vp(vo), vp(cr), vp(tb), int(device), ctypes.byref(h))
        except VbfError as e:
            _raise("memtable_open", e)
        return cls(h)

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            lib.vbf_memtable_free(h)
        self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def entries(self):
        return lib.vbf_memtable_entries(self._h)

    @property
    def key_bytes(self):
        return lib.vbf_memtable_key_bytes(self._h)

    @property
    def device(self):
        return lib.vbf_memtable_device(self._h)

    def export(self):
        """The sorted entries, in the layout of gc.collect_device's overlay."""
        n, kb = self.entries, self.key_bytes
        keys, off = np.zeros(kb + 1, np.uint8), np.zeros(n + 1, np.uint64)
        vo, cr, tb = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.int64), np.zeros(n + 1, np.uint8)
        try:
            call("vbf_memtable_export_host", self._h, keys.ctypes.data, kb, off.ctypes.data, vo.ctypes.data, cr.ctypes.data,
                 tb.ctypes.data, n)
        except VbfError as e:
            _raise("memtable_export", e)
        return MemEntries(pack_offsets(keys[:kb], off), vo[:n], cr[:n], tb[:n])

    def flush(self):
        """Flusher::flush of this table -> FlushResult; `ids` is None (the handle holds no put indices).
        An empty table raises AssertionError ("Cannot flush an empty table", flusher.rs:40-44)."""
        n, kb = self.entries, self.key_bytes
        data, index = np.zeros(kb + 17 * n + 1, np.uint8), np.zeros(kb + 8 * n + 1, np.uint8)
        dl, il = ctypes.c_uint64(), ctypes.c_uint64()
        try:
            call("vbf_memtable_encode_host", self._h, data.ctypes.data, data.size, ctypes.byref(dl), index.ctypes.data,
                 index.size, ctypes.byref(il))
        except VbfError as e:
            _raise("memtable_encode", e)
        ent = self.export()
        return FlushResult(data[:dl.value].copy(), index[:il.value].copy(), None, _key(ent.keys, 0), _key(ent.keys, n - 1))

    @staticmethod
    def get_many(keys, active=None, read_only=(), gc=None, vlog=None):
        """Steps 0-2 of DataStore::get for every key: `gc` (needs `vlog`: a gc hit stands only with a
        live value in the log), then `active`, then the newest of `read_only` -> MemGet."""
        b = _batch(keys)
        ro, rh = _handles(read_only)
        res = MemGet(np.zeros(b.n, np.uint8), np.zeros(b.n, np.uint32), np.zeros(b.n, np.uint32), np.zeros(b.n, np.uint64))
        d, o = b.ptrs()
        vp = lambda x: x.ctypes.data if x.size else None
        h = lambda t: t._h if t is not None else None
        try:
            call("vbf_memtable_get_host", d, o, b.stride, b.n, h(gc), h(active), len(ro), rh, h(vlog), vp(res.found),
                 vp(res.layer), vp(res.val_offsets), vp(res.created_ms))
        except VbfError as e:
            _raise("memtable_get", e)
        return res
