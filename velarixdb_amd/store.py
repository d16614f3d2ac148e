"""The whole get on the GPU: a batch of keys from bytes to values in one device pass.

DataStore::get (src/db/store.rs:442-481) asks the GC's not-yet-synced entries, the active memtable,
the read-only memtables and the SSTs, in that order, and reads the value log for the winner.  Here
the memtables (memtable.MemTable), the tables (table.Table) and a window of the log (vlog.ValueLog)
are resident on one device and a batch of keys goes through all of them in one call (C ABI
vbf_store_get_host): the keys are uploaded once and nothing returns to the host in between.

  get_many(keys, tables, vlog, active=None, read_only=(), gc=None, filters=None, check_keys=False)
      -> StoreGet(found, layer, table, val_offsets, created_ms, values)
      found 0 = nowhere, 1 = live, 2 = tombstone; layer = memtable.LAYER_GC, LAYER_ACTIVE,
      LAYER_READ_ONLY + r, LAYER_TABLE | index into `tables`, or LAYER_NONE; values is a
      vlog.Values over the batch (SKIPPED unless found == 1).

  scan_many(ranges, tables, vlog, active=None, read_only=(), gc=None, keep_tombstones=False,
            end_exclusive=False, check_keys=False)
      -> StoreScan(range_off, keys, key_off, tombstones, layer, table, val_offsets, created_ms, values)
      DataStore::seek (src/range/range_iterator.rs:47-60) for a batch of (lo, hi) ranges over the same
      layers (C ABI vbf_store_scan_host): per range, in key order, every key of any layer inside the
      bounds that get_many finds, with get_many's answer and value for it.

validate_size (an empty key is an error in the reference, store.rs:443) stays with the caller.
"""
import ctypes
from dataclasses import dataclass

import numpy as np

from ._lib import VBF_EINVAL, VBF_SCAN_END_EXCLUSIVE, VBF_SCAN_KEEP_TOMBSTONES, VbfError, check, lib
from .filter import _raise
from .keys import HostBatch, pack
from .memtable import _handles
from .vlog import Values


VALUE_GUESS = 48  # bytes of value per key the first call makes room for


@dataclass
class StoreGet:
    found: np.ndarray        # uint8: 0 nowhere, 1 live, 2 tombstone
    layer: np.ndarray        # uint32, see the module docstring
    table: np.ndarray        # uint32 index into `tables`, 0xFFFFFFFF when no table answered
    val_offsets: np.ndarray  # uint32
    created_ms: np.ndarray   # uint64
    values: Values

    def value(self, j):
        """What DataStore::get returns for key j: the value, or None (absent, deleted, no value in the log)."""
        return self.values.value(j)


def get_many(keys, tables, vlog, active=None, read_only=(), gc=None, filters=None, check_keys=False):
    """DataStore::get for every key."""
    b = keys if isinstance(keys, HostBatch) else pack(keys)
    n = b.n
    tables, th = _handles(tables)
    nsst = len(tables)
    fh = None
    if filters is not None:
        filters, fh = _handles(filters)
        if len(filters) != nsst:
            raise ValueError("one filter per table")
    ro, rh = _handles(read_only)
    found, layer, tidx = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    vo, cr = np.zeros(n, np.uint32), np.zeros(n, np.uint64)
    vals = Values(np.zeros(n, np.uint8), None, np.zeros(n + 1, np.uint64))
    d, o = b.ptrs()
    vp = lambda x: x.ctypes.data if x.size else None
    h = lambda t: t._h if t is not None else None
    head = (d, o, b.stride, n, h(gc), h(active), len(ro), rh, nsst, th, fh, h(vlog), int(bool(check_keys)))
    nb = ctypes.c_uint64()
    # one call when the values fit the first guess (VALUE_GUESS bytes per key); otherwise the call
    # reports the size and touches no array, and a second call gets exactly that much
    cap = max(4096, VALUE_GUESS * n)
    for _ in range(2):
        vals.values = np.empty(cap, np.uint8)
        rc = lib.vbf_store_get_host(*head, vp(found), vp(layer), vp(tidx), vp(vo), vp(cr), vp(vals.status),
                                    vals.values.ctypes.data, cap, vals.value_off.ctypes.data, ctypes.byref(nb))
        if rc != VBF_EINVAL or nb.value <= cap:
            break
        cap = nb.value
    try:
        check("vbf_store_get_host", rc)
    except VbfError as e:
        _raise("store_get", e)
    vals.values = vals.values[:nb.value]
    return StoreGet(found, layer, tidx, vo, cr, vals)


ENTRY_GUESS = 64  # listed entries per range the first call makes room for
KEY_GUESS = 32    # bytes of key per listed entry


@dataclass
class StoreScan:
    range_off: np.ndarray    # uint64 [nranges + 1]: range r lists outputs range_off[r] .. range_off[r+1]
    keys: np.ndarray         # uint8: the listed keys back to back
    key_off: np.ndarray      # uint64 [n + 1]: key i = keys[key_off[i] .. key_off[i+1])
    tombstones: np.ndarray   # uint8: 1 only with keep_tombstones
    layer: np.ndarray        # uint32, as StoreGet.layer
    table: np.ndarray        # uint32 index into `tables`, 0xFFFFFFFF when a memtable answered
    val_offsets: np.ndarray  # uint32
    created_ms: np.ndarray   # uint64
    values: Values           # over the listed entries (SKIPPED for a listed tombstone)

    def range(self, r):
        """(key bytes, value or None) for every entry of range r, in key order: what get_many returns
        for that key (None: deleted, or no value in the log)."""
        kb = self.keys.tobytes()
        for i in range(int(self.range_off[r]), int(self.range_off[r + 1])):
            yield kb[int(self.key_off[i]):int(self.key_off[i + 1])], self.values.value(i)


def scan_many(ranges, tables, vlog, active=None, read_only=(), gc=None, keep_tombstones=False, end_exclusive=False,
              check_keys=False, capacities=None):
    """DataStore::seek for every (lo, hi) of `ranges` (bytes, both ends inclusive unless
    end_exclusive): the keys of any layer inside the bounds that get_many over the same layers finds,
    ascending, with get_many's answer and value for each (C ABI vbf_store_scan_host).  capacities =
    (entries, key bytes, value bytes) replaces the first call's guess, for a caller that knows the
    answer's sizes; a first call that is too small costs the whole device pass a second time."""
    ranges = [(bytes(lo), bytes(hi)) for lo, hi in ranges]
    nr = len(ranges)
    tables, th = _handles(tables)
    ro, rh = _handles(read_only)
    flat = [b for pair in ranges for b in pair]
    bounds = np.frombuffer(b"".join(flat) + b"\0", np.uint8)  # never NULL
    boff = np.concatenate([[0], np.cumsum([len(b) for b in flat], dtype=np.uint64)]).astype(np.uint64)
    flags = (VBF_SCAN_KEEP_TOMBSTONES if keep_tombstones else 0) | (VBF_SCAN_END_EXCLUSIVE if end_exclusive else 0)
    h = lambda t: t._h if t is not None else None
    head = (bounds.ctypes.data, boff.ctypes.data, nr, h(gc), h(active), len(ro), rh, len(tables), th, h(vlog), flags,
            int(bool(check_keys)))
    n, kb, vb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    # one call when the answer fits the first guess; otherwise the call reports the three sizes and
    # touches no array, and a second call gets exactly that much
    ecap = max(256, ENTRY_GUESS * nr)
    kcap, vcap = KEY_GUESS * ecap, VALUE_GUESS * ecap
    if capacities is not None:
        ecap, kcap, vcap = (max(int(c), 1) for c in capacities)
    roff = np.zeros(nr + 1, np.uint64)
    for _ in range(2):
        keys, koff, tomb = np.empty(kcap, np.uint8), np.zeros(ecap + 1, np.uint64), np.zeros(ecap, np.uint8)
        layer, tidx, vo = np.zeros(ecap, np.uint32), np.zeros(ecap, np.uint32), np.zeros(ecap, np.uint32)
        cr, status, voff = np.zeros(ecap, np.uint64), np.zeros(ecap, np.uint8), np.zeros(ecap + 1, np.uint64)
        values = np.empty(vcap, np.uint8)
        rc = lib.vbf_store_scan_host(*head, roff.ctypes.data, keys.ctypes.data, kcap, koff.ctypes.data, tomb.ctypes.data,
                                     layer.ctypes.data, tidx.ctypes.data, vo.ctypes.data, cr.ctypes.data,
                                     status.ctypes.data, ecap, values.ctypes.data, vcap, voff.ctypes.data,
                                     ctypes.byref(n), ctypes.byref(kb), ctypes.byref(vb))
        if rc != VBF_EINVAL or (n.value <= ecap and kb.value <= kcap and vb.value <= vcap):
            break
        ecap, kcap, vcap = max(n.value, 1), max(kb.value, 1), max(vb.value, 1)
    try:
        check("vbf_store_scan_host", rc)
    except VbfError as e:
        _raise("store_scan", e)
    m = n.value
    return StoreScan(roff, keys[:kb.value], koff[:m + 1], tomb[:m], layer[:m], tidx[:m], vo[:m], cr[:m],
                     Values(status[:m], values[:vb.value], voff[:m + 1]))
