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

validate_size (an empty key is an error in the reference, store.rs:443) stays with the caller.
"""
import ctypes
from dataclasses import dataclass

import numpy as np

from ._lib import VBF_EINVAL, VbfError, check, lib
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
