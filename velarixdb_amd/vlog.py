"""Batched value-log reads and appends on the GPU: the last step of a get, the first of a put.

velarixdb's value log (src/vlog/v_log.rs) is one file of entries laid back to back,

    u32 key_len | u32 val_len | u64 created_at ms | u8 tombstone | key | value

addressed by the file position of an entry's first byte -- the `val_offset` an SST entry carries.
ValueLog::get (v_log.rs:205-207, VLogFileNode::get, fs/mod.rs:470-518) seeks there and returns the
value; get_value_from_vlog (db/store.rs:628-641) turns a tombstone into None; ValueLog::append
(v_log.rs:173-196) writes an entry at the file's size and returns that position.  Here a window of
the log is opened once on the device and a batch of offsets is fetched in one call (C ABI
vbf_vlog_*, velarixdb_amd/csrc/vbf_vlog.hip).

  ValueLog.open(bytes, base=0)       -> ValueLog   the file's bytes [base, base + len), uploaded
  ValueLog.open_file(path, base=0)   -> ValueLog   the same from a file, read from `base` on
  vlog.get_many(val_offsets, found=None, keys=None) -> Values(status, values, value_off)
      status per item: SKIPPED (found[j] != 1), VALUE, TOMBSTONE, NONE (at or past the end), BAD
      (outside the window or cut by its end), KEY_MISMATCH (keys given and the entry holds another)
  ValueLog.encode(keys, values, created_ms=None, tombstones=None, base=0) -> (log bytes, val_offsets)
      what append writes for a batch of puts when the file's size is `base`
  vlog.walk(start=None, budget=None, values=True) -> Walk   the entries from `start` on, in file order
      (C ABI vbf_vlog_walk_*, velarixdb_amd/csrc/vbf_vlog_walk.hip); its two named uses:
  vlog.recover(head)            ValueLog::recover (fs/mod.rs:520-577)
  vlog.read_chunk(budget, tail) read_chunk_to_garbage_collect (fs/mod.rs:579-651)
"""
import ctypes
from dataclasses import dataclass

import numpy as np

from ._lib import (VBF_VLOG_BAD, VBF_VLOG_KEY_MISMATCH, VBF_VLOG_NONE, VBF_VLOG_SKIPPED, VBF_VLOG_TOMBSTONE,
                   VBF_VLOG_VALUE, VBF_WALK_BUDGET, VBF_WALK_END, VBF_WALK_TORN, VbfError, call, lib)
from .filter import _raise
from .keys import HostBatch, pack, pack_offsets
from .sst import _buf

SKIPPED, VALUE, TOMBSTONE, NONE, BAD, KEY_MISMATCH = (VBF_VLOG_SKIPPED, VBF_VLOG_VALUE, VBF_VLOG_TOMBSTONE,
                                                      VBF_VLOG_NONE, VBF_VLOG_BAD, VBF_VLOG_KEY_MISMATCH)


@dataclass
class Values:
    status: np.ndarray     # uint8 per item, the constants above
    values: np.ndarray     # uint8: the fetched values back to back, in item order
    value_off: np.ndarray  # uint64 [n + 1]: item j's value = values[value_off[j] .. value_off[j+1])

    def value(self, j):
        """The value of item j, or None when it has none (every status but VALUE)."""
        if self.status[j] != VALUE:
            return None
        return self.values[int(self.value_off[j]):int(self.value_off[j + 1])].tobytes()


WALK_END, WALK_BUDGET, WALK_TORN = VBF_WALK_END, VBF_WALK_BUDGET, VBF_WALK_TORN
_NO_BUDGET = 2**64 - 1


@dataclass
class Walk:
    entry_off: np.ndarray   # uint64 [n + 1]: the entries' file positions, then end_off
    keys: HostBatch         # the entries' keys, in file order
    values: np.ndarray      # uint8: the entries' own values back to back, or None (values=False)
    value_off: np.ndarray   # uint64 [n + 1]: entry i's value = values[value_off[i] .. value_off[i+1])
    created_ms: np.ndarray  # int64: the stored created_at
    tombstones: np.ndarray  # uint8: 1 iff the entry's byte is 1
    end_off: int            # where the walk stopped: the bytes read are end_off - start
    stop: int               # WALK_END, WALK_BUDGET or WALK_TORN (end_off is then the torn entry)

    @property
    def n(self):
        return self.created_ms.size

    @property
    def val_offsets(self):
        """entry_off[:n] as uint32: what memtable.flush and get_many take (ValueError at 2^32 or beyond)."""
        if self.n and int(self.entry_off[self.n - 1]) >= 2**32:
            raise ValueError("an entry lies at or beyond 2^32")
        return self.entry_off[:self.n].astype(np.uint32)

    def key(self, i):
        return self.keys.data[int(self.keys.offsets[i]):int(self.keys.offsets[i + 1])].tobytes()

    def value(self, i):
        return self.values[int(self.value_off[i]):int(self.value_off[i + 1])].tobytes()


def _key_ptrs(keys):
    """(batch, keys pointer -- never NULL, a NULL pointer means "no check" --, offsets pointer)"""
    b = keys if isinstance(keys, HostBatch) else pack(keys)
    data = b.data if b.data.size else np.zeros(1, np.uint8)
    return b, data, data.ctypes.data, (b.offsets.ctypes.data if b.offsets is not None else None)


class ValueLog:
    """A window of the value log resident on `device`."""

    def __init__(self, _handle):
        self._h = _handle

    @classmethod
    def open(cls, data, base=0, device=0):
        a, pa = _buf(data)
        h = ctypes.c_void_p()
        try:
            call("vbf_vlog_open_host", pa, a.size, int(base), int(device), ctypes.byref(h))
        except VbfError as e:
            _raise("vlog_open", e)
        return cls(h)

    @classmethod
    def open_file(cls, path, base=0, device=0):
        with open(path, "rb") as f:
            f.seek(int(base))
            return cls.open(f.read(), base=base, device=device)

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            lib.vbf_vlog_free(h)
        self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def nbytes(self):
        return lib.vbf_vlog_bytes(self._h)

    @property
    def base(self):
        return lib.vbf_vlog_base(self._h)

    @property
    def device(self):
        return lib.vbf_vlog_device(self._h)

    def get_many(self, val_offsets, found=None, keys=None):
        """ValueLog::get for every offset.  `found` (get_many's GetResult.found) restricts the fetch to
        its live items; `keys` makes every fetch check that the entry holds that key.  One size query,
        then one filling call."""
        vo = np.ascontiguousarray(val_offsets, dtype=np.uint32)
        n = vo.size
        fd = None if found is None else np.ascontiguousarray(found, dtype=np.uint8)
        if fd is not None and fd.size != n:
            raise ValueError("one found flag per offset")
        kp = op = None
        stride = 0
        if keys is not None:
            b, _keep, kp, op = _key_ptrs(keys)
            if b.n != n:
                raise ValueError("one key per offset")
            stride = b.stride
        vp = lambda x: x.ctypes.data if x is not None and x.size else None
        res = Values(np.zeros(n, np.uint8), None, np.zeros(n + 1, np.uint64))
        head = (self._h, vp(vo), vp(fd), n, kp, op, stride)
        nb = ctypes.c_uint64()
        try:
            call("vbf_vlog_get_host", *head, None, None, 0, None, ctypes.byref(nb))
            res.values = np.zeros(nb.value, np.uint8)
            call("vbf_vlog_get_host", *head, vp(res.status), vp(res.values), nb.value, res.value_off.ctypes.data,
                 ctypes.byref(nb))
        except VbfError as e:
            _raise("vlog_get", e)
        return res

    def walk(self, start=None, budget=None, values=True):
        """The entries from file position `start` (the window's base) on, in file order, until the end
        of the log, a torn entry, or the entry that brings the bytes read to `budget` or more (None:
        no budget).  values=False leaves the value bytes behind (value_off is still filled).  One size
        query, then one filling call."""
        start = self.base if start is None else int(start)
        budget = _NO_BUDGET if budget is None else int(budget)
        sc = [ctypes.c_uint64() for _ in range(4)]
        stop = ctypes.c_int()
        tail = [ctypes.byref(x) for x in sc] + [ctypes.byref(stop)]
        try:
            call("vbf_vlog_walk_host", self._h, start, budget, None, None, None, 0, None, None, 0, None, None, None, 0,
                 *tail)
            n, kb, vb = sc[0].value, sc[1].value, sc[2].value
            eo, ko, vo = (np.zeros(n + 1, np.uint64) for _ in range(3))
            kd, vd = np.zeros(kb, np.uint8), np.zeros(vb if values else 0, np.uint8)
            cr, tb = np.zeros(n, np.int64), np.zeros(n, np.uint8)
            vp = lambda x: x.ctypes.data if x.size else None
            call("vbf_vlog_walk_host", self._h, start, budget, vp(eo), None, vp(kd), kb, vp(ko), vp(vd), vd.size, vp(vo),
                 vp(cr), vp(tb), n, *tail)
        except VbfError as e:
            _raise("vlog_walk", e)
        return Walk(eo, pack_offsets(kd, ko), vd if values else None, vo, cr, tb, sc[3].value, stop.value)

    def recover(self, head):
        """ValueLog::recover(head) (fs/mod.rs:520-577): every entry from the head offset to the end."""
        return self.walk(start=head)

    def read_chunk(self, budget, tail):
        """read_chunk_to_garbage_collect(budget, tail) (fs/mod.rs:579-651): entries from the tail until
        at least `budget` bytes were read; the bytes read are walk.end_off - tail."""
        return self.walk(start=tail, budget=budget)

    @staticmethod
    def encode(keys, values, created_ms=None, tombstones=None, base=0, device=0):
        """ValueLog::append for a batch: -> (the bytes appended, uint32 val_offsets), entry j at
        base + the sizes of the entries before it."""
        b, _keep, kp, op = _key_ptrs(keys)
        values = [bytes(v) for v in values]
        n = b.n
        if len(values) != n:
            raise ValueError("one value per key")
        vals = np.frombuffer(b"".join(values) + b"\0", np.uint8)  # never NULL
        voff = np.concatenate([[0], np.cumsum([len(v) for v in values])]).astype(np.uint64)
        cr = None if created_ms is None else np.ascontiguousarray(created_ms, dtype=np.int64)
        tb = None if tombstones is None else np.ascontiguousarray(tombstones, dtype=np.uint8)
        if any(x is not None and x.size != n for x in (cr, tb)):
            raise ValueError("one created_ms / tombstone per key")
        vp = lambda x: x.ctypes.data if x is not None and x.size else None
        head = (kp, op, b.stride, n, vals.ctypes.data, voff.ctypes.data, vp(cr), vp(tb), int(base))
        ln = ctypes.c_uint64()
        try:
            call("vbf_vlog_encode_host", *head, None, 0, ctypes.byref(ln), None, int(device))
            out, vo = np.zeros(ln.value, np.uint8), np.zeros(n, np.uint32)
            call("vbf_vlog_encode_host", *head, vp(out), ln.value, ctypes.byref(ln), vp(vo), int(device))
        except VbfError as e:
            _raise("vlog_encode", e)
        return out.tobytes(), vo
