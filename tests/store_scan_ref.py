"""The checker for the whole-store range scan (vbf_store_scan_host), built on the get checker.

A scan has no semantics of its own: for a range [lo, hi] over a store_get_ref.Store it lists, in
ascending key order, every distinct key of any layer (the gc entries, the active memtable, the
read-only memtables, the SSTs) inside the bounds for which Store.get finds something, with that
get's answer.

  keys inside the bounds   collected from every layer with Python's bytes comparison (= Rust's
                           `Ord for [u8]`): lo <= k <= hi, or lo <= k < hi with END_EXCLUSIVE
  per key                  Store.get(key): found 0 -> not listed; found 2 -> listed with tombstone = 1
                           only with KEEP_TOMBSTONES; the listed entry carries the get's layer, table,
                           val_offset, created_ms, status and value

`scan` is the statement.  `scan_many` answers the same for a batch from one sorted union of the
layers' keys, cut at the bounds by bisection (the same bytes comparison), and gets every key once;
tests/test_store_scan_ref.py holds the two to the same answers.  The product never imports this
module.
"""
import bisect

import numpy as np

import vlog_ref as vr

KEEP_TOMBSTONES, END_EXCLUSIVE = 1, 2
FIELDS = ("range_off", "keys", "key_off", "tombstones", "layer", "table", "val_offsets", "created_ms", "status",
          "values", "value_off")


def layers(store):
    """The key sets of every layer, in DataStore::get's order."""
    mems = [store.gc or {}, store.active or {}] + [t or {} for t in store.read_only]
    return [set(m) for m in mems] + [set(t.starts) for t in store.tables]


def union(store):
    return sorted(set().union(*layers(store)))


def listed(got, flags):
    return got.found == 1 or (got.found == 2 and bool(flags & KEEP_TOMBSTONES))


def scan(store, lo, hi, flags=0, check_keys=False):
    """[(key, Got)] in ascending key order."""
    inside = set()
    for keys in layers(store):
        for k in keys:
            if lo <= k and (k < hi if flags & END_EXCLUSIVE else k <= hi):
                inside.add(k)
    out = []
    for k in sorted(inside):
        g = store.get(k, check_key=check_keys)
        if listed(g, flags):
            out.append((k, g))
    return out


def cut(keys, lo, hi, flags):
    """The slice of the sorted list `keys` inside the bounds."""
    first = bisect.bisect_left(keys, lo)
    end = bisect.bisect_left(keys, hi) if flags & END_EXCLUSIVE else bisect.bisect_right(keys, hi)
    return first, max(first, end)


def scan_many(store, ranges, flags=0, check_keys=False, memo=None):
    """The arrays vbf_store_scan_host fills for `ranges` = [(lo, hi), ...], by name (FIELDS).  memo: a
    dict key -> Got kept between calls over one store and one check_keys (the get of a key does not
    depend on the range or the flags)."""
    keys = union(store)
    memo = {} if memo is None else memo
    rows, range_off = [], [0]
    for lo, hi in ranges:
        first, end = cut(keys, lo, hi, flags)
        for k in keys[first:end]:
            if k not in memo:
                memo[k] = store.get(k, check_key=check_keys)
            if listed(memo[k], flags):
                rows.append((k, memo[k]))
        range_off.append(len(rows))
    lens = [len(g.value) if g.status == vr.VALUE else 0 for _, g in rows]
    return {
        "range_off": np.asarray(range_off, np.uint64),
        "keys": np.frombuffer(b"".join(k for k, _ in rows), np.uint8).copy(),
        "key_off": np.concatenate([[0], np.cumsum([len(k) for k, _ in rows])]).astype(np.uint64),
        "tombstones": np.asarray([g.found == 2 for _, g in rows], np.uint8),
        "layer": np.asarray([g.layer for _, g in rows], np.uint32),
        "table": np.asarray([g.table for _, g in rows], np.uint32),
        "val_offsets": np.asarray([g.val_offset for _, g in rows], np.uint32),
        "created_ms": np.asarray([g.created_ms for _, g in rows], np.uint64),
        "status": np.asarray([g.status for _, g in rows], np.uint8),
        "values": np.frombuffer(b"".join(g.value for _, g in rows if g.status == vr.VALUE), np.uint8).copy(),
        "value_off": np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64),
    }
