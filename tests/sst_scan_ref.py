"""The checker for the range scans (vbf_table_scan_*), built on the lookup checker.

A scan has no semantics of its own: for a range [lo, hi] and tables in the caller's order it lists,
in ascending key order, every distinct key of any table inside the bounds for which the point lookup
(sst_get_ref.search, the reference's fold restated) finds a winner, with that winner's fields.

  keys inside the bounds   collected from the parsed files with Python's bytes comparison (= Rust's
                           `Ord for [u8]`): lo <= k <= hi, or lo <= k < hi with END_EXCLUSIVE
  per key                  ref.search(key, tables): found 0 -> not listed; found 2 (the winner is a
                           tombstone) -> listed with tombstone = 1 only with KEEP_TOMBSTONES

`scan` is the statement.  `scan_many` answers the same for a batch from one sorted list of all the
tables' keys, cut at the bounds by bisection (the same bytes comparison), and looks every key up
once; tests/test_sst_scan_ref.py holds the two to the same answers.  The product never imports this
module.
"""
import bisect

import numpy as np

import sst_get_ref as ref

KEEP_TOMBSTONES, END_EXCLUSIVE = 1, 2


def parse(tables):
    return [t if isinstance(t, ref.Sst) else ref.Sst(*t) for t in tables]


def scan(lo, hi, tables, flags=0):
    """[(key, table_idx, val_offset, created_ms, tombstone)] in ascending key order."""
    tables = parse(tables)
    inside = set()
    for t in tables:
        for k in t.starts:
            if lo <= k and (k < hi if flags & END_EXCLUSIVE else k <= hi):
                inside.add(k)
    out = []
    for k in sorted(inside):
        found, who, val, created = ref.search(k, tables)
        if found == 0 or (found == 2 and not flags & KEEP_TOMBSTONES):
            continue
        out.append((k, who, val, created, 1 if found == 2 else 0))
    return out


def scan_many(ranges, tables, flags=0):
    """The arrays vbf_table_scan_* fills for `ranges` = [(lo, hi), ...]:
    (range_off u64, keys u8, key_off u64, table u32, val_offsets u32, created_ms u64, tombstones u8)."""
    tables = parse(tables)
    union = sorted(set().union(*[t.starts.keys() for t in tables])) if tables else []
    memo = {}  # the lookup of a key does not depend on the range
    rows, range_off = [], [0]
    for lo, hi in ranges:
        first = bisect.bisect_left(union, lo)
        end = bisect.bisect_left(union, hi) if flags & END_EXCLUSIVE else bisect.bisect_right(union, hi)
        for k in union[first:end]:
            if k not in memo:
                memo[k] = ref.search(k, tables)
            found, who, val, created = memo[k]
            if found == 0 or (found == 2 and not flags & KEEP_TOMBSTONES):
                continue
            rows.append((k, who, val, created, 1 if found == 2 else 0))
        range_off.append(len(rows))
    key_off = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.uint64)
    return (np.asarray(range_off, np.uint64), np.frombuffer(b"".join(r[0] for r in rows), np.uint8), key_off,
            np.asarray([r[1] for r in rows], np.uint32), np.asarray([r[2] for r in rows], np.uint32),
            np.asarray([r[3] for r in rows], np.uint64), np.asarray([r[4] for r in rows], np.uint8))
