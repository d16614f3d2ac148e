"""The checker for the table lookups: velarixdb's read path restated over file bytes, scan for scan.

Written from the file formats (entry = u32 key_len | key | u32 value offset | u64 created_at ms | u8
tombstone; index record = u32 key_len | key | u32 block offset) and the behaviour of the three
steps, not for speed:

  get_from_index   scans index.db from its start for the first record whose key is >= the searched
                   key and returns that record's offset.  Its `block_offset` variable starts at -1
                   and is never reassigned, so reaching the end of the file yields None.
  find_entry       scans data.db from that offset TO THE END OF THE FILE, entry by entry, for a key
                   equal to the searched one (no ordering test, no stop at the block's end);
                   tombstone = (byte == 1).
  search           the fold of search_key_in_sstables: the winner starts at time 0 and a hit
                   replaces it only when its created_at is strictly greater; a winner still at time
                   0 counts as not found.

A zero-length key is an ordinary key here (the format allows it).  The product never imports this
module.

The three functions above are the statement.  `Sst` answers the same two questions from one parse
of the files, for tests that ask tens of thousands of them: the first index record with key >=
the searched one by bisection when the index keys are nondecreasing (checked; otherwise the scan),
and the first entry at or after `offset` with an equal key from a map key -> entry starts when
`offset` is an entry start (checked; otherwise the scan).  tests/test_sst_get_ref.py holds the two
to the same answers.
"""
import bisect
import struct

import numpy as np

NO_TABLE = 0xFFFFFFFF


def _u32(b, p):
    return struct.unpack_from("<I", b, p)[0]


def get_from_index(index, key):
    block_offset = -1  # never reassigned
    p = 0
    while True:
        if p >= len(index):  # nothing left to read
            if block_offset == -1:
                return None
            return block_offset
        klen = _u32(index, p)
        k = index[p + 4:p + 4 + klen]
        offset = _u32(index, p + 4 + klen)
        p += klen + 8
        if k < key:
            continue
        return offset


def find_entry(data, offset, key):
    p = offset
    while True:
        if p >= len(data):
            return None
        klen = _u32(data, p)
        k = data[p + 4:p + 4 + klen]
        val = _u32(data, p + 4 + klen)
        created = struct.unpack_from("<Q", data, p + 8 + klen)[0]
        tomb = data[p + 16 + klen] == 1
        p += klen + 17
        if k == key:
            return val, created, tomb


def table_get(data, index, key):
    """Index::get then Table::get on one SST: (val_offset, created_ms, tombstone) or None."""
    off = get_from_index(index, key)
    if off is None:
        return None
    return find_entry(data, off, key)


class Sst:
    """One SST's two files, parsed once (see the module docstring)."""

    def __init__(self, data, index):
        self.data, self.index = bytes(data), bytes(index)
        self.ikeys, self.ioffs = [], []
        p = 0
        while p < len(self.index):
            klen = _u32(self.index, p)
            self.ikeys.append(self.index[p + 4:p + 4 + klen])
            self.ioffs.append(_u32(self.index, p + 4 + klen))
            p += klen + 8
        self.index_sorted = all(a <= b for a, b in zip(self.ikeys, self.ikeys[1:]))
        self.starts, self.fields = {}, {}
        p = 0
        while p < len(self.data):
            klen = _u32(self.data, p)
            k = self.data[p + 4:p + 4 + klen]
            self.starts.setdefault(k, []).append(p)
            self.fields[p] = (_u32(self.data, p + 4 + klen), struct.unpack_from("<Q", self.data, p + 8 + klen)[0],
                              self.data[p + 16 + klen] == 1)
            p += klen + 17

    def get_from_index(self, key):
        if not self.index_sorted:
            return get_from_index(self.index, key)
        i = bisect.bisect_left(self.ikeys, key)
        return self.ioffs[i] if i < len(self.ikeys) else None

    def find_entry(self, offset, key):
        if offset not in self.fields:
            return find_entry(self.data, offset, key)
        at = self.starts.get(key, ())
        i = bisect.bisect_left(at, offset)
        return self.fields[at[i]] if i < len(at) else None

    def get(self, key):
        off = self.get_from_index(key)
        return None if off is None else self.find_entry(off, key)


def search(key, tables, allowed=None):
    """tables: [Sst or (data bytes, index bytes), ...] in order; allowed: per-table booleans or None.
    -> (found, table_idx, val_offset, created_ms) as vbf_table_get_* reports them."""
    insert_time, offset, deleted, who = 0, 0, False, NO_TABLE
    for t, tab in enumerate(tables):
        if allowed is not None and not allowed[t]:
            continue
        r = tab.get(key) if isinstance(tab, Sst) else table_get(tab[0], tab[1], key)
        if r is not None:
            val, created, tomb = r
            if created > insert_time:
                offset, insert_time, deleted, who = val, created, tomb, t
    if insert_time > 0:
        return (2 if deleted else 1), who, offset, insert_time
    return 0, NO_TABLE, 0, 0


def search_many(keys, tables, allowed=None):
    """Four numpy arrays (found u8, table u32, val_offsets u32, created_ms u64) for a list of keys;
    allowed: [n][nsst] or None."""
    tables = [t if isinstance(t, Sst) else Sst(*t) for t in tables]
    n = len(keys)
    found, who = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    val, created = np.zeros(n, np.uint32), np.zeros(n, np.uint64)
    for j, k in enumerate(keys):
        found[j], who[j], val[j], created[j] = search(bytes(k), tables, None if allowed is None else allowed[j])
    return found, who, val, created
