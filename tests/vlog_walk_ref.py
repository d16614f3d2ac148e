"""The checker for the walk of the value log and for the GC's handler: velarixdb restated over bytes.

walk() is VLogFileNode::recover (fs/mod.rs:520-577) and read_chunk_to_garbage_collect
(fs/mod.rs:579-651) as one literal serial loop: read an entry at p, go to p + 17 + key_len + val_len,
and after each whole entry test `bytes read >= budget` (:646-649).  `log` holds the file's bytes
[base, base + len(log)).  The library's reading of a torn tail (vbf.h): the entries before it are
returned, end_off is the torn entry's position and the stop is TORN.

gc_handler() is GC::gc_handler (gc/garbage_collector.rs:168-262) over Python dicts.  The product
never imports this module.
"""
import struct

import numpy as np

END, BUDGET, TORN = 0, 1, 2
HEADER = 17
UINT64_MAX = 2**64 - 1
TOMB_STONE_MARKER = b"*"
TAIL_ENTRY_KEY = b"tail"


def walk(log, start=0, budget=UINT64_MAX, base=0):
    """-> ([(offset, key, value, created_at as i64, tombstone byte == 1)], end_off, stop)"""
    log = bytes(log)
    end = base + len(log)
    assert base <= start <= end
    entries, p = [], start
    while True:
        if p == end:
            return entries, p, END
        q = p - base
        if q + HEADER > len(log):
            return entries, p, TORN
        kl, vl, created, tomb = struct.unpack_from("<IIqB", log, q)
        if q + HEADER + kl + vl > len(log):  # Python integers: no wrap
            return entries, p, TORN
        entries.append((p, log[q + HEADER:q + HEADER + kl], log[q + HEADER + kl:q + HEADER + kl + vl], created,
                        1 if tomb == 1 else 0))
        p += HEADER + kl + vl
        if p - start >= budget:
            return entries, p, BUDGET


def arrays(entries, end_off):
    """The walk's outputs as vbf_vlog_walk_* fills them:
    -> (entry_off u64 [n+1], val_offsets u32 [n], keys u8, key_off u64 [n+1], values u8, value_off u64 [n+1],
        created_ms i64 [n], tombstones u8 [n])"""
    cat = lambda parts: np.frombuffer(b"".join(parts), np.uint8).copy()
    cum = lambda parts: np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.uint64)
    offs = [e[0] for e in entries]
    keys, vals = [e[1] for e in entries], [e[2] for e in entries]
    return (np.array(offs + [end_off], np.uint64), np.array([o & 0xFFFFFFFF for o in offs], np.uint32), cat(keys),
            cum(keys), cat(vals), cum(vals), np.array([e[3] for e in entries], np.int64),
            np.array([e[4] for e in entries], np.uint8))


def gc_handler(log, base, tail, chunk_bytes, log_size, now_ms, lookup):
    """GC::gc_handler over one chunk.  lookup(key) is GC::get: -> (value, creation time ms) of the most
    recent entry, or None for the reference's NotFoundInDB.
    -> None when no entry is invalid (garbage_collector.rs:228-230), else a dict:
       invalid (ids in the chunk), total_bytes_read, new_tail, append (entries (key, value, created,
       tombstone) appended at log_size: the tail entry, then the valid ones in chunk order), puts
       ((key, val_offset, now_ms, tombstone) for the GC table)."""
    entries, end_off, _ = walk(log, tail, chunk_bytes, base)
    total = end_off - tail
    invalid, valid = [], []
    for i, (_, key, _, created, _) in enumerate(entries):
        got = lookup(key)
        if got is None:                                   # handle_deleted_entries: NotFoundInDB
            invalid.append(i)
        elif created < got[1] or got[0] == TOMB_STONE_MARKER:  # :205-208
            invalid.append(i)
        else:
            valid.append((key, got[0]))                   # :210, the most recent value
    if not invalid:
        return None
    new_tail = tail + total                               # :231
    append = [(TAIL_ENTRY_KEY, struct.pack("<Q", new_tail), now_ms, 0)]  # :232-238, write_tail_to_disk
    append += [(k, v, now_ms, 0) for k, v in valid]       # write_valid_entries_to_vlog: tombstone false
    offs, p = [], log_size
    for k, v, *_ in append:
        offs.append(p)
        p += HEADER + len(k) + len(v)
    puts = [(k, o, now_ms, 1 if len(v) == 0 else 0) for (k, v, *_), o in zip(append, offs)]  # GC::put :404-419
    return {"invalid": invalid, "total_bytes_read": total, "new_tail": new_tail, "append": append, "puts": puts}
