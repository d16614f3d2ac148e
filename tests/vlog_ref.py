"""The checker for the value-log reads and appends: velarixdb's ValueLog restated over file bytes.

Written from the entry format (v_log.rs:291-309, little-endian, no padding, no index)

    u32 key_len | u32 val_len | u64 created_at ms | u8 tombstone | key | value

and from what VLogFileNode::get (fs/mod.rs:470-518) does with an offset: nothing at or past the end
of the file, otherwise one 17-byte header, the key skipped, the value returned; get_value_from_vlog
(db/store.rs:628-641) turns a tombstone (byte == 1) into nothing.  `log` holds the file's bytes
[base, base + len(log)): the tail the GC left.  Two readings of the library's, stated in vbf.h: a
zero-length value (or key) is an ordinary one, and an entry whose header or body runs past the end
is BAD, never a short value.  The product never imports this module.
"""
import struct

import numpy as np

SKIPPED, VALUE, TOMBSTONE, NONE, BAD, KEY_MISMATCH = 0, 1, 2, 3, 4, 5
HEADER = 17


def parse(log, base=0):
    """-> [(offset, key, value, created_at, tombstone byte)] for a log made of whole entries;
    AssertionError when the last entry does not end exactly at the end."""
    log = bytes(log)
    out, p = [], 0
    while p < len(log):
        assert p + HEADER <= len(log), "header of the entry at %d crosses the end" % (base + p)
        kl, vl, created, tomb = struct.unpack_from("<IIQB", log, p)
        assert p + HEADER + kl + vl <= len(log), "body of the entry at %d crosses the end" % (base + p)
        out.append((base + p, log[p + HEADER:p + HEADER + kl], log[p + HEADER + kl:p + HEADER + kl + vl], created, tomb))
        p += HEADER + kl + vl
    return out


def get(log, offset, base=0, key=None, found=1):
    """-> (status, value bytes or None) for one item, the six statuses of vbf_vlog_get_*."""
    if found != 1:
        return SKIPPED, None
    end = base + len(log)
    if offset >= end:
        return NONE, None
    if offset < base or offset + HEADER > end:
        return BAD, None
    p = offset - base
    kl, vl, _, tomb = struct.unpack_from("<IIQB", log, p)
    if offset + HEADER + kl + vl > end:  # Python integers: 0xFFFFFFFF + 0xFFFFFFFF does not wrap
        return BAD, None
    if key is not None and bytes(key) != bytes(log[p + HEADER:p + HEADER + kl]):
        return KEY_MISMATCH, None
    if tomb == 1:
        return TOMBSTONE, None
    return VALUE, bytes(log[p + HEADER + kl:p + HEADER + kl + vl])


def get_many(log, val_offsets, base=0, found=None, keys=None):
    """-> (status u8 [n], values u8, value_off u64 [n + 1]) as vbf_vlog_get_* fills them."""
    log = bytes(log)
    status, chunks, off = [], [], [0]
    for j, o in enumerate(val_offsets):
        st, v = get(log, int(o), base, None if keys is None else keys[j], 1 if found is None else int(found[j]))
        status.append(st)
        if v:
            chunks.append(v)
        off.append(off[-1] + (len(v) if v is not None else 0))
    return (np.array(status, np.uint8), np.frombuffer(b"".join(chunks), np.uint8).copy(),
            np.array(off, np.uint64))


def encode(entries, base=0):
    """entries: [(key, value, created_at, tombstone)] -> (log bytes, [offset of each entry]): what
    ValueLog::append writes when the file's size is `base`; a tombstone != 0 is written as 1."""
    out, offs, p = [], [], base
    for key, value, created, tomb in entries:
        offs.append(p)
        out.append(struct.pack("<IIQB", len(key), len(value), created & 0xFFFFFFFFFFFFFFFF, 1 if tomb else 0))
        out.append(bytes(key))
        out.append(bytes(value))
        p += HEADER + len(key) + len(value)
    return b"".join(out), offs
