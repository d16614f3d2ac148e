"""The value-log checker (tests/vlog_ref.py) against the reference's own fixture: the first 76 784
bytes of src/tests/fixtures/data/v_log/val_log.bin, the log the SST fixtures point into.  No GPU."""
import hashlib
import json
import os
import struct

import sst_get_ref as ref
import vlog_ref as vr
from conftest import GOLDEN

DIR = os.path.join(GOLDEN, "vlog_fixture")
SST1 = os.path.join(GOLDEN, "sst_fixtures", "sstable_1720785462309")


def prefix():
    with open(os.path.join(DIR, "val_log_prefix.bin"), "rb") as f:
        return f.read()


def meta():
    with open(os.path.join(DIR, "val_log_prefix.json")) as f:
        return json.load(f)


def sst1():
    with open(os.path.join(SST1, "data.db"), "rb") as f:
        data = f.read()
    with open(os.path.join(SST1, "index.db"), "rb") as f:
        return ref.Sst(data, f.read())


def test_prefix_is_whole_entries():
    log, m = prefix(), meta()
    assert len(log) == m["bytes"] == 76784
    assert hashlib.sha256(log).hexdigest() == m["sha256"]
    entries = vr.parse(log)  # asserts that the last entry ends exactly at the end
    assert len(entries) == m["entries"]
    last = entries[-1]
    assert last[0] + vr.HEADER + len(last[1]) + len(last[2]) == 76784


def test_sst1_points_into_the_prefix():
    log, m, s = prefix(), meta(), sst1()
    assert len(s.fields) == 2844
    at = {e[0]: e for e in vr.parse(log)}
    odd = []
    for key, starts in s.starts.items():
        val_off, created, _ = s.fields[starts[0]]
        off, k, v, c, _ = at[val_off]  # every offset is an entry start
        if (k, c) != (key, created):
            odd.append((key, val_off, k, v))
    q = m["head_quirk"]
    assert odd == [(q["sst_key"].encode(), q["val_offset"], q["log_key"].encode(), q["log_value"].encode())]
    assert odd[0] == (b"head", 76757, b"mYjgx", b"6YLW8")
    assert vr.get(log, 76757) == (vr.VALUE, b"6YLW8")
    assert vr.get(log, 76757, key=b"head") == (vr.KEY_MISMATCH, None)
    assert vr.get(log, 76757, key=b"mYjgx") == (vr.VALUE, b"6YLW8")


def test_encode_inverts_parse():
    log = prefix()
    entries = vr.parse(log)
    out, offs = vr.encode([(k, v, c, t) for _, k, v, c, t in entries])
    assert out == log and offs == [e[0] for e in entries]
    out, offs = vr.encode([(k, v, c, t) for _, k, v, c, t in entries[:50]], base=1000)
    assert offs == [e[0] + 1000 for e in entries[:50]] and out == log[:len(out)]
    assert [e[0] for e in vr.parse(out, base=1000)] == offs


def test_the_six_statuses():
    log, offs = vr.encode([(b"k1", b"value-1", 5, 0), (b"", b"", 6, 0), (b"k3", b"gone", 7, 1), (b"k4", b"x", 8, 0)],
                          base=100)
    log = bytearray(log)
    log[offs[3] - 100 + 16] = 2  # the encoder writes 0 or 1
    log = bytes(log)
    end = 100 + len(log)
    assert vr.get(log, offs[0], 100) == (vr.VALUE, b"value-1")
    assert vr.get(log, offs[1], 100) == (vr.VALUE, b"")        # an empty value is a value
    assert vr.get(log, offs[2], 100) == (vr.TOMBSTONE, None)
    assert vr.get(log, offs[3], 100) == (vr.VALUE, b"x")       # only byte == 1 is a tombstone
    assert vr.get(log, offs[0], 100, found=0) == (vr.SKIPPED, None)
    assert vr.get(log, offs[0], 100, found=2) == (vr.SKIPPED, None)
    assert vr.get(log, end, 100) == (vr.NONE, None) and vr.get(log, 0xFFFFFFFF, 100) == (vr.NONE, None)
    assert vr.get(log, end - 1, 100) == (vr.BAD, None) and vr.get(log, 99, 100) == (vr.BAD, None)
    assert vr.get(log, offs[0], 100, key=b"k2") == (vr.KEY_MISMATCH, None)
    assert vr.get(log, offs[2], 100, key=b"k") == (vr.KEY_MISMATCH, None)   # before the tombstone
    huge = struct.pack("<IIQB", 0xFFFFFFFF, 0xFFFFFFFF, 0, 0) + b"\0" * 40
    assert vr.get(huge, 0) == (vr.BAD, None)
    st, vals, voff = vr.get_many(log, [offs[0], offs[2], offs[0], end], 100)
    assert st.tolist() == [1, 2, 1, 3] and voff.tolist() == [0, 7, 7, 14, 14] and vals.tobytes() == b"value-1" * 2
