"""Pins the walk's checker (tests/vlog_walk_ref.py) to the reference's value-log fixture, and its
gc_handler restatement to a hand-made chunk (no GPU needed)."""
import os
import struct

import vlog_ref as vr
import vlog_walk_ref as wr
from conftest import GOLDEN


def fixture_log():
    with open(os.path.join(GOLDEN, "vlog_fixture", "val_log_prefix.bin"), "rb") as f:
        return f.read()


def test_fixture_from_the_start():
    log = fixture_log()
    entries, end, stop = wr.walk(log)
    assert (len(entries), end, stop) == (2844, 76784, wr.END) and len(log) == 76784
    assert [e[1] for e in entries[:2]] == [b"tail", b"head"]
    # the same entries as the get checker's parse
    assert [(e[0], e[1], e[2]) for e in entries] == [(o, k, v) for o, k, v, _, _ in vr.parse(log)]


def test_fixture_budgets():
    log = fixture_log()
    entries, end, stop = wr.walk(log, 25, 0)
    assert (len(entries), end, stop) == (1, 50, wr.BUDGET)
    entries, end, stop = wr.walk(log, 0, 4096)
    assert (len(entries), end, stop) == (152, 4100, wr.BUDGET)
    entries, end, stop = wr.walk(log, 0, 4101)  # one byte more than was read: one entry more
    assert len(entries) == 153 and stop == wr.BUDGET


def test_fixture_last_entry():
    log = fixture_log()
    entries, end, stop = wr.walk(log, 76757)
    assert [(e[1], e[2]) for e in entries] == [(b"mYjgx", b"6YLW8")] and (end, stop) == (76784, wr.END)
    assert wr.walk(log, 76784) == ([], 76784, wr.END)
    # the budget met by the entry that also ends the log: the budget's return comes first (fs/mod.rs:646-649)
    assert wr.walk(log, 76757, 27)[2] == wr.BUDGET and wr.walk(log, 76757, 28)[2] == wr.END


def test_torn_and_window():
    log, offs = vr.encode([(b"a", b"xy", 5, 0), (b"", b"", 6, 1), (b"bcd", b"z" * 40, 7, 2)], base=1000)
    whole = wr.walk(log, 1000, base=1000)
    assert [e[0] for e in whole[0]] == offs and whole[1:] == (1000 + len(log), wr.END)
    assert [e[4] for e in whole[0]] == [0, 1, 1]  # the encoder writes a tombstone != 0 as 1
    assert wr.walk(log[:-60], 1000, base=1000)[1:] == (offs[2], wr.END)  # cut at the entry's first byte: no tear
    for cut in (1, 40, 41, 43, 44, 59):  # inside the value, the key and the header of the last entry
        got = wr.walk(log[:-cut], 1000, base=1000)
        assert [e[0] for e in got[0]] == offs[:2] and got[1:] == (offs[2], wr.TORN)
    huge = struct.pack("<IIQB", 0xFFFFFFFF, 0xFFFFFFFF, 1, 0) + b"abc"
    got = wr.walk(log + huge, 1000, base=1000)
    assert len(got[0]) == 3 and got[1:] == (1000 + len(log), wr.TORN)
    arr = wr.arrays(*whole[:2])
    assert arr[0].tolist() == offs + [1000 + len(log)] and arr[3].tolist() == [0, 1, 1, 4] and arr[5].tolist() == [0, 2, 2, 42]


def test_gc_handler_restatement():
    T = 1000
    chunk = [(b"live", b"v1", T, 0), (b"old", b"v-old", T, 0), (b"gone", b"g", T, 0), (b"none", b"n", T, 0),
             (b"star", b"s", T, 0), (b"empty", b"e", T, 0)]
    log, offs = vr.encode(chunk, base=0)
    db = {b"live": (b"v1-new", T), b"old": (b"v-new", T + 1), b"gone": None, b"star": (b"*", T), b"empty": (b"", T)}
    got = wr.gc_handler(log, 0, 0, len(log), 5000, 77, lambda k: db.get(k))
    assert got["invalid"] == [1, 2, 3, 4] and got["total_bytes_read"] == len(log) and got["new_tail"] == len(log)
    assert got["append"] == [(b"tail", struct.pack("<Q", len(log)), 77, 0), (b"live", b"v1-new", 77, 0), (b"empty", b"", 77, 0)]
    assert got["puts"] == [(b"tail", 5000, 77, 0), (b"live", 5000 + 29, 77, 0), (b"empty", 5000 + 29 + 27, 77, 1)]
    # a chunk without an invalid entry produces nothing
    assert wr.gc_handler(log, 0, 0, 1, 5000, 77, lambda k: db.get(k)) is None
