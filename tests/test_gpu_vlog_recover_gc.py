"""GPU parity for the two users of the value-log walk: memtable.recover_puts (the data side of
recover_memtable, src/db/recovery.rs:245-286) and gc.collect (GC::gc_handler,
src/gc/garbage_collector.rs:168-262), against tests/vlog_walk_ref.py."""
import os

import numpy as np
import pytest

import scan_cases as sc
import sst_get_ref as ref
import vlog_ref as vr
import vlog_walk_ref as wr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
T0 = sc.T0


def fixture_log():
    with open(os.path.join(GOLDEN, "vlog_fixture", "val_log_prefix.bin"), "rb") as f:
        return f.read()


def test_recover_puts_then_flush(vbf):
    from velarixdb_amd import ValueLog, memtable
    log = fixture_log()
    entries, end, stop = wr.walk(log, 25)
    assert stop == wr.END and entries[0][1] == b"head"
    puts = entries[1:]  # the head entry is already in an SST (recovery.rs:261-264)
    with ValueLog.open(log) as vl:
        keys, vo, cr, tb = memtable.recover_puts(vl, 25)
        assert keys.n == len(puts) == 2842
        assert [memtable._key(keys, j) for j in range(keys.n)] == [e[1] for e in puts]
        assert vo.tolist() == [e[0] for e in puts] and cr.tolist() == [e[3] for e in puts]
        assert tb.tolist() == [e[4] for e in puts]
        got = memtable.flush(keys, vo, cr, tb)
        want = memtable.flush([e[1] for e in puts], [e[0] for e in puts], [e[3] for e in puts], [e[4] for e in puts])
        assert np.array_equal(got.data, want.data) and np.array_equal(got.index, want.index)
        assert np.array_equal(got.ids, want.ids) and (got.smallest, got.biggest) == (want.smallest, want.biggest)
        # from the last entry on only the head entry is left, from the end nothing: no puts
        for head in (76757, 76784):
            keys, vo, cr, tb = memtable.recover_puts(vl, head)
            assert (keys.n, vo.size, cr.size, tb.size) == (0, 0, 0, 0)
    # a crash mid-append: the torn entry is no put
    with ValueLog.open(log[:-3]) as vl:
        keys, vo, _, _ = memtable.recover_puts(vl, 25)
        assert keys.n == 2841 and vo.tolist() == [e[0] for e in puts[:-1]]


def lookup_over(log, base, ssts, overlay=None):
    """GC::get over Python objects: the overlay (steps 1 and 2), else the tables (step 3), then
    get_value_from_vlog; None is NotFoundInDB."""
    def lookup(key):
        if overlay and key in overlay:
            vo, created, tomb = overlay[key]
            found = 2 if tomb else 1
        else:
            found, _, vo, created = ref.search(key, ssts)
        if found != 1:
            return None
        st, v = vr.get(log, int(vo), base)
        assert st not in (vr.BAD, vr.KEY_MISMATCH)
        return (v, int(created)) if st == vr.VALUE else None
    return lookup


def same_gc(got, want, log_size, now_ms):
    if want is None:
        assert got is None
        return
    assert got is not None and got.invalid.tolist() == want["invalid"]
    assert (got.total_bytes_read, got.new_tail) == (want["total_bytes_read"], want["new_tail"])
    parsed = vr.parse(got.append, base=log_size)  # the bytes to append, read back by the checker
    assert [(k, v, c, t) for _, k, v, c, t in parsed] == want["append"]
    puts = list(zip(got.put_keys, got.put_val_offsets.tolist(), got.put_created_ms.tolist(), got.put_tombstones.tolist()))
    assert puts == want["puts"] and [o for o, *_ in parsed] == [p[1] for p in want["puts"]]
    assert all(c == now_ms for *_, c, _ in puts)


def test_gc_collect_over_the_fixture(vbf):
    from velarixdb_amd import Table, ValueLog, gc
    log = fixture_log()
    ssts = [ref.Sst(*sc.read_fixture(name)) for name in sc.NAMES]
    assert len(ssts) == 7
    now = T0 + 10**6
    tables = [Table.open_dir(os.path.join(sc.SST, name)) for name in sc.NAMES]
    try:
        with ValueLog.open(log) as vl:
            for tail, chunk in ((0, 20000), (25, 1), (50, 3000)):
                want = wr.gc_handler(log, 0, tail, chunk, len(log), now, lookup_over(log, 0, ssts))
                same_gc(gc.collect(vl, tables, tail, chunk, len(log), now), want, len(log), now)
    finally:
        for t in tables:
            t.close()


def test_gc_collect_every_branch(vbf, ora):
    from velarixdb_amd import Table, ValueLog, gc
    base = 300
    entries = [(b"a-live", b"value-a", T0, 0),           # 0 valid
               (b"b-over", b"old", T0, 0),               # 1 overwritten later: older than the table's entry
               (b"c-del", b"c", T0, 0),                  # 2 the winning table entry is a tombstone
               (b"d-none", b"d", T0, 0),                 # 3 in no table
               (b"e-star", b"*", T0, 0),                 # 4 the fetched value is "*"
               (b"f-ovl", b"f-old", T0, 0),              # 5 an overlay hit that points at a newer entry
               (b"g-ovl", b"g", T0, 0),                  # 6 an overlay hit on the entry itself: valid
               (b"h-ovl", b"h", T0, 0),                  # 7 an overlay tombstone
               (b"i-tomb", b"i", T0, 1),                 # 8 the table says live, the log's entry is a tombstone
               (b"j-past", b"j", T0, 0),                 # 9 the table points past the end of the log
               (b"k-empty", b"", T0, 0),                 # 10 valid with an empty value: a tombstone put
               (b"l-both", b"l", T0 + 3, 0),             # 11 two tables hold it, the newer one points here
               (b"b-over", b"new", T0 + 5, 0),           # 12 valid: the entry the table knows
               (b"f-ovl", b"f-new", T0 + 9, 0)]          # 13 valid through the overlay
    log, offs = vr.encode(entries, base)
    end = base + len(log)
    older = sorted([(b"a-live", offs[0], T0, 0), (b"b-over", offs[1], T0, 0), (b"c-del", offs[2], T0 - 5, 0),
                    (b"l-both", offs[3], T0 + 1, 0), (b"j-past", end + 40, T0, 0)])
    newer = sorted([(b"b-over", offs[12], T0 + 5, 0), (b"c-del", 0, T0 + 1, 1), (b"e-star", offs[4], T0, 0),
                    (b"i-tomb", offs[8], T0, 0), (b"k-empty", offs[10], T0, 0), (b"l-both", offs[11], T0 + 3, 0)])
    files = [sc.write(ora, older), sc.write(ora, newer)]
    ssts = [ref.Sst(*f) for f in files]
    overlay = {b"f-ovl": (offs[13], T0 + 9, 0), b"g-ovl": (offs[6], T0, 0), b"h-ovl": (offs[7], T0, 1)}
    now = T0 + 777
    tables = [Table.open(*f) for f in files]
    try:
        with ValueLog.open(log, base=base) as vl:
            want = wr.gc_handler(log, base, base, len(log), end, now, lookup_over(log, base, ssts, overlay))
            assert want["invalid"] == [1, 2, 3, 4, 5, 7, 8, 9]
            assert [k for k, *_ in want["append"]] == [b"tail", b"a-live", b"g-ovl", b"k-empty", b"l-both", b"b-over", b"f-ovl"]
            assert want["append"][5][1] == b"new" and want["puts"][3][3] == 1
            same_gc(gc.collect(vl, tables, base, len(log), end, now, overlay=overlay), want, end, now)
            # without the overlay the three overlay keys are in no table: invalid
            want = wr.gc_handler(log, base, base, len(log), end, now, lookup_over(log, base, ssts))
            assert want["invalid"] == [1, 2, 3, 4, 5, 6, 7, 8, 9, 13]
            same_gc(gc.collect(vl, tables, base, len(log), end, now), want, end, now)
            # a chunk that stops after its first entry, which is valid: nothing is produced
            assert wr.gc_handler(log, base, base, 1, end, now, lookup_over(log, base, ssts, overlay)) is None
            assert gc.collect(vl, tables, base, 1, end, now, overlay=overlay) is None
            # a chunk from the middle: entries 10.. are all valid
            assert gc.collect(vl, tables, offs[10], 10**6, end, now, overlay=overlay) is None
    finally:
        for t in tables:
            t.close()
