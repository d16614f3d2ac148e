"""GPU parity for vbf_gc_collect_host / gc.collect_device: GC::gc_handler over one chunk in one device
pass (src/gc/garbage_collector.rs:168-262), against tests/vlog_walk_ref.py::gc_handler and, byte for
byte, against gc.collect, the composition of the four host calls it fuses."""
import ctypes
import struct
import threading
import traceback

import numpy as np
import pytest

import scan_cases as sc
import sst_get_ref as ref
import vlog_ref as vr
import vlog_walk_ref as wr
from test_gpu_vlog_recover_gc import fixture_log, same_gc

pytestmark = pytest.mark.gpu
T0 = sc.T0
GUARD, PAD = 0xA5, 64
SCALARS = ("n_chunk", "n_invalid", "n_puts", "append_len", "end_off", "stop")
ARRAYS = (("verdict", np.uint8), ("append", np.uint8), ("put_ids", np.uint32), ("put_val_offsets", np.uint32),
          ("put_tombstones", np.uint8))


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


def same_bytes(got, want):
    """collect_device's result against gc.collect's, byte for byte."""
    if want is None:
        assert got is None
        return
    assert got is not None and got.append == want.append and got.put_keys == want.put_keys
    assert (got.total_bytes_read, got.new_tail) == (want.total_bytes_read, want.new_tail)
    for name in ("invalid", "put_val_offsets", "put_created_ms", "put_tombstones"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == w.dtype and np.array_equal(g, w), name
    assert got.verdict.dtype == np.uint8 and np.flatnonzero(got.verdict).tolist() == want.invalid.tolist()


class Raw:
    """One call of vbf_gc_collect_host with guard bytes around every output array."""

    def __init__(self, vl, tables, tail, chunk, log_size, now, filters=None, overlay=None, caps=None, only=None):
        from velarixdb_amd import gc
        from velarixdb_amd._lib import lib
        nsst = len(tables)
        th = (ctypes.c_void_p * max(nsst, 1))(*[t._h.value for t in tables])
        fh = (ctypes.c_void_p * max(nsst, 1))(*[f._h.value for f in filters]) if filters is not None else None
        ov_n, *ov = gc._pack_overlay(overlay)
        head = (vl._h, tail, chunk, log_size, now, nsst, th, fh)
        head += tuple(x.ctypes.data if x.size else None for x in ov) + (ov_n,) if ov_n else (None,) * 5 + (0,)
        sc_ = [ctypes.c_uint64(7) for _ in range(5)] + [ctypes.c_int(7)]
        tail_args = [ctypes.byref(x) for x in sc_]
        self.rc_query = lib.vbf_gc_collect_host(*head, None, 0, None, 0, None, None, None, 0, *tail_args)
        self.query = {n: x.value for n, x in zip(SCALARS, sc_)}
        self.msg_query = lib.vbf_last_error().decode()
        q = self.query
        size = dict(verdict=q["n_chunk"], append=q["append_len"], put_ids=q["n_puts"], put_val_offsets=q["n_puts"],
                    put_tombstones=q["n_puts"])
        size.update(caps or {})
        self.buf = {n: np.full(size[n] + 2 * PAD, GUARD, dt) for n, dt in ARRAYS}
        ptr = {n: (self.buf[n][PAD:].ctypes.data if only is None or n in only else None) for n, _ in ARRAYS}
        puts_cap = min(size["put_ids"], size["put_val_offsets"], size["put_tombstones"])
        for x in sc_:
            x.value = 7
        self.rc = lib.vbf_gc_collect_host(*head, ptr["verdict"], size["verdict"], ptr["append"], size["append"],
                                          ptr["put_ids"], ptr["put_val_offsets"], ptr["put_tombstones"], puts_cap,
                                          *tail_args)
        self.msg = lib.vbf_last_error().decode()
        self.scalars = {n: x.value for n, x in zip(SCALARS, sc_)}
        self.size = size

    def guards_intact(self):
        return all((b[:PAD] == GUARD).all() and (b[-PAD:] == GUARD).all() for b in self.buf.values())

    def untouched(self):
        return all((b == GUARD).all() for b in self.buf.values())

    def out(self, name):
        b = self.buf[name]
        return b[PAD:b.size - PAD]


def open_tables(files):
    from velarixdb_amd import Table
    return [Table.open(*f) for f in files]


def close_all(tables):
    for t in tables:
        t.close()


def check(vl, tables, log, base, ssts, tail, chunk, log_size, now, overlay=None, filters=None):
    """collect_device against the checker and against gc.collect -> (result, the checker's)"""
    from velarixdb_amd import gc
    want = wr.gc_handler(log, base, tail, chunk, log_size, now, lookup_over(log, base, ssts, overlay))
    got = gc.collect_device(vl, tables, tail, chunk, log_size, now, filters=filters, overlay=overlay)
    same_gc(got, want, log_size, now)
    same_bytes(got, gc.collect(vl, tables, tail, chunk, log_size, now, filters=filters, overlay=overlay))
    return got, want


# ---- 1. the reference's fixture log over its 7 SSTs ----

def test_fixture_log(vbf):
    from velarixdb_amd import Table, ValueLog
    import os
    log = fixture_log()
    ssts = [ref.Sst(*sc.read_fixture(name)) for name in sc.NAMES]
    now = T0 + 10**6
    tables = [Table.open_dir(os.path.join(sc.SST, name)) for name in sc.NAMES]
    try:
        with ValueLog.open(log) as vl:
            for tail, chunk in ((0, 20000), (25, 1), (50, 3000)):
                check(vl, tables, log, 0, ssts, tail, chunk, len(log), now)
    finally:
        close_all(tables)


# ---- 2. every branch ----

def branch_case(ora):
    base = 300
    entries = [(b"a-live", b"value-a", T0, 0), (b"b-over", b"old", T0, 0), (b"c-del", b"c", T0, 0),
               (b"d-none", b"d", T0, 0), (b"e-star", b"*", T0, 0), (b"f-ovl", b"f-old", T0, 0), (b"g-ovl", b"g", T0, 0),
               (b"h-ovl", b"h", T0, 0), (b"i-tomb", b"i", T0, 1), (b"j-past", b"j", T0, 0), (b"k-empty", b"", T0, 0),
               (b"l-both", b"l", T0 + 3, 0), (b"b-over", b"new", T0 + 5, 0), (b"f-ovl", b"f-new", T0 + 9, 0)]
    log, offs = vr.encode(entries, base)
    end = base + len(log)
    older = sorted([(b"a-live", offs[0], T0, 0), (b"b-over", offs[1], T0, 0), (b"c-del", offs[2], T0 - 5, 0),
                    (b"l-both", offs[3], T0 + 1, 0), (b"j-past", end + 40, T0, 0)])
    newer = sorted([(b"b-over", offs[12], T0 + 5, 0), (b"c-del", 0, T0 + 1, 1), (b"e-star", offs[4], T0, 0),
                    (b"i-tomb", offs[8], T0, 0), (b"k-empty", offs[10], T0, 0), (b"l-both", offs[11], T0 + 3, 0)])
    files = [sc.write(ora, older), sc.write(ora, newer)]
    overlay = {b"f-ovl": (offs[13], T0 + 9, 0), b"g-ovl": (offs[6], T0, 0), b"h-ovl": (offs[7], T0, 1)}
    return base, log, offs, files, overlay


def test_every_branch(vbf, ora):
    from velarixdb_amd import ValueLog, gc
    base, log, offs, files, overlay = branch_case(ora)
    ssts = [ref.Sst(*f) for f in files]
    end, now = base + len(log), T0 + 777
    tables = open_tables(files)
    try:
        with ValueLog.open(log, base=base) as vl:
            got, want = check(vl, tables, log, base, ssts, base, len(log), end, now, overlay=overlay)
            assert want["invalid"] == [1, 2, 3, 4, 5, 7, 8, 9]
            # entry 1 b-over and entry 5 f-ovl are OLDER: the table / the overlay knows a later put of the key
            assert got.verdict.tolist() == [0, 5, 2, 1, 6, 5, 0, 2, 4, 3, 0, 0, 0, 0]
            assert [k for k in got.put_keys] == [b"tail", b"a-live", b"g-ovl", b"k-empty", b"l-both", b"b-over", b"f-ovl"]
            assert got.put_tombstones.tolist() == [0, 0, 0, 1, 0, 0, 0]
            r = Raw(vl, tables, base, len(log), end, now, overlay=overlay)
            assert r.rc == 0 and r.out("put_ids").tolist() == [0xFFFFFFFF, 0, 6, 10, 11, 12, 13]
            got, want = check(vl, tables, log, base, ssts, base, len(log), end, now)
            assert want["invalid"] == [1, 2, 3, 4, 5, 6, 7, 8, 9, 13]
            assert got.verdict.tolist() == [0, 5, 2, 1, 6, 1, 1, 1, 4, 3, 0, 0, 0, 1]
            # nothing to collect: the one-entry chunk and the chunk from the middle
            for tail, chunk, n in ((base, 1, 1), (offs[10], 10**6, 4)):
                assert wr.gc_handler(log, base, tail, chunk, end, now, lookup_over(log, base, ssts, overlay)) is None
                assert gc.collect_device(vl, tables, tail, chunk, end, now, overlay=overlay) is None
                r = Raw(vl, tables, tail, chunk, end, now, overlay=overlay, caps=dict(append=8, put_ids=2, put_val_offsets=2,
                                                                                     put_tombstones=2))
                assert r.rc == 0 and r.guards_intact()
                assert (r.scalars["n_chunk"], r.scalars["n_invalid"], r.scalars["n_puts"], r.scalars["append_len"]) == (n, 0, 0, 0)
                assert r.out("verdict").tolist() == [0] * n  # verdict is still filled
                assert (r.out("append") == GUARD).all() and (r.out("put_ids") == GUARD).all()
    finally:
        close_all(tables)


# ---- 3. shapes at which the copy can go wrong ----

VAL_LENS = (0, 1, 15, 16, 17, 31, 32, 33, 16383, 16384, 16385, 40000)
KEY_LENS = (1, 7, 8, 9, 16, 17, 255, 4079)
NEG = -5


def shape_case(ora):
    """-> (base, log, offs, files, overlay, log_size): 19 entries at an odd base, appended at an odd size"""
    base = 4099
    rng = np.random.default_rng(0x6C)
    entries = []
    for i, vl in enumerate(VAL_LENS):
        key = bytes([65 + i]) + b"k" * (KEY_LENS[i % len(KEY_LENS)] - 1)
        value = bytes(rng.integers(97, 123, vl, dtype=np.uint8))  # letters: never "*"
        entries.append((key, value, T0 + i, 0))
    entries += [(b"star", b"*", T0, 0), (b"plus", b"+", T0, 0),
                (b"twin", b"first", T0 + 50, 0), (b"twin", b"second-value", T0 + 50, 0),
                (b"ow", b"short", T0 + 60, 0), (b"ow", b"n" * 300, T0 + 61, 0),
                (b"neg", b"negative-clock", NEG, 0)]
    log, offs = vr.encode(entries, base)
    items = {k: (o, c, 0) for (k, _, c, _), o in zip(entries, offs) if k != b"neg"}  # the later entry of a key wins
    files = [sc.write(ora, sorted((k, o, c, t) for k, (o, c, t) in items.items()))]
    overlay = {b"neg": (offs[18], NEG, 0)}
    return base, log, offs, files, overlay, (base + len(log) + 1000) | 1


def test_copy_shapes(vbf, ora):
    from velarixdb_amd import ValueLog
    base, log, offs, files, overlay, log_size = shape_case(ora)
    ssts = [ref.Sst(*f) for f in files]
    now = T0 + 10**5
    tables = open_tables(files)
    try:
        with ValueLog.open(log, base=base) as vl:
            got, want = check(vl, tables, log, base, ssts, base, 10**9, log_size, now, overlay=overlay)
            assert want["invalid"] == [12, 16] and len(got.verdict) == 19 and got.verdict[12] == 6 and got.verdict[16] == 5
            vals = {k: v for k, v, *_ in want["append"]}
            assert vals[b"twin"] == b"second-value" and [k for k, *_ in want["append"]].count(b"twin") == 2
            assert vals[b"ow"] == b"n" * 300 and vals[b"neg"] == b"negative-clock" and vals[b"plus"] == b"+"
            # a budget that ends one byte before an entry's end: that entry is still read
            twin_end = offs[15] - offs[12]
            got, want = check(vl, tables, log, base, ssts, offs[12], twin_end - 1, log_size, now, overlay=overlay)
            assert want["invalid"] == [0] and got.put_keys == [b"tail", b"plus", b"twin"]
            assert got.total_bytes_read == twin_end
            # every entry as a chunk's first, and every entry as its last
            for i in range(19):
                check(vl, tables, log, base, ssts, offs[i], 10**9, log_size, now, overlay=overlay)
                check(vl, tables, log, base, ssts, base, offs[i] - base + 1, log_size, now, overlay=overlay)
    finally:
        close_all(tables)


# ---- 4. a chunk that crosses the walk's 8 MiB segment ----

def segment_case(ora):
    base, n, vl = 777, 13, 800 * 1024
    rng = np.random.default_rng(0x5E6)
    blob = rng.integers(0, 256, vl + n, dtype=np.uint8).tobytes()
    entries = [(b"seg-key-%02d" % i, blob[i:i + vl], T0 + i, 0) for i in range(n)]
    # 3 is overwritten later; 9 has a twin of the same millisecond later in the log, which the table knows
    entries += [(b"seg-key-03", b"late-three", T0 + 100, 0), (b"seg-key-09", blob[:70001], T0 + 9, 0)]
    log, offs = vr.encode(entries, base)
    items = {k: (o, c, 0) for (k, _, c, _), o in zip(entries, offs)}
    files = [sc.write(ora, sorted((k, o, c, t) for k, (o, c, t) in items.items()))]
    return base, log, offs, files


def test_chunk_crosses_a_segment(vbf, ora):
    from velarixdb_amd import ValueLog
    base, log, offs, files = segment_case(ora)
    assert len(log) > 10 * 2**20
    ssts = [ref.Sst(*f) for f in files]
    tables = open_tables(files)
    try:
        with ValueLog.open(log, base=base) as vl:
            chunk = offs[12] - base  # the first 12 entries: the most recent entries of 3 and 9 lie behind the chunk
            assert chunk > 8 * 2**20
            got, want = check(vl, tables, log, base, ssts, base, chunk, base + len(log), T0 + 10**4)
            assert want["invalid"] == [3] and len(got.verdict) == 12
            assert want["append"][9][0] == b"seg-key-09" and len(want["append"][9][1]) == 70001
            assert got.total_bytes_read == chunk
    finally:
        close_all(tables)


# ---- 5, 6. all entries invalid; a torn chunk ----

def test_all_invalid_and_torn(vbf, ora):
    from velarixdb_amd import ValueLog
    from velarixdb_amd._lib import VBF_WALK_TORN
    base, log, offs, files, overlay = branch_case(ora)
    ssts = [ref.Sst(*f) for f in files]
    end, now = base + len(log), T0 + 777
    tables = open_tables(files)
    try:
        with ValueLog.open(log, base=base) as vl:
            tail, chunk = offs[1], offs[6] - offs[1]  # entries 1..5 without the overlay: every one invalid
            got, want = check(vl, tables, log, base, ssts, tail, chunk, end, now)
            assert want["invalid"] == [0, 1, 2, 3, 4] and len(got.append) == 29 and got.put_keys == [b"tail"]
            assert got.append[:17] == struct.pack("<IIqB", 4, 8, now, 0) and got.append[17:21] == b"tail"
            assert got.append[21:] == struct.pack("<Q", got.new_tail) and got.new_tail == offs[6]
            assert got.put_val_offsets.tolist() == [end] and got.put_tombstones.tolist() == [0]
        cut = log[:-3]
        del overlay[b"f-ovl"]  # it points at the entry the cut tears: BAD, see the errors' test
        with ValueLog.open(cut, base=base) as vl:
            got, want = check(vl, tables, cut, base, ssts, base, 10**6, end - 3, now, overlay=overlay)
            assert want["invalid"] == [1, 2, 3, 4, 5, 7, 8, 9]
            r = Raw(vl, tables, base, 10**6, end - 3, now, overlay=overlay)
            assert r.rc == 0 and r.scalars["stop"] == VBF_WALK_TORN and r.scalars["end_off"] == offs[13]
            assert r.scalars["n_chunk"] == 13 and got.new_tail == offs[13]
    finally:
        close_all(tables)


# ---- 7. errors and capacities ----

def test_errors_and_capacities(vbf, ora):
    from velarixdb_amd import ValueLog, gc
    from velarixdb_amd._lib import VBF_EINVAL, VBF_WALK_END
    base, log, offs, files, overlay = branch_case(ora)
    end, now = base + len(log), T0 + 777
    tables = open_tables(files)
    try:
        with ValueLog.open(log, base=base) as vl:
            whole = Raw(vl, tables, base, len(log), end, now, overlay=overlay)
            assert whole.rc_query == 0 and whole.rc == 0 and whole.guards_intact()
            want = gc.collect(vl, tables, base, len(log), end, now, overlay=overlay)
            sizes = dict(n_chunk=14, n_invalid=8, n_puts=7, append_len=len(want.append), end_off=end,
                         stop=wr.walk(log, base, len(log), base)[2])
            assert whole.query == sizes and whole.scalars == sizes  # the size query
            assert whole.out("append").tobytes() == want.append
            assert np.array_equal(whole.out("put_val_offsets"), want.put_val_offsets)
            assert np.array_equal(whole.out("put_tombstones"), want.put_tombstones)
            # each array alone
            for name, _ in ARRAYS:
                one = Raw(vl, tables, base, len(log), end, now, overlay=overlay, only=(name,))
                assert one.rc == 0 and one.guards_intact() and np.array_equal(one.out(name), whole.out(name))
            # each capacity too small by one: the sizes written, no array touched
            for name, full in (("verdict", 14), ("append", len(want.append)), ("put_ids", 7), ("put_val_offsets", 7),
                               ("put_tombstones", 7)):
                r = Raw(vl, tables, base, len(log), end, now, overlay=overlay, caps={name: full - 1})
                assert r.rc == VBF_EINVAL and "cap" in r.msg and r.scalars == sizes and r.untouched(), name
            # tail outside the window; an empty chunk
            for tail in (base - 1, end + 1):
                r = Raw(vl, tables, tail, 10, end, now)
                assert r.rc_query == VBF_EINVAL and "outside the window" in r.msg_query
                assert r.query == dict(n_chunk=0, n_invalid=0, n_puts=0, append_len=0, end_off=tail, stop=VBF_WALK_END)
            r = Raw(vl, tables, end, 10, end, now)
            assert r.rc_query == 0 and r.rc == 0 and r.untouched()
            assert r.scalars == dict(n_chunk=0, n_invalid=0, n_puts=0, append_len=0, end_off=end, stop=VBF_WALK_END)
            assert gc.collect_device(vl, tables, end, 10, end, now) is None
            # no table at all, an overlay only
            ssts = []
            got, want2 = check(vl, [], log, base, ssts, base, len(log), end, now, overlay=overlay)
            assert got.verdict.tolist() == [1, 1, 1, 1, 1, 5, 0, 2, 1, 1, 1, 1, 1, 0]
        # a table entry that points at a cut entry inside the window
        cut = log[:-3]
        with ValueLog.open(cut, base=base) as vl:
            r = Raw(vl, tables, base, 10**6, end - 3, now, overlay=overlay, caps=dict(
                verdict=14, append=400, put_ids=8, put_val_offsets=8, put_tombstones=8))
            assert r.rc_query == VBF_EINVAL and r.rc == VBF_EINVAL and r.untouched()
            assert "chunk entry 5, at %d" % offs[13] in r.msg
            with pytest.raises(ValueError, match="chunk entry 5, at %d" % offs[13]):
                gc.collect_device(vl, tables, base, 10**6, end - 3, now, overlay=overlay)
            with pytest.raises(ValueError, match="chunk entry 5, at %d" % offs[13]):
                gc.collect(vl, tables, base, 10**6, end - 3, now, overlay=overlay)
    finally:
        close_all(tables)


# ---- 7b. an appended entry at 2^32 or beyond ----

def test_append_reaches_the_u32_limit(vbf, ora):
    """log_size is only a number: the same chunk appended where its last put starts at 2^32 - 1 (taken,
    byte for byte gc.collect's) and at 2^32 (VBF_EINVAL as vbf_vlog_encode_* gives it, sizes written)."""
    from velarixdb_amd import ValueLog, gc
    from velarixdb_amd._lib import VBF_EINVAL
    base, log, offs, files, overlay = branch_case(ora)
    ssts = [ref.Sst(*f) for f in files]
    end, now = base + len(log), T0 + 777
    tables = open_tables(files)
    try:
        with ValueLog.open(log, base=base) as vl:
            at_end = gc.collect(vl, tables, base, len(log), end, now, overlay=overlay)
            last = int(at_end.put_val_offsets[-1]) - end  # the last put's start within the appended bytes
            assert last >= 29 and len(at_end.append) > last
            fits = 2**32 - 1 - last
            got, _ = check(vl, tables, log, base, ssts, base, len(log), fits, now, overlay=overlay)
            assert got.put_val_offsets[-1] == 2**32 - 1 and fits + len(got.append) > 2**32
            for log_size in (fits + 1, 2**32 - 100):
                r = Raw(vl, tables, base, len(log), log_size, now, overlay=overlay,
                        caps=dict(verdict=14, append=len(at_end.append), put_ids=7, put_val_offsets=7, put_tombstones=7))
                assert r.rc_query == VBF_EINVAL and r.rc == VBF_EINVAL and "2^32" in r.msg and r.untouched()
                assert (r.scalars["n_chunk"], r.scalars["n_invalid"], r.scalars["n_puts"], r.scalars["append_len"]) == \
                    (14, 8, 7, len(at_end.append))
                with pytest.raises(ValueError, match="2\\^32"):
                    gc.collect_device(vl, tables, base, len(log), log_size, now, overlay=overlay)
                with pytest.raises(AssertionError, match="2\\^32"):  # vbf_vlog_encode_host's, through gc.collect
                    gc.collect(vl, tables, base, len(log), log_size, now, overlay=overlay)
            # the `tail` entry alone still fits there: a chunk with no valid entry
            check(vl, tables, log, base, ssts, offs[1], offs[6] - offs[1], 2**32 - 100, now)
    finally:
        close_all(tables)


# ---- 8. with filters and without ----

def test_filters_change_nothing(vbf):
    from velarixdb_amd import BloomFilter, Table, ValueLog, gc
    import os
    log = fixture_log()
    files = [sc.read_fixture(name) for name in sc.NAMES]
    ssts = [ref.Sst(*f) for f in files]
    now = T0 + 10**6
    tables = [Table.open_dir(os.path.join(sc.SST, name)) for name in sc.NAMES]
    filters = []
    try:
        for (d, i), s in zip(files, ssts):
            f = BloomFilter(0.01, len(s.fields))
            assert f.rebuild_from_sst(d, i) == len(s.fields)
            filters.append(f)
        with ValueLog.open(log) as vl:
            for tail, chunk in ((0, 20000), (50, 3000)):
                got, _ = check(vl, tables, log, 0, ssts, tail, chunk, len(log), now, filters=filters)
                same_bytes(got, gc.collect_device(vl, tables, tail, chunk, len(log), now))
    finally:
        close_all(tables)
        del filters


# ---- 9. stale state ----

def test_state_between_calls(vbf, ora):
    """The largest case, the smallest, the largest again, and once more after the workspaces were
    released: identical bytes each time."""
    from velarixdb_amd import ValueLog, gc
    base, log, offs, files = segment_case(ora)
    sbase, slog, soffs, sfiles, soverlay = branch_case(ora)
    big, small = open_tables(files), open_tables(sfiles)
    try:
        with ValueLog.open(log, base=base) as vl, ValueLog.open(slog, base=sbase) as svl:
            large = lambda: gc.collect_device(vl, big, base, offs[12] - base, base + len(log), T0 + 5)
            tiny = lambda: gc.collect_device(svl, small, soffs[1], soffs[6] - soffs[1], sbase + len(slog), T0 + 5)
            first, t0 = large(), tiny()
            again = large()
            vbf.lib.vbf_release_workspaces()
            third, t1 = large(), tiny()
            assert len(first.append) > 7 * 2**20 and len(t0.append) == 29  # ten 800 KiB values and one of 70 001
            for other in (again, third):
                same_bytes(other, first)
                assert np.array_equal(other.verdict, first.verdict)
            same_bytes(t1, t0)
    finally:
        close_all(big + small)


# ---- 10. four threads on one log handle and one set of tables ----

THREADS, ROUNDS, CAP = 4, 3, 120.0


def test_four_threads_collect_one_log(vbf, ora):
    from velarixdb_amd import ValueLog, gc
    base, log, offs, files, overlay, log_size = shape_case(ora)
    now = T0 + 10**5
    jobs = ((base, 10**9), (offs[12], 69), (offs[8], offs[17] - offs[8]), (offs[1], offs[13] - offs[1]))
    tables = open_tables(files)
    try:
        with ValueLog.open(log, base=base) as vl:
            run = lambda job: gc.collect_device(vl, tables, job[0], job[1], log_size, now, overlay=overlay)
            wants = [run(job) for job in jobs]  # the single-caller answers
            assert all(w is not None for w in wants) and len({len(w.append) for w in wants}) == THREADS
            for job, want in zip(jobs, wants):
                same_bytes(want, gc.collect(vl, tables, job[0], job[1], log_size, now, overlay=overlay))
            results, errors = [[] for _ in range(THREADS)], []
            start = threading.Barrier(THREADS)

            def work(t):
                try:
                    start.wait()
                    for _ in range(ROUNDS):
                        results[t].append(run(jobs[t]))
                except Exception:
                    errors.append((t, traceback.format_exc()))

            threads = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(THREADS)]
            for th in threads:
                th.start()
            for th in threads:
                th.join(CAP)
            assert not any(th.is_alive() for th in threads), "a thread is still inside a call after %g s" % CAP
            assert not errors, errors[0][1]
            for t in range(THREADS):
                assert len(results[t]) == ROUNDS
                for got in results[t]:
                    same_bytes(got, wants[t])
                    assert np.array_equal(got.verdict, wants[t].verdict)
    finally:
        close_all(tables)
