"""vbf_store_scan_host, the whole-store range scan, against the scan checker (tests/store_scan_ref.py,
pinned by tests/test_store_scan_ref.py) on all eleven output arrays, against the library's own get
(the definition), against the table scan where there are no memtables, and against one store_model
history read between its flushes.

Shapes: memtable layers of 300, 5000, 2049, 1 and 4097 entries (one past the sort tile, one past the
lookup's 4096-word sample), the two first fixture SSTs plus the world's 600-entry table, 1 / 50 / 300
ranges (300 x 8 layers: more than one 256-lane workgroup of pairs), bounds_off[0] != 0."""
import ctypes

import numpy as np
import pytest

import store_get_cases as cases
import store_get_ref as sg
import store_model as sm
import store_scan_cases as sc
import store_scan_ref as ref
import vlog_ref as vr
from scan_cases import NAMES, read_fixture, write
from test_gpu_memtable_get import Opened

pytestmark = pytest.mark.gpu
KEEP, EXCL = ref.KEEP_TOMBSTONES, ref.END_EXCLUSIVE
FIELDS = ref.FIELDS
DTYPES = dict(zip(FIELDS, (np.uint64, np.uint8, np.uint64, np.uint8, np.uint32, np.uint32, np.uint32, np.uint64, np.uint8,
                           np.uint8, np.uint64)))
GUARD, LEAD = 0xA5, 3


class Rig:
    """A world's layers and three tables on the device, beside the checker's Store over the same."""

    def __init__(self, vbf, ora, world):
        self.o = Opened(vbf, world)
        self.files = [read_fixture(NAMES[0]), read_fixture(NAMES[1]), write(ora, world.sst_items)]
        self.tables = [vbf.Table.open(d, i) for d, i in self.files]
        self.st = cases.store(world, self.files)
        self.union = ref.union(self.st)
        self.ranges = sc.ranges(self.union, 300)
        self.memo = {False: {}, True: {}}

    def want(self, ranges, flags=0, check_keys=False):
        return ref.scan_many(self.st, ranges, flags, check_keys, self.memo[bool(check_keys)])

    def sub(self, gc=True, active=True, ro=True, tables=True):
        """(keyword arguments for raw() / scan_many, the checker's Store) for a subset of the layers."""
        o, st = self.o, self.st
        kw = dict(gc=o.gc if gc else None, active=o.active if active else None, ro=o.ro if ro else [],
                  tables=self.tables if tables else [])
        return kw, sg.Store(st.log, st.base, st.gc if gc else None, st.active if active else None,
                            st.read_only if ro else [], st.tables if tables else [])

    def close(self):
        self.o.close()
        for t in self.tables:
            t.close()


@pytest.fixture(scope="module")
def rigs(vbf, ora):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Rig(vbf, ora, cases.world(*{"main": sc.MAIN, "truth": sc.TRUTH, "tables": (0, 0, ())}[name]))
        return cache[name]
    yield get
    for r in cache.values():
        r.close()


def _h(t):
    return t._h if t is not None else None


def _arr(ts):
    return (ctypes.c_void_p * max(len(ts), 1))(*[t._h.value for t in ts])


def raw(vlog, ranges, flags=0, check_keys=False, gc=None, active=None, ro=(), tables=(), caps=None, want=FIELDS):
    """The C ABI itself, bounds_off[0] = LEAD: a size query, then a filling call into guard-filled arrays
    of exactly the reported sizes (caps = (entries, key bytes, value bytes) overrides the capacities
    passed; the arrays keep the reported sizes + 8 guard items).  -> (rc, arrays by name, sizes)"""
    from velarixdb_amd._lib import lib
    flat = [b for pair in ranges for b in pair]
    bounds = np.frombuffer(b"\xEE" * LEAD + b"".join(flat) + b"\xEE", np.uint8)
    boff = (np.concatenate([[0], np.cumsum([len(b) for b in flat])]) + LEAD).astype(np.uint64)
    ro, tables = list(ro), list(tables)
    head = (bounds.ctypes.data, boff.ctypes.data, len(ranges), _h(gc), _h(active), len(ro), _arr(ro), len(tables),
            _arr(tables), vlog._h, flags, int(check_keys))
    n, kb, vb = ctypes.c_uint64(77), ctypes.c_uint64(77), ctypes.c_uint64(77)
    sizes = (ctypes.byref(n), ctypes.byref(kb), ctypes.byref(vb))
    rc = lib.vbf_store_scan_host(*head, None, None, 0, None, None, None, None, None, None, None, 0, None, 0, None, *sizes)
    assert rc == 0, lib.vbf_last_error()
    got = (n.value, kb.value, vb.value)
    count = {"range_off": len(ranges) + 1, "keys": got[1], "key_off": got[0] + 1, "values": got[2], "value_off": got[0] + 1}
    out = {f: np.full(count.get(f, got[0]) + 8, GUARD, DTYPES[f]) for f in FIELDS}
    p = {f: out[f].ctypes.data if f in want else None for f in FIELDS}
    ecap, kcap, vcap = caps or got
    n, kb, vb = ctypes.c_uint64(77), ctypes.c_uint64(77), ctypes.c_uint64(77)
    sizes = (ctypes.byref(n), ctypes.byref(kb), ctypes.byref(vb))
    rc = lib.vbf_store_scan_host(*head, p["range_off"], p["keys"], kcap, p["key_off"], p["tombstones"], p["layer"], p["table"],
                                 p["val_offsets"], p["created_ms"], p["status"], ecap, p["values"], vcap, p["value_off"],
                                 *sizes)
    assert (n.value, kb.value, vb.value) == got, "the size query and the filling call disagree"
    if rc == 0:
        for f in FIELDS:
            m = count.get(f, got[0])
            guard = np.full(1, GUARD, DTYPES[f])[0]
            assert (out[f][m:] == guard).all(), "wrote past the end of " + f
            out[f] = out[f][:m] if f in want else None
    return rc, out, got


def same(got, want, fields=FIELDS):
    for f in fields:
        g, w = got[f], want[f]
        assert g.shape == w.shape, (f, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, "%s differs at %d of %d places, first %d: got %r, want %r" % (
            f, bad.size, g.size, bad[0], g[bad[0]], w[bad[0]])


def arrays(r):
    return {"range_off": r.range_off, "keys": r.keys, "key_off": r.key_off, "tombstones": r.tombstones, "layer": r.layer,
            "table": r.table, "val_offsets": r.val_offsets, "created_ms": r.created_ms, "status": r.values.status,
            "values": r.values.values, "value_off": r.values.value_off}


# ---- 1. the checker ---------------------------------------------------------------------------

@pytest.mark.parametrize("check_keys", (False, True))
@pytest.mark.parametrize("flags", (0, KEEP, EXCL, KEEP | EXCL))
@pytest.mark.parametrize("name", ("main", "tables"))
def test_equals_the_checker(rigs, name, flags, check_keys):
    rig = rigs(name)
    kw, _ = rig.sub()
    want = rig.want(rig.ranges, flags, check_keys)
    assert want["layer"].size > (10000 if name == "main" else 1000) and (want["layer"] >= sg.LAYER_TABLE).sum() > 100
    assert not (check_keys and name == "main") or (want["status"] == vr.KEY_MISMATCH).any()
    rc, got, sizes = raw(rig.o.vlog, rig.ranges, flags, check_keys, **kw)
    assert rc == 0 and sizes == (want["layer"].size, want["keys"].size, want["values"].size)
    same(got, want)


@pytest.mark.parametrize("count", (1, 50))
def test_fewer_ranges(rigs, count):
    rig = rigs("main")
    kw, _ = rig.sub()
    rs = rig.ranges[:count]
    rc, got, _ = raw(rig.o.vlog, rs, KEEP, True, **kw)
    assert rc == 0
    same(got, rig.want(rs, KEEP, True))


def test_the_python_layer(vbf, rigs):
    """store.scan_many gives the same arrays with one call at the guessed capacities, with two calls,
    and with one call at capacities the caller names."""
    from velarixdb_amd import store
    rig = rigs("main")
    o = rig.o
    call = lambda rs, **kw: store.scan_many(rs, rig.tables, o.vlog, active=o.active, read_only=o.ro, gc=o.gc, **kw)
    want = rig.want(rig.ranges, KEEP, False)
    same(arrays(call(rig.ranges, keep_tombstones=True)), want)          # larger than the guess: two calls
    few = rig.ranges[1:20]
    r = call(few, end_exclusive=True, check_keys=True)                    # fits the guess: one call
    same(arrays(r), rig.want(few, EXCL, True))
    pairs = [list(r.range(i)) for i in range(len(few))]
    assert sum(map(len, pairs)) == r.layer.size and [k for p in pairs for k, _ in p] == [
        r.keys[int(a):int(b)].tobytes() for a, b in zip(r.key_off[:-1], r.key_off[1:])]
    sizes = (want["layer"].size, want["keys"].size, want["values"].size)
    same(arrays(call(rig.ranges, keep_tombstones=True, capacities=sizes)), want)   # exactly enough: one call
    same(arrays(call(rig.ranges, keep_tombstones=True, capacities=(1, 1, 1))), want)


# ---- 2. memtables alone, and each layer absent in turn ------------------------------------------

@pytest.mark.parametrize("absent", ("none", "gc", "active", "ro", "all but gc", "all but tables"))
def test_memtables_alone(rigs, absent):
    rig = rigs("main")
    pick = {"none": {}, "gc": {"gc": False}, "active": {"active": False}, "ro": {"ro": False},
            "all but gc": {"active": False, "ro": False}, "all but tables": {"gc": False, "active": False, "ro": False}}[absent]
    kw, st = rig.sub(tables=absent == "all but tables", **pick)
    rs = rig.ranges[:120]
    for flags, ck in ((KEEP, False), (EXCL, True)):
        rc, got, _ = raw(rig.o.vlog, rs, flags, ck, **kw)
        assert rc == 0
        same(got, ref.scan_many(st, rs, flags, ck))
        assert absent == "all but tables" or (got["table"] == sg.NO_TABLE).all()


# ---- 3. the definition: the library's own get -----------------------------------------------------

@pytest.mark.parametrize("flags", (0, KEEP))
def test_parity_with_the_get(rigs, flags):
    from velarixdb_amd import store
    rig = rigs("main")
    o = rig.o
    kw, _ = rig.sub()
    rs = rig.ranges[:60]
    rc, got, _ = raw(o.vlog, rs, flags, True, **kw)
    assert rc == 0
    kb = got["keys"].tobytes()
    keys = [kb[int(a):int(b)] for a, b in zip(got["key_off"][:-1], got["key_off"][1:])]
    g = store.get_many(keys, rig.tables, o.vlog, active=o.active, read_only=o.ro, gc=o.gc, check_keys=True)
    assert np.array_equal(g.found, np.where(got["tombstones"] != 0, 2, 1))
    for f, a in (("layer", g.layer), ("table", g.table), ("val_offsets", g.val_offsets), ("created_ms", g.created_ms),
                 ("status", g.values.status), ("values", g.values.values), ("value_off", g.values.value_off)):
        assert np.array_equal(got[f], a), f
    # the keys of U_r the scan left out: the get does not find them (or finds a tombstone, without KEEP)
    omitted = []
    for r, (lo, hi) in enumerate(rs):
        a, b = ref.cut(rig.union, lo, hi, flags)
        here = set(keys[int(got["range_off"][r]):int(got["range_off"][r + 1])])
        assert here <= set(rig.union[a:b])
        omitted += [k for k in rig.union[a:b] if k not in here]
    assert len(omitted) > 100
    g = store.get_many(omitted, rig.tables, o.vlog, active=o.active, read_only=o.ro, gc=o.gc)
    assert set(g.found.tolist()) == ({0} if flags & KEEP else {0, 2})


# ---- 4. no memtables: the table scan ----------------------------------------------------------------

@pytest.mark.parametrize("flags", (0, KEEP, EXCL, KEEP | EXCL))
def test_parity_with_the_table_scan(vbf, rigs, flags):
    rig = rigs("main")
    kw, _ = rig.sub(gc=False, active=False, ro=False)
    rc, got, _ = raw(rig.o.vlog, rig.ranges, flags, False, **kw)
    assert rc == 0
    t = vbf.table.scan_many(rig.ranges, rig.tables, keep_tombstones=bool(flags & KEEP), end_exclusive=bool(flags & EXCL))
    assert t.table.size > 5000
    for f, a in (("range_off", t.range_off), ("keys", t.keys), ("key_off", t.key_off), ("table", t.table),
                 ("val_offsets", t.val_offsets), ("created_ms", t.created_ms), ("tombstones", t.tombstones)):
        assert np.array_equal(got[f], a), f
    assert np.array_equal(got["layer"], t.table | np.uint32(sg.LAYER_TABLE))


# ---- 5. the truth table ---------------------------------------------------------------------------

def test_truth_table_and_the_bad_gc_offsets(rigs):
    """Every row as tests/test_store_scan_ref.py pins it, in the world whose every layer holds its rows."""
    rig = rigs("truth")
    kw, _ = rig.sub()
    rs = [(k, k) for k in cases.ROW_KEYS.values()]
    rc, got, _ = raw(rig.o.vlog, rs, KEEP, True, **kw)
    assert rc == 0
    same(got, rig.want(rs, KEEP, True))
    for r, row in enumerate(cases.ROWS):
        found, layer, status = cases.ROWS[row][4]
        a, b = int(got["range_off"][r]), int(got["range_off"][r + 1])
        if found == 0:
            assert a == b, row
            continue
        assert b == a + 1, row
        assert (2 if got["tombstones"][a] else 1, got["layer"][a], got["status"][a]) == (found, layer, status), row
        assert got["keys"][int(got["key_off"][a]):int(got["key_off"][a + 1])].tobytes() == cases.ROW_KEYS[row]
        if row in ("gc_log_bad_lo", "gc_log_bad_hi"):  # reported BAD, not dropped
            assert (got["layer"][a], got["status"][a]) == (0, vr.BAD) and got["value_off"][a] == got["value_off"][a + 1]


# ---- 6. sizing ------------------------------------------------------------------------------------

def test_one_call_equals_query_then_fill_and_short_capacities(rigs):
    from velarixdb_amd._lib import VBF_EINVAL, lib
    rig = rigs("main")
    kw, _ = rig.sub()
    rs = rig.ranges[:50]
    want = rig.want(rs, KEEP, False)
    rc, got, (n, kb, vb) = raw(rig.o.vlog, rs, KEEP, False, **kw)
    assert rc == 0 and n > 1000 and kb > n and vb > n
    same(got, want)
    rc, one, _ = raw(rig.o.vlog, rs, KEEP, False, caps=(n + 5, kb + 7, vb + 9), **kw)   # roomier than needed
    assert rc == 0
    same(one, want)
    rc, part, _ = raw(rig.o.vlog, rs, KEEP, False, want=("range_off", "layer", "values"), **kw)  # the rest NULL
    assert rc == 0 and part["keys"] is None
    same(part, want, ("range_off", "layer", "values"))
    for caps, what in (((n - 1, kb, vb), b"entries_cap"), ((n, kb - 1, vb), b"keys_cap"), ((n, kb, vb - 1), b"values_cap")):
        rc, out, sizes = raw(rig.o.vlog, rs, KEEP, False, caps=caps, **kw)
        assert rc == VBF_EINVAL and what in lib.vbf_last_error() and sizes == (n, kb, vb)
        for f in FIELDS:  # every element still holds the guard it was filled with
            assert (out[f] == np.full(1, GUARD, DTYPES[f])[0]).all(), f
    # value_off needs entries_cap + 1 slots like key_off: given alone with a short entries_cap it is refused too
    rc, out, _ = raw(rig.o.vlog, rs, KEEP, False, caps=(n - 1, kb, vb), want=("value_off",), **kw)
    assert rc == VBF_EINVAL and (out["value_off"] == GUARD).all()


# ---- 7. the cached workspaces -----------------------------------------------------------------------

def test_a_larger_call_leaves_nothing_behind(rigs):
    rig = rigs("main")
    kw, _ = rig.sub()
    rc, big, _ = raw(rig.o.vlog, rig.ranges, KEEP, True, **kw)
    assert rc == 0
    same(big, rig.want(rig.ranges, KEEP, True))
    for rs in ([], rig.ranges[3:4], rig.ranges[1:2], rig.ranges[5:12], [(b"\xff" * 302, b"\xff" * 303)]):
        for flags in (0, KEEP | EXCL):
            rc, got, _ = raw(rig.o.vlog, rs, flags, False, **kw)
            assert rc == 0
            same(got, rig.want(rs, flags, False))
    kw, st = rig.sub(tables=False)
    rs = rig.ranges[20:23]
    rc, got, _ = raw(rig.o.vlog, rs, 0, True, **kw)
    assert rc == 0
    same(got, ref.scan_many(st, rs, 0, True))


# ---- 8. a store's history ---------------------------------------------------------------------------

@pytest.mark.parametrize("flushed", (0, 3))
def test_a_history_scanned_between_its_flushes(vbf, ora, flushed):
    """The first `flushed` generations of "plain" are tables, the later ones still memtables (the last
    one active).  Its clocks are positive and grow from generation to generation, so the dictionary
    says what both states must list: every key it holds live, with its value -- before the flush over
    memtables plus tables, after it over the tables alone."""
    from velarixdb_amd import store
    h = sm.history("plain")
    model, steps = sm.build(ora, "plain")
    tables = [vbf.Table.open(t.data, t.index) for t in model.tables]
    mems = [vbf.MemTable.open(g.keys, offs, g.created, g.tombs) for g, (_, offs, _) in list(zip(h.gens, steps))[flushed:]]
    vlog = vbf.ValueLog.open(model.log_bytes(), base=model.base)
    try:
        rs = [sm.FULL] + h.ranges
        before = store.scan_many(rs, tables[:flushed], vlog, active=mems[-1], read_only=mems[:-1], check_keys=True)
        after = store.scan_many(rs, tables, vlog, check_keys=True)
        live = [k for k in h.universe if model.expect(k) is not None]
        assert len(live) > 300 and len(live) < len(h.universe)
        for r, (lo, hi) in enumerate(rs):
            want = [(k, model.expect(k)) for k in live if lo <= k <= hi]
            assert list(before.range(r)) == want, (lo, hi)
            assert list(after.range(r)) == want, (lo, hi)
        assert (before.layer < sg.LAYER_TABLE).any() and (after.layer >= sg.LAYER_TABLE).all()
        assert np.array_equal(before.created_ms, after.created_ms) and np.array_equal(before.val_offsets, after.val_offsets)
    finally:
        for t in tables + mems + [vlog]:
            t.close()
