"""vbf_store_get_host, the whole get in one device pass, against the get checker
(tests/store_get_ref.py) on all eight output arrays: with and without filters, without tables, with
the key check; over the two first fixture SSTs plus the world's own table and a log window whose
base is not 0.  And one store_model history read between its flushes, against the dictionary."""
import ctypes
import os

import numpy as np
import pytest

import store_get_cases as cases
import store_get_ref as sg
import store_model as sm
import vlog_ref as vr
from test_gpu_memtable_get import Opened
from test_gpu_table_get import NAMES, read_fixture, write

pytestmark = pytest.mark.gpu
FIELDS = ("found", "layer", "table", "val_offsets", "created_ms", "status", "values", "value_off")


class Rig:
    def __init__(self, vbf, ora, world):
        self.o = Opened(vbf, world)
        self.files = [read_fixture(NAMES[0]), read_fixture(NAMES[1]), write(ora, world.sst_items)]
        self.tables = [vbf.Table.open(d, i) for d, i in self.files]
        self.filters = []
        for (d, i), t in zip(self.files, self.tables):
            f = vbf.BloomFilter(0.01, max(t.entries, 1))
            f.rebuild_from_sst(d, i)
            self.filters.append(f)
        self.st = cases.store(world, self.files)
        ref = self.st.tables
        fix = [k for s in ref[:2] for k in list(s.starts)[::9]]
        self.keys = list(cases.ROW_KEYS.values()) + world.queries[:6000] + fix + [k + b"\0" for k in fix[::3]]

    def get(self, keys, tables=True, filters=False, check_keys=False):
        from velarixdb_amd import store
        o = self.o
        return store.get_many(keys, self.tables if tables else [], o.vlog, active=o.active, read_only=o.ro, gc=o.gc,
                              filters=self.filters if filters else None, check_keys=check_keys)

    def close(self):
        self.o.close()
        for t in self.tables:
            t.close()


@pytest.fixture(scope="module")
def rig(vbf, ora):
    r = Rig(vbf, ora, cases.world(2049, 8193, (8193, 40, 2049)))  # every layer holds its rows
    yield r
    r.close()


def arrays(r):
    return {"found": r.found, "layer": r.layer, "table": r.table, "val_offsets": r.val_offsets, "created_ms": r.created_ms,
            "status": r.values.status, "values": r.values.values, "value_off": r.values.value_off}


def same(got, want, keys):
    for f in FIELDS:
        g, w = got[f], want[f]
        assert g.shape == w.shape, (f, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, "%s differs at %d places, first %d (key %r): got %r, want %r" % (
            f, bad.size, bad[0], keys[bad[0]] if f not in ("values", "value_off") else None, g[bad[0]], w[bad[0]])


@pytest.mark.parametrize("filters", (False, True))
@pytest.mark.parametrize("check_keys", (False, True))
def test_equals_the_checker(rig, filters, check_keys):
    want = rig.st.get_many(rig.keys, check_keys=check_keys)
    assert {1, 2, 3, 4}.issubset(set(want["status"].tolist())) and ((want["layer"] >= sg.LAYER_TABLE) & (want["found"] != 0)).sum() > 100
    assert not check_keys or (want["status"] == vr.KEY_MISMATCH).any()
    same(arrays(rig.get(rig.keys, filters=filters, check_keys=check_keys)), want, rig.keys)


def test_plain_kernel_gives_the_same(rig):
    os.environ["VBF_MEMGET"] = "0"
    try:
        got = arrays(rig.get(rig.keys, filters=True))
    finally:
        del os.environ["VBF_MEMGET"]
    same(got, rig.st.get_many(rig.keys), rig.keys)


def test_without_tables(rig):
    st = sg.Store(rig.st.log, rig.st.base, rig.st.gc, rig.st.active, rig.st.read_only, [])
    got = arrays(rig.get(rig.keys, tables=False))
    same(got, st.get_many(rig.keys), rig.keys)
    assert (got["table"] == sg.NO_TABLE).all()


def test_truth_table_and_the_bad_gc_offset(rig):
    keys = list(cases.ROW_KEYS.values())
    got = arrays(rig.get(keys, filters=True, check_keys=True))
    for j, row in enumerate(cases.ROWS):
        assert (got["found"][j], got["layer"][j], got["status"][j]) == cases.ROWS[row][4], row
    at = {row: j for j, row in enumerate(cases.ROWS)}
    for row in ("gc_log_bad_lo", "gc_log_bad_hi"):  # reported BAD, not dropped
        j = at[row]
        assert (got["found"][j], got["layer"][j], got["status"][j]) == (1, 0, vr.BAD)
        assert got["value_off"][j] == got["value_off"][j + 1]


def _raw(rig, keys, values_cap=None, poison=0xA5):
    """The C ABI itself: a size query, then the filling call with guard-filled arrays -> (rc, arrays, bytes)."""
    from velarixdb_amd._lib import lib
    from velarixdb_amd.keys import pack
    b = pack(keys)
    d, p = b.ptrs()
    n = b.n
    o = rig.o
    th = (ctypes.c_void_p * 3)(*[t._h.value for t in rig.tables])
    rh = (ctypes.c_void_p * 3)(*[t._h.value for t in o.ro])
    head = (d, p, b.stride, n, o.gc._h, o.active._h, 3, rh, 3, th, None, o.vlog._h, 0)
    nb = ctypes.c_uint64()
    st0, vo0 = np.zeros(n, np.uint8), np.zeros(n + 1, np.uint64)
    rc = lib.vbf_store_get_host(*head, None, None, None, None, None, st0.ctypes.data, None, 0, vo0.ctypes.data, ctypes.byref(nb))
    assert rc == 0 and nb.value == vo0[-1]
    cap = nb.value if values_cap is None else values_cap
    out = {"found": np.full(n, poison, np.uint8), "layer": np.full(n, poison, np.uint32), "table": np.full(n, poison, np.uint32),
           "val_offsets": np.full(n, poison, np.uint32), "created_ms": np.full(n, poison, np.uint64),
           "status": np.full(n, poison, np.uint8), "values": np.full(nb.value + 8, poison, np.uint8),
           "value_off": np.full(n + 1, poison, np.uint64)}
    nb2 = ctypes.c_uint64()
    rc = lib.vbf_store_get_host(*head, *[out[f].ctypes.data for f in FIELDS[:6]], out["values"].ctypes.data, cap,
                                out["value_off"].ctypes.data, ctypes.byref(nb2))
    return rc, out, (nb.value, nb2.value), (st0, vo0)


def test_size_query_then_fill_and_a_short_capacity(rig):
    from velarixdb_amd._lib import VBF_EINVAL, lib
    keys = rig.keys[:2000]
    want = rig.st.get_many(keys)
    rc, out, (nb, nb2), (st0, vo0) = _raw(rig, keys)
    assert rc == 0 and nb == nb2 == want["values"].size > 0
    assert np.array_equal(st0, want["status"]) and np.array_equal(vo0, want["value_off"])  # the size query fills them too
    assert (out["values"][nb:] == 0xA5).all()
    out["values"] = out["values"][:nb]
    same(out, want, keys)
    rc, out, (nb, nb2), _ = _raw(rig, keys, values_cap=nb - 1)
    assert rc == VBF_EINVAL and nb2 == nb and b"values_cap" in lib.vbf_last_error()
    for f in FIELDS:  # every element still holds the poison it was filled with
        assert (out[f] == 0xA5).all(), f


def test_a_larger_call_leaves_nothing_behind(rig):
    big = arrays(rig.get(rig.keys, filters=True, check_keys=True))
    same(big, rig.st.get_many(rig.keys, check_keys=True), rig.keys)
    for n in (0, 1, 65):
        keys = rig.keys[100:100 + n]
        same(arrays(rig.get(keys, filters=True)), rig.st.get_many(keys), keys)
        same(arrays(rig.get(keys, tables=False)), sg.Store(rig.st.log, rig.st.base, rig.st.gc, rig.st.active,
                                                           rig.st.read_only, []).get_many(keys), keys)


@pytest.mark.parametrize("name,flushed", [("plain", 0), ("plain", 4), ("big", 3)])
def test_a_history_read_between_its_flushes(vbf, ora, name, flushed):
    """The first `flushed` generations are tables; the later ones are still memtables, the last one the
    active one.  Every get returns what the dictionary holds (the clocks of the read-only generations
    are positive and grow; the high clock of "big" lies in the active memtable, which decides whatever
    its time)."""
    from velarixdb_amd import store
    h = sm.history(name)
    model, steps = sm.build(ora, name)
    tables = [vbf.Table.open(t.data, t.index) for t in model.tables[:flushed]]
    mems = [vbf.MemTable.open(g.keys, offs, g.created, g.tombs) for g, (_, offs, _) in list(zip(h.gens, steps))[flushed:]]
    vlog = vbf.ValueLog.open(model.log_bytes(), base=model.base)
    try:
        keys = h.universe + h.absent
        r = store.get_many(keys, tables, vlog, active=mems[-1], read_only=mems[:-1], check_keys=True)
        for j, k in enumerate(keys):
            assert r.value(j) == model.expect(k), k
            assert (r.found[j] == 0) == (k not in model.dict), k
            if r.found[j] == 1:
                assert r.values.status[j] == vr.VALUE and int(r.created_ms[j]) == model.dict[k][1]
        assert (r.layer[r.found != 0] < sg.LAYER_TABLE).any() and (flushed == 0 or (r.layer[r.found != 0] >= sg.LAYER_TABLE).any())
    finally:
        for t in tables + mems + [vlog]:
            t.close()
