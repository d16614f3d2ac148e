"""vbf_memtable_get_host / _dev against the get checker (tests/store_get_ref.py), key for key.

Worlds from tests/store_get_cases.py: a gc table, an active memtable and 0, 1 or 3 read-only tables
with sizes mixed from {0, 1, 2049, 8193} (the sort's tile edge, the lookup's LDS sample edge: 8193
entries are sampled at every third), holding the truth table's rows; batches of 0, 1, 63, 64, 65 and
about 10 000 keys with duplicates, the zero-length key and absent keys around the present ones.
Every result must be identical under VBF_MEMGET=0, the plain kernel."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest

import store_get_cases as cases
import store_get_ref as sg

pytestmark = pytest.mark.gpu
# (gc, active, read-only sizes)
WORLDS = {
    "full3": (2049, 8193, (8193, 1, 2049)),
    "ro1": (1, 2049, (8193,)),
    "ro0": (8193, 1, ()),
    "holes": (0, 0, (0, 2049, 1)),       # no gc table, no active memtable, an empty read-only table
    "small3": (40, 40, (40, 40, 40)),    # every row of the truth table fits every layer
}
BATCHES = (0, 1, 63, 64, 65)


class Opened:
    """A world's layers as MemTable handles and its log as a ValueLog, beside the checker's Store."""

    def __init__(self, vbf, w):
        self.w, self.st = w, cases.store(w)
        opn = lambda n: vbf.MemTable.open(*w.layers[n]) if n in w.layers else None
        self.gc = opn("gc") if w.layers["gc"][0] else None
        self.active = opn("active") if w.layers["active"][0] else None
        self.ro = [opn(("ro", r)) for r in range(w.nro)]
        self.vlog = vbf.ValueLog.open(w.log, base=w.base)

    def close(self):
        for t in [self.gc, self.active, self.vlog] + self.ro:
            if t is not None:
                t.close()


@pytest.fixture(scope="module")
def opened(vbf):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Opened(vbf, cases.world(*WORLDS[name]))
        return cache[name]
    yield get
    for o in cache.values():
        o.close()


def run(vbf, o, keys, plain=False):
    old = os.environ.pop("VBF_MEMGET", None)
    if plain:
        os.environ["VBF_MEMGET"] = "0"
    try:
        r = vbf.MemTable.get_many(keys, active=o.active, read_only=o.ro, gc=o.gc, vlog=o.vlog)
    finally:
        os.environ.pop("VBF_MEMGET", None)
        if old is not None:
            os.environ["VBF_MEMGET"] = old
    return r.found, r.layer, r.val_offsets, r.created_ms


def same(got, want, keys):
    for g, w, what in zip(got, want, ("found", "layer", "val_offsets", "created_ms")):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, "%s differs at %d of %d keys, first %r: got %r, want %r" % (
            what, bad.size, len(keys), keys[bad[0]], g[bad[0]], w[bad[0]])


@pytest.mark.parametrize("name", list(WORLDS))
def test_every_query(vbf, opened, name):
    o = opened(name)
    keys = o.w.queries
    assert len(keys) >= 10000 or name == "small3"
    assert b"" in keys and len(set(keys)) < len(keys)
    want = o.st.memtable_many(keys)
    got = run(vbf, o, keys)
    same(got, want, keys)
    same(run(vbf, o, keys, plain=True), got, keys)
    assert {int(x) for x in want[1]} >= ({0, 1} if name == "full3" else set())


@pytest.mark.parametrize("name", ["full3", "holes"])
@pytest.mark.parametrize("n", BATCHES)
def test_small_batches(vbf, opened, name, n):
    o = opened(name)
    rows = list(cases.ROW_KEYS.values())
    keys = (rows + o.w.queries)[:n]
    want = o.st.memtable_many(keys)
    for plain in (False, True):
        got = run(vbf, o, keys, plain)
        assert all(g.size == n for g in got)
        same(got, want, keys)


def test_truth_table_rows_are_in_the_data(vbf, opened):
    """Every row's key is asked for in a world that holds every layer of it, and answers as the
    hand-written table says (the SST rows: not found in the memtables)."""
    o = opened("small3")
    keys = list(cases.ROW_KEYS.values())
    assert set(keys) <= set(o.w.queries)
    f, l, v, c = run(vbf, o, keys)
    for j, row in enumerate(cases.ROWS):
        found, layer, _ = cases.ROWS[row][4]
        if layer != sg.LAYER_NONE and layer & sg.LAYER_TABLE:
            found, layer = 0, sg.LAYER_NONE
        assert (f[j], l[j]) == (found, layer), row
    # times at 0, negative, and past 2^63 as u64; a tie across read-only tables
    at = {row: j for j, row in enumerate(cases.ROWS)}
    assert c[at["active_time_zero"]] == 0 and f[at["active_time_zero"]] == 1
    assert c[at["active_time_neg"]] == cases.NEG
    assert l[at["ro_tie"]] == sg.LAYER_RO and l[at["ro_pos_then_neg"]] == sg.LAYER_RO and c[at["ro_pos_then_neg"]] == 5
    ro = [cases.mem(o.w, ("ro", r)) for r in range(3)]
    k = cases.ROW_KEYS["ro_tie"]
    assert ro[0][k].created_at == ro[2][k].created_at and v[at["ro_tie"]] == ro[0][k].val_offset != ro[2][k].val_offset


def test_fixed_stride_keys(vbf, opened):
    o = opened("full3")
    from velarixdb_amd.keys import HostBatch
    present = [k for k in o.w.queries if len(k) == 23][:500]
    assert len(present) > 50
    rows = present + [bytes(23)] * 3 + [k[:-1] + b"\xfe" for k in present[:100]]
    b = HostBatch(np.frombuffer(b"".join(rows), np.uint8).copy(), None, 23, len(rows), 1)
    same(run(vbf, o, b), o.st.memtable_many(rows), rows)


def test_null_outputs_and_no_gc_means_no_log(vbf, opened):
    from velarixdb_amd._lib import call
    from velarixdb_amd.keys import pack
    o = opened("ro1")
    keys = o.w.queries[:700]
    b = pack(keys)
    d, p = b.ptrs()
    want = sg.Store(o.w.log, o.w.base, None, o.st.active, o.st.read_only).memtable_many(keys)
    lay = np.zeros(b.n, np.uint32)
    rh = (ctypes.c_void_p * 1)(o.ro[0]._h.value)
    call("vbf_memtable_get_host", d, p, b.stride, b.n, None, o.active._h, 1, rh, None, None, lay.ctypes.data, None, None)
    assert np.array_equal(lay, want[1])


def test_dev_on_a_side_stream_with_inputs_pending(vbf, opened):
    """vbf_memtable_get_dev on a non-blocking side stream, its keys and offsets copied on that stream
    just before the call (the rig of tests/test_gpu_dev_streams.py: decoys until the copy lands)."""
    from test_gpu_dev_streams import Rig, side_stream, verify
    from velarixdb_amd._lib import lib
    o = opened("full3")
    keys = o.w.queries[:3000]
    decoy = [k[::-1] for k in keys]  # the same lengths, other answers
    data = np.frombuffer(b"".join(keys) + b"\0", np.uint8).copy()
    offs = np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.uint64)
    want, dwant = o.st.memtable_many(keys), o.st.memtable_many(decoy)
    assert any(not np.array_equal(a, b) for a, b in zip(want, dwant))
    case = SimpleNamespace(call="vbf_memtable_get_dev", ident="full3", meta={}, sizes={}, decoy_sizes={},
                           real={"keys": data, "offsets": offs},
                           decoy={"keys": np.frombuffer(b"".join(decoy) + b"\0", np.uint8).copy(), "offsets": offs},
                           want=list(want), decoy_want=list(dwant))
    rig = Rig(side_stream(), case)
    n = len(keys)
    outs = [rig.out(name, n * w.itemsize, want=i) for i, (name, w) in enumerate(zip(("found", "layer", "val", "created"), want))]
    rh = (ctypes.c_void_p * 3)(*[t._h.value for t in o.ro])
    rc = rig.launch(lambda: lib.vbf_memtable_get_dev(rig.p("keys"), rig.p("offsets"), 0, n, o.gc._h, o.active._h, 3, rh,
                                                     o.vlog._h, *outs, rig.sp))
    assert rc == 0, rig.error()
    verify(case, rig.collect())
