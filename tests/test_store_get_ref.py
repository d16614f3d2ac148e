"""The get checker (tests/store_get_ref.py) pinned: on the hand-written truth table of
tests/store_get_cases.py, one row per sentence of DataStore::get's rules (src/db/store.rs:442-501),
and against store_model's dictionary where the reference keeps the dictionary's claim."""
import numpy as np
import pytest

import sst_get_ref as gref
import store_get_cases as cases
import store_get_ref as sg
import store_model as sm
import vlog_ref as vr
from test_gpu_table_get import write


@pytest.fixture(scope="module")
def full(ora):
    w = cases.world(40, 40, (40, 40, 40))
    return w, cases.store(w, [(b"", b""), (b"", b""), write(ora, w.sst_items)])


@pytest.mark.parametrize("row", list(cases.ROWS))
def test_truth_table(full, row):
    w, st = full
    found, layer, status = cases.ROWS[row][4]
    g = st.get(cases.ROW_KEYS[row], check_key=True)
    assert (g.found, g.layer, g.status) == (found, layer, status), (row, g)
    assert g.table == (layer & 0x7FFFFFFF if layer != sg.LAYER_NONE and layer & sg.LAYER_TABLE else sg.NO_TABLE)
    assert (g.value is not None) == (status == vr.VALUE)
    if found == 0:
        assert (g.val_offset, g.created_ms) == (0, 0)


def test_the_winner_is_the_named_layers_entry(full):
    """The fields come from the winning layer's own entry (every layer's entry of a row points to a log
    entry of its own)."""
    w, st = full
    g = st.get(cases.ROW_KEYS["ro_tie"])
    e = st.read_only[0][cases.ROW_KEYS["ro_tie"]]
    assert (g.val_offset, g.created_ms) == (e.val_offset, e.created_at) and not e.is_tombstone
    assert st.read_only[2][cases.ROW_KEYS["ro_tie"]].val_offset != e.val_offset
    g = st.get(cases.ROW_KEYS["active_time_neg"])
    assert g.created_ms == cases.NEG  # the i64's bits
    g = st.get(cases.ROW_KEYS["gc_live"])
    assert g.value.startswith(b"v:'gc':")
    assert st.memtable_step(cases.ROW_KEYS["ro_time_zero_sst"]) == (0, sg.LAYER_NONE, 0, 0)
    assert st.memtable_step(cases.ROW_KEYS["sst_only"]) == (0, sg.LAYER_NONE, 0, 0)


def test_get_many_layout(full):
    w, st = full
    keys = w.queries[:300]
    r = st.get_many(keys, check_keys=True)
    assert r["value_off"][0] == 0 and r["value_off"][-1] == r["values"].size
    for j, k in enumerate(keys):
        g = st.get(k, check_key=True)
        assert (r["found"][j], r["layer"][j], r["status"][j]) == (g.found, g.layer, g.status)
        lo, hi = int(r["value_off"][j]), int(r["value_off"][j + 1])
        assert r["values"][lo:hi].tobytes() == (g.value or b"")
    f, l, v, c = st.memtable_many(keys)
    assert ((f == 0) == (l == sg.LAYER_NONE)).all() and (l[f != 0] < sg.LAYER_TABLE).all()
    assert st.memtable_many([])[0].size == 0


@pytest.mark.parametrize("name", ["plain", "partial"])
@pytest.mark.parametrize("flushed", [0, 2, 5])
def test_against_the_dictionary(ora, name, flushed):
    """A store_model history read between its flushes: the first `flushed` generations are tables, the
    last one is the active memtable, the ones between are read-only.  Every clock of these scenarios is
    positive and grows from generation to generation, so the reference's answer is the dictionary's.
    The one exception is the key put on both sides of the millisecond seam: both copies carry the same
    value, so the claim (the value) still holds."""
    h = sm.history(name)
    store, steps = sm.build(ora, name)
    mems = [sg.memtable(g.keys, offs, g.created, g.tombs) for g, (_, offs, _) in zip(h.gens, steps)]
    st = sg.Store(store.log_bytes(), store.base, None, mems[-1], mems[flushed:-1], [t.sst for t in store.tables[:flushed]])
    for k in h.universe + h.absent:
        g = st.get(k, check_key=True)
        assert g.value == store.expect(k), k
        assert (g.found == 0) == (k not in store.dict)
        if g.found == 1:
            assert g.status == vr.VALUE and g.created_ms == store.dict[k][1]


def test_high_clock_is_where_the_claim_breaks(ora):
    """created_at >= 2^63 is negative in the memtable's DateTime: a read-only memtable's entry at such a
    time never wins (store.rs:461), so the get falls back to what the SSTs hold."""
    h = sm.history("big")
    assert h.scenario.high_clock_gen == 6
    store, steps = sm.build(ora, "big")
    g6, offs = h.gens[6], steps[6][1]
    ro = sg.memtable(g6.keys, offs, g6.created, g6.tombs)
    st = sg.Store(store.log_bytes(), store.base, None, {}, [ro], [t.sst for t in store.tables[:6]])
    below, _ = sm.build(ora, "big", upto=6)
    for k in sorted(set(g6.keys))[:50]:
        assert st.get(k).value == below.expect(k)
        assert sg.Store(store.log_bytes(), store.base, None, ro, [], []).get(k).value == store.expect(k)  # active: any time
