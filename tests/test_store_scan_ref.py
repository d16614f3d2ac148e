"""The whole-store scan checker (tests/store_scan_ref.py) pinned: `scan` (the statement) and
`scan_many` (the batch form the GPU tests compare with) give the same answers, and the worlds and
ranges of tests/store_scan_cases.py hold the conditions tests/test_gpu_store_scan.py relies on."""
import collections

import numpy as np
import pytest

import store_get_cases as cases
import store_get_ref as sg
import store_scan_cases as sc
import store_scan_ref as ref
import vlog_ref as vr
from scan_cases import NAMES, read_fixture, write

KEEP, EXCL = ref.KEEP_TOMBSTONES, ref.END_EXCLUSIVE


@pytest.fixture(scope="module")
def main(ora):
    w = cases.world(*sc.MAIN)
    files = [read_fixture(NAMES[0]), read_fixture(NAMES[1]), write(ora, w.sst_items)]
    return w, cases.store(w, files)


def rows_of(res, r):
    """[(key, found, layer, status)] of range r."""
    kb = res["keys"].tobytes()
    out = []
    for i in range(int(res["range_off"][r]), int(res["range_off"][r + 1])):
        out.append((kb[int(res["key_off"][i]):int(res["key_off"][i + 1])], 2 if res["tombstones"][i] else 1,
                    int(res["layer"][i]), int(res["status"][i])))
    return out


def test_the_main_world_without_tables(ora):
    """The main world in numbers: 10 615 keys in the union of its layers and its own table; looked up
    with no tables, every outcome of the get is among them (a key that only the table holds is then
    not found)."""
    w = cases.world(*sc.MAIN)
    st = cases.store(w)
    keys = ref.union(cases.store(w, [write(ora, w.sst_items)]))
    got = [st.get(k) for k in keys]
    assert len(keys) == 10615 and len(ref.union(st)) == 10204
    assert sum(g.found == 0 for g in got) == 784 and sum(g.found == 2 for g in got) == 1647
    by = collections.Counter(g.status for g in got if g.found == 1)
    # one entry in ten of the worlds' logs is a tombstone; the one NONE is the row active_log_none
    assert (by[vr.VALUE], by[vr.TOMBSTONE], by[vr.NONE], by[vr.BAD]) == (7421, 760, 1, 2)
    full = ref.scan_many(st, [sc.FULL], 0)
    assert full["layer"].size == 7421 + 760 + 1 + 2 and not full["tombstones"].any()
    assert ref.scan_many(st, [sc.FULL], KEEP)["tombstones"].sum() == 1647


@pytest.mark.parametrize("flags", (0, KEEP, EXCL, KEEP | EXCL))
@pytest.mark.parametrize("check_keys", (False, True))
def test_scan_and_scan_many_agree(main, flags, check_keys):
    w, st = main
    rs = sc.ranges(ref.union(st), 80)
    many = ref.scan_many(st, rs, flags, check_keys)
    assert many["range_off"][0] == 0 and many["range_off"][-1] == many["layer"].size
    assert many["key_off"][-1] == many["keys"].size and many["value_off"][-1] == many["values"].size
    kb, vb = many["keys"].tobytes(), many["values"].tobytes()
    for r, (lo, hi) in enumerate(rs):
        one = ref.scan(st, lo, hi, flags, check_keys)
        a, b = int(many["range_off"][r]), int(many["range_off"][r + 1])
        assert b - a == len(one), (lo, hi)
        for i, (k, g) in zip(range(a, b), one):
            assert kb[int(many["key_off"][i]):int(many["key_off"][i + 1])] == k
            assert (many["tombstones"][i], many["layer"][i], many["table"][i], many["val_offsets"][i], many["created_ms"][i],
                    many["status"][i]) == (g.found == 2, g.layer, g.table, g.val_offset, g.created_ms, g.status)
            assert vb[int(many["value_off"][i]):int(many["value_off"][i + 1])] == (g.value or b"")
    if check_keys:
        assert (many["status"] == vr.KEY_MISMATCH).any()


def test_the_full_range_omits_what_the_get_does_not_find(main):
    w, st = main
    keys = ref.union(st)
    assert all(sc.FULL[0] <= k <= sc.FULL[1] for k in keys)
    got = {k: st.get(k) for k in keys}
    plain, keep = ref.scan_many(st, [sc.FULL], 0), ref.scan_many(st, [sc.FULL], KEEP)
    listed = {k for k, *_ in rows_of(plain, 0)}
    assert listed == {k for k in keys if got[k].found == 1} and len(listed) < len(keys)
    assert any(got[k].found == 2 for k in keys) and not listed & {k for k in keys if got[k].found == 2}
    kept = rows_of(keep, 0)
    assert {k for k, *_ in kept} == {k for k in keys if got[k].found != 0}
    assert [k for k, *_ in kept] == sorted(k for k, *_ in kept)
    # every layer kind answers somewhere, and a table's answer carries its index
    assert {0, 1, 2, 4} <= set(keep["layer"].tolist()) and (keep["layer"] >= sg.LAYER_TABLE).sum() > 100
    assert ((keep["table"] == sg.NO_TABLE) == (keep["layer"] < sg.LAYER_TABLE)).all()
    assert {vr.VALUE, vr.NONE, vr.TOMBSTONE, vr.BAD, vr.SKIPPED} <= set(keep["status"].tolist())


@pytest.fixture(scope="module")
def truth(ora):
    w = cases.world(*sc.TRUTH)
    files = [read_fixture(NAMES[0]), read_fixture(NAMES[1]), write(ora, w.sst_items)]
    return w, cases.store(w, files)


def test_every_row_of_the_truth_table_is_in_the_ranges(truth):
    """In the world whose every layer holds its rows (the main world's one-entry read-only memtable
    holds only the first of its five)."""
    w, st = truth
    keys = ref.union(st)
    rs = sc.ranges(keys, 300)
    assert len(rs) == 300
    res = ref.scan_many(st, rs, KEEP, True)
    seen = {}
    for r in range(len(rs)):
        for k, found, layer, status in rows_of(res, r):
            seen.setdefault(k, set()).add((found, layer, status))
    for row, spec in cases.ROWS.items():
        k = cases.ROW_KEYS[row]
        held = spec[0] or spec[1] or spec[2] or spec[3]  # "nowhere" is the one row no layer holds
        assert (k in keys) == bool(held), row  # in U of its own lo == hi range at least
        assert any(lo <= k <= hi for lo, hi in rs)
        if spec[4][0] == 0:
            assert k not in seen, row
        else:
            assert seen[k] == {spec[4]}, (row, seen.get(k))


def test_the_range_set_holds_every_edge(main):
    w, st = main
    keys = ref.union(st)
    present = set(keys)
    rs = sc.ranges(keys, 300)
    assert rs[0] == sc.FULL and sc.ranges(keys, 1) == [sc.FULL] and sc.ranges(keys, 50) == rs[:50]
    assert any(lo == hi and lo in present for lo, hi in rs)
    assert any(lo == hi and lo not in present for lo, hi in rs)
    assert any(lo > hi for lo, hi in rs)
    assert any(lo == b"" and hi != b"" for lo, hi in rs)
    assert (b"k\0", b"k\0\0") in rs and (b"k\0\0", b"k\0\0") in rs and b"k\0\0" in present
    stem = [(lo, hi) for lo, hi in rs if lo.startswith(cases.STEM) and hi.startswith(cases.STEM) and lo < hi]
    assert stem and len(cases.STEM) > 8
    # lo == hi with END_EXCLUSIVE is empty, and a present hi is left out
    ex = ref.scan_many(st, rs, EXCL | KEEP)
    inc = ref.scan_many(st, rs, KEEP)
    r = rs.index((sc.PRESENT, sc.PRESENT))
    assert ex["range_off"][r] == ex["range_off"][r + 1] and inc["range_off"][r] + 1 == inc["range_off"][r + 1]
    assert ex["layer"].size < inc["layer"].size
    # some range has candidates in several layers at once and some has none
    sizes = np.diff(inc["range_off"])
    assert (sizes == 0).any() and (sizes > 100).any()
