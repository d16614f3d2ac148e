"""Pins the range-scan checker (tests/sst_scan_ref.py) to an independent statement of a scan -- a dict
key -> its copies, reduced by the fold's rule (scan_cases.fold) -- on the reference's fixture SSTs
and on a hand-written three-table case with a tie, a time-0 entry and a tombstone over an older live
entry, whose expected lists are written out literally (no GPU needed)."""
import numpy as np

import scan_cases as sc
import sst_get_ref as ref
import sst_scan_ref as scan_ref


def rows_of(arrays):
    """scan_many's seven arrays -> per range the list of (key, table, val, created, tomb)."""
    range_off, keys, key_off, table, val, created, tomb = arrays
    kb = keys.tobytes()
    rows = [(kb[int(key_off[i]):int(key_off[i + 1])], int(table[i]), int(val[i]), int(created[i]), int(tomb[i]))
            for i in range(table.size)]
    return [rows[int(range_off[r]):int(range_off[r + 1])] for r in range(range_off.size - 1)]


def test_hand_written_case_literally(ora):
    files = sc.hand_files(ora)
    for lo, hi, flags, order, want in sc.HAND_EXPECT:
        tabs = [files[t] for t in order]
        assert scan_ref.scan(lo, hi, tabs, flags) == want, (lo, hi, flags, order)
        assert rows_of(scan_ref.scan_many([(lo, hi)], tabs, flags)) == [want]
        holders = {}
        for t, src in enumerate(order):
            for k, v, c, tb in sc.HAND[src]:
                holders.setdefault(k, []).append((c, t, v, tb))
        assert sc.expected(holders, lo, hi, flags) == want
    # a batch: the ranges' lists back to back, range_off between them
    batch = [(lo, hi) for lo, hi, flags, order, _ in sc.HAND_EXPECT if flags == 1 and order == (0, 1, 2)]
    want = [w for _, _, flags, order, w in sc.HAND_EXPECT if flags == 1 and order == (0, 1, 2)]
    got = scan_ref.scan_many(batch, files, 1)
    assert rows_of(got) == want and got[0].tolist() == np.cumsum([0] + [len(w) for w in want]).tolist()
    assert got[2][-1] == got[1].size == sum(len(r[0]) for w in want for r in w)


def test_fixtures_against_the_independent_statement(ora):
    files = [sc.read_fixture(n) for n in sc.NAMES]
    ssts = [ref.Sst(*f) for f in files]
    holders = {}
    for t, (data, _) in enumerate(files):
        keys, offs, val, cr, tb = ora.sst_decode(np.frombuffer(data, np.uint8))
        for j in range(offs.size - 1):
            holders.setdefault(keys[int(offs[j]):int(offs[j + 1])].tobytes(), []).append(
                (int(cr[j]), t, int(val[j]), int(tb[j])))
    allk = sorted(holders)
    assert len(allk) == 19908
    full = sc.expected(holders, *sc.FULL, 0)
    assert len(full) == 19908  # no tombstone and no time 0 in the fixtures: every key is listed
    assert scan_ref.scan(*sc.FULL, ssts, 0) == full
    rng = np.random.default_rng(0x5CA9)
    ranges = [sc.FULL]
    for _ in range(12):
        i, n = int(rng.integers(0, len(allk))), int(rng.integers(0, 60))
        ranges.append((allk[i], allk[min(i + n, len(allk) - 1)]))
    ranges += [(allk[5] + b"\0", allk[9][:-1]), (allk[7], allk[7]), (allk[9], allk[3]), (b"zz", b"zzz")]
    for flags in (0, 1, 2, 3):
        want = [sc.expected(holders, lo, hi, flags) for lo, hi in ranges]
        assert rows_of(scan_ref.scan_many(ranges, ssts, flags)) == want
        for (lo, hi), w in list(zip(ranges, want))[1:6]:
            assert scan_ref.scan(lo, hi, ssts, flags) == w
    # the one key that lives in all seven tables is listed once, from the table that holds its latest copy
    shared = [k for k, h in holders.items() if len(h) > 1]
    assert len(shared) == 1
    (row,) = scan_ref.scan(shared[0], shared[0], ssts)
    assert row[1] == max(holders[shared[0]])[1] and row[3] == max(holders[shared[0]])[0]


def test_no_tables_and_empty_tables():
    empty = ref.Sst(b"", b"")
    for tabs in ([], [empty], [empty, empty]):
        got = scan_ref.scan_many([(b"", b"\xff"), (b"a", b"b")], tabs, 1)
        assert got[0].tolist() == [0, 0, 0] and got[2].tolist() == [0] and all(a.size == 0 for a in got[3:])
        assert scan_ref.scan(b"", b"\xff", tabs) == []
