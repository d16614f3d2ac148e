"""CPU checks of the compaction cases (compaction_cases.py) through oracle.compact_merge: every
case keeps some entries, drops some and changes the map, so a device result that equals the
oracle's has exercised the fold; and the oracle itself is pinned, on the time and map cases, by a
per-key model of the fold written from sized.rs:170-320 without looking at oracle.c's
table-at-a-time merge.

As compaction_cases.py says, `created + ttl` wraps in u64 in the oracle, the model and the kernel
alike; nothing here claims what the Rust reference does at times outside the range of real clocks."""
import numpy as np
import pytest

import compaction_cases as cc
from test_gpu_compaction import _arena


def oracle_merge(ora, case):
    runs, start, use_ttl, ettl, tttl, now = case
    keys, offs, cr, tb, ro = _arena(runs)
    m = ora.TombstoneMap(start)
    ids = ora.compact_merge(keys, offs, cr, tb, ro, use_ttl, ettl, tttl, now, m)
    return ids.tolist(), m.items()


def model_merge(case):
    """The fold one key at a time.  A key's outcome depends only on its own entries (at most one per
    table) and its own map value: merged = tables[0]; at merge j the survivor meets table j's entry
    (the newer wins, a tie goes to table j), and whatever is left passes tombstone_check again --
    also at a merge whose table has no entry of the key, or no entry at all."""
    runs, start, use_ttl, ettl, tttl, now = case
    tmap, by_key, e = dict(start), {}, 0
    for r, (ks, cr, tb) in enumerate(runs):
        for k, c, t in zip(ks, cr.tolist(), tb.tolist()):
            by_key.setdefault(k, {})[r] = (e, c, t)
            e += 1

    def expired(c, ttl):  # Entry::has_expired in u64: now > created + ttl, the sum wrapping
        return now > (c % 2**64 + ttl) % 2**64

    def check(k, c, t):  # tombstone_check (sized.rs:291-320)
        if k in tmap:
            if not c > tmap[k]:
                return False
            if t:
                tmap[k] = c
                return not expired(c, tttl)
        elif t:
            tmap[k] = c
            return not expired(c, tttl)
        return not expired(c, ettl) if use_ttl else True

    out = []
    for k in sorted(by_key):
        cur = by_key[k].get(0)
        for j in range(1, len(runs)):
            b = by_key[k].get(j)
            pick = b if cur is None else cur if b is None else (cur if cur[1] > b[1] else b)
            cur = pick if pick is not None and check(k, pick[1], pick[2]) else None
        if cur is not None:
            out.append(cur[0])
    return out, tmap


def test_case_names_and_families():
    assert len(cc.CASES) == len(cc.GEOMETRY) + len(cc.TIMES) + len(cc.MAPS) == 12 + 6 + 5
    assert set(cc.TO_FILES) <= set(cc.CASES) and cc.NO_ENTRIES in cc.GEOMETRY
    for name, fn in cc.CASES.items():  # deterministic: two calls give the same bucket
        a, b = fn(), fn()
        assert a[1:] == b[1:] and len(a[0]) == len(b[0]), name
        for (k1, c1, t1), (k2, c2, t2) in zip(a[0], b[0]):
            assert k1 == k2 and np.array_equal(c1, c2) and np.array_equal(t1, t2), name
            assert k1 == sorted(set(k1)), name  # every table strictly increasing (a SkipMap)


@pytest.mark.parametrize("name", list(cc.CASES))
def test_case_keeps_drops_and_changes_the_map(ora, name):
    case = cc.CASES[name]()
    runs, start = case[0], case[1]
    total = sum(len(ks) for ks, _, _ in runs)
    ids, new = oracle_merge(ora, case)
    print("%s: %d of %d kept, map %d -> %d keys, %d changed" % (
        name, len(ids), total, len(start), len(new), sum(1 for k in new if start.get(k) != new[k])))
    if name == cc.NO_ENTRIES:
        assert total == 0 and ids == [] and new == start
        return
    assert total <= 30_000
    assert 0 < len(ids) < total
    assert new != start and all(new[k] >= t for k, t in start.items())  # times in the map only grow


def test_geometry_sizes_are_what_they_say():
    for name, sizes in zip(cc.GEOMETRY, cc.GEOMETRY_SIZES):
        assert tuple(len(ks) for ks, _, _ in cc.CASES[name]()[0]) == sizes
    runs = cc.CASES["every_key_in_every_table"]()[0]
    assert len(runs) == 9 and all(ks == runs[0][0] and len(ks) == 600 for ks, _, _ in runs)
    runs = cc.CASES["empty_key_tables"]()[0]
    assert all(ks == [b""] for ks, _, _ in runs) and int(_arena(runs)[1][-1]) == 0  # no key bytes


def test_empty_key_tables_by_hand(ora):
    ids, new = oracle_merge(ora, cc.CASES["empty_key_tables"]())
    assert ids == [4] and new == {b"": cc.T0 + 22}


def test_time_cases_reach_every_value_and_wrap():
    for name in cc.TIMES[:-1]:
        runs, start, _, ettl, tttl, now = cc.CASES[name]()
        seen = set(np.concatenate([c for _, c, _ in runs]).tolist())
        assert seen == set(cc.TIME_VALUES) and set(start.values()) == set(cc.TIME_VALUES), name
    wraps = [(c % 2**64 + ttl) >= 2**64 for _, e, t in cc.TIME_SETTINGS for c in cc.TIME_VALUES for ttl in (e, t)]
    assert any(wraps) and not all(wraps)
    runs, start, *_ = cc.CASES["times_high_word"]()
    lows = {c & 0xFFFFFFFF for _, cr, _ in runs for c in cr.tolist()} | {t & 0xFFFFFFFF for t in start.values()}
    assert lows == {cc.T0 & 0xFFFFFFFF}
    assert len({c >> 32 for _, cr, _ in runs for c in cr.tolist()}) == 6


def test_map_cases_are_what_they_say():
    held = {k for ks, _, _ in cc.CASES["map_one_key"]()[0] for k in ks}
    lo, hi = min(held), max(held)
    assert len(cc.CASES["map_one_key"]()[1]) == 1 and set(cc.CASES["map_one_key"]()[1]) <= held
    below, above = cc.CASES["map_all_below"]()[1], cc.CASES["map_all_above"]()[1]
    assert below and all(k < lo for k in below) and above and all(k > hi for k in above)
    assert set(cc.CASES["map_every_key"]()[1]) == held
    runs, start, *_ = cc.CASES["map_time_equals_created"]()
    newest = cc.newest_created(runs)
    assert sum(1 for k, t in start.items() if newest[k] == t) >= 50


@pytest.mark.parametrize("name", cc.TIMES + cc.MAPS + ["empty_key_tables", "sizes_0_5_0_7_0", "sizes_300_0_0"])
def test_model_agrees_with_oracle(ora, name):
    case = cc.CASES[name]()
    ids, new = oracle_merge(ora, case)
    want_ids, want_map = model_merge(case)
    assert ids == want_ids
    assert new == want_map


def test_time_equal_to_created_drops_the_key(ora):
    """The c > t edge on the map_time_equals_created case: no entry of a key whose map time equals
    its newest `created` survives, and that key's map value does not move."""
    case = cc.CASES["map_time_equals_created"]()
    runs, start = case[0], case[1]
    newest = cc.newest_created(runs)
    pinned = {k for k, t in start.items() if newest[k] == t}
    ids, new = oracle_merge(ora, case)
    keys, offs = _arena(runs)[:2]
    kept = {keys[offs[i]:offs[i + 1]].tobytes() for i in ids}
    assert len(pinned) >= 50 and not (kept & pinned)
    assert all(new[k] == start[k] for k in pinned)
