"""The dictionary against the store composed from the checkers (tests/store_model.py).  CPU only.

This file settles what the dictionary may be held to before any GPU run: wherever the composition
of the reference's steps and "last put wins" part, the composition is the expectation and the
claim is dropped here, with the reference lines that cause it.

Kept, for every scenario:
  * after every generation a get of every universe key and of 200 absent keys, and the full-range
    and sub-range scans, equal the dictionary (found code, created_at, value);
  * recover(head), head at the last put of generation g, yields exactly the puts of generations
    g + 1 onward (recovery.rs:261-264 drops the head entry), and a log cut 3 bytes short loses its
    last put alone;
  * after gc + apply_gc no live answer carries a val_offset inside [tail, new_tail), except for the
    keys named below.

Kept where created_at stays below 2^63 (every scenario but "big"):
  * after a full compaction with a fresh tombstone map and no expiry the one table reads back the
    dictionary.

Dropped:
  * Partial compaction (two buckets of three tables, the runner's tombstone map kept between them)
    does not read back the dictionary: tombstone_check (sized.rs:286-320) drops a tombstone at the
    merge after the one that recorded it, because `created > map time` is false for the tombstone
    itself, and a put of the key in a table outside the bucket shows again.  Every scenario asserts
    that this happens for at least one key.
  * With created_at >= 2^63 ("big", last generation) a full compaction does not read back the
    dictionary either: the fold compares created_at as the signed DateTime of the reference
    (sized.rs:249 and :298; i64 in the arena), the lookups compare the u64 of the file
    (store.rs:579-612 as sst_get_ref restates it), so the put the get calls newest loses the merge.
  * After gc + apply_gc a key whose most recent value is empty and whose entry the chunk held reads
    as deleted: GC::put stores is_tombstone = value.is_empty() (garbage_collector.rs:404-419).
    Every other key, and the new `tail` key, reads back the dictionary.
  * After gc + apply_gc a live key whose value is "*" keeps its val_offset inside the collected
    chunk: the handler calls such an entry invalid (garbage_collector.rs:205-208) and does not
    rewrite it, though no newer entry exists.
"""
import struct
import time

import numpy as np
import pytest

import store_model as sm
import vlog_walk_ref as wr

NAMES = list(sm.SCENARIOS)
_built = {}


def built(ora, name):
    """The scenario's store after all generations, built once; tests that change it clone it."""
    if name not in _built:
        t = time.perf_counter()
        _built[name] = sm.build(ora, name)
        print("%s: generated and composed in %.2f s" % (name, time.perf_counter() - t))
    return _built[name]


def all_keys(h):
    return h.universe + h.absent


def reads_differ(store, keys):
    """The keys whose get over the files is not the dictionary's answer."""
    return [k for k in keys if store.get(k)[4] != store.expect(k)]


def check_reads(store, h):
    for k in all_keys(h):
        found, _, _, created, value = store.get(k)
        hit = store.dict.get(k)
        if hit is None:
            assert (found, value) == (0, None), k
        else:
            assert (found, created, value) == (2 if hit[2] else 1, hit[1], None if hit[2] else hit[0]), k


def check_scans(store, h):
    log, base = store.log_bytes(), store.base
    for (lo, hi), flags in [(sm.FULL, 0), (sm.FULL, sm.END_EXCLUSIVE)] + [(r, 0) for r in h.ranges[:5] + h.ranges[-1:]] + \
            [(h.ranges[0], sm.END_EXCLUSIVE)]:
        got = [(k, sm.vr.get(log, vo, base, k)[1]) for k, _, vo, _, _ in store.scan(lo, hi, flags)]
        assert got == store.expect_slice(lo, hi, flags), (lo, hi, flags)


def test_the_generator_cuts_at_the_edges():
    sizes = set()
    for name in NAMES:
        h = sm.history(name)
        sizes.update(h.scenario.sizes)
        assert len(h.universe) <= 4000 and len(h.absent) == 200 and not set(h.absent) & set(h.universe)
        put = set().union(*[g.keys for g in h.gens])
        assert put <= set(h.universe)
        assert {b"", b"a", b"abcdefg", sm.LONGEST, sm.STEM, sm.STEM + b"\0"} <= put, name
        clock = np.concatenate([g.created for g in h.gens])
        assert (np.diff(clock.astype(object)) >= 0).all() and clock[0] > sm.T0  # never decreases, as u64
        for g, (a, b) in enumerate(zip(h.gens, h.gens[1:])):                    # no tie crosses tables but the seam
            assert int(a.created[-1]) < int(b.created[0]) or g == h.scenario.seam_gen
        ties = any((np.diff(g.created.astype(object)) == 0).any() for g in h.gens)
        assert ties == h.scenario.ties
        if not ties:  # strictly increasing, but for the one tie at the seam
            assert (np.diff(clock.astype(object)) == 0).sum() == (h.scenario.seam_gen >= 0)
        deletes = np.concatenate([g.tombs for g in h.gens]).mean()
        assert 0.1 < deletes < 0.25
        vals = [v for g in h.gens for v in g.values]
        assert b"" in vals and b"*" in vals and max(map(len, vals)) >= 190
    assert sizes == {1, 300, 2047, 2049, 4097, 6145}
    big = sm.history("big")
    assert big.scenario.base == 12_345 and sm.history("plain").scenario.base == 0
    assert int(big.gens[-1].created[0]) >= 2**63 and all(int(g.created[-1]) < 2**63 for g in big.gens[:-1])
    log = sum(17 + len(k) + len(v) for g in big.gens for k, v in zip(g.keys, g.values))
    assert log > 8 * 1024 * 1024 and big.scenario.base + log < 2**32
    assert sorted(len(v) for g in big.gens for v in g.values)[-7:] == [70_000] + [1536 * 1024] * 6
    seam = sm.history("partial")
    a, b = seam.gens[seam.scenario.seam_gen], seam.gens[seam.scenario.seam_gen + 1]
    assert (a.keys[-1], a.values[-1], a.created[-1], a.tombs[-1]) == (b.keys[0], b.values[0], b.created[0], b.tombs[0])
    assert sum(g.keys.count(sm.SEAM_KEY) for g in seam.gens) == 2 and b.created[-1] > b.created[0]
    again = sm.history.__wrapped__("tiles")
    assert again.gens[3].keys == sm.history("tiles").gens[3].keys and again.ranges == sm.history("tiles").ranges


@pytest.mark.parametrize("name", NAMES)
def test_reads_after_every_generation(ora, name):
    h = sm.history(name)
    t = time.perf_counter()
    store = sm.ModelStore(ora, h.scenario.base)
    for g in h.gens:
        store.put_batch(g.keys, g.values, g.created, g.tombs)
        check_reads(store, h)
        check_scans(store, h)
    print("%s: every generation read back in %.2f s" % (name, time.perf_counter() - t))


@pytest.mark.parametrize("name", NAMES)
def test_full_compaction_reads_back_the_dictionary(ora, name):
    h = sm.history(name)
    store = built(ora, name)[0].clone()
    every = list(range(len(store.tables)))
    for order in (every, every[::-1]):
        s = store.clone()
        s.replace(order, s.compact(order, ora.TombstoneMap()))
        assert len(s.tables) == 1
        wrong = reads_differ(s, all_keys(h))
        if h.scenario.high_clock_gen < 0:
            assert not wrong
            check_scans(s, h)
        else:  # created_at >= 2^63: the fold's signed compare keeps the older put (module docstring)
            late = set(h.gens[h.scenario.high_clock_gen].keys)
            assert wrong and set(wrong) <= late


@pytest.mark.parametrize("name", NAMES)
def test_partial_compaction_resurrects_an_older_put(ora, name):
    h = sm.history(name)
    s = built(ora, name)[0].clone()
    tmap = ora.TombstoneMap()
    s.replace((0, 1, 2), s.compact((0, 1, 2), tmap))
    first = len(tmap)
    s.replace((1, 2, 3), s.compact((1, 2, 3), tmap))  # generations 3-5; the first merged table stays outside
    assert len(s.tables) == len(h.gens) - 4 and first > 0 and len(tmap) > first
    back = [k for k in reads_differ(s, all_keys(h)) if s.expect(k) is None and s.get(k)[4] is not None]
    assert back, "no deleted key shows an older put again: the seed does not exercise the path"
    for k in back[:20]:  # deleted in the second bucket, the put that shows lies in the first
        assert s.get(k)[1] == 0 and s.dict[k][2] == 1 and tmap.get(k) == s.dict[k][1]


@pytest.mark.parametrize("name", NAMES)
def test_gc_then_reads(ora, name):
    h = sm.history(name)
    store, steps = built(ora, name)
    s = store.clone()
    tail, chunk = sm.gc_chunk([offs for _, offs, _ in steps], s.base)
    res = s.gc(tail, chunk)
    new_tail = res["new_tail"]
    assert steps[1][1][0] < new_tail <= steps[1][1][-1]  # the chunk ends inside generation 1
    entries = wr.walk(s.log_bytes(), tail, chunk, s.base)[0]
    why = {"valid": 0, "overwritten": 0, "deleted": 0, "star": 0, "empty": 0}
    for i, (_, key, _, created, _) in enumerate(entries):
        got = s.lookup(key)
        kind = "deleted" if got is None else "star" if got[0] == b"*" else "overwritten" if created < got[1] else \
            "empty" if got[0] == b"" else "valid"
        why[kind] += 1
        assert (i in res["invalid"]) == (kind in ("deleted", "star", "overwritten"))
    assert all(why.values()), why
    # the GC's puts carry its clock: one loses the get to a put at 2^63 or later ("big")
    rewritten_empty = {k for k, v, *_ in res["append"][1:] if v == b"" and s.dict[k][1] < sm.GC_NOW}
    star_live = {e[1] for e in entries if s.expect(e[1]) == b"*" and tail <= s.get(e[1])[2] < new_tail}
    s.apply_gc(res)
    assert s.dict[b"tail"][0] == struct.pack("<Q", new_tail) and s.get(b"tail")[4] == struct.pack("<Q", new_tail)
    keys = all_keys(h) + [b"tail"]
    assert set(reads_differ(s, keys)) == rewritten_empty and rewritten_empty
    assert all(s.get(k)[0] == 2 for k in rewritten_empty)  # GC::put wrote them as tombstones
    inside = {k for k in keys if s.get(k)[0] == 1 and tail <= s.get(k)[2] < new_tail}
    assert inside == star_live


@pytest.mark.parametrize("name", NAMES)
def test_recover_yields_the_later_generations(ora, name):
    h = sm.history(name)
    store, steps = built(ora, name)
    puts = [[(o, k, v, int(c) - 2**64 if int(c) >= 2**63 else int(c), int(t))
             for o, k, v, c, t in zip(offs, g.keys, g.values, g.created, g.tombs)] for (_, offs, _), g in zip(steps, h.gens)]
    for g in range(len(h.gens)):
        later = [p for gen in puts[g + 1:] for p in gen]
        assert store.recover(steps[g][1][-1]) == later
    assert store.recover(steps[0][1][-1], cut=3) == [p for gen in puts[1:] for p in gen][:-1]
