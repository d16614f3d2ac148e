"""CPU checks of the jobs of host_call_cases.py, which test_gpu_host_threads.py hands to concurrent
threads: every expectation is non-trivial (hits and misses, non-empty ranges, merges that drop and
keep), and the jobs that different threads hold in one round differ in their inputs, their sizes
and their expected bytes -- two identical jobs could swap answers without anyone noticing."""
import itertools

import numpy as np
import pytest

import compaction_cases as cc
import host_call_cases as hc

FAMILIES = {
    "encode": hc.encode_jobs, "decode": hc.decode_jobs, "open": hc.open_jobs, "get": hc.get_jobs,
    "scan": hc.scan_jobs, "merge": hc.merge_jobs, "write": hc.write_jobs, "probe": hc.probe_jobs,
    "rebuild": hc.rebuild_jobs,
}
# how many different sizes the family's rotation holds
SIZES = {"encode": 5, "decode": 5, "open": 6, "get": 4, "scan": 4, "merge": 4, "write": 4, "probe": 2, "rebuild": 4}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_threads_hold_different_jobs_in_every_round(ora, family):
    per_thread = FAMILIES[family](ora)
    assert len(per_thread) == hc.THREADS and all(len(jobs) == hc.ROUNDS >= 12 for jobs in per_thread)
    for r in range(hc.ROUNDS):
        row = [jobs[r] for jobs in per_thread]
        for a, b in itertools.combinations(row, 2):
            # rebuild: the SST alone is the input (args[2:]); its first two name the thread's filter
            ia, ib = (a.args[2:], b.args[2:]) if family == "rebuild" else (a.args, b.args)
            assert hc.fingerprint(ia) != hc.fingerprint(ib), (family, r, a.ident, b.ident)
            assert hc.fingerprint(a.want) != hc.fingerprint(b.want), (family, r, a.ident, b.ident)
        assert len({j.size for j in row}) == min(hc.THREADS, SIZES[family]), (family, r)
    for jobs in per_thread:  # one thread: the sizes go up and down, never twice the same in a row
        sizes = [j.size for j in jobs]
        assert all(a != b for a, b in zip(sizes, sizes[1:]))
        assert any(a < b for a, b in zip(sizes, sizes[1:])) and any(a > b for a, b in zip(sizes, sizes[1:]))


def test_jobs_are_deterministic(ora):
    hc.get_case.cache_clear()
    a = hc.get_jobs(ora)[1][1]
    hc.get_case.cache_clear()
    b = hc.get_jobs(ora)[1][1]
    assert a is not b and a.args == b.args and hc.blob(a.want) == hc.blob(b.want)


def test_encode_and_decode_tables(ora):
    seen = set()
    for jobs in hc.encode_jobs(ora):
        for j in jobs[:len(hc.SST_SIZES)]:
            keys, offs, val, cr, tb = j.args
            data, index, blocks = j.want
            lens = np.diff(offs)
            seen.add(j.size)
            assert data.size == int(offs[-1]) + 17 * j.size and blocks.size >= 1 and blocks[0] == 0
            if j.ident.endswith("block"):
                assert lens.tolist() == list(hc.BLOCK_LENS) and blocks.tolist()[:2] == [0, 4096]  # a full first block
            elif j.size >= 300:
                assert lens.min() == 0 and lens.max() == 70 and blocks.size > 1
                assert 0 < int(tb.sum()) < j.size
    assert seen == {1, 4, 300, 5_000, 40_000}
    for jobs in hc.decode_jobs(ora):
        for j in jobs[:len(hc.SST_SIZES)]:
            assert j.want[1].size == j.size + 1 and j.want[0].size == int(j.want[1][-1])


def test_gets_hit_and_miss(ora):
    assert [len(s.ikeys) > 1 for s in hc.read_tables(ora)[2]] == [True] * 3  # several blocks per table
    for jobs in hc.get_jobs(ora):
        for j in jobs[:len(hc.GET_SIZES)]:
            found, table, val, created = j.want
            assert len(j.args[0]) == j.size == found.size
            if j.size >= 257:
                assert (found == 0).any() and (found == 1).any() and (found == 2).any()
                assert len(set(table[found != 0].tolist())) == 3  # every table wins somewhere
    assert {j.size for j in hc.get_jobs(ora)[0]} == {1, 257, 4_099, 20_000}
    assert hc.get_jobs(ora, with_filters=True)[0][0].want is hc.get_jobs(ora)[0][0].want


def test_scans_list_entries_under_both_flags(ora):
    flags = set()
    for jobs in hc.scan_jobs(ora):
        for j in jobs[:len(hc.SCAN_SHAPES)]:
            ranges, f = j.args
            range_off, keys, key_off, table, val, created, tomb = j.want
            flags.add(f)
            assert len(ranges) == j.size == range_off.size - 1
            n = int(range_off[-1])
            assert n > 0 and key_off.size == n + 1 and keys.size == int(key_off[-1]) > 0
            assert bool(tomb.any()) == bool(f & hc.KEEP) or j.size == 1
            if j.size >= 64:
                assert (np.diff(range_off) > 0).sum() > j.size // 2
    assert flags == {0, hc.KEEP, hc.EXCL, hc.KEEP | hc.EXCL}
    assert {j.size for j in hc.scan_jobs(ora)[0]} == {1, 7, 64, 400}


def test_open_tables(ora):
    jobs = hc.open_jobs(ora)[0][:6]
    assert {1, 300, 5_000} < {j.want[0] for j in jobs}
    assert len({j.want[2:] for j in jobs}) == 6  # six different key ranges
    assert all(j.want[1] >= 1 and j.want[2] <= j.want[3] for j in jobs)
    assert max(j.want[1] for j in jobs) > 20


def test_merges_drop_and_keep(ora):
    totals = []
    for j in hc.merge_jobs(ora)[0][:len(hc.MERGE_CASES)]:
        ids, new = j.want
        start = cc.CASES[j.ident]()[1]
        totals.append(j.size)
        assert 0 < ids.size < j.size and new != start
    assert min(totals) < 20 and max(totals) > 6_000
    assert set(hc.MERGE_CASES[2:]) <= set(cc.TO_FILES) and set(hc.MERGE_CASES[:2]) <= set(cc.GEOMETRY)
    for j in hc.write_jobs(ora)[0][:len(hc.MERGE_CASES)]:
        data, index, m, k, words, n, new = j.want
        assert data.size > 17 * n > 0 and index.size > 0 and words.size == (m + 31) // 32 and words.any() and k > 0


def test_probes_hit_and_miss_in_disjoint_sets(ora):
    a, b = hc.probe_set(ora, 0), hc.probe_set(ora, 1)
    assert not ({k for f in a for k in f[0]} & {k for f in b for k in f[0]})
    assert len({(f[1], f[2]) for f in a + b}) >= 2 and all(f[3].any() for f in a + b)
    for jobs in hc.probe_jobs(ora):
        for j in jobs[:4]:
            (want,) = j.want
            assert want.shape == (j.size, 3) and j.size in hc.PROBE_BATCHES and j.size > 256
            for col in range(3):
                assert 0 < int(want[:, col].sum()) < j.size
            assert (want.sum(axis=1) >= 2).any()  # a key in two overlapping filters


def test_rebuilds(ora):
    seen = set()
    for j in hc.rebuild_jobs(ora)[0][:4]:
        n, m, k, words = j.want
        seen.add((m, k))
        assert n == j.size and 0 < int(np.unpackbits(words.view(np.uint8)).sum()) < m
    assert len(seen) == 4
    filters = {j.args[:2] for jobs in hc.rebuild_jobs(ora) for j in jobs}
    assert len(filters) == 16  # a filter per (thread, SST): no two threads write one filter


def test_rebuilds_that_take_the_partitioned_build(ora):
    per_thread = hc.rebuild_build_jobs(ora)
    assert len(per_thread) == hc.BUILD_THREADS == 2 and all(len(jobs) == hc.BUILD_ROUNDS == 12 for jobs in per_thread)
    for r in range(hc.BUILD_ROUNDS):
        a, b = per_thread[0][r], per_thread[1][r]
        assert {a.size, b.size} == {240_000, 3_000}, r  # one of each kind in every round
        assert hc.fingerprint(a.args[2:]) != hc.fingerprint(b.args[2:]) and hc.fingerprint(a.want) != hc.fingerprint(b.want)
    for jobs in per_thread:
        assert all(x.size != y.size for x, y in zip(jobs, jobs[1:]))  # alternating
        for j in jobs[:2]:
            n, m, k, words = j.want
            assert k == 19 and m == ora.num_bits(n, hc.P_BUILD) and words.size == (m + 31) // 32
            assert (n * k >= 2**22) == (n == 240_000)  # AUTO's threshold between the two builds
            assert 0 < int(np.unpackbits(words.view(np.uint8)).sum()) < m
    tables = {j.args[:2] for jobs in per_thread for j in jobs}
    assert len(tables) == 4  # a filter per (thread, SST)


def test_one_shot_and_flush_jobs(ora):
    for j in hc.build_host_jobs(ora)[:4]:
        keys, m, k = j.args
        assert j.want[0].any() and keys.n == j.size
    for j in hc.probe_host_jobs(ora)[:4]:
        hits = j.want[0]
        assert hits[:(j.size + 1) // 2].all() and not hits.all()  # every member is found, not every stranger
    assert {j.size for j in hc.flush_jobs(ora)} == set(hc.FLUSH_SIZES)
    for j in hc.flush_jobs(ora)[:4]:
        data, index, entries, blocks, lo, hi = j.want
        assert entries == j.size and lo <= hi and data.size > 0 and index.size > 0


def test_lock_order_case(ora):
    lo = hc.lock_order_case(ora)
    assert len(lo["others"]) >= 12 and not (set(lo["t_keys"]) & {k for b in lo["others"] for k in b})
    first, final = lo["first"], lo["final"]
    assert (first & final == first).all() and (final != first).any()  # bits are only added
    jobs = hc.lock_order_probe_jobs(ora)
    assert {j.size for j in jobs} == set(hc.PROBE_BATCHES)
    for j in jobs:
        exact, before, after = j.want
        assert not exact[:, 0].any() and exact[:, 1].any() and exact[:, 2].any()
        assert (before <= after).all() and before.any() and not after.all()
