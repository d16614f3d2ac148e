"""vbf_memtable_sort_host, vbf_flush_write_host and vbf_filter_insert_host under concurrent callers
on one device (include/vbf.h, "Threads").  Four threads, each with a batch of its own; one
device-resident filter is shared by all of them (two flush into it, two insert into it).  The
expected outputs come from the Python restatement and from a serial run before any thread starts;
every answer is compared on the main thread after the threads have ended.

The shared filter's element count depends on the order the threads reach it, so only its bits are
checked: the OR of all the batches."""
import threading
import traceback

import numpy as np
import pytest

import memtable_ref as ref

pytestmark = pytest.mark.gpu
THREADS, ROUNDS = 4, 4
CAP = 120.0  # seconds after which a thread still alive counts as hung (a deadlock guard)
M, K = 200_003, 7


def _batch(t):
    rng = np.random.default_rng(0x3E37 + t)
    n = 3000 + 1100 * t
    uni = [b"t%d-" % t + rng.bytes(int(L)) for L in rng.integers(0, 20, n // 3)]
    keys = [uni[i] for i in rng.integers(0, len(uni), n)]
    return keys, rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)


def _run(t, job, shared):
    """One round of thread t: a sort, a flush (into the shared filter on even threads) and an insert
    (into the shared filter on odd threads, into a filter of its own otherwise)."""
    from velarixdb_amd import BloomFilter, memtable
    keys, val = job
    ids = memtable.sort_ids(keys)
    res = memtable.flush(keys, val, filter=shared if t % 2 == 0 else None)
    own = BloomFilter.sized(M, K)
    n_new = (shared if t % 2 else own).insert_many(keys)
    return ids, res.data, res.index, res.ids, n_new, own.words()


def _check(t, job, got, want):
    ids, data, index, rids, n_new, own = got
    assert np.array_equal(ids, ref.sort_ids(job[0])) and np.array_equal(rids, ids)
    assert np.array_equal(data, want[1]) and np.array_equal(index, want[2])
    if t % 2 == 0:  # the filter of its own: the single caller's count and bits
        assert n_new == want[4] and np.array_equal(own, want[5])


def test_four_threads_sort_flush_and_insert(vbf, ora):
    from velarixdb_amd import BloomFilter
    from velarixdb_amd.keys import pack
    jobs = [_batch(t) for t in range(THREADS)]
    serial = BloomFilter.sized(M, K)
    want = [_run(t, jobs[t], serial) for t in range(THREADS)]  # the single-caller answers
    for t in range(THREADS):
        _check(t, jobs[t], want[t], want[t])
    all_bits = ora.build_words(pack([k for keys, _ in jobs for k in keys]), M, K)
    assert np.array_equal(serial.words(), all_bits)
    shared = BloomFilter.sized(M, K)
    results, errors = [[] for _ in range(THREADS)], []
    start = threading.Barrier(THREADS)

    def work(t):
        try:
            start.wait()
            for _ in range(ROUNDS):
                results[t].append(_run(t, jobs[t], shared))
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
            _check(t, jobs[t], got, want[t])
    assert np.array_equal(shared.words(), all_bits)
    assert 0 < shared.num_elements() <= sum(len(set(keys)) for keys, _ in jobs)
