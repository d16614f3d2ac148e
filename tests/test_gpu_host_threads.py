"""The host entry points under concurrent callers (include/vbf.h, "Threads").

Every `_host` entry point stages into workspaces cached on the device's shared stream.  The library
serialises such calls per device (Staging::host_mu, csrc/vbf_api.hip); without that, two threads
inside one of them read each other's staged keys, offsets or descriptors, or use a workspace the
other has just freed to grow it.  Here up to 8 threads of this process call them at once, each with
jobs of its own from host_call_cases.py, whose expected outputs (the C oracle, sst_get_ref,
sst_scan_ref) were computed before any thread started and differ between the threads of a round.
Every output is compared byte for byte, on the main thread, after the threads have ended.

Each test first runs its jobs on one thread, interleaved round-robin -- the order a lock would
produce -- and compares them: a wrong expectation or stale bytes from an earlier, larger call on a
workspace that only grows fail there, not in the threaded run.  The threaded run then asserts that
every pair of threads overlapped in time, and a thread still inside a call 120 s after the start
fails the test with the call's name (a deadlock guard, not a timing claim: the serial run of the
same jobs takes well under a tenth of that, printed and asserted).

Which workspace slots the threads of each test would share without the lock is listed at the test."""
import threading
import time
import traceback

import numpy as np
import pytest

import host_call_cases as hc

pytestmark = pytest.mark.gpu
CAP = 120.0  # seconds after the common start at which a thread still alive counts as hung


# ---- what the jobs run on -----------------------------------------------------------------------

class Ctx:
    """The handles the jobs share: the three read tables open on the device, a filter per table
    rebuilt from its SST, the two probe sets, a filter per (thread, SST) for the rebuilds."""

    def __init__(self, vbf, ora):
        from velarixdb_amd import Table
        from velarixdb_amd.key_range import SstRange
        self.vbf, self.ora = vbf, ora
        _, files, parsed, _ = hc.read_tables(ora)
        self.tables = [Table.open(d, i) for d, i in files]
        self.filters = []
        for t, (d, i) in enumerate(files):
            m, k, words = hc.rebuild_words(ora, t)
            f = vbf.BloomFilter(hc.P, len(parsed[t].fields))
            assert f.rebuild_from_sst(d, i) == len(parsed[t].fields)
            assert (f.num_bits(), f.no_of_hash_func) == (m, k) and np.array_equal(f.words(), words)
            self.filters.append(f)
        self.probe_ranges = []
        for which in (0, 1):
            ranges = []
            for keys, m, k, words, lo, hi in hc.probe_set(ora, which):
                f = vbf.BloomFilter.sized(m, k, hc.P)
                f.set_many(keys)
                assert np.array_equal(f.words(), words)
                ranges.append(SstRange(lo, hi, f))
            self.probe_ranges.append(ranges)
        self.rebuild_filters = {(t, i): vbf.BloomFilter(hc.P, n)
                                for t in range(hc.THREADS) for i, n in enumerate(hc.REBUILD_SIZES)}
        self.build_filters = {}  # (thread, SST) -> the filter of a rebuild_build job
        self.packed = {}       # job ident -> HostBatch: packed once, in the serial run
        self.sst_tables = {}   # merge case -> [SstEntries]
        self.lock_filter = None
        self.lock_ranges = None

    def batch(self, job, keys):
        key = (job.call, job.ident)
        if key not in self.packed:
            from velarixdb_amd.keys import pack
            self.packed[key] = pack(keys)
        return self.packed[key]


@pytest.fixture(scope="module")
def ctx(vbf, ora):
    c = Ctx(vbf, ora)
    yield c
    for t in c.tables:
        t.close()


def _get(job, ctx, filters=None):
    from velarixdb_amd import get_many
    r = get_many(ctx.batch(job, job.args[0]), ctx.tables, filters)
    return r.found, r.table, r.val_offsets, r.created_ms


def run_encode(job, ctx):
    from test_gpu_sst_encode import encode_host
    keys, offs, val, cr, tb = job.args
    return encode_host(keys, offs, 0, job.size, val, cr, tb)


def run_decode(job, ctx):
    e = ctx.vbf.sst.load_entries(*job.args)
    return e.keys, e.offsets, e.val_offsets, e.created_ms, e.tombstones.astype(np.uint8)


def run_open(job, ctx):
    from velarixdb_amd import Table
    with Table.open(*job.args) as t:
        return (t.entries, t.blocks) + t.key_range()


def run_scan(job, ctx):
    from velarixdb_amd.table import scan_many
    ranges, flags = job.args
    r = scan_many(ranges, ctx.tables, keep_tombstones=bool(flags & hc.KEEP), end_exclusive=bool(flags & hc.EXCL))
    return r.range_off, r.keys, r.key_off, r.table, r.val_offsets, r.created_ms, r.tombstones


def run_scan_two_calls(job, ctx):
    """The sizing protocol by hand (scan_host of test_gpu_table_scan.py): it asserts that the size
    query and the filling call report the same sizes and that nothing is written past them."""
    from test_gpu_table_scan import scan_host
    ranges, flags = job.args
    got, _ = scan_host([t._h for t in ctx.tables], ranges, flags)
    return got


def run_merge(job, ctx):
    from test_gpu_compaction_shapes import _host_merge
    ids, new = _host_merge(*job.args)
    return np.asarray(ids, np.uint32), new


def run_write(job, ctx):
    from test_gpu_compaction_shapes import _bucket, _merger, _sst_tables
    name, val = job.args
    case = _bucket(name)[0]
    if name not in ctx.sst_tables:
        ctx.sst_tables[name] = _sst_tables(case[0], val)
    mg = _merger(name)
    data, index, bf, n = mg.merge_bucket_sst(ctx.sst_tables[name], now_ms=case[5])
    assert bf.num_elements() == n
    return data, index, bf.num_bits(), bf.no_of_hash_func, bf.words(), n, mg.tombstones


def run_probe(job, ctx):
    from velarixdb_amd.key_range import candidates
    which, queries = job.args
    return (candidates(ctx.batch(job, queries), ctx.probe_ranges[which]).astype(np.uint8),)


def run_rebuild(job, ctx):
    t, i, data, index = job.args
    f = ctx.rebuild_filters[t, i]
    return f.rebuild_from_sst(data, index), f.num_bits(), f.no_of_hash_func, f.words()


def run_rebuild_build(job, ctx):
    t, i, data, index = job.args
    if (t, i) not in ctx.build_filters:  # created in the serial control, which runs first
        ctx.build_filters[t, i] = ctx.vbf.BloomFilter(hc.P_BUILD, job.size)
    f = ctx.build_filters[t, i]
    return f.rebuild_from_sst(data, index), f.num_bits(), f.no_of_hash_func, f.words()


def run_build_host(job, ctx):
    from velarixdb_amd._lib import call
    keys, m, k = job.args
    words = np.zeros((m + 31) // 32, np.uint32)
    d, o = keys.ptrs()
    call("vbf_build_host", d, o, keys.stride, keys.n, keys.len_prefix, m, k, words.ctypes.data, words.size, 0)
    return (words,)


def run_probe_host(job, ctx):
    from velarixdb_amd._lib import call
    q, m, k, words = job.args
    out = np.full(q.n, 9, np.uint8)
    d, o = q.ptrs()
    call("vbf_probe_host", d, o, q.stride, q.n, q.len_prefix, m, k, words.ctypes.data, words.size, out.ctypes.data, 0)
    return (out,)


def run_flush(job, ctx):
    from velarixdb_amd import Table
    from velarixdb_amd.sst import SstEntries, write_entries
    keys, offs, val, cr, tb = job.args
    data, index = write_entries(SstEntries(keys, offs, val, cr, tb.astype(bool)))
    with Table.open(data, index) as t:
        return (data, index, t.entries, t.blocks) + t.key_range()


def run_lock_set(job, ctx):
    keys, asynchronous = job.args
    if asynchronous:
        ctx.lock_filter.set_many_async(ctx.batch(job, keys))
    else:
        ctx.lock_filter.set_many(ctx.batch(job, keys))
    return ()


def run_lock_probe(job, ctx):
    from velarixdb_amd.key_range import candidates
    return (candidates(ctx.batch(job, job.args[0]), ctx.lock_ranges).astype(np.uint8),)


def run_lock_rebuild(job, ctx):
    return (ctx.lock_filter.rebuild_from_sst(*job.args),)


def run_release(job, ctx):
    from velarixdb_amd._lib import call
    call("vbf_release_workspaces")
    return ()


RUN = {
    "release": run_release,
    "encode": run_encode, "decode": run_decode, "open": run_open, "get": _get,
    "get_filtered": lambda job, ctx: _get(job, ctx, ctx.filters), "scan": run_scan,
    "scan_two_calls": run_scan_two_calls, "merge": run_merge, "write": run_write, "probe": run_probe,
    "rebuild": run_rebuild, "rebuild_build": run_rebuild_build, "build_host": run_build_host, "probe_host": run_probe_host, "flush": run_flush,
    "lock_set": run_lock_set, "lock_probe": run_lock_probe, "lock_rebuild": run_lock_rebuild,
    "lock_get": lambda job, ctx: _get(job, ctx, [ctx.lock_filter] + ctx.filters[1:]),
}


# ---- comparing ----------------------------------------------------------------------------------

def check(job, got):
    where = "%s %s" % (job.call, job.ident)
    if job.call == "lock_probe":
        # the written filter's column lies between its bits before and after; the others are exact
        (c,), (exact, before, after) = got, job.want
        assert np.array_equal(c[:, 1:], exact[:, 1:]), where
        assert (before <= c[:, 0]).all(), where + ": a false negative in the filter being written"
        assert (c[:, 0] <= after).all(), where + ": a hit that the final bits do not explain"
        return
    assert len(got) == len(job.want), where
    for i, (g, w) in enumerate(zip(got, job.want)):
        if hc.blob(g) != hc.blob(w):
            detail = ""
            if isinstance(g, np.ndarray) and isinstance(w, np.ndarray):
                detail = ": %d vs %d items" % (g.size, w.size)
                if g.shape == w.shape:
                    bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
                    detail = ": %d of %d items differ, first at %d" % (bad.size, g.size, bad[0] if bad.size else -1)
            raise AssertionError("%s: output %d differs from the expectation%s" % (where, i, detail))


def run_serial(per_thread, ctx):
    """The control: the same jobs on this thread, round-robin over the lists.  -> seconds"""
    t0 = time.perf_counter()
    for r in range(max(len(jobs) for jobs in per_thread)):
        for jobs in per_thread:
            if r < len(jobs):
                check(jobs[r], RUN[jobs[r].call](jobs[r], ctx))
    took = time.perf_counter() - t0
    print("serial control: %d jobs in %.3f s" % (sum(len(j) for j in per_thread), took))
    assert took < CAP / 10, "the serial control took %.1f s: shrink the jobs, the hang cap is %d s" % (took, CAP)
    return took


def run_threads(jobs_per_thread, ctx):
    """Starts one daemon thread per job list behind a barrier, joins them with the cap, then checks
    on this thread: nobody hung, nobody raised, every pair overlapped, every output is right."""
    n = len(jobs_per_thread)
    assert 2 <= n <= 8 and all(len(jobs) >= 12 for jobs in jobs_per_thread)
    barrier = threading.Barrier(n + 1)
    state = [dict(at="the barrier", out=[], err=None, t0=None, t1=None) for _ in range(n)]

    def body(i):
        st = state[i]
        try:
            barrier.wait(CAP)
            st["t0"] = time.monotonic()
            for job in jobs_per_thread[i]:
                st["at"] = "%s %s" % (job.call, job.ident)
                st["out"].append(RUN[job.call](job, ctx))
            st["at"] = None
        except BaseException:
            st["err"] = traceback.format_exc()
        finally:
            st["t1"] = time.monotonic()

    threads = [threading.Thread(target=body, args=(i,), daemon=True, name="caller-%d" % i) for i in range(n)]
    for th in threads:
        th.start()
    barrier.wait(CAP)
    start = time.monotonic()
    for th in threads:
        th.join(max(0.0, start + CAP - time.monotonic()))
    hung = ["thread %d in %s" % (i, state[i]["at"]) for i, th in enumerate(threads) if th.is_alive()]
    if hung:
        # the thread holds locks of the library: no later GPU test of this process could finish
        pytest.exit("still inside a call %d s after the common start: %s" % (CAP, "; ".join(hung)), returncode=1)
    for i, st in enumerate(state):
        assert st["err"] is None, "thread %d raised in %s:\n%s" % (i, st["at"], st["err"])
    for a in range(n):
        for b in range(a + 1, n):
            both = min(state[a]["t1"], state[b]["t1"]) - max(state[a]["t0"], state[b]["t0"])
            assert both > 0, "threads %d and %d never ran at the same time" % (a, b)
    spans = [st["t1"] - st["t0"] for st in state]
    shared = min(st["t1"] for st in state) - max(st["t0"] for st in state)
    print("threads: %s; all %d at once for %.3f s" % (
        ", ".join("%d %s jobs in %.3f s" % (len(jobs), jobs[-1].call, t) for jobs, t in zip(jobs_per_thread, spans)),
        n, shared))
    for jobs, st in zip(jobs_per_thread, state):
        assert len(st["out"]) == len(jobs)
        for job, got in zip(jobs, st["out"]):
            check(job, got)


def both(per_thread, ctx):
    run_serial(per_thread, ctx)
    run_threads(per_thread, ctx)


# ---- 1. one entry point, different inputs, four threads ----------------------------------------

# the workspace slots (WsSlot, csrc/vbf_api.hip) the four threads of each family would share
FAMILIES = {
    "encode": (hc.encode_jobs, "kWsSstEncIO, kWsSstEnc"),
    "decode": (hc.decode_jobs, "kWsSstInput, kWsSstKeys, kWsSstScratch"),
    "open": (hc.open_jobs, "kWsTableOpen, kWsSstScratch"),
    "get": (hc.get_jobs, "kWsTableIO, kWsTableDesc"),
    "get_filtered": (lambda ora: hc.get_jobs(ora, with_filters=True), "kWsTableIO, kWsTableDesc, kWsMulti"),
    "scan": (hc.scan_jobs, "kWsTableScanIO (twice per call), kWsTableDesc, kWsTableScanPairs, kWsTableScan"),
    "merge": (hc.merge_jobs, "kWsCompactIn, kWsCompact"),
    "write": (hc.write_jobs, "kWsCompactIn, kWsCompact, kWsGather, kWsCompactOut, kWsSstEnc"),
    "probe": (hc.probe_jobs, "kWsMultiKeys, kWsMulti"),
    "rebuild": (hc.rebuild_jobs, "kWsSstInput, kWsSstKeys, kWsSstScratch"),
    "rebuild_build": (hc.rebuild_build_jobs, "kWsSstInput, kWsSstKeys, kWsSstScratch, kWsBuild"),
}
# kWsBuild, which compact_write and rebuild_from_sst also reach, is used only by builds of 2^22 bit
# indices or more (the partitioned build).  The tables of the other families stay far below that;
# "rebuild_build" (two threads) alternates a table of 240 000 entries at k = 19, whose rebuild takes
# the partitioned build and with it kWsBuild, with one of 3 000, whose rebuild builds with atomics.


@pytest.mark.parametrize("family", list(FAMILIES))
def test_same_entry_point_different_inputs(ctx, family):
    """Four threads (two for rebuild_build) in one entry point, sizes rotating per round: each thread's
    staged inputs share FAMILIES[family][1] with the others', at a different size each."""
    both(FAMILIES[family][0](ctx.ora), ctx)


# ---- 2. the store's shape ------------------------------------------------------------------------

def test_readers_compaction_flush_recovery_build_probe(ctx):
    """Eight threads as the store runs them: three readers (filtered gets and scans alternating over
    the same open tables: kWsTableDesc shared by both, kWsTableIO, kWsTableScan*, kWsMulti), a
    compaction (kWsCompact*, kWsGather, kWsSstEnc), a flush that opens what it encoded (kWsSstEncIO,
    kWsSstEnc with the compaction, kWsTableOpen, kWsSstScratch), a recovery (kWsSstInput, kWsSstKeys,
    kWsSstScratch with the flush's opens), and vbf_build_host / vbf_probe_host, which share the
    staging streams and their buffers under the staging lock."""
    ora = ctx.ora
    half = hc.ROUNDS // 2
    gets, scans = hc.get_jobs(ora, 3, with_filters=True, rounds=half), hc.scan_jobs(ora, 3, rounds=half)
    readers = [[j for pair in zip(g, s) for j in pair] for g, s in zip(gets, scans)]
    # the one-shot build and probe take a fifth of a millisecond a call: eight times the jobs, so that
    # these two threads last about as long as the others
    per_thread = readers + [hc.write_jobs(ora)[0], hc.flush_jobs(ora), hc.rebuild_jobs(ora)[0],
                            hc.build_host_jobs(ora, 8 * hc.ROUNDS), hc.probe_host_jobs(ora, 8 * hc.ROUNDS)]
    assert len(per_thread) == 8 and all(len(jobs) >= hc.ROUNDS for jobs in per_thread)
    both(per_thread, ctx)


# ---- 3. lock order -------------------------------------------------------------------------------

def test_lock_order_filter_then_device(ctx):
    """One filter F written, read through, probed and rebuilt at once.  Thread 0 sets new keys into F
    (filter lock, then the staging lock; every other batch through the device's worker), thread 1
    gets with F among the filters (filter locks and their drain, then the device), thread 2 probes F
    and two others (the same), thread 3 rebuilds F from its table's SST (the same).  A call that took
    the device before a filter lock, or waited for the worker while holding the device, could stop
    here for good: the run has to end inside the cap.  Filters only prune and F only gains bits, so
    every get equals the filter-less expectation; F ends as the oracle's build of everything set."""
    from velarixdb_amd.key_range import SstRange
    vbf, ora = ctx.vbf, ctx.ora
    lo = hc.lock_order_case(ora)
    F = vbf.BloomFilter.sized(lo["m"], lo["k"], hc.P)
    F.set_many(lo["t_keys"])
    assert np.array_equal(F.words(), lo["first"])
    ctx.lock_filter = F
    ctx.lock_ranges = [SstRange(*t.key_range(), f) for t, f in zip(ctx.tables, [F] + ctx.filters[1:])]
    sets = [hc.Job("lock_set", "batch%d" % r, (keys, r % 2 == 1), (), len(keys)) for r, keys in enumerate(lo["others"])]
    gets = [j._replace(call="lock_get") for j in hc.get_jobs(ora, 1, rounds=len(sets), first_thread=1)[0]]
    probes = hc.lock_order_probe_jobs(ora, len(sets))
    rebuilds = [hc.Job("lock_rebuild", "round%d" % r, lo["files"], (len(lo["t_keys"]),), len(lo["t_keys"]))
                for r in range(len(sets))]
    per_thread = [sets, gets, probes, rebuilds]
    try:
        both(per_thread, ctx)
        F.sync()
        assert np.array_equal(F.words(), lo["final"])
        # set twice (control and threads) and rebuilt twice per round: the counter saw every call
        assert F.num_elements() == len(lo["t_keys"]) + 2 * (lo["n"] - len(lo["t_keys"])) + 2 * len(sets) * len(lo["t_keys"])
    finally:
        ctx.lock_filter = ctx.lock_ranges = None


# ---- 4. the sizing protocol under contention ----------------------------------------------------

def test_scan_size_query_and_fill_stay_a_threads_own(ctx):
    """vbf_table_scan_host is called twice per scan (sizes, then fill), and the lock is dropped in
    between: two threads' scans of different range sets interleave call by call, and a third thread's
    gets run between them (kWsTableDesc, kWsTableScanIO, kWsTableScanPairs, kWsTableScan).  Each
    filling call must report the sizes its own query reported, and fill its own thread's bytes."""
    ora = ctx.ora
    scans = [[j._replace(call="scan_two_calls") for j in jobs] for jobs in hc.scan_jobs(ora, 2, first_thread=2)]
    both(scans + hc.get_jobs(ora, 1, first_thread=3), ctx)


# ---- 5. workspaces released under the callers' feet ---------------------------------------------

def test_release_workspaces_beside_host_calls(ctx):
    """vbf_release_workspaces frees every cached workspace.  Beside `_host` calls it has to wait for
    the one in flight and hold the next back (include/vbf.h); otherwise an encode, a get or a scan
    or a decode goes on with a pointer that was just freed (every slot of theirs).  Each call after a
    release allocates its workspaces again; vbf_build_host runs beside them under the staging lock,
    which the release takes too."""
    ora = ctx.ora
    release = [j for r, d in enumerate(hc.decode_jobs(ora)[0])
               for j in (hc.Job("release", "round%d" % r, (), (), 0), d)]  # a decode after every release
    both([release, hc.encode_jobs(ora)[1], hc.get_jobs(ora, 1, first_thread=2)[0], hc.scan_jobs(ora)[3],
          hc.build_host_jobs(ora, 8 * hc.ROUNDS)], ctx)
