"""vbf_vlog_get_host and vbf_vlog_encode_host under concurrent callers, beside vbf_table_get_host on
one device (include/vbf.h, "Threads").  Four threads, each with inputs of its own; the expected
outputs (tests/vlog_ref.py, tests/sst_get_ref.py) are computed before any thread starts and every
answer is compared on the main thread after the threads have ended.  One value-log handle and one
table are read by all threads at once.  The same jobs run serially first, so a wrong expectation
fails there and not in the threaded run."""
import os
import threading
import traceback

import numpy as np
import pytest

import scan_cases as sc
import sst_get_ref as ref
import vlog_ref as vr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
THREADS, ROUNDS = 4, 6
CAP = 120.0  # seconds after which a thread still alive counts as hung (a deadlock guard)


def _jobs(t, log, parsed, s):
    """Thread t's inputs and expected outputs: a fetch of offsets of its own (some past the end, some
    masked, keys checked on odd threads), an append of entries of its own, a lookup of its own keys."""
    rng = np.random.default_rng(0x7EAD + t)
    pick = rng.integers(0, len(parsed), 700 + 150 * t)
    vo = np.array([parsed[i][0] for i in pick] + [len(log), len(log) - 1], np.uint32)
    found = (rng.integers(0, 4, vo.size) != 0).astype(np.uint8)
    keys = [parsed[i][1] for i in pick] + [b"x", b"y"] if t % 2 else None
    want_get = vr.get_many(log, vo, 0, found, keys)
    entries = [(rng.bytes(int(rng.integers(0, 30))), rng.bytes(int(rng.integers(0, 3000 * (t + 1)))),
                sc.T0 + j, j % 5 == t) for j in range(300 + 100 * t)]
    want_enc = vr.encode(entries, base=1000 * t)
    all_keys = sorted(s.starts)
    ask = [all_keys[i] for i in rng.integers(0, len(all_keys), 500)] + [b"absent-%d-%d" % (t, j) for j in range(40)]
    want_tab = ref.search_many(ask, [s])
    return (vo, found, keys, want_get), (entries, 1000 * t, want_enc), (ask, want_tab)


def _run(job, vl, tab):
    from velarixdb_amd import ValueLog, get_many
    (vo, found, keys, _), (entries, base, _), (ask, _) = job
    g = vl.get_many(vo, found=found, keys=keys)
    log, offs = ValueLog.encode([e[0] for e in entries], [e[1] for e in entries], [e[2] for e in entries],
                                [e[3] for e in entries], base=base)
    r = get_many(ask, [tab])
    return (g.status, g.values, g.value_off), (log, offs), (r.found, r.table, r.val_offsets, r.created_ms)


def _check(job, got):
    (_, _, _, want_get), (_, _, want_enc), (_, want_tab) = job
    for g, w in zip(got[0], want_get):
        assert np.array_equal(g, w)
    assert got[1][0] == want_enc[0] and got[1][1].tolist() == want_enc[1]
    for g, w in zip(got[2], want_tab):
        assert np.array_equal(g, w)


def test_four_threads_fetch_append_and_look_up(vbf, ora):
    from velarixdb_amd import Table, ValueLog
    name = "sstable_1720785462309"
    with open(os.path.join(GOLDEN, "vlog_fixture", "val_log_prefix.bin"), "rb") as f:
        log = f.read()
    parsed = vr.parse(log)
    s = ref.Sst(*sc.read_fixture(name))
    jobs = [_jobs(t, log, parsed, s) for t in range(THREADS)]
    with Table.open_dir(os.path.join(sc.SST, name)) as tab, ValueLog.open(log) as vl:
        for job in jobs:  # the serial run
            _check(job, _run(job, vl, tab))
        results, errors = [[] for _ in range(THREADS)], []
        start = threading.Barrier(THREADS)

        def work(t):
            try:
                start.wait()
                for _ in range(ROUNDS):
                    results[t].append(_run(jobs[t], vl, tab))
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
                _check(jobs[t], got)
