"""vbf_vlog_walk_host under concurrent callers on one handle (include/vbf.h, "Threads").  Four
threads, each with a start and a budget of its own; the expected outputs (tests/vlog_walk_ref.py) are
computed before any thread starts and every answer is compared on the main thread after the threads
have ended.  The same jobs run serially first, so a wrong expectation fails there."""
import os
import threading
import traceback

import numpy as np
import pytest

import vlog_walk_ref as wr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
THREADS, ROUNDS = 4, 6
CAP = 120.0  # seconds after which a thread still alive counts as hung (a deadlock guard)
JOBS = ((0, None), (25, 4096), (50, 30000), (76757, 0))  # (start, budget)


def _run(vl, start, budget):
    w = vl.walk(start=start, budget=budget)
    return (w.entry_off, w.val_offsets, w.keys.data, w.keys.offsets, w.values, w.value_off, w.created_ms,
            w.tombstones), w.end_off, w.stop


def _check(got, want):
    for g, w in zip(got[0], want[0]):
        assert np.array_equal(g, w)
    assert got[1:] == want[1:]


def test_four_threads_walk_one_log(vbf):
    from velarixdb_amd import ValueLog
    with open(os.path.join(GOLDEN, "vlog_fixture", "val_log_prefix.bin"), "rb") as f:
        log = f.read()
    wants = []
    for start, budget in JOBS:
        entries, end, stop = wr.walk(log, start, wr.UINT64_MAX if budget is None else budget)
        wants.append((wr.arrays(entries, end), end, stop))
    assert [w[2] for w in wants] == [wr.END, wr.BUDGET, wr.BUDGET, wr.BUDGET] and wants[0][0][1].size == 2844
    with ValueLog.open(log) as vl:
        for job, want in zip(JOBS, wants):  # the serial run
            _check(_run(vl, *job), want)
        results, errors = [[] for _ in range(THREADS)], []
        start = threading.Barrier(THREADS)

        def work(t):
            try:
                start.wait()
                for _ in range(ROUNDS):
                    results[t].append(_run(vl, *JOBS[t]))
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
                _check(got, wants[t])
