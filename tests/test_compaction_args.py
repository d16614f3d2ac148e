"""The compaction merge's checks that return before any device work (no GPU needed): argument
validation of vbf_compact_merge_dev / _host, vbf_compact_write_host and vbf_gather_entries_dev,
buckets without entries, and the 2^31 entry limit.  _dev and _host share one validation, so they
give the same code and message."""
import ctypes

import numpy as np
import pytest

POISON = 7


def _arena(n=3):
    """n one-byte keys in one table, as host arrays (never read by a call that fails its checks)"""
    return dict(keys=np.arange(97, 97 + n, dtype=np.uint8), offsets=np.arange(n + 1, dtype=np.uint64),
                created=np.arange(n, dtype=np.int64), tomb=np.zeros(n, np.uint8),
                run_off=np.asarray([0, n], np.uint64), out_ids=np.zeros(n, np.uint32))


def _p(a):
    return None if a is None else a if isinstance(a, int) else a.ctypes.data


def _merge(which, a, nruns=1, map_keys=None, map_off=None, map_time=None, map_n=0, n_out=True):
    """-> (rc, message, *n_out, *n_upd); both counters start poisoned"""
    from velarixdb_amd._lib import lib
    n, nu = ctypes.c_uint64(POISON), ctypes.c_uint64(POISON)
    head = (_p(a["keys"]), _p(a["offsets"]), _p(a["created"]), _p(a["tomb"]), _p(a["run_off"]), nruns,
            _p(map_keys), _p(map_off), _p(map_time), map_n, 1, 20, 25, 40)
    pn = ctypes.byref(n) if n_out else None
    if which == "write":
        dl, il, h = ctypes.c_uint64(POISON), ctypes.c_uint64(POISON), ctypes.c_void_p()
        rc = lib.vbf_compact_write_host(*head, None, 0.01, ctypes.byref(h), None, 0, ctypes.byref(dl), None, 0,
                                        ctypes.byref(il), pn, None, None, ctypes.byref(nu), 0)
        assert not h.value and (dl.value, il.value) == (0, 0)
    else:
        fn = lib.vbf_compact_merge_dev if which == "dev" else lib.vbf_compact_merge_host
        rc = fn(*head, _p(a["out_ids"]), pn, None, None, ctypes.byref(nu), None if which == "dev" else 0)
    return rc, lib.vbf_last_error(), n.value, nu.value


MERGE = ("dev", "host")
ALL = ("dev", "host", "write")


@pytest.mark.parametrize("which", MERGE)
def test_n_out_null(which):
    from velarixdb_amd._lib import VBF_EINVAL
    rc, msg, _, nu = _merge(which, _arena(), n_out=False)
    assert rc == VBF_EINVAL and b"n_out is NULL" in msg


@pytest.mark.parametrize("which", MERGE)
def test_no_tables_is_ok(which):
    from velarixdb_amd._lib import VBF_OK
    a = dict.fromkeys(_arena())  # every pointer NULL
    rc, msg, n, nu = _merge(which, a, nruns=0)
    assert (rc, n, nu) == (VBF_OK, 0, 0)


@pytest.mark.parametrize("which", ALL)
def test_run_off_null(which):
    from velarixdb_amd._lib import VBF_EINVAL
    a = _arena()
    a["run_off"] = None
    rc, msg, n, nu = _merge(which, a)
    assert rc == VBF_EINVAL and b"run_off is NULL" in msg and (n, nu) == (0, 0)


@pytest.mark.parametrize("which", ALL)
def test_run_off_not_starting_at_zero(which):
    from velarixdb_amd._lib import VBF_EINVAL
    a = _arena()
    a["run_off"] = np.asarray([1, 3], np.uint64)
    rc, msg, n, nu = _merge(which, a)
    assert rc == VBF_EINVAL and b"run_off must start at 0" in msg and (n, nu) == (0, 0)


@pytest.mark.parametrize("which", ALL)
def test_run_off_decreasing(which):
    from velarixdb_amd._lib import VBF_EINVAL
    a = _arena()
    a["run_off"] = np.asarray([0, 2, 1, 3], np.uint64)
    rc, msg, n, nu = _merge(which, a, nruns=3)
    assert rc == VBF_EINVAL and b"run_off not nondecreasing at 1" in msg and (n, nu) == (0, 0)


@pytest.mark.parametrize("which", ALL)
def test_map_without_its_arrays(which):
    from velarixdb_amd._lib import VBF_EINVAL
    mk, mo, mt = np.asarray([97], np.uint8), np.asarray([0, 1], np.uint64), np.asarray([5], np.int64)
    for missing in range(3):
        arrs = [None if i == missing else x for i, x in enumerate((mk, mo, mt))]
        rc, msg, n, nu = _merge(which, _arena(), map_keys=arrs[0], map_off=arrs[1], map_time=arrs[2], map_n=1)
        assert rc == VBF_EINVAL and b"map arrays are NULL" in msg and (n, nu) == (0, 0)


# vbf_compact_write_host has no out_ids: the ids stay on the device
@pytest.mark.parametrize("which,missing", [(w, m) for w in ALL for m in ("offsets", "created", "tomb", "out_ids")
                                           if (w, m) != ("write", "out_ids")])
def test_entries_without_an_array(which, missing):
    from velarixdb_amd._lib import VBF_EINVAL
    a = _arena()
    a[missing] = None
    rc, msg, n, nu = _merge(which, a)
    assert rc == VBF_EINVAL and b"NULL argument" in msg and (n, nu) == (0, 0)


@pytest.mark.parametrize("which", MERGE)
def test_only_empty_tables_need_no_device(which):
    from velarixdb_amd._lib import VBF_OK, lib
    a = dict.fromkeys(_arena())
    a["run_off"] = np.zeros(4, np.uint64)
    rc, msg, n, nu = _merge(which, a, nruns=3)
    assert (rc, n, nu) == (VBF_OK, 0, 0) and lib.vbf_last_error() == b""


def test_write_of_no_entries_is_an_empty_merge():
    """BloomFilter::new(p, 0) asserts (bf.rs:67): no tables or only empty ones cannot be written."""
    from velarixdb_amd._lib import VBF_EINVAL
    a = dict.fromkeys(_arena())
    for nruns, ro in ((0, None), (3, np.zeros(4, np.uint64))):
        a["run_off"] = ro
        rc, msg, n, nu = _merge("write", a, nruns=nruns)
        assert rc == VBF_EINVAL and msg.startswith(b"empty merge") and (n, nu) == (0, 0)


@pytest.mark.parametrize("which", ALL)
@pytest.mark.parametrize("total", [2**31, 2**32 - 2, 2**40])
def test_too_many_entries(which, total):
    """hipcub's selects run over the entry count: 2^31 and more is refused.  Every data pointer is
    NULL and the limit is checked first, so the call fails before it could start any device work."""
    from velarixdb_amd._lib import VBF_EINVAL
    a = dict.fromkeys(_arena())
    a["run_off"] = np.asarray([0, total], np.uint64)
    rc, msg, n, nu = _merge(which, a)
    assert rc == VBF_EINVAL and b"too many entries" in msg and (n, nu) == (0, 0)


def test_largest_count_passes_the_limit():
    """2^31 - 1 entries are within the limit: with NULL arrays the next check answers instead."""
    from velarixdb_amd._lib import VBF_EINVAL
    a = dict.fromkeys(_arena())
    a["run_off"] = np.asarray([0, 2**31 - 1], np.uint64)
    for which in ALL:
        rc, msg, n, nu = _merge(which, a)
        assert rc == VBF_EINVAL and b"NULL argument" in msg


def _gather(offsets=1, ids=1, n=3, out_offsets=1, created=None, tomb=None, val=None, out_created=None, out_tomb=None,
            out_val=None):
    """Pointers are never dereferenced by a call that fails its checks: 1 stands for 'not NULL'."""
    from velarixdb_amd._lib import lib
    buf = np.zeros(8, np.uint64)
    P = lambda x: buf.ctypes.data if x else None
    kb = ctypes.c_uint64(POISON)
    rc = lib.vbf_gather_entries_dev(P(1), P(offsets), P(created), P(tomb), P(val), P(ids), n, P(1), 64, P(out_offsets),
                                    P(out_created), P(out_tomb), P(out_val), ctypes.byref(kb), None)
    return rc, lib.vbf_last_error()


def test_gather_out_offsets_null():
    from velarixdb_amd._lib import VBF_EINVAL
    rc, msg = _gather(out_offsets=None)
    assert rc == VBF_EINVAL and b"out_offsets is NULL" in msg


def test_gather_output_without_its_input():
    from velarixdb_amd._lib import VBF_EINVAL
    for kw in (dict(out_created=1), dict(out_tomb=1), dict(out_val=1),
               dict(out_created=1, created=1, tomb=1, out_val=1)):
        rc, msg = _gather(**kw)
        assert rc == VBF_EINVAL and b"an output array without its input" in msg, kw


def test_gather_entries_without_ids_or_offsets():
    from velarixdb_amd._lib import VBF_EINVAL
    for kw in (dict(ids=None), dict(offsets=None)):
        rc, msg = _gather(**kw)
        assert rc == VBF_EINVAL and b"NULL argument" in msg, kw


@pytest.mark.parametrize("n", [2**31 - 1, 2**31, 2**40])
def test_gather_too_many_entries(n):
    """The offsets' scan runs over n + 1 items.  Every pointer NULL: the limit is checked first."""
    from velarixdb_amd._lib import VBF_EINVAL
    rc, msg = _gather(offsets=None, ids=None, out_offsets=None, n=n)
    assert rc == VBF_EINVAL and b"too many entries" in msg
