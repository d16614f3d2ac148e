"""The range scans' checks that return before any device work (no GPU needed)."""
import ctypes

import numpy as np


def _scan(fn, bounds, boff, nranges, nsst, tables, flags=0, n_out=True, key_bytes=True):
    """All outputs NULL (a size query); -> (rc, n_out, key_bytes) with the two sizes preset to 7."""
    from velarixdb_amd._lib import lib
    n, kb = ctypes.c_uint64(7), ctypes.c_uint64(7)
    pn = ctypes.byref(n) if n_out else None
    pk = ctypes.byref(kb) if key_bytes else None
    head = (bounds, boff, nranges, nsst, tables, flags, None, None, 0, None, None, None, None, None, 0, pn, pk)
    rc = lib.vbf_table_scan_dev(*head, None) if fn == "dev" else lib.vbf_table_scan_host(*head)
    return rc, n.value, kb.value


def _bounds():
    b = np.frombuffer(b"abcd", np.uint8)
    off = np.array([0, 1, 2, 3, 4], np.uint64)  # two ranges
    return b, off


def test_null_tables_and_null_table():
    from velarixdb_amd._lib import VBF_EINVAL, lib
    b, off = _bounds()
    for fn in ("dev", "host"):
        assert _scan(fn, b.ctypes.data, off.ctypes.data, 2, 3, None)[0] == VBF_EINVAL
        assert b"tables is NULL" in lib.vbf_last_error()
        slots = (ctypes.c_void_p * 3)()  # three NULL handles
        assert _scan(fn, b.ctypes.data, off.ctypes.data, 2, 3, slots)[0] == VBF_EINVAL
        assert b"tables[0] is NULL" in lib.vbf_last_error()


def test_null_sizes():
    from velarixdb_amd._lib import VBF_EINVAL, lib
    b, off = _bounds()
    for fn in ("dev", "host"):
        for which in ("n_out", "key_bytes"):
            rc, n, kb = _scan(fn, b.ctypes.data, off.ctypes.data, 2, 0, None, **{which: False})
            assert rc == VBF_EINVAL and b"is NULL" in lib.vbf_last_error()
            assert (n, kb) == (7, 7)  # nothing written through the pointer that was given


def test_descending_bounds_off_host():
    from velarixdb_amd._lib import VBF_EINVAL, lib
    b = np.frombuffer(b"abcd", np.uint8)
    for bad in ([0, 2, 1, 3, 4], [1, 0, 2, 3, 4], [0, 1, 2, 4, 3]):
        off = np.array(bad, np.uint64)
        rc, n, kb = _scan("host", b.ctypes.data, off.ctypes.data, 2, 0, None)
        assert rc == VBF_EINVAL and b"bounds_off decreases" in lib.vbf_last_error(), bad
        assert (n, kb) == (0, 0)


def test_null_bounds_with_ranges():
    from velarixdb_amd._lib import VBF_EINVAL, lib
    b, off = _bounds()
    for fn in ("dev", "host"):
        assert _scan(fn, None, off.ctypes.data, 2, 0, None)[0] == VBF_EINVAL
        assert b"bounds is NULL" in lib.vbf_last_error()
        assert _scan(fn, b.ctypes.data, None, 2, 0, None)[0] == VBF_EINVAL
        assert b"bounds_off is NULL" in lib.vbf_last_error()


def test_unknown_flag_bit():
    from velarixdb_amd._lib import VBF_EINVAL, lib
    b, off = _bounds()
    for fn in ("dev", "host"):
        for flags in (4, 8, 0x80000000, 7):
            assert _scan(fn, b.ctypes.data, off.ctypes.data, 2, 0, None, flags)[0] == VBF_EINVAL
            assert b"unknown flag" in lib.vbf_last_error()


def test_no_ranges_is_ok_with_zero_sizes():
    from velarixdb_amd._lib import VBF_OK, lib
    off = np.zeros(1, np.uint64)
    for fn in ("dev", "host"):
        for args in ((None, None), (None, off.ctypes.data)):
            for flags in (0, 1, 2, 3):
                assert _scan(fn, *args, 0, 0, None, flags) == (VBF_OK, 0, 0)
                assert lib.vbf_last_error() == b""


def test_host_without_tables_gives_empty_ranges():
    """nsst == 0 needs no device: range_off and key_off[0] are zero-filled on the host."""
    from velarixdb_amd._lib import VBF_OK, lib
    b, off = _bounds()
    n, kb = ctypes.c_uint64(7), ctypes.c_uint64(7)
    range_off, key_off = np.full(3, 9, np.uint64), np.full(1, 9, np.uint64)
    rc = lib.vbf_table_scan_host(b.ctypes.data, off.ctypes.data, 2, 0, None, 3, range_off.ctypes.data, None, 0,
                                 key_off.ctypes.data, None, None, None, None, 0, ctypes.byref(n), ctypes.byref(kb))
    assert rc == VBF_OK and (n.value, kb.value) == (0, 0)
    assert not range_off.any() and not key_off.any()
