"""The table handle's and the lookup's checks that return before any device work (no GPU needed)."""
import ctypes

import numpy as np


def test_open_needs_out():
    from velarixdb_amd._lib import VBF_EINVAL, lib
    assert lib.vbf_table_open_dev(None, 0, None, 0, None, 0, None, None) == VBF_EINVAL
    assert b"out is NULL" in lib.vbf_last_error()
    assert lib.vbf_table_open_host(None, 0, None, 0, 0, None) == VBF_EINVAL
    assert b"out is NULL" in lib.vbf_last_error()


def test_open_null_buffers_with_sizes():
    from velarixdb_amd._lib import VBF_EINVAL, lib
    h = ctypes.c_void_p(7)
    assert lib.vbf_table_open_dev(None, 100, None, 0, None, 0, None, ctypes.byref(h)) == VBF_EINVAL
    assert b"NULL" in lib.vbf_last_error() and not h.value
    h = ctypes.c_void_p(7)
    assert lib.vbf_table_open_host(None, 0, None, 12, 0, ctypes.byref(h)) == VBF_EINVAL
    assert b"NULL" in lib.vbf_last_error() and not h.value


def test_open_host_truncated_index_is_rejected_before_the_device():
    from velarixdb_amd._lib import VBF_EINVAL, lib
    data, index = np.zeros(21, np.uint8), np.zeros(11, np.uint8)  # a record needs at least 8 bytes + key
    index[0] = 4
    h = ctypes.c_void_p(7)
    assert lib.vbf_table_open_host(data.ctypes.data, 21, index.ctypes.data, 11, 0, ctypes.byref(h)) == VBF_EINVAL
    assert b"truncated" in lib.vbf_last_error() and not h.value


def _get(fn, keys, offsets, stride, n, nsst, tables, outs=(None, None, None, None)):
    from velarixdb_amd._lib import lib
    if fn == "dev":
        return lib.vbf_table_get_dev(keys, offsets, stride, n, nsst, tables, None, *outs, None)
    return lib.vbf_table_get_host(keys, offsets, stride, n, nsst, tables, None, *outs)


def test_get_null_tables():
    from velarixdb_amd._lib import VBF_EINVAL, lib
    keys = np.zeros(160, np.uint8)
    for fn in ("dev", "host"):
        assert _get(fn, keys.ctypes.data, None, 16, 10, 3, None) == VBF_EINVAL
        assert b"tables is NULL" in lib.vbf_last_error()
        slots = (ctypes.c_void_p * 3)()  # three NULL handles
        assert _get(fn, keys.ctypes.data, None, 16, 10, 3, slots) == VBF_EINVAL
        assert b"tables[0] is NULL" in lib.vbf_last_error()


def test_get_null_keys():
    from velarixdb_amd._lib import VBF_EINVAL, lib
    for fn in ("dev", "host"):
        assert _get(fn, None, None, 16, 10, 0, None) == VBF_EINVAL
        assert b"keys is NULL" in lib.vbf_last_error()


def test_get_of_no_keys_is_ok():
    from velarixdb_amd._lib import VBF_OK, lib
    offs = np.zeros(1, np.uint64)
    for fn in ("dev", "host"):
        assert _get(fn, None, offs.ctypes.data, 0, 0, 0, None) == VBF_OK
        assert lib.vbf_last_error() == b""
        assert _get(fn, None, None, 16, 0, 0, None) == VBF_OK


def test_get_host_without_tables_zero_fills():
    from velarixdb_amd._lib import VBF_OK
    keys = np.zeros(48, np.uint8)
    found, idx = np.full(3, 9, np.uint8), np.full(3, 9, np.uint32)
    val, cr = np.full(3, 9, np.uint32), np.full(3, 9, np.uint64)
    outs = (found.ctypes.data, idx.ctypes.data, val.ctypes.data, cr.ctypes.data)
    assert _get("host", keys.ctypes.data, None, 16, 3, 0, None, outs) == VBF_OK
    assert not found.any() and not idx.any() and not val.any() and not cr.any()


def test_accessors_of_a_null_handle():
    from velarixdb_amd._lib import VBF_EINVAL, lib
    assert lib.vbf_table_entries(None) == 0 and lib.vbf_table_blocks(None) == 0
    n = ctypes.c_uint64()
    assert lib.vbf_table_key_range(None, None, 0, ctypes.byref(n), None, 0, ctypes.byref(n)) == VBF_EINVAL
    lib.vbf_table_free(None)
