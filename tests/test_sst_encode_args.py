"""The SST encoder's checks that return before any device work (no GPU needed): argument
validation of vbf_sst_encode_dev / _host and the empty table."""
import ctypes

import numpy as np


def _sizes():
    dl, il, nb = ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_uint64(7)
    return (dl, il, nb), (ctypes.byref(dl), ctypes.byref(il), ctypes.byref(nb))


def test_null_keys_with_entries():
    from velarixdb_amd._lib import VBF_EINVAL, lib
    for fn, last in ((lib.vbf_sst_encode_dev, None), (lib.vbf_sst_encode_host, 0)):
        v, S = _sizes()
        assert fn(None, None, 16, 10, None, None, None, None, 0, S[0], None, 0, S[1], None, 0, S[2], last) == VBF_EINVAL
        assert b"keys is NULL" in lib.vbf_last_error()
        assert [x.value for x in v] == [0, 0, 0]


def test_null_size_pointers():
    from velarixdb_amd._lib import VBF_EINVAL, lib
    keys = np.zeros(160, np.uint8)
    for fn, last in ((lib.vbf_sst_encode_dev, None), (lib.vbf_sst_encode_host, 0)):
        for missing in range(3):
            _, S = _sizes()
            S = [None if i == missing else s for i, s in enumerate(S)]
            rc = fn(keys.ctypes.data, None, 16, 10, None, None, None, None, 0, S[0], None, 0, S[1], None, 0, S[2], last)
            assert rc == VBF_EINVAL and b"NULL" in lib.vbf_last_error()


def test_stride_longer_than_a_block():
    """A key of 4080 bytes makes an entry of 4097: the reference fails the flush with BlockIsFull."""
    from velarixdb_amd._lib import VBF_EINVAL, lib
    keys = np.zeros(2 * 4080, np.uint8)
    for fn, last in ((lib.vbf_sst_encode_dev, None), (lib.vbf_sst_encode_host, 0)):
        v, S = _sizes()
        rc = fn(keys.ctypes.data, None, 4080, 2, None, None, None, None, 0, S[0], None, 0, S[1], None, 0, S[2], last)
        assert rc == VBF_EINVAL and b"BlockIsFull" in lib.vbf_last_error()
        assert [x.value for x in v] == [0, 0, 0]


def test_no_entries_needs_no_device():
    from velarixdb_amd._lib import VBF_OK, lib
    offs = np.zeros(1, np.uint64)
    for fn, last in ((lib.vbf_sst_encode_dev, None), (lib.vbf_sst_encode_host, 0)):
        v, S = _sizes()
        assert fn(None, offs.ctypes.data, 0, 0, None, None, None, None, 0, S[0], None, 0, S[1], None, 0, S[2], last) == VBF_OK
        assert [x.value for x in v] == [0, 0, 0]
        assert lib.vbf_last_error() == b""


def test_write_entries_of_an_empty_table():
    from velarixdb_amd import sst
    ent = sst.SstEntries(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32),
                         np.zeros(0, np.uint64), np.zeros(0, bool))
    data, index = sst.write_entries(ent)
    assert data.dtype == np.uint8 and index.dtype == np.uint8 and data.size == 0 and index.size == 0
