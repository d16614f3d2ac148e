"""The value-log entry points' checks that return before any device work (no GPU needed)."""
import ctypes

import numpy as np

FAKE = ctypes.c_void_p(0x1000)  # a non-NULL handle or pointer that a failing check never follows


def _get(fn, h, val_offsets, n, value_bytes=True, found=None, keys=None, offsets=None, stride=0, value_off=None):
    """A size query (status and values NULL); -> (rc, value_bytes) with the size preset to 7."""
    from velarixdb_amd._lib import lib
    vb = ctypes.c_uint64(7)
    head = (h, val_offsets, found, n, keys, offsets, stride, None, None, 0, value_off,
            ctypes.byref(vb) if value_bytes else None)
    rc = lib.vbf_vlog_get_dev(*head, None) if fn == "dev" else lib.vbf_vlog_get_host(*head)
    return rc, vb.value


def _enc(fn, keys, offsets, stride, n, values, value_off, base=0, out_len=True, out=None, out_cap=0, val_offsets=None):
    """-> (rc, out_len) with the size preset to 7."""
    from velarixdb_amd._lib import lib
    ln = ctypes.c_uint64(7)
    head = (keys, offsets, stride, n, values, value_off, None, None, base, out, out_cap,
            ctypes.byref(ln) if out_len else None, val_offsets)
    rc = lib.vbf_vlog_encode_dev(*head, None) if fn == "dev" else lib.vbf_vlog_encode_host(*head, 0)
    return rc, ln.value


def test_open_checks():
    from velarixdb_amd._lib import VBF_EINVAL, lib
    h = ctypes.c_void_p(5)
    for fn, tail in ((lib.vbf_vlog_open_dev, ()), (lib.vbf_vlog_open_host, (0,))):
        assert fn(FAKE, 10, 0, *tail, None) == VBF_EINVAL and b"out is NULL" in lib.vbf_last_error()
        assert fn(None, 10, 0, *tail, ctypes.byref(h)) == VBF_EINVAL and b"bytes is NULL" in lib.vbf_last_error()
        assert h.value is None  # *out is cleared first
        h = ctypes.c_void_p(5)
        assert fn(FAKE, 10, 2**64 - 5, *tail, ctypes.byref(h)) == VBF_EINVAL and b"wraps" in lib.vbf_last_error()
    assert lib.vbf_vlog_bytes(None) == 0 and lib.vbf_vlog_base(None) == 0 and lib.vbf_vlog_device(None) == -1
    lib.vbf_vlog_free(None)


def test_get_null_arguments():
    from velarixdb_amd._lib import VBF_EINVAL, lib
    vo = np.zeros(3, np.uint32)
    for fn in ("dev", "host"):
        rc, vb = _get(fn, FAKE, vo.ctypes.data, 3, value_bytes=False)
        assert rc == VBF_EINVAL and b"value_bytes is NULL" in lib.vbf_last_error()
        assert vb == 7  # nothing written through the pointer that was not given
        assert _get(fn, None, vo.ctypes.data, 3) == (VBF_EINVAL, 0) and b"vlog is NULL" in lib.vbf_last_error()
        assert _get(fn, None, None, 0) == (VBF_EINVAL, 0) and b"vlog is NULL" in lib.vbf_last_error()
        assert _get(fn, FAKE, None, 3) == (VBF_EINVAL, 0) and b"val_offsets is NULL" in lib.vbf_last_error()
        assert _get(fn, FAKE, vo.ctypes.data, 2**31 - 1) == (VBF_EINVAL, 0) and b"too many items" in lib.vbf_last_error()


def test_get_descending_key_offsets_host():
    from velarixdb_amd._lib import VBF_EINVAL, lib
    vo, keys = np.zeros(2, np.uint32), np.zeros(8, np.uint8)
    off = np.array([0, 4, 3], np.uint64)
    # FAKE stands for a handle: the check returns before the handle is read
    assert _get("host", FAKE, vo.ctypes.data, 2, keys=keys.ctypes.data, offsets=off.ctypes.data) == (VBF_EINVAL, 0)
    assert b"offsets descend at key 1" in lib.vbf_last_error()


def test_get_no_items():
    from velarixdb_amd._lib import VBF_OK, lib
    for fn in ("dev", "host"):
        assert _get(fn, FAKE, None, 0) == (VBF_OK, 0)
        assert lib.vbf_last_error() == b""
    voff = np.full(1, 9, np.uint64)
    assert _get("host", FAKE, None, 0, value_off=voff.ctypes.data) == (VBF_OK, 0) and voff[0] == 0


def test_encode_null_arguments():
    from velarixdb_amd._lib import VBF_EINVAL, lib
    keys, vals = np.zeros(8, np.uint8), np.zeros(8, np.uint8)
    off, voff = np.array([0, 4, 8], np.uint64), np.array([0, 3, 8], np.uint64)
    K, O, V, VO = keys.ctypes.data, off.ctypes.data, vals.ctypes.data, voff.ctypes.data
    for fn in ("dev", "host"):
        rc, ln = _enc(fn, K, O, 0, 2, V, VO, out_len=False)
        assert rc == VBF_EINVAL and b"out_len is NULL" in lib.vbf_last_error() and ln == 7
        assert _enc(fn, K, O, 0, 2, V, None) == (VBF_EINVAL, 0) and b"value_off is NULL" in lib.vbf_last_error()
        assert _enc(fn, None, None, 4, 2, V, VO) == (VBF_EINVAL, 0) and b"keys is NULL" in lib.vbf_last_error()
        assert _enc(fn, K, None, 2**32, 2, V, VO) == (VBF_EINVAL, 0) and b"key_len is a u32" in lib.vbf_last_error()
    # decidable on the host in _host: NULL arrays behind nonzero lengths
    assert _enc("host", None, O, 0, 2, V, VO) == (VBF_EINVAL, 0) and b"keys is NULL" in lib.vbf_last_error()
    assert _enc("host", K, O, 0, 2, None, VO) == (VBF_EINVAL, 0) and b"values is NULL" in lib.vbf_last_error()


def test_encode_no_entries():
    from velarixdb_amd._lib import VBF_OK, lib
    for fn in ("dev", "host"):
        for base in (0, 2**32 + 5):
            assert _enc(fn, None, None, 0, 0, None, None, base) == (VBF_OK, 0)
            assert lib.vbf_last_error() == b""


def test_encode_limit_of_two_to_the_32():
    """base = 2^32 - 10 with two entries: the second would start at 2^32 + 7 or later, whatever the
    lengths -- decided before any device work in both entry points."""
    from velarixdb_amd._lib import VBF_EINVAL, VBF_OK, lib
    keys, vals = np.zeros(8, np.uint8), np.zeros(8, np.uint8)
    off, voff = np.array([0, 0, 0], np.uint64), np.array([0, 0, 0], np.uint64)
    K, O, V, VO = keys.ctypes.data, off.ctypes.data, vals.ctypes.data, voff.ctypes.data
    for fn in ("dev", "host"):
        assert _enc(fn, K, O, 0, 2, V, VO, base=2**32 - 10) == (VBF_EINVAL, 0)
        assert b"entry 1 would start at or beyond 2^32" in lib.vbf_last_error()
        assert _enc(fn, K, O, 0, 1, V, VO, base=2**32) == (VBF_EINVAL, 0)
        assert b"entry 0 would start at or beyond 2^32" in lib.vbf_last_error()
    # one entry at 2^32 - 10 is fine (the host's size query needs no device): 17 bytes
    assert _enc("host", K, O, 0, 1, V, VO, base=2**32 - 10) == (VBF_OK, 17)
    # the lengths push the second entry over: base + 17 + 4 + 5 = 2^32
    off2, voff2 = np.array([0, 4, 8], np.uint64), np.array([0, 5, 8], np.uint64)
    assert _enc("host", K, off2.ctypes.data, 0, 2, V, voff2.ctypes.data, base=2**32 - 26) == (VBF_EINVAL, 0)
    assert b"last entry would start at 4294967296" in lib.vbf_last_error()
    assert _enc("host", K, off2.ctypes.data, 0, 2, V, voff2.ctypes.data, base=2**32 - 27) == (VBF_OK, 50)


def test_encode_host_offsets_and_capacity():
    from velarixdb_amd._lib import VBF_EINVAL, VBF_OK, lib
    keys, vals = np.zeros(8, np.uint8), np.zeros(8, np.uint8)
    K, V = keys.ctypes.data, vals.ctypes.data
    good = np.array([0, 4, 8], np.uint64)
    for bad in ([0, 5, 4], [3, 2, 8]):
        b = np.array(bad, np.uint64)
        assert _enc("host", K, good.ctypes.data, 0, 2, V, b.ctypes.data) == (VBF_EINVAL, 0)
        assert b"descend at entry" in lib.vbf_last_error()
        assert _enc("host", K, b.ctypes.data, 0, 2, V, good.ctypes.data) == (VBF_EINVAL, 0)
        assert b"descend at entry" in lib.vbf_last_error()
    # offsets[0] != 0 and a fixed stride size alike; the size query is host arithmetic
    lead = np.array([3, 4, 8], np.uint64)
    assert _enc("host", K, lead.ctypes.data, 0, 2, V, lead.ctypes.data) == (VBF_OK, 34 + 5 + 5)
    assert _enc("host", K, None, 4, 2, V, good.ctypes.data) == (VBF_OK, 34 + 8 + 8)
    # a capacity one short: the size is written, the outputs are not
    out, vo = np.full(64, 0xA5, np.uint8), np.full(2, 0xA5A5A5A5, np.uint32)
    rc, ln = _enc("host", K, good.ctypes.data, 0, 2, V, good.ctypes.data, out=out.ctypes.data, out_cap=49,
                  val_offsets=vo.ctypes.data)
    assert (rc, ln) == (VBF_EINVAL, 50) and b"out_cap 49 < 50" in lib.vbf_last_error()
    assert (out == 0xA5).all() and (vo == 0xA5A5A5A5).all()
