"""vbf_store_scan_host: the checks that return before any HIP call (no GPU needed).

An empty memtable opens without device work, so real handles (on device 0 and on device 1) stand in
where a check follows a handle; FAKE is a non-NULL handle that a failing check never follows."""
import ctypes

import numpy as np
import pytest

from test_store_get_args import FAKE, POISON, _open


@pytest.fixture(scope="module")
def empty():
    """Two empty memtables on device 0, one on device 1."""
    from velarixdb_amd._lib import lib
    hs = []
    for dev in (0, 0, 1):
        rc, msg, h = _open("host", None, None, 0, 0, device=dev)
        assert rc == 0 and h.value, msg
        hs.append(h)
    yield hs
    for h in hs:
        lib.vbf_memtable_free(h)


def _bounds(ranges):
    flat = [b for pair in ranges for b in pair]
    off = np.concatenate([[0], np.cumsum([len(b) for b in flat])]).astype(np.uint64)
    return np.frombuffer(b"".join(flat) + b"\0", np.uint8), off


def _scan(ranges=((b"a", b"z"),), boff=None, log=FAKE, gc=None, active=None, nro=0, ro=None, nsst=0, tables=None, flags=0,
          sizes=(1, 1, 1), nranges=None):
    """-> (rc, message, (n_out, key_bytes, value_bytes), (range_off, key_off[0], value_off[0]))"""
    from velarixdb_amd._lib import lib
    b, off = _bounds(ranges)
    off = off if boff is None else np.asarray(boff, np.uint64)
    nr = len(ranges) if nranges is None else nranges
    n, kb, vb = ctypes.c_uint64(POISON), ctypes.c_uint64(POISON), ctypes.c_uint64(POISON)
    roff = np.full(min(nr, 16) + 1, POISON, np.uint64)
    koff, voff = np.full(1, POISON, np.uint64), np.full(1, POISON, np.uint64)
    ref = [ctypes.byref(x) if s else None for x, s in zip((n, kb, vb), sizes)]
    rc = lib.vbf_store_scan_host(b.ctypes.data, off.ctypes.data, nr, gc, active, nro, ro, nsst, tables, log, flags, 0,
                                 roff.ctypes.data, None, 0, koff.ctypes.data, None, None, None, None, None, None, 0,
                                 None, 0, voff.ctypes.data, *ref)
    return rc, lib.vbf_last_error(), (n.value, kb.value, vb.value), (roff, int(koff[0]), int(voff[0]))


@pytest.mark.parametrize("missing", (0, 1, 2))
def test_the_three_sizes_are_required(missing):
    from velarixdb_amd._lib import VBF_EINVAL
    sizes = [1, 1, 1]
    sizes[missing] = 0
    rc, msg, got, (roff, *_) = _scan(sizes=sizes)
    assert rc == VBF_EINVAL and b"is NULL" in msg and b"n_out / key_bytes / value_bytes" in msg
    assert (roff == POISON).all() and all(g == POISON for g in got)


def test_handle_checks(empty):
    from velarixdb_amd._lib import VBF_EINVAL
    a, b, c = empty
    rc, msg, sizes, (roff, k0, v0) = _scan(log=None)
    assert rc == VBF_EINVAL and b"vlog is NULL" in msg and sizes == (0, 0, 0) and (roff == POISON).all()
    assert (k0, v0) == (POISON, POISON)
    rc, msg, *_ = _scan(log=None, gc=FAKE)
    assert rc == VBF_EINVAL and b"a gc table needs the log: log is NULL" in msg
    rc, msg, *_ = _scan(nro=2, ro=None)
    assert rc == VBF_EINVAL and b"ro is NULL" in msg
    rc, msg, *_ = _scan(nro=2, ro=(ctypes.c_void_p * 2)(0x1000, None))
    assert rc == VBF_EINVAL and b"ro[1] is NULL" in msg
    rc, msg, *_ = _scan(nsst=2, tables=None)
    assert rc == VBF_EINVAL and b"tables is NULL" in msg
    rc, msg, *_ = _scan(nsst=2, tables=(ctypes.c_void_p * 2)(0x1000, None))
    assert rc == VBF_EINVAL and b"tables[1] is NULL" in msg
    # handles on two devices: the memtables among themselves, before the log is followed
    rc, msg, *_ = _scan(active=a, nro=2, ro=(ctypes.c_void_p * 2)(b.value, c.value))
    assert rc == VBF_EINVAL and b"lives on device 1" in msg
    rc, msg, *_ = _scan(active=c, nro=1, ro=(ctypes.c_void_p * 1)(a.value))
    assert rc == VBF_EINVAL and b"lives on device 0, the other handles on 1" in msg


def test_flags_and_bounds():
    from velarixdb_amd._lib import VBF_EINVAL
    for flags in (4, 8, 0x80000000, 7):
        rc, msg, sizes, (roff, *_) = _scan(flags=flags)
        assert rc == VBF_EINVAL and b"unknown flags" in msg and sizes == (0, 0, 0) and (roff == POISON).all()
    rc, msg, *_ = _scan(ranges=((b"ab", b"cd"), (b"e", b"f")), boff=[0, 2, 4, 3, 6])
    assert rc == VBF_EINVAL and b"bounds_off decreases at entry 3" in msg
    rc, msg, *_ = _scan(ranges=((b"ab", b"cd"),), boff=[5, 2, 4])
    assert rc == VBF_EINVAL and b"bounds_off decreases at entry 1" in msg
    rc, msg, *_ = _scan(nranges=1 << 30, sizes=(1, 1, 1))  # 2^30 ranges x 2 layers: decided before bounds_off is read
    assert rc == VBF_EINVAL and b"too many entries" in msg


def test_no_range_and_no_layer_need_no_device():
    from velarixdb_amd._lib import VBF_OK
    rc, msg, sizes, (roff, k0, v0) = _scan(ranges=())
    assert (rc, msg) == (VBF_OK, b"") and sizes == (0, 0, 0) and roff.tolist() == [0] and (k0, v0) == (0, 0)
    # no layer at all: every range is empty
    for flags in (0, 1, 2, 3):
        rc, msg, sizes, (roff, k0, v0) = _scan(ranges=((b"", b"\xff"), (b"b", b"a"), (b"k", b"k")), flags=flags)
        assert (rc, msg) == (VBF_OK, b"") and sizes == (0, 0, 0) and roff.tolist() == [0, 0, 0, 0] and (k0, v0) == (0, 0)


def test_signature_and_python_layer():
    import velarixdb_amd as v
    from velarixdb_amd import _lib
    res, args = _lib.SIGNATURES["vbf_store_scan_host"]
    assert res is ctypes.c_int and len(args) == 29
    assert v.store_scan_many is v.store.scan_many and v.scan_many is v.table.scan_many
    assert list(v.StoreScan.__dataclass_fields__) == ["range_off", "keys", "key_off", "tombstones", "layer", "table",
                                                      "val_offsets", "created_ms", "values"]
    r = v.store.scan_many([(b"a", b"b"), (b"", b"\xff")], [], FAKE_VLOG)  # no layer: no device
    assert r.range_off.tolist() == [0, 0, 0] and r.keys.size == 0 and r.key_off.tolist() == [0]
    assert r.values.value_off.tolist() == [0] and list(r.range(1)) == []


class _Fake:
    _h = FAKE


FAKE_VLOG = _Fake()
