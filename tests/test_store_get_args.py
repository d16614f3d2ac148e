"""vbf_memtable_* and vbf_store_get_host: the checks that return before any HIP call (no GPU needed).

An empty memtable opens without device work, so real handles (on device 0 and on device 1) stand in
where a check follows a handle; FAKE is a non-NULL handle that a failing check never follows."""
import ctypes

import numpy as np
import pytest

FAKE = ctypes.c_void_p(0x1000)
POISON = 7


def _p(a):
    return None if a is None else a if isinstance(a, (int, ctypes.c_void_p)) else a.ctypes.data


def _keys(n=3):
    return np.arange(97, 97 + n, dtype=np.uint8), np.arange(n + 1, dtype=np.uint64)


def _open(which, keys, offsets, stride, n, out=True, device=0):
    from velarixdb_amd._lib import lib
    h = ctypes.c_void_p(POISON)
    po = ctypes.byref(h) if out else None
    if which == "dev":
        rc = lib.vbf_memtable_open_dev(_p(keys), _p(offsets), stride, n, None, None, None, None, po)
    else:
        rc = lib.vbf_memtable_open_host(_p(keys), _p(offsets), stride, n, None, None, None, device, po)
    return rc, lib.vbf_last_error(), h


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


@pytest.mark.parametrize("which", ("dev", "host"))
def test_open_checks(which):
    from velarixdb_amd._lib import VBF_EINVAL
    k, o = _keys()
    rc, msg, _ = _open(which, k, o, 0, 3, out=False)
    assert rc == VBF_EINVAL and b"out is NULL" in msg
    rc, msg, h = _open(which, None, None, 1, 1 << 31)
    assert rc == VBF_EINVAL and b"too many entries" in msg and h.value is None
    rc, msg, h = _open(which, None, None, 4, 3)
    assert rc == VBF_EINVAL and b"keys is NULL" in msg and h.value is None


def test_open_host_descending_offsets():
    from velarixdb_amd._lib import VBF_EINVAL
    rc, msg, h = _open("host", np.zeros(8, np.uint8), np.asarray([0, 4, 2, 8], np.uint64), 0, 3)
    assert rc == VBF_EINVAL and b"offsets descend at entry 1" in msg and h.value is None


def test_empty_memtable_and_accessors(empty):
    from velarixdb_amd._lib import VBF_EINVAL, lib
    a, _, c = empty
    assert (lib.vbf_memtable_entries(a), lib.vbf_memtable_key_bytes(a), lib.vbf_memtable_device(a)) == (0, 0, 0)
    assert lib.vbf_memtable_device(c) == 1
    assert (lib.vbf_memtable_entries(None), lib.vbf_memtable_key_bytes(None), lib.vbf_memtable_device(None)) == (0, 0, -1)
    lib.vbf_memtable_free(None)
    # export: the size query, and an empty table's one offset
    assert lib.vbf_memtable_export_host(a, None, 0, None, None, None, None, 0) == 0
    off = np.full(1, POISON, np.uint64)
    assert lib.vbf_memtable_export_host(a, None, 0, off.ctypes.data, None, None, None, 0) == 0 and off[0] == 0
    assert lib.vbf_memtable_export_host(None, None, 0, None, None, None, None, 0) == VBF_EINVAL
    assert b"memtable is NULL" in lib.vbf_last_error()
    # encode: "Cannot flush an empty table"
    dl, il = ctypes.c_uint64(POISON), ctypes.c_uint64(POISON)
    rc = lib.vbf_memtable_encode_host(a, None, 0, ctypes.byref(dl), None, 0, ctypes.byref(il))
    assert rc == VBF_EINVAL and b"Cannot flush an empty table" in lib.vbf_last_error() and (dl.value, il.value) == (0, 0)
    assert lib.vbf_memtable_encode_host(a, None, 0, None, None, 0, ctypes.byref(il)) == VBF_EINVAL
    assert lib.vbf_memtable_encode_host(None, None, 0, ctypes.byref(dl), None, 0, ctypes.byref(il)) == VBF_EINVAL


def _get(which, keys, offsets, stride, n, gc=None, active=None, nro=0, ro=None, log=None):
    from velarixdb_amd._lib import lib
    head = (_p(keys), _p(offsets), stride, n, gc, active, nro, ro, log, None, None, None, None)
    rc = lib.vbf_memtable_get_dev(*head, None) if which == "dev" else lib.vbf_memtable_get_host(*head)
    return rc, lib.vbf_last_error()


@pytest.mark.parametrize("which", ("dev", "host"))
def test_get_checks(which, empty):
    from velarixdb_amd._lib import VBF_EINVAL, VBF_OK
    a, b, c = empty
    k, o = _keys()
    assert _get(which, None, None, 0, 0) == (VBF_OK, b"")                       # no keys: nothing to do
    assert _get(which, None, None, 0, 0, active=a, nro=1, ro=(ctypes.c_void_p * 1)(b.value)) == (VBF_OK, b"")
    rc, msg = _get(which, None, None, 1, (1 << 31) - 1, active=FAKE)
    assert rc == VBF_EINVAL and b"too many keys" in msg
    rc, msg = _get(which, None, None, 4, 3, active=FAKE)
    assert rc == VBF_EINVAL and b"keys is NULL" in msg
    rc, msg = _get(which, k, o, 0, 3, active=FAKE, nro=2, ro=None)
    assert rc == VBF_EINVAL and b"ro is NULL" in msg
    rc, msg = _get(which, k, o, 0, 3, active=FAKE, nro=2, ro=(ctypes.c_void_p * 2)(0x1000, None))
    assert rc == VBF_EINVAL and b"ro[1] is NULL" in msg
    rc, msg = _get(which, k, o, 0, 3, gc=FAKE, active=FAKE)
    assert rc == VBF_EINVAL and b"log is NULL" in msg
    # all handles on one device
    rc, msg = _get(which, k, o, 0, 3, active=a, nro=2, ro=(ctypes.c_void_p * 2)(b.value, c.value))
    assert rc == VBF_EINVAL and b"lives on device 1" in msg
    rc, msg = _get(which, k, o, 0, 3, active=c, nro=1, ro=(ctypes.c_void_p * 1)(a.value))
    assert rc == VBF_EINVAL and b"lives on device 0, the other handles on 1" in msg


def test_get_host_descending_offsets_and_no_layer(empty):
    from velarixdb_amd._lib import VBF_EINVAL, lib
    rc, msg = _get("host", np.zeros(8, np.uint8), np.asarray([0, 4, 2, 8], np.uint64), 0, 3, active=empty[0])
    assert rc == VBF_EINVAL and b"offsets descend at entry 1" in msg
    # no memtable at all: nothing is found, and no device is needed to say so
    k, o = _keys()
    f, l = np.full(3, POISON, np.uint8), np.full(3, POISON, np.uint32)
    v, c = np.full(3, POISON, np.uint32), np.full(3, POISON, np.uint64)
    rc = lib.vbf_memtable_get_host(k.ctypes.data, o.ctypes.data, 0, 3, None, None, 0, None, None, f.ctypes.data,
                                   l.ctypes.data, v.ctypes.data, c.ctypes.data)
    assert rc == 0 and not f.any() and (l == 0xFFFFFFFF).all() and not v.any() and not c.any()


def _store(keys, offsets, stride, n, log=FAKE, gc=None, active=None, nro=0, ro=None, nsst=0, tables=None, filters=None,
           nbytes=True):
    from velarixdb_amd._lib import lib
    nb = ctypes.c_uint64(POISON)
    voff = np.full(1, POISON, np.uint64)
    rc = lib.vbf_store_get_host(_p(keys), _p(offsets), stride, n, gc, active, nro, ro, nsst, tables, filters, log, 0,
                                None, None, None, None, None, None, None, 0, voff.ctypes.data,
                                ctypes.byref(nb) if nbytes else None)
    return rc, lib.vbf_last_error(), nb.value, int(voff[0])


def test_store_get_checks(empty):
    from velarixdb_amd._lib import VBF_EINVAL
    a, b, c = empty
    k, o = _keys()
    rc, msg, nb, _ = _store(k, o, 0, 3, nbytes=False)
    assert rc == VBF_EINVAL and b"value_bytes is NULL" in msg and nb == POISON
    rc, msg, nb, _ = _store(k, o, 0, 3, log=None)
    assert rc == VBF_EINVAL and b"vlog is NULL" in msg and nb == 0
    rc, msg, nb, _ = _store(None, None, 1, (1 << 31) - 1)
    assert rc == VBF_EINVAL and b"too many keys" in msg and nb == 0
    rc, msg, *_ = _store(None, None, 4, 3)
    assert rc == VBF_EINVAL and b"keys is NULL" in msg
    rc, msg, *_ = _store(k, o, 0, 3, nro=1, ro=None)
    assert rc == VBF_EINVAL and b"ro is NULL" in msg
    rc, msg, *_ = _store(k, o, 0, 3, nro=1, ro=(ctypes.c_void_p * 1)(None))
    assert rc == VBF_EINVAL and b"ro[0] is NULL" in msg
    rc, msg, *_ = _store(np.zeros(8, np.uint8), np.asarray([0, 4, 2, 8], np.uint64), 0, 3)
    assert rc == VBF_EINVAL and b"offsets descend at entry 1" in msg
    rc, msg, *_ = _store(k, o, 0, 3, nsst=2, tables=None)
    assert rc == VBF_EINVAL and b"tables is NULL" in msg
    rc, msg, *_ = _store(k, o, 0, 3, nsst=2, tables=(ctypes.c_void_p * 2)(0x1000, None))
    assert rc == VBF_EINVAL and b"tables[1] is NULL" in msg
    rc, msg, *_ = _store(k, o, 0, 3, nsst=2, tables=(ctypes.c_void_p * 2)(0x1000, 0x1000),
                         filters=(ctypes.c_void_p * 2)(None, 0x1000))
    assert rc == VBF_EINVAL and b"filters[0] is NULL" in msg
    # the memtables among themselves, before the log is followed
    rc, msg, *_ = _store(k, o, 0, 3, active=a, nro=1, ro=(ctypes.c_void_p * 1)(c.value))
    assert rc == VBF_EINVAL and b"lives on device 1" in msg


def test_signatures_and_python_layer():
    import velarixdb_amd as v
    from velarixdb_amd import _lib
    for name, nargs in (("vbf_memtable_open_host", 9), ("vbf_memtable_open_dev", 9), ("vbf_memtable_export_host", 8),
                        ("vbf_memtable_encode_host", 7), ("vbf_memtable_get_dev", 14), ("vbf_memtable_get_host", 13),
                        ("vbf_store_get_host", 23)):
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs, name
    assert v.MemTable is v.memtable.MemTable and callable(v.store.get_many) and callable(v.MemTable.get_many)
    assert list(v.store.StoreGet.__dataclass_fields__) == ["found", "layer", "table", "val_offsets", "created_ms", "values"]
    assert list(v.memtable.MemGet.__dataclass_fields__) == ["found", "layer", "val_offsets", "created_ms"]
    assert (v.memtable.LAYER_GC, v.memtable.LAYER_ACTIVE, v.memtable.LAYER_READ_ONLY) == (0, 1, 2)
    assert _lib.PHASES[30] == "mem_get"
    with v.MemTable.open([], np.zeros(0, np.uint32)) as mt:  # an empty memtable needs no device
        assert mt.entries == 0 and mt.device == 0
        with pytest.raises(AssertionError, match="Cannot flush an empty table"):
            mt.flush()
    assert mt._h is None
