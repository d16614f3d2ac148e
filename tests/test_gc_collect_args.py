"""vbf_gc_collect_host: the checks that return before any device work (no GPU needed)."""
import ctypes

import numpy as np

FAKE = ctypes.c_void_p(0x1000)  # a non-NULL handle that a failing check never follows
SCALARS = ("n_chunk", "n_invalid", "n_puts", "append_len", "end_off", "stop")


def overlay(keys, off=None):
    """-> (ov_keys, ov_off, ov_val_offsets, ov_created_ms, ov_tombstones, ov_n) and the arrays that back them"""
    n = len(keys)
    kd = np.frombuffer(b"".join(keys) + b"\0", np.uint8)
    ko = np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.uint64) if off is None else np.array(off, np.uint64)
    vo, cr, tb = np.zeros(n, np.uint32), np.zeros(n, np.int64), np.zeros(n, np.uint8)
    keep = (kd, ko, vo, cr, tb)
    return [x.ctypes.data for x in keep] + [n], keep


def _collect(v=FAKE, tail=0, log_size=0, nsst=0, tables=None, filters=None, ov=None, missing=None):
    """A size query with every scalar preset to 7; -> (rc, [the six scalars], the message)"""
    from velarixdb_amd._lib import lib
    sc = [ctypes.c_uint64(7) for _ in range(5)] + [ctypes.c_int(7)]
    scalars = [None if name == missing else ctypes.byref(x) for name, x in zip(SCALARS, sc)]
    ov = ov or [None, None, None, None, None, 0]
    rc = lib.vbf_gc_collect_host(v, tail, 100, log_size, 5, nsst, tables, filters, *ov, None, 0, None, 0, None, None, None,
                                 0, *scalars)
    return rc, [x.value for x in sc], lib.vbf_last_error()


def test_signature_and_the_seven_constants():
    from velarixdb_amd import _lib
    res, args = _lib.SIGNATURES["vbf_gc_collect_host"]
    assert res is ctypes.c_int and len(args) == 28
    assert args[4] is ctypes.c_int64 and args[-1] == ctypes.POINTER(ctypes.c_int)
    assert hasattr(_lib.lib, "vbf_gc_collect_host")
    assert (_lib.VBF_GC_VALID, _lib.VBF_GC_ABSENT, _lib.VBF_GC_DELETED, _lib.VBF_GC_LOG_NONE, _lib.VBF_GC_LOG_TOMBSTONE,
            _lib.VBF_GC_OLDER, _lib.VBF_GC_STAR) == (0, 1, 2, 3, 4, 5, 6)


def test_null_scalars_write_nothing():
    from velarixdb_amd._lib import VBF_EINVAL
    for name in SCALARS:
        rc, sc, msg = _collect(missing=name, tail=12)
        assert rc == VBF_EINVAL and ("%s is NULL" % name).encode() in msg
        assert sc == [7] * 6


def test_null_log_after_the_scalars():
    from velarixdb_amd._lib import VBF_EINVAL
    rc, sc, msg = _collect(v=None, tail=12)
    assert rc == VBF_EINVAL and b"vlog is NULL" in msg
    assert sc == [0, 0, 0, 0, 12, 0]  # the scalars are written first: no entry, end_off = tail, VBF_WALK_END


def test_tables_and_filters():
    from velarixdb_amd._lib import VBF_EINVAL
    rc, sc, msg = _collect(nsst=2, tables=None)
    assert rc == VBF_EINVAL and b"tables is NULL" in msg and sc == [0, 0, 0, 0, 0, 0]
    th = (ctypes.c_void_p * 2)(0x1000, None)
    rc, _, msg = _collect(nsst=2, tables=th)
    assert rc == VBF_EINVAL and b"tables[1] is NULL" in msg
    th = (ctypes.c_void_p * 2)(0x1000, 0x1000)
    fh = (ctypes.c_void_p * 2)(None, 0x1000)
    rc, _, msg = _collect(nsst=2, tables=th, filters=fh)
    assert rc == VBF_EINVAL and b"filters[0] is NULL" in msg


def test_overlay_arrays():
    from velarixdb_amd._lib import VBF_EINVAL
    names = ("ov_keys", "ov_off", "ov_val_offsets", "ov_created_ms", "ov_tombstones")
    for i, name in enumerate(names):
        ov, _keep = overlay([b"a", b"b"])
        ov[i] = None
        rc, sc, msg = _collect(ov=ov)
        assert rc == VBF_EINVAL and ("%s is NULL" % name).encode() in msg and sc == [0, 0, 0, 0, 0, 0]
    ov, _keep = overlay([b"a", b"b"], off=[0, 2, 1])
    rc, _, msg = _collect(ov=ov)
    assert rc == VBF_EINVAL and b"ov_off descends at key 1" in msg


def test_overlay_order():
    from velarixdb_amd._lib import VBF_EINVAL
    for keys, at in (([b"a", b"b", b"b", b"c"], 2),          # equal neighbours
                     ([b"a", b"c", b"b"], 2),                # descending
                     ([b"ab", b"a"], 1),                     # a prefix sorts first (Ord for [u8])
                     ([b"", b""], 1)):
        ov, _keep = overlay(keys)
        rc, _, msg = _collect(ov=ov)
        assert rc == VBF_EINVAL and ("not strictly ascending at key %d" % at).encode() in msg, keys
    # an ascending overlay passes this check: the next one to fail is the log_size rule
    ov, _keep = overlay([b"", b"a", b"a\0", b"ab", b"b"])
    rc, _, msg = _collect(ov=ov, log_size=2**32 - 24)
    assert rc == VBF_EINVAL and b"2^32" in msg


def test_log_size_at_the_u32_limit():
    from velarixdb_amd._lib import VBF_EINVAL
    for log_size in (2**32 - 24, 2**32, 2**64 - 1):
        rc, sc, msg = _collect(log_size=log_size)  # FAKE is not followed: rejected before any device work
        assert rc == VBF_EINVAL and b"2^32" in msg and sc == [0, 0, 0, 0, 0, 0]


def test_python_layer_exports():
    import velarixdb_amd as v
    assert callable(v.gc.collect_device) and v.collect_device is v.gc.collect_device and callable(v.gc.collect)
    fields = list(v.gc.GcResult.__dataclass_fields__)
    assert fields[-1] == "verdict" and v.gc.GcResult.__dataclass_fields__["verdict"].default is None
    assert "gc_judge" in v._lib.PHASES and v._lib.PHASES.index("gc_judge") == 28 and v._lib.PHASES[29] == "gc_emit"
