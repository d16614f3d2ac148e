"""vbf_vlog_walk_*: the checks that return before any device work (no GPU needed)."""
import ctypes

import numpy as np

FAKE = ctypes.c_void_p(0x1000)  # a non-NULL handle that a failing check never follows
SCALARS = ("n_out", "key_bytes", "value_bytes", "end_off", "stop")


def _walk(fn, h, start=0, budget=0, missing=None):
    """A size query with every scalar preset to 7; -> (rc, [the five scalars])"""
    from velarixdb_amd._lib import lib
    sc = [ctypes.c_uint64(7) for _ in range(4)] + [ctypes.c_int(7)]
    tail = [None if name == missing else ctypes.byref(x) for name, x in zip(SCALARS, sc)]
    head = (h, start, budget, None, None, None, 0, None, None, 0, None, None, None, 0)
    rc = lib.vbf_vlog_walk_dev(*head, *tail, None) if fn == "dev" else lib.vbf_vlog_walk_host(*head, *tail)
    return rc, [x.value for x in sc]


def test_signatures_hold_both_symbols_and_the_constants():
    from velarixdb_amd import _lib
    assert "vbf_vlog_walk_dev" in _lib.SIGNATURES and "vbf_vlog_walk_host" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["vbf_vlog_walk_dev"][1]) == len(_lib.SIGNATURES["vbf_vlog_walk_host"][1]) + 1 == 20
    assert (_lib.VBF_WALK_END, _lib.VBF_WALK_BUDGET, _lib.VBF_WALK_TORN) == (0, 1, 2)


def test_null_scalars():
    from velarixdb_amd._lib import VBF_EINVAL, lib
    for fn in ("dev", "host"):
        for name in SCALARS:
            rc, sc = _walk(fn, FAKE, missing=name)
            assert rc == VBF_EINVAL and ("%s is NULL" % name).encode() in lib.vbf_last_error()
            assert sc == [7] * 5  # nothing is written when a scalar is missing


def test_null_handle():
    from velarixdb_amd._lib import VBF_EINVAL, lib
    for fn in ("dev", "host"):
        rc, sc = _walk(fn, None, start=12, budget=5)
        assert rc == VBF_EINVAL and b"vlog is NULL" in lib.vbf_last_error()
        assert sc == [0, 0, 0, 12, 0]  # the scalars are written first: no entry, end_off = start


def test_python_layer_exports():
    import velarixdb_amd as v
    assert hasattr(v.ValueLog, "walk") and hasattr(v.ValueLog, "recover") and hasattr(v.ValueLog, "read_chunk")
    assert hasattr(v.memtable, "recover_puts") and hasattr(v.gc, "collect")
    assert (v.vlog.WALK_END, v.vlog.WALK_BUDGET, v.vlog.WALK_TORN) == (0, 1, 2)
    w = v.Walk(np.array([0, 20], np.uint64), v.pack_offsets(np.frombuffer(b"abc", np.uint8), [0, 3]),
               np.frombuffer(b"", np.uint8), np.array([0, 0], np.uint64), np.array([5], np.int64), np.zeros(1, np.uint8), 20, 0)
    assert (w.n, w.key(0), w.value(0), w.val_offsets.tolist()) == (1, b"abc", b"", [0])
