"""The device-resident memtable handle: vbf_memtable_open_host / _dev, export and encode.

Reference: memtable_ref.sort_ids (SkipMap order, the last put of a key wins) applied to the puts, and
vbf_flush_write_host over the same puts for the files.  Every comparison is exact.  The put counts
stand at the sort's 2048-entry tile edge and at the lookup's 4096-word LDS sample edge."""
import ctypes
import functools

import numpy as np
import pytest

import key_torture as kt
import memtable_ref as mref

pytestmark = pytest.mark.gpu
SIZES = (0, 1, 2047, 2048, 2049, 4097, 8193)
MAX_KEY = 4079  # the encoder's longest key


@functools.lru_cache(maxsize=None)
def puts(n, seed=0x4A7D):
    """n puts, about 30 % of them of a key put before: keys of the ordering universe (families past 8
    equal bytes, pairs that differ by trailing zero bytes) and torture keys."""
    rng = np.random.default_rng([seed, n])
    uni = kt.ordered_universe()
    tor = [k for k in kt.torture_keys(5) if len(k) <= MAX_KEY]
    keys = []
    for j in range(n):
        if keys and rng.random() < 0.3:
            keys.append(keys[int(rng.integers(0, len(keys)))])
        else:
            src = uni if rng.random() < 0.6 else tor
            keys.append(src[int(rng.integers(0, len(src)))])
    if n >= 2047:
        keys[:4] = [b"ab", b"ab\0", b"", b"ab\0\0"]
        keys[-2:] = [b"ab\0", b""]
    vo = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    cr = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
    tb = (rng.integers(0, 4, n) == 0).astype(np.uint8)
    return keys, vo, cr, tb


def expected(keys, vo, cr, tb):
    ids = mref.sort_ids(keys).astype(np.int64)
    return [keys[i] for i in ids.tolist()], vo[ids], cr[ids], tb[ids]


def check_export(mt, want):
    wk, wvo, wcr, wtb = want
    assert mt.entries == len(wk) and mt.key_bytes == sum(len(k) for k in wk) and mt.device == 0
    e = mt.export()
    assert e.keys.offsets[0] == 0 and e.keys.offsets.size == len(wk) + 1
    assert e.keys.data.tobytes() == b"".join(wk)
    assert e.keys.offsets.tolist() == np.concatenate([[0], np.cumsum([len(k) for k in wk])]).astype(np.uint64).tolist()
    assert np.array_equal(e.val_offsets, wvo) and np.array_equal(e.created_ms, wcr) and np.array_equal(e.tombstones, wtb)


@pytest.mark.parametrize("n", SIZES)
def test_open_host_and_export(vbf, n):
    keys, vo, cr, tb = puts(n)
    with vbf.MemTable.open(keys, vo, cr, tb) as mt:
        check_export(mt, expected(keys, vo, cr, tb))


def open_dev(keys_arr, offs, stride, n, vo, cr, tb, lead=0):
    import torch
    from velarixdb_amd import MemTable
    from velarixdb_amd._lib import call
    keep = []

    def up(a):
        if a is None:
            return None
        t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")
        keep.append(t)
        return ctypes.c_void_p(t.data_ptr())
    h = ctypes.c_void_p()
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    call("vbf_memtable_open_dev", up(keys_arr), up(offs), stride, n, up(vo), up(cr), up(tb), sp, ctypes.byref(h))
    for t in keep:  # the handle copies: the caller's arrays may go
        t.fill_(0xEE)
    torch.cuda.synchronize()
    return MemTable(h)


@pytest.mark.parametrize("n", SIZES)
def test_open_dev_and_export(vbf, n):
    keys, vo, cr, tb = puts(n)
    data, offs = kt.pack_lead(keys, lead=13)  # offsets[0] != 0
    with open_dev(data if data.size else np.zeros(1, np.uint8), offs, 0, n, vo, cr, tb) as mt:
        check_export(mt, expected(keys, vo, cr, tb))


@pytest.mark.parametrize("which", ("host", "dev"))
def test_fixed_stride_and_absent_arrays(vbf, which):
    """Keys by stride (no offsets) and NULL per-entry arrays, which mean zeros."""
    rng = np.random.default_rng(0x57)
    n, stride = 2500, 9
    rows = rng.integers(0, 3, (n, stride), dtype=np.uint8)  # few distinct bytes: many equal prefixes, some equal keys
    keys = [r.tobytes() for r in rows]
    tb = (rng.integers(0, 2, n)).astype(np.uint8) * 7          # a tombstone byte != 0 is a tombstone, kept as given
    if which == "host":
        from velarixdb_amd.keys import HostBatch
        mt = vbf.MemTable.open(HostBatch(rows.reshape(-1).copy(), None, stride, n, 1), None, None, tb)
    else:
        mt = open_dev(rows.reshape(-1), None, stride, n, None, None, tb)
    with mt:
        wk, _, _, wtb = expected(keys, np.zeros(n, np.uint32), np.zeros(n, np.int64), tb)
        check_export(mt, (wk, np.zeros(len(wk), np.uint32), np.zeros(len(wk), np.int64), wtb))


@pytest.mark.parametrize("n", SIZES[1:])
def test_encode_equals_flush_write(vbf, n):
    from velarixdb_amd import memtable
    keys, vo, cr, tb = puts(n)
    want = memtable.flush(keys, vo, cr, tb)
    with vbf.MemTable.open(keys, vo, cr, tb) as mt:
        got = mt.flush()
        assert got.data.tobytes() == want.data.tobytes() and got.index.tobytes() == want.index.tobytes()
        assert (got.smallest, got.biggest) == (want.smallest, want.biggest)
        # the size query, then capacities one byte short: the sizes are written, the outputs untouched
        from velarixdb_amd._lib import VBF_EINVAL, lib
        dl, il = ctypes.c_uint64(), ctypes.c_uint64()
        assert lib.vbf_memtable_encode_host(mt._h, None, 0, ctypes.byref(dl), None, 0, ctypes.byref(il)) == 0
        assert (dl.value, il.value) == (want.data.size, want.index.size)
        d, i = np.full(dl.value, 0xA5, np.uint8), np.full(il.value, 0xA5, np.uint8)
        for dc, ic in ((dl.value - 1, il.value), (dl.value, il.value - 1)):
            dl2, il2 = ctypes.c_uint64(), ctypes.c_uint64()
            rc = lib.vbf_memtable_encode_host(mt._h, d.ctypes.data, dc, ctypes.byref(dl2), i.ctypes.data, ic, ctypes.byref(il2))
            assert rc == VBF_EINVAL and (dl2.value, il2.value) == (dl.value, il.value)
            assert (d == 0xA5).all() and (i == 0xA5).all()


def test_export_capacities(vbf):
    from velarixdb_amd._lib import VBF_EINVAL, lib
    keys, vo, cr, tb = puts(2049)
    with vbf.MemTable.open(keys, vo, cr, tb) as mt:
        n, kb = mt.entries, mt.key_bytes
        k, off = np.full(kb, 0xA5, np.uint8), np.full(n + 1, 0xA5A5, np.uint64)
        assert lib.vbf_memtable_export_host(mt._h, k.ctypes.data, kb - 1, None, None, None, None, 0) == VBF_EINVAL
        assert lib.vbf_memtable_export_host(mt._h, k.ctypes.data, kb, off.ctypes.data, None, None, None, n - 1) == VBF_EINVAL
        assert (k == 0xA5).all() and (off == 0xA5A5).all()
        assert lib.vbf_memtable_export_host(mt._h, None, 0, off.ctypes.data, None, None, None, n) == 0
        assert off[0] == 0 and off[-1] == kb and (k == 0xA5).all()


def test_open_dev_descending_offsets(vbf):
    import torch
    from velarixdb_amd._lib import VBF_EINVAL, lib
    k = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    o = torch.tensor([0, 4, 2, 8], dtype=torch.int64, device="cuda:0")
    h = ctypes.c_void_p()
    rc = lib.vbf_memtable_open_dev(ctypes.c_void_p(k.data_ptr()), ctypes.c_void_p(o.data_ptr()), 0, 3, None, None, None,
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(h))
    assert rc == VBF_EINVAL and b"offsets descend at entry 1" in lib.vbf_last_error() and not h.value
