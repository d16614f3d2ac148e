"""GPU parity for the memtable flush: vbf_memtable_sort_*, vbf_filter_insert_* and
vbf_flush_write_host against the Python restatement (tests/memtable_ref.py), the oracle's
Table::write_to_file and its filter build.  Every comparison is exact equality.

The sort's tile is 2048 entries (the merge's): the sizes below sit on its edges, give odd
segment counts at a merge level, and 3 and 5 tiles."""
import ctypes

import numpy as np
import pytest

import key_torture as kt
import memtable_ref as ref
from test_memtable_args import insert_cases

pytestmark = pytest.mark.gpu
T0 = 1_720_785_462_309  # a real clock (ms): created_at == 0 never wins a get (store.rs:616-618)


def _sort_host(data, offsets, stride, n):
    from velarixdb_amd._lib import call
    ids, c = np.zeros(max(n, 1), np.uint32), ctypes.c_uint64()
    call("vbf_memtable_sort_host", data.ctypes.data if data.size else None,
         None if offsets is None else offsets.ctypes.data, stride, n, ids.ctypes.data, ctypes.byref(c), 0)
    return ids[:c.value]


def _sort_dev(data, offsets, stride, n):
    """The same batch from device memory on the current torch stream."""
    import torch
    from velarixdb_amd._lib import call
    dev = torch.device("cuda:0")
    d = torch.from_numpy(data if data.size else np.zeros(1, np.uint8)).to(dev)
    o = None if offsets is None else torch.from_numpy(offsets.view(np.int64)).to(dev)
    ids = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    c = ctypes.c_uint64()
    call("vbf_memtable_sort_dev", d.data_ptr(), None if o is None else o.data_ptr(), stride, n, ids.data_ptr(),
         ctypes.byref(c), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    return ids.cpu().numpy().view(np.uint32)[:c.value]


def _check(keys):
    """sort_ids (Python API, _host) and _dev against the restatement."""
    from velarixdb_amd import memtable
    from velarixdb_amd.keys import pack
    want = ref.sort_ids(keys)
    got = memtable.sort_ids(keys)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    b = pack(keys)
    assert np.array_equal(_sort_dev(b.data, b.offsets, b.stride, b.n), want)


def _dup_keys(rng, n):
    """n random 1-24-byte keys from a universe of n / 4: about four copies each, across tiles."""
    uni = [rng.bytes(int(L)) for L in rng.integers(1, 25, max(1, n // 4))]
    return [uni[i] for i in rng.integers(0, len(uni), n)]


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 6145, 10241])
def test_sort_sizes_with_duplicates(vbf, n):
    _check(_dup_keys(np.random.default_rng([0x3E37, n]), n))


def test_sort_degenerate_batches(vbf):
    _check([b"the-one-key"] * 5000)
    _check([b"left", b"right"] * 2048 + [b"left"])  # 4097 entries
    asc = [b"key%06d" % i for i in range(4500)]
    _check(asc)
    _check(asc[::-1])


def test_sort_shared_prefix_and_length_chain(vbf):
    rng = np.random.default_rng(0x5A4ED)
    stem = b"user0000-0000000"  # 16 bytes: every compare past the 8-byte prefix reads the key bytes
    _check([stem + bytes([int(x)]) + b"tail" * int(y) for x, y in zip(rng.integers(0, 256, 5000), rng.integers(0, 3, 5000))])
    chain = [b"a" * i for i in range(41)] * 60  # b"", b"a", b"aa", ...: a proper prefix sorts first
    _check([chain[i] for i in rng.permutation(len(chain))])
    _check(kt.ordered_universe()[::-1] + kt.ordered_universe())


def test_sort_torture_batch_twice(vbf):
    """20 011 keys with 65 536-byte ones, 0x00 / 0xff runs and truncation pairs, then a shuffled copy
    of the same keys: every key occurs at least twice."""
    keys = kt.torture_keys(7)
    rng = np.random.default_rng(0x70C7)
    _check(keys + [keys[i] for i in rng.permutation(len(keys))])


def test_sort_first_offset_not_zero(vbf):
    keys = _dup_keys(np.random.default_rng(0x1EAD), 5000)
    want = ref.sort_ids(keys)
    for lead in (1, 13, 4096):
        data, offsets = kt.pack_lead(keys, lead)
        assert np.array_equal(_sort_host(data, offsets, 0, len(keys)), want)
        assert np.array_equal(_sort_dev(data, offsets, 0, len(keys)), want)


@pytest.mark.parametrize("stride", [1, 7, 16, 33])
def test_sort_fixed_strides(vbf, stride):
    rng = np.random.default_rng([0x57D1, stride])
    n = 5000
    uni = rng.integers(0, 256, (min(256 ** min(stride, 2), 1200), stride), dtype=np.uint8)
    rows = uni[rng.integers(0, len(uni), n)]
    rows[:, : stride // 2] = rows[0, : stride // 2]  # a shared first half: ties in the 8-byte prefix
    data = np.ascontiguousarray(rows).reshape(-1)
    want = ref.sort_ids([r.tobytes() for r in rows])
    assert stride > 1 or want.size <= 256
    assert np.array_equal(_sort_host(data, None, stride, n), want)
    assert np.array_equal(_sort_dev(data, None, stride, n), want)


def test_sort_empty_keys_only(vbf):
    """stride 0 without offsets: n empty keys, one distinct key, its last put."""
    assert _sort_host(np.zeros(0, np.uint8), None, 0, 3000).tolist() == [2999]
    assert _sort_dev(np.zeros(0, np.uint8), None, 0, 3000).tolist() == [2999]


def test_sort_dev_reports_descending_offsets(vbf):
    """_dev finds them in its first pass; the later passes then see empty keys only."""
    import torch
    from velarixdb_amd._lib import VBF_EINVAL, lib
    dev = torch.device("cuda:0")
    off = np.arange(0, 4 * 3001, 4, dtype=np.uint64)
    off[1700] = 3  # descends at entry 1699 (and rises again)
    d = torch.zeros(4 * 3000, dtype=torch.uint8, device=dev)
    o = torch.from_numpy(off.view(np.int64)).to(dev)
    ids = torch.zeros(3000, dtype=torch.int32, device=dev)
    c = ctypes.c_uint64(7)
    rc = lib.vbf_memtable_sort_dev(d.data_ptr(), o.data_ptr(), 0, 3000, ids.data_ptr(), ctypes.byref(c),
                                   ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == VBF_EINVAL and b"offsets descend at entry 1699" in lib.vbf_last_error() and c.value == 0


# ---- the flush ----

def _gather(b, ids):
    """numpy gather of the batch's keys by ids -> (keys, offsets)"""
    ids = ids.astype(np.int64)
    off = b.offsets if b.offsets is not None else np.arange(b.n + 1, dtype=np.uint64) * np.uint64(b.stride)
    lens = (off[ids + 1] - off[ids]).astype(np.int64)
    goff = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    src = np.repeat(off[ids].astype(np.int64) - goff[:-1].astype(np.int64), lens) + np.arange(int(goff[-1]), dtype=np.int64)
    return (b.data[src] if src.size else np.zeros(0, np.uint8)), goff


def _flush_batches():
    rng = np.random.default_rng(0xF1A5)
    stem = b"user0000-0000000"
    return [("dups6145", _dup_keys(rng, 6145)),
            ("prefix", [stem + bytes([int(x)]) for x in rng.integers(0, 256, 3000)]),
            # 16-byte rows that differ in their last 6 bytes only, 4^6 values: duplicates, prefix ties
            ("stride16", [b"0123456789" + bytes(r) for r in rng.integers(0, 4, (4500, 6), dtype=np.uint8) * 60]),
            ("one", [b"k"]),
            ("lengths", [b"v" * int(L) for L in rng.integers(0, 300, 2500)] + [b"w" * 4079, b""])]


@pytest.mark.parametrize("case", _flush_batches(), ids=lambda c: c[0])
@pytest.mark.parametrize("arrays", ["all", "none"])
def test_flush_files(vbf, ora, case, arrays):
    from velarixdb_amd import Table, get_many, memtable
    from velarixdb_amd.keys import pack
    keys = case[1]
    n = len(keys)
    rng = np.random.default_rng(n)
    val = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    cr = (T0 + rng.integers(0, 50, n)).astype(np.int64) if arrays == "all" else None  # many ties, none 0
    tb = (rng.integers(0, 5, n) == 0).astype(np.uint8) if arrays == "all" else None
    b = pack(keys)
    res = memtable.flush(b, val, cr, tb)
    ids = ref.sort_ids(keys)
    assert np.array_equal(res.ids, ids)
    i64 = ids.astype(np.int64)
    gkeys, goff = _gather(b, ids)
    want_d, want_i = ora.sst_write(gkeys, goff, val[i64], None if cr is None else cr[i64].view(np.uint64),
                                   None if tb is None else tb[i64])
    assert np.array_equal(res.data, want_d) and np.array_equal(res.index, want_i)
    assert (res.smallest, res.biggest) == (min(keys), max(keys))
    ent = vbf.sst.load_entries(res.data, res.index)
    assert ent.key_list() == sorted(set(keys)) and np.array_equal(ent.val_offsets, val[i64])
    if arrays == "all":
        assert np.array_equal(ent.created_ms, cr[i64].view(np.uint64)) and np.array_equal(ent.tombstones, tb[i64] != 0)
        with Table.open(res.data, res.index) as tab:  # open validates strict key order
            assert tab.entries == ids.size and tab.key_range() == (res.smallest, res.biggest)
            r = get_many(b, [tab])
        last = {k: j for j, k in enumerate(keys)}
        at = np.asarray([last[k] for k in keys])
        assert np.array_equal(r.found, np.where(tb[at] != 0, 2, 1))
        assert np.array_equal(r.val_offsets, val[at]) and np.array_equal(r.created_ms, cr[at].view(np.uint64))
    else:
        assert not ent.created_ms.any() and not ent.tombstones.any()


def _flush_raw(b, filt=None, data_cap=None, index_cap=None, query=False):
    """vbf_flush_write_host with poisoned outputs -> (rc, message, sizes, data, index, ids)"""
    from velarixdb_amd._lib import lib
    kb = int(b.offsets[-1] - b.offsets[0]) if b.offsets is not None else b.n * b.stride
    data, index = np.full(kb + 17 * b.n, 0xA5, np.uint8), np.full(kb + 8 * b.n, 0xA5, np.uint8)
    ids = np.full(b.n, 0xA5A5A5A5, np.uint32)
    dl, il, c = ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_uint64(7)
    d, o = b.ptrs()
    rc = lib.vbf_flush_write_host(d, o, b.stride, b.n, None, None, None, filt,
                                  None if query else data.ctypes.data, data.size if data_cap is None else data_cap,
                                  ctypes.byref(dl), None if query else index.ctypes.data,
                                  index.size if index_cap is None else index_cap, ctypes.byref(il),
                                  None if query else ids.ctypes.data, ctypes.byref(c), 0)
    return rc, lib.vbf_last_error(), (dl.value, il.value, c.value), data, index, ids


def test_flush_size_query_and_small_capacities(vbf, ora):
    from velarixdb_amd._lib import VBF_EINVAL, VBF_OK
    from velarixdb_amd.keys import pack
    keys = _dup_keys(np.random.default_rng(0xCA9), 3000)
    b = pack(keys)
    ids = ref.sort_ids(keys)
    want_d, want_i = ora.sst_write(*_gather(b, ids))
    sizes = (want_d.size, want_i.size, ids.size)
    rc, msg, got, *_ = _flush_raw(b, query=True)
    assert (rc, got) == (VBF_OK, sizes)
    rc, msg, got, data, index, out = _flush_raw(b)
    assert (rc, got) == (VBF_OK, sizes)
    assert np.array_equal(data[:sizes[0]], want_d) and np.array_equal(index[:sizes[1]], want_i)
    assert (data[sizes[0]:] == 0xA5).all() and (index[sizes[1]:] == 0xA5).all()  # nothing past the sizes
    assert np.array_equal(out[:ids.size], ids) and (out[ids.size:] == 0xA5A5A5A5).all()
    for caps in (dict(data_cap=sizes[0] - 1), dict(index_cap=sizes[1] - 1)):
        rc, msg, got, data, index, out = _flush_raw(b, **caps)
        assert rc == VBF_EINVAL and b"holds" in msg and got == sizes  # the sizes written, no output touched
        assert (data == 0xA5).all() and (index == 0xA5).all() and (out == 0xA5A5A5A5).all()


def test_flush_key_too_long_touches_nothing(vbf):
    """One 4080-byte key: the encoder's BlockIsFull, before any output or the filter is written."""
    from velarixdb_amd import BloomFilter
    from velarixdb_amd._lib import VBF_EINVAL
    from velarixdb_amd.keys import pack
    keys = [b"k%04d" % i for i in range(2500)]
    keys[1234] = b"L" * 4080
    f = BloomFilter.sized(9815, 19)
    rc, msg, got, data, index, out = _flush_raw(pack(keys), filt=f._h)
    assert rc == VBF_EINVAL and b"BlockIsFull" in msg
    assert (data == 0xA5).all() and (index == 0xA5).all() and (out == 0xA5A5A5A5).all()
    assert f.num_elements() == 0 and not f.words().any()


@pytest.mark.parametrize("case", insert_cases(), ids=lambda c: c[0])
def test_filter_insert_on_the_device(vbf, ora, case):
    """The filter step through its three routes onto a device-resident filter -- the flush, insert_many
    (vbf_filter_insert_host) and vbf_filter_insert_dev -- against the model and the oracle's words."""
    import torch
    from velarixdb_amd import BloomFilter, memtable
    from velarixdb_amd._lib import call
    from velarixdb_amd.keys import pack
    _, m, k, prior, keys = case
    b = pack(keys)
    fs = [BloomFilter.sized(m, k, 1e-4) for _ in range(3)]
    for f in fs:
        if prior:
            f.set_many(prior)
    n0 = len(prior)
    model, want = ref.insert_model(ora, b, m, k, fs[0].words())
    words = ora.build_words(pack(prior + keys), m, k)
    assert np.array_equal(model.words(), words)
    memtable.flush(b, np.zeros(b.n, np.uint32), filter=fs[0])
    assert fs[1].insert_many(b) == want
    dev = torch.device("cuda:0")
    d = torch.from_numpy(b.data).to(dev)
    o = None if b.offsets is None else torch.from_numpy(b.offsets.view(np.int64)).to(dev)
    c = ctypes.c_uint64(7)
    call("vbf_filter_insert_dev", fs[2]._h, d.data_ptr(), None if o is None else o.data_ptr(), b.stride, b.n, 1,
         ctypes.byref(c), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert c.value == want and (k == 0) == (want == 0)
    for f in fs:
        assert np.array_equal(f.words(), words)
        assert f.num_elements() == n0 + want
        assert f.contains_many(b).all()
    assert fs[1].insert_many(b) == 0 and fs[1].num_elements() == n0 + want  # every key contained now


def test_put_many_round_trip(vbf):
    """DataStore::put for a batch, then a get of every key: the last put's value, None after a
    delete."""
    from velarixdb_amd import Table, ValueLog, get_values, memtable
    from velarixdb_amd.vlog import SKIPPED, VALUE
    rng = np.random.default_rng(0x9A7)
    keys = _dup_keys(rng, 5000)
    values = [rng.bytes(int(L)) for L in rng.integers(0, 200, len(keys))]
    cr = (T0 + np.arange(len(keys))).astype(np.int64)
    tb = (rng.integers(0, 6, len(keys)) == 0).astype(np.uint8)
    base = 12_345
    log, res = memtable.put_many(keys, values, cr, tb, base=base)
    last = {k: j for j, k in enumerate(keys)}
    assert np.array_equal(res.ids, ref.sort_ids(keys))
    with ValueLog.open(log, base=base) as vl, Table.open(res.data, res.index) as tab:
        r, v = get_values(keys, [tab], vl, check_keys=True)
    for j, k in enumerate(keys):
        w = last[k]
        if tb[w]:
            assert r.found[j] == 2 and v.status[j] == SKIPPED and v.value(j) is None
        else:
            assert r.found[j] == 1 and v.status[j] == VALUE and v.value(j) == values[w]


def test_flush_to_dir(vbf, tmp_path):
    from velarixdb_amd import memtable
    keys = [b"b", b"a", b"b", b"c"]
    res = memtable.flush_to_dir(tmp_path / "sst", keys, [1, 2, 3, 4], [T0] * 4)
    assert res.ids.tolist() == [1, 2, 3]
    ent = vbf.sst.load_entries_from_dir(tmp_path / "sst")
    assert ent.key_list() == [b"a", b"b", b"c"] and ent.val_offsets.tolist() == [2, 3, 4]
    with pytest.raises(AssertionError, match="Cannot flush an empty table"):
        memtable.flush([], [])
