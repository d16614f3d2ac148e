"""The memtable flush's checks that return before any device work, and vbf_filter_insert_host on a
host-resident filter, which runs the literal loop on the CPU (no GPU needed).

The flush's size query and its too-small capacities need the number of distinct keys, which only
the sort knows: those two conventions are checked on the GPU (tests/test_gpu_memtable.py)."""
import ctypes

import numpy as np
import pytest

import memtable_ref as ref

POISON = 7


def _keys(n=3):
    return np.arange(97, 97 + n, dtype=np.uint8), np.arange(n + 1, dtype=np.uint64)


def _p(a):
    return None if a is None else a if isinstance(a, int) else a.ctypes.data


def _sort(which, keys, offsets, stride, n, out=True, n_out=True):
    from velarixdb_amd._lib import lib
    ids = np.zeros(max(min(n, 16), 1), np.uint32)
    c = ctypes.c_uint64(POISON)
    fn = lib.vbf_memtable_sort_dev if which == "dev" else lib.vbf_memtable_sort_host
    rc = fn(_p(keys), _p(offsets), stride, n, ids.ctypes.data if out else None, ctypes.byref(c) if n_out else None,
            None if which == "dev" else 0)
    return rc, lib.vbf_last_error(), c.value


def _flush(keys, offsets, stride, n, filt=None, sizes=True, n_out=True):
    from velarixdb_amd._lib import lib
    dl, il, c = ctypes.c_uint64(POISON), ctypes.c_uint64(POISON), ctypes.c_uint64(POISON)
    rc = lib.vbf_flush_write_host(_p(keys), _p(offsets), stride, n, None, None, None, filt, None, 0,
                                  ctypes.byref(dl) if sizes else None, None, 0, ctypes.byref(il),
                                  None, ctypes.byref(c) if n_out else None, 0)
    return rc, lib.vbf_last_error(), (dl.value, il.value, c.value)


BOTH = ("dev", "host")


@pytest.mark.parametrize("which", BOTH)
def test_sort_null_pointers(which):
    from velarixdb_amd._lib import VBF_EINVAL
    k, o = _keys()
    rc, msg, _ = _sort(which, k, o, 0, 3, n_out=False)
    assert rc == VBF_EINVAL and b"n_out is NULL" in msg
    rc, msg, c = _sort(which, k, o, 0, 3, out=False)
    assert rc == VBF_EINVAL and b"out_ids is NULL" in msg and c == 0
    rc, msg, c = _sort(which, None, None, 4, 3)
    assert rc == VBF_EINVAL and b"keys is NULL" in msg and c == 0


@pytest.mark.parametrize("which", BOTH)
def test_sort_of_nothing_is_ok(which):
    from velarixdb_amd._lib import VBF_OK
    rc, msg, c = _sort(which, None, None, 0, 0, out=False)
    assert (rc, msg, c) == (VBF_OK, b"", 0)


@pytest.mark.parametrize("which", BOTH)
def test_sort_entry_limit(which):
    """2^31 entries: refused before the pointers are looked at, as the merge refuses them."""
    from velarixdb_amd._lib import VBF_EINVAL
    rc, msg, c = _sort(which, None, None, 1, 1 << 31, out=False)
    assert rc == VBF_EINVAL and b"too many entries" in msg and c == 0


def test_sort_host_descending_offsets():
    from velarixdb_amd._lib import VBF_EINVAL
    k = np.zeros(8, np.uint8)
    rc, msg, c = _sort("host", k, np.asarray([0, 4, 2, 8], np.uint64), 0, 3)
    assert rc == VBF_EINVAL and b"offsets descend at entry 1" in msg and c == 0


def test_flush_checks():
    from velarixdb_amd import HOST, BloomFilter
    from velarixdb_amd._lib import VBF_EDIVZERO, VBF_EINVAL
    k, o = _keys()
    rc, msg, _ = _flush(k, o, 0, 3, sizes=False)
    assert rc == VBF_EINVAL and b"NULL" in msg
    rc, msg, _ = _flush(k, o, 0, 3, n_out=False)
    assert rc == VBF_EINVAL and b"NULL" in msg
    rc, msg, sizes = _flush(None, None, 0, 0)  # flusher.rs:40-44
    assert rc == VBF_EINVAL and b"Cannot flush an empty table" in msg and sizes == (0, 0, 0)
    rc, msg, sizes = _flush(None, None, 1, 1 << 31)
    assert rc == VBF_EINVAL and b"too many entries" in msg and sizes == (0, 0, 0)
    rc, msg, sizes = _flush(np.zeros(8, np.uint8), np.asarray([0, 4, 2, 8], np.uint64), 0, 3)
    assert rc == VBF_EINVAL and b"offsets descend at entry 1" in msg and sizes == (0, 0, 0)
    rc, msg, sizes = _flush(np.zeros(4080 * 2, np.uint8), None, 4080, 2)  # the encoder's BlockIsFull
    assert rc == VBF_EINVAL and b"BlockIsFull" in msg and sizes == (0, 0, 0)
    # a host-resident filter: the memtable's own stays with its caller
    f = BloomFilter.sized(64, 3, device=HOST)
    rc, msg, sizes = _flush(k, o, 0, 3, filt=f._h)
    assert rc == VBF_EINVAL and b"host-resident" in msg and sizes == (0, 0, 0)
    assert f.num_elements() == 0 and not f.words().any()
    zero, big = BloomFilter.sized(0, 3, device=HOST), BloomFilter.sized((1 << 30) + 1, 3, device=HOST)
    rc, msg, _ = _flush(k, o, 0, 3, filt=zero._h)
    assert rc == VBF_EDIVZERO
    rc, msg, _ = _flush(k, o, 0, 3, filt=big._h)
    assert rc == VBF_EINVAL and b"2^30" in msg


def _insert(which, f, keys, offsets, stride, n, lp=1, want_new=True):
    from velarixdb_amd._lib import lib
    c = ctypes.c_uint64(POISON)
    pc = ctypes.byref(c) if want_new else None
    if which == "dev":
        rc = lib.vbf_filter_insert_dev(f, _p(keys), _p(offsets), stride, n, lp, pc, None)
    else:
        rc = lib.vbf_filter_insert_host(f, _p(keys), _p(offsets), stride, n, lp, pc)
    return rc, lib.vbf_last_error(), c.value


@pytest.mark.parametrize("which", BOTH)
def test_insert_checks(which):
    from velarixdb_amd import HOST, BloomFilter
    from velarixdb_amd._lib import VBF_EDIVZERO, VBF_EINVAL
    k, o = _keys()
    rc, msg, c = _insert(which, None, k, o, 0, 3)
    assert rc == VBF_EINVAL and b"filter is NULL" in msg and c == 0
    f = BloomFilter.sized(64, 3, device=HOST)
    rc, msg, c = _insert(which, f._h, None, None, 4, 3)
    assert rc == VBF_EINVAL and b"keys is NULL" in msg and c == 0
    rc, msg, c = _insert(which, f._h, None, None, 1, (1 << 32) - 1)
    assert rc == VBF_EINVAL and b"too many keys" in msg and c == 0
    # the cap on m names itself, before any work and whatever the residency
    big = BloomFilter.sized((1 << 30) + 1, 3, device=HOST)
    rc, msg, c = _insert(which, big._h, k, o, 0, 3)
    assert rc == VBF_EINVAL and b"2^30" in msg and c == 0 and big.host_bytes == 0
    zero = BloomFilter.sized(0, 3, device=HOST)
    rc, msg, c = _insert(which, zero._h, k, o, 0, 3)
    assert rc == VBF_EDIVZERO and c == 0
    assert f.num_elements() == 0 and not f.words().any()


def test_insert_dev_needs_a_device_filter():
    from velarixdb_amd import HOST, BloomFilter
    from velarixdb_amd._lib import VBF_EINVAL
    k, o = _keys()
    f = BloomFilter.sized(64, 3, device=HOST)
    rc, msg, c = _insert("dev", f._h, k, o, 0, 3)
    assert rc == VBF_EINVAL and b"host-resident" in msg and c == 0


def test_insert_host_descending_offsets():
    from velarixdb_amd import HOST, BloomFilter
    from velarixdb_amd._lib import VBF_EINVAL
    f = BloomFilter.sized(64, 3, device=HOST)
    rc, msg, c = _insert("host", f._h, np.zeros(8, np.uint8), np.asarray([0, 4, 2, 8], np.uint64), 0, 3)
    assert rc == VBF_EINVAL and b"offsets descend" in msg and c == 0 and not f.words().any()


def insert_cases():
    """(name, m, k, prior keys set before the batch, the batch): the shapes the GPU test reuses."""
    rng = np.random.default_rng(0x1A5E27)
    small = [rng.bytes(int(n)) for n in rng.integers(0, 25, 200)]
    full = [b"key%06d" % i for i in range(3000)]
    dup = [small[i] for i in rng.integers(0, 40, 300)]
    return [("collisions", 64, 3, [], small),
            ("overfull", 9815, 19, [], full),            # the fixtures' shape: 3000 keys in a 512-entry filter
            ("prefilled", 9815, 19, full[:700], full[500:1500] + small),
            ("duplicates", 1021, 5, [], dup),
            ("k0", 64, 0, [], small)]


@pytest.mark.parametrize("case", insert_cases(), ids=lambda c: c[0])
def test_insert_host_matches_model(ora, case):
    from velarixdb_amd import HOST, BloomFilter
    from velarixdb_amd.keys import pack
    _, m, k, prior, keys = case
    f = BloomFilter.sized(m, k, 1e-4, device=HOST)
    if prior:
        f.set_many(prior)
    n0 = f.num_elements()
    model, want = ref.insert_model(ora, pack(keys), m, k, f.words())
    got = f.insert_many(keys)
    assert got == want and (k == 0) == (want == 0)
    assert np.array_equal(f.words(), model.words())
    assert np.array_equal(f.words(), ora.build_words(pack(prior + keys), m, k))  # == a set of every key
    assert f.num_elements() == n0 + want
    assert f.serialize() == np.asarray([k, n0 + want], "<u4").tobytes() + np.float64(1e-4).tobytes()
    assert f.insert_many(keys) == 0 and f.num_elements() == n0 + want  # all contained now
    assert f.insert_many([]) == 0


def test_insert_host_counter_wraps_and_null_count():
    from velarixdb_amd import HOST, BloomFilter
    f = BloomFilter.sized(9815, 19, device=HOST)
    f.set_num_elements(0xFFFFFFFF)
    k = np.frombuffer(b"abcdefgh", np.uint8)
    rc, msg, c = _insert("host", f._h, k, None, 4, 2, want_new=False)
    assert rc == 0 and c == POISON and f.num_elements() == 1  # u32, wrapping
