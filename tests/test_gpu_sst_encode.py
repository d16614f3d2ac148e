"""GPU parity for the SST data.db / index.db encoder.

Oracle: oracle.sst_write (Table::write_to_file, table.rs:287-340), pinned byte for byte by the
reference's fixture files in tests/test_sst.py.  Every comparison here is byte-exact: data.db,
index.db and the block start offsets.  The device API runs on torch buffers with guard bytes
around every output."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
SST = os.path.join(GOLDEN, "sst_fixtures")
NAMES = sorted(os.listdir(SST))
GUARD = 0xA5
FIB = [1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987]  # the set of test_gpu_sst.py


def _up(a, shift=0):
    """numpy array -> (device byte tensor, pointer `shift` bytes into it); None -> (None, None)."""
    import torch
    if a is None:
        return None, None
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.zeros(raw.size + shift + 16, dtype=torch.uint8, device="cuda:0")
    if raw.size:
        t[shift:shift + raw.size] = torch.from_numpy(raw.copy()).to("cuda:0")
    return t, ctypes.c_void_p(t.data_ptr() + shift)


def _out(nbytes, shift=0):
    import torch
    t = torch.full((shift + nbytes + 16,), GUARD, dtype=torch.uint8, device="cuda:0")
    return t, ctypes.c_void_p(t.data_ptr() + shift)


def _down(t, nbytes, shift=0):
    """The output bytes; asserts the guard bytes before and after them are untouched."""
    h = t.cpu().numpy()
    assert (h[:shift] == GUARD).all() and (h[shift + nbytes:] == GUARD).all(), "wrote outside the output"
    return h[shift:shift + nbytes].copy()


def encode_dev(keys, offs, stride, n, val=None, cr=None, tb=None, key_shift=0, out_shift=0, key_base=0):
    """vbf_sst_encode_dev: the all-NULL size query, then the three outputs at exactly those sizes.
    key_base: offsets are absolute positions in a buffer whose first key_base bytes precede `keys`."""
    import torch
    from velarixdb_amd._lib import call
    keep = []

    def up(a, shift=0):
        t, p = _up(a, shift)
        keep.append(t)
        return p

    pk = up(keys, key_shift) if keys is not None else None
    if pk is not None and key_base:
        pk = ctypes.c_void_p(pk.value - key_base)  # only positions >= offsets[0] are read
    po = up(offs)
    pv, pc, pt = up(val), up(cr), up(tb)
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dl, il, nb = ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_uint64(7)
    sizes = (ctypes.byref(dl), ctypes.byref(il), ctypes.byref(nb))
    call("vbf_sst_encode_dev", pk, po, stride, n, pv, pc, pt, None, 0, sizes[0], None, 0, sizes[1], None, 0,
         sizes[2], sp)
    want = (dl.value, il.value, nb.value)
    td, pd = _out(want[0], out_shift)
    ti, pi = _out(want[1], out_shift)
    tb_, pb = _out(4 * want[2])
    call("vbf_sst_encode_dev", pk, po, stride, n, pv, pc, pt, pd, want[0], sizes[0], pi, want[1], sizes[1], pb,
         want[2], sizes[2], sp)
    torch.cuda.synchronize()
    assert (dl.value, il.value, nb.value) == want
    return _down(td, want[0], out_shift), _down(ti, want[1], out_shift), _down(tb_, 4 * want[2]).view(np.uint32)


def encode_host(keys, offs, stride, n, val=None, cr=None, tb=None):
    from velarixdb_amd._lib import call
    P = lambda a: a.ctypes.data if a is not None and a.size else None
    dl, il, nb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    sizes = (ctypes.byref(dl), ctypes.byref(il), ctypes.byref(nb))
    call("vbf_sst_encode_host", P(keys), P(offs), stride, n, P(val), P(cr), P(tb), None, 0, sizes[0], None, 0,
         sizes[1], None, 0, sizes[2], 0)
    data = np.full(dl.value + 8, GUARD, np.uint8)
    index = np.full(il.value + 8, GUARD, np.uint8)
    blocks = np.zeros(nb.value + 1, np.uint32)
    call("vbf_sst_encode_host", P(keys), P(offs), stride, n, P(val), P(cr), P(tb), data.ctypes.data, dl.value,
         sizes[0], index.ctypes.data, il.value, sizes[1], blocks.ctypes.data, nb.value, sizes[2], 0)
    assert (data[dl.value:] == GUARD).all() and (index[il.value:] == GUARD).all()
    return data[:dl.value], index[:il.value], blocks[:nb.value]


def _u64(cr):
    return None if cr is None else cr.view(np.uint64)


def _same(ora, got, keys, offs, val=None, cr=None, tb=None):
    want_d, want_i = ora.sst_write(keys, offs, val, _u64(cr), tb)
    data, index, blocks = got
    assert data.size == want_d.size and index.size == want_i.size
    assert np.array_equal(data, want_d)
    assert np.array_equal(index, want_i)
    assert np.array_equal(blocks, ora.sst_index_blocks(want_i))


def _table(seed, lens):
    """A random table with the given key lengths: keys, offsets, val, created (i64), tombstones."""
    rng = np.random.default_rng(seed)
    L = np.asarray(lens, np.uint64)
    n = L.size
    offs = np.concatenate([[0], np.cumsum(L)]).astype(np.uint64)
    keys = rng.integers(0, 256, size=int(offs[-1]), dtype=np.uint8)
    val = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    cr = rng.integers(-2**63, 2**63 - 1, size=n, dtype=np.int64)
    tb = rng.integers(0, 2, size=n, dtype=np.uint8)
    return keys, offs, val, cr, tb


def _rand_lens(seed, n, lengths):
    return np.random.default_rng(seed).choice(lengths, size=n)


@pytest.mark.parametrize("name", NAMES)
def test_reference_fixtures(vbf, ora, name):
    """The reference's own SSTs: decode (oracle), encode (GPU) -> the files on disk."""
    with open(os.path.join(SST, name, "data.db"), "rb") as f:
        data = np.frombuffer(f.read(), np.uint8)
    with open(os.path.join(SST, name, "index.db"), "rb") as f:
        index = np.frombuffer(f.read(), np.uint8)
    keys, offs, val, cr, tb = ora.sst_decode(data)
    n = offs.size - 1
    for got in (encode_dev(keys, offs, 0, n, val, cr.view(np.int64), tb),
                encode_host(keys, offs, 0, n, val, cr.view(np.int64), tb)):
        assert np.array_equal(got[0], data)
        assert np.array_equal(got[1], index)
        assert np.array_equal(got[2], ora.sst_index_blocks(index))


@pytest.mark.parametrize("L", [16, 0])
def test_walks_that_never_converge(vbf, ora, L):
    """Equal entries: block walks from different entries never meet (124 entries per block at
    L = 16, 240 at L = 0, the deepest entry into a tile), so the cut must be carried exactly
    through 293 tiles.  The stride path gives the same bytes."""
    n = 300_001
    keys, offs, val, cr, tb = _table(20 + L, np.full(n, L))
    got = encode_dev(keys, offs, 0, n, val, cr, tb)
    _same(ora, got, keys, offs, val, cr, tb)
    fixed = encode_dev(keys if L else None, None, L, n, val, cr, tb)
    for a, b in zip(got, fixed):
        assert np.array_equal(a, b)


MIXED = {
    "0..40": lambda: _rand_lens(3, 5000, list(range(0, 41))),
    "0..299": lambda: _rand_lens(4, 3000, list(range(0, 300))),
    "block-sized": lambda: _rand_lens(5, 200, [4079, 4078, 4000, 1, 0]),
    "16x60+17": lambda: _rand_lens(9, 20000, [16] * 60 + [17]),
    "16x200+0": lambda: _rand_lens(10, 20000, [16] * 200 + [0]),
    "fibonacci": lambda: _rand_lens(8, 4000, FIB),
    "alternating 4079/0": lambda: np.tile([4079, 0], 550),   # every entry its own block
    "all 2031": lambda: np.full(1500, 2031),                 # two 2048-byte entries fill a block exactly
    "all 2032": lambda: np.full(1500, 2032),                 # one per block
}


@pytest.mark.parametrize("via", ["dev", "host"])
@pytest.mark.parametrize("case", list(MIXED))
def test_mixed_lengths(vbf, ora, case, via):
    keys, offs, val, cr, tb = _table(100 + list(MIXED).index(case), MIXED[case]())
    n = offs.size - 1
    enc = encode_dev if via == "dev" else encode_host
    _same(ora, enc(keys, offs, 0, n, val, cr, tb), keys, offs, val, cr, tb)


@pytest.mark.parametrize("L", [16, 0])
@pytest.mark.parametrize("n", [1, 2, 123, 124, 125, 240, 241, 4095, 4096, 4097, 65535, 65536, 65537])
def test_boundaries(vbf, ora, n, L):
    keys, offs, val, cr, tb = _table(n + L, np.full(n, L))
    _same(ora, encode_dev(keys, offs, 0, n, val, cr, tb), keys, offs, val, cr, tb)
    _same(ora, encode_dev(keys if L else None, None, L, n, val, cr, tb), keys, offs, val, cr, tb)


@pytest.mark.parametrize("drop", ["val", "created", "tomb", "all"])
def test_optional_arrays(vbf, ora, drop):
    """A NULL per-entry array writes zeros; through the offsets and the stride path."""
    keys, offs, val, cr, tb = _table(31, _rand_lens(31, 3000, list(range(0, 50))))
    n = offs.size - 1
    val = None if drop in ("val", "all") else val
    cr = None if drop in ("created", "all") else cr
    tb = None if drop in ("tomb", "all") else tb
    _same(ora, encode_dev(keys, offs, 0, n, val, cr, tb), keys, offs, val, cr, tb)
    _same(ora, encode_host(keys, offs, 0, n, val, cr, tb), keys, offs, val, cr, tb)
    k2, o2 = _table(32, np.full(n, 7))[:2]
    _same(ora, encode_dev(k2, None, 7, n, val, cr, tb), k2, o2, val, cr, tb)


def test_tombstone_bytes_and_created_range(vbf, ora):
    """A tombstone byte != 0 is written as 1; created_at is the i64's bits."""
    n = 2000
    keys, offs, val, cr, tb = _table(33, _rand_lens(33, n, list(range(0, 30))))
    tb = np.tile(np.array([0, 1, 2, 255], np.uint8), n // 4)
    cr = np.tile(np.array([-1, np.iinfo(np.int64).max, np.iinfo(np.int64).min, 0, -1720785462000], np.int64), n // 5)
    got = encode_dev(keys, offs, 0, n, val, cr, tb)
    _same(ora, got, keys, offs, val, cr, tb)
    ends = offs[1:].astype(np.int64) + 17 * np.arange(1, n + 1) - 1  # each entry's last byte
    assert got[0][ends].tolist() == [0, 1, 1, 1] * (n // 4)
    _same(ora, encode_host(keys, offs, 0, n, val, cr, tb), keys, offs, val, cr, tb)


@pytest.mark.parametrize("first", [5, 4093])
def test_offsets_not_starting_at_zero(vbf, ora, first):
    keys, offs, val, cr, tb = _table(40 + first, _rand_lens(41, 3000, list(range(0, 70))))
    n = offs.size - 1
    rng = np.random.default_rng(first)
    shifted = np.concatenate([rng.integers(0, 256, size=first, dtype=np.uint8), keys])
    want = ora.sst_write(keys, offs, val, _u64(cr), tb)
    got = encode_dev(keys, offs + np.uint64(first), 0, n, val, cr, tb, key_base=first)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    got = encode_host(shifted, offs + np.uint64(first), 0, n, val, cr, tb)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], ora.sst_index_blocks(want[1]))


@pytest.mark.parametrize("key_shift,out_shift", [(1, 0), (3, 1), (7, 3), (0, 1), (0, 3)])
def test_unaligned_addresses(vbf, ora, key_shift, out_shift):
    keys, offs, val, cr, tb = _table(50 + key_shift, _rand_lens(51, 3000, list(range(0, 70))))
    n = offs.size - 1
    _same(ora, encode_dev(keys, offs, 0, n, val, cr, tb, key_shift=key_shift, out_shift=out_shift),
          keys, offs, val, cr, tb)
    k2, o2 = _table(52, np.full(n, 13))[:2]
    _same(ora, encode_dev(k2, None, 13, n, val, cr, tb, key_shift=key_shift, out_shift=out_shift),
          k2, o2, val, cr, tb)


def test_sizes_and_errors(vbf, ora):
    import torch
    from velarixdb_amd._lib import VBF_EINVAL, VBF_OK, lib
    keys, offs, val, cr, tb = _table(60, _rand_lens(60, 3000, list(range(0, 70))))
    n = offs.size - 1
    want_d, want_i = ora.sst_write(keys, offs, val, _u64(cr), tb)
    want_nb = ora.sst_index_blocks(want_i).size
    tk, pk = _up(keys)
    to, po = _up(offs)
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dl, il, nb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    S = (ctypes.byref(dl), ctypes.byref(il), ctypes.byref(nb))
    enc = lib.vbf_sst_encode_dev
    # the all-NULL size query
    assert enc(pk, po, 0, n, None, None, None, None, 0, S[0], None, 0, S[1], None, 0, S[2], sp) == VBF_OK
    assert (dl.value, il.value, nb.value) == (want_d.size, want_i.size, want_nb)
    # each capacity one short: VBF_EINVAL, the sizes still reported, nothing written
    for short in range(3):
        caps = [want_d.size, want_i.size, want_nb]
        caps[short] -= 1
        td, pd = _out(want_d.size)
        ti, pi = _out(want_i.size)
        tb_, pb = _out(4 * want_nb)
        dl.value = il.value = nb.value = 0
        rc = enc(pk, po, 0, n, None, None, None, pd, caps[0], S[0], pi, caps[1], S[1], pb, caps[2], S[2], sp)
        assert rc == VBF_EINVAL and b"holds" in lib.vbf_last_error()
        assert (dl.value, il.value, nb.value) == (want_d.size, want_i.size, want_nb)
        torch.cuda.synchronize()
        for t in (td, ti, tb_):
            assert bool((t == GUARD).all())
    # one key of 4080 bytes among short ones (the reference: BlockIsFull)
    lens = np.full(2500, 9)
    lens[1700] = 4080
    k2, o2 = _table(61, lens)[:2]
    t2, p2 = _up(k2)
    t3, p3 = _up(o2)
    assert enc(p2, p3, 0, 2500, None, None, None, None, 0, S[0], None, 0, S[1], None, 0, S[2], sp) == VBF_EINVAL
    assert b"BlockIsFull" in lib.vbf_last_error() and b"1700" in lib.vbf_last_error()
    lens[1700] = 4079
    k2, o2 = _table(61, lens)[:2]
    _same(ora, encode_dev(k2, o2, 0, 2500), k2, o2)
    # descending offsets
    bad = offs.copy()
    bad[2000] = bad[1999] - np.uint64(1)
    t4, p4 = _up(bad)
    assert enc(pk, p4, 0, n, None, None, None, None, 0, S[0], None, 0, S[1], None, 0, S[2], sp) == VBF_EINVAL
    assert b"descend" in lib.vbf_last_error()
    # n = 0
    dl.value = il.value = nb.value = 9
    assert enc(None, None, 0, 0, None, None, None, None, 0, S[0], None, 0, S[1], None, 0, S[2], sp) == VBF_OK
    assert (dl.value, il.value, nb.value) == (0, 0, 0)


def test_device_round_trip(vbf, ora):
    """encode_dev -> vbf_sst_decode_dev fed the `blocks` output directly returns the inputs."""
    import torch
    from velarixdb_amd._lib import call
    keys, offs, val, cr, tb = _table(70, _rand_lens(70, 5000, list(range(0, 300))))
    n = offs.size - 1
    tk, pk = _up(keys)
    to, po = _up(offs)
    tv, pv = _up(val)
    tc, pc = _up(cr)
    tt, pt = _up(tb)
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dl, il, nb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    S = (ctypes.byref(dl), ctypes.byref(il), ctypes.byref(nb))
    call("vbf_sst_encode_dev", pk, po, 0, n, pv, pc, pt, None, 0, S[0], None, 0, S[1], None, 0, S[2], sp)
    td, pd = _out(dl.value)
    tb_, pb = _out(4 * nb.value)
    call("vbf_sst_encode_dev", pk, po, 0, n, pv, pc, pt, pd, dl.value, S[0], None, 0, S[1], pb, nb.value, S[2], sp)
    ok_, pok = _out(keys.size)
    oo, poo = _out(8 * (n + 1))
    ov, pov = _out(4 * n)
    oc, poc = _out(8 * n)
    ot, pot = _out(n)
    got = ctypes.c_uint64()
    call("vbf_sst_decode_dev", pd, dl.value, pb, nb.value, pok, keys.size, poo, pov, poc, pot, n + 1,
         ctypes.byref(got), sp)
    torch.cuda.synchronize()
    assert got.value == n
    assert np.array_equal(_down(ok_, keys.size), keys)
    assert np.array_equal(_down(oo, 8 * (n + 1)).view(np.uint64), offs)
    assert np.array_equal(_down(ov, 4 * n).view(np.uint32), val)
    assert np.array_equal(_down(oc, 8 * n).view(np.int64), cr)
    assert np.array_equal(_down(ot, n), tb)


def test_python_write_sst_files(vbf, tmp_path):
    """write_sst_files is the inverse of load_entries_from_dir, and reproduces the fixture's files."""
    src = os.path.join(SST, NAMES[0])
    ent = vbf.sst.load_entries_from_dir(src)
    vbf.sst.write_sst_files(tmp_path / "sst", ent)
    for f in ("data.db", "index.db"):
        with open(os.path.join(src, f), "rb") as a, open(tmp_path / "sst" / f, "rb") as b:
            assert a.read() == b.read(), f
    back = vbf.sst.load_entries_from_dir(tmp_path / "sst")
    assert np.array_equal(back.keys, ent.keys) and np.array_equal(back.offsets, ent.offsets)
    assert np.array_equal(back.val_offsets, ent.val_offsets) and np.array_equal(back.created_ms, ent.created_ms)
    assert np.array_equal(back.tombstones, ent.tombstones)
