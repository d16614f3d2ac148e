"""GPU parity for the batched point lookups in SST tables.

Checker: tests/sst_get_ref.py (the reference's two scans and its fold restated over file bytes,
pinned on the reference's fixture SSTs by tests/test_sst_get_ref.py).  Every comparison is exact on
all four output arrays.  Tables are written with oracle.sst_write; the device API runs on torch
buffers with guard bytes around every output."""
import ctypes
import functools
import itertools
import os
import struct

import numpy as np
import pytest

import key_torture as kt
import sst_get_ref as ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
SST = os.path.join(GOLDEN, "sst_fixtures")
NAMES = sorted(os.listdir(SST))
GUARD, PAD = 0xA5, 16
T0 = 1720785462000


# ---- tables -------------------------------------------------------------------------------

def write(ora, items):
    """items: [(key, value offset, created_at ms, tombstone byte)] in file order -> (data, index)
    bytes as Table::write_to_file lays them out; a tombstone byte above 1 is patched in afterwards."""
    keys = np.frombuffer(b"".join(k for k, *_ in items) or b"\0", np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(k) for k, *_ in items])]).astype(np.uint64)
    data, index = ora.sst_write(keys, offs, np.array([v for _, v, _, _ in items], np.uint32),
                                np.array([c for _, _, c, _ in items], np.uint64),
                                np.array([t for *_, t in items], np.uint8))
    p = 0
    for k, _, _, t in items:
        if t > 1:
            data[p + 16 + len(k)] = t
        p += len(k) + 17
    return data.tobytes(), index.tobytes()


def simple(ora, keys, salt=0, created=None):
    """A table of `keys` (sorted here) with distinct fields derived from the position and `salt`."""
    keys = sorted(keys)
    return write(ora, [(k, (j * 2654435761 + salt) & 0xFFFFFFFF, created or T0 + salt * 100003 + j, j % 5 == 0)
                       for j, k in enumerate(keys)])


def read_fixture(name):
    with open(os.path.join(SST, name, "data.db"), "rb") as f:
        data = f.read()
    with open(os.path.join(SST, name, "index.db"), "rb") as f:
        index = f.read()
    return data, index


def keys_of(sst):
    return [k for k in sst.starts]


class Tables:
    """Handles opened with vbf_table_open_host for [(data, index), ...], freed on exit, next to
    the checker's parse of the same bytes."""

    def __init__(self, files):
        self.files = files
        self.ref = [ref.Sst(d, i) for d, i in files]
        self.h = []

    def __enter__(self):
        for d, i in self.files:
            self.h.append(open_host(d, i))
        return self

    def __exit__(self, *exc):
        from velarixdb_amd._lib import lib
        for h in self.h:
            lib.vbf_table_free(h)


def _np(b):
    return np.frombuffer(b, np.uint8)


def open_host(data, index, expect=0):
    from velarixdb_amd._lib import lib
    d, i = _np(data), _np(index)
    h = ctypes.c_void_p()
    rc = lib.vbf_table_open_host(d.ctypes.data if d.size else None, d.size, i.ctypes.data if i.size else None,
                                 i.size, 0, ctypes.byref(h))
    assert rc == expect, lib.vbf_last_error()
    assert bool(h.value) == (rc == 0)
    return h


def handles(hs):
    return (ctypes.c_void_p * max(len(hs), 1))(*[h.value for h in hs])


# ---- queries ------------------------------------------------------------------------------

def offsets_batch(queries, lead=0):
    """(bytes with `lead` filler bytes in front, u64 offsets starting at `lead`)"""
    offs = np.concatenate([[0], np.cumsum([len(q) for q in queries])]).astype(np.uint64) + np.uint64(lead)
    return np.frombuffer(b"\xEE" * lead + b"".join(queries) + b"\xEE", np.uint8), offs


def _up(a, shift=0):
    import torch
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.full((raw.size + shift + 16,), 0xEE, dtype=torch.uint8, device="cuda:0")
    if raw.size:
        t[shift:shift + raw.size] = torch.from_numpy(raw.copy()).to("cuda:0")
    return t, ctypes.c_void_p(t.data_ptr() + shift)


def _out(nbytes):
    import torch
    t = torch.full((PAD + nbytes + PAD,), GUARD, dtype=torch.uint8, device="cuda:0")
    return t, ctypes.c_void_p(t.data_ptr() + PAD)


def _down(t, nbytes, dtype):
    h = t.cpu().numpy()
    assert (h[:PAD] == GUARD).all() and (h[PAD + nbytes:] == GUARD).all(), "wrote outside the output"
    return h[PAD:PAD + nbytes].copy().view(dtype)


def get_dev(hs, keys, offs, stride, n, cand=None, shift=0, want=(1, 1, 1, 1)):
    """vbf_table_get_dev on uploaded keys (`shift` bytes into their buffer); outputs between guard
    bytes; want[i] == 0 passes NULL for output i (None comes back)."""
    import torch
    from velarixdb_amd._lib import call
    tk, pk = _up(keys, shift)
    if offs is not None:
        to, po = _up(offs)
    else:
        po = None
    if cand is not None:
        tc, pc = _up(np.ascontiguousarray(cand, np.uint8))
    else:
        pc = None
    sizes, dts = (n, 4 * n, 4 * n, 8 * n), (np.uint8, np.uint32, np.uint32, np.uint64)
    outs = [_out(s) if w else (None, None) for s, w in zip(sizes, want)]
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    call("vbf_table_get_dev", pk, po, stride, n, len(hs), handles(hs), pc, *[p for _, p in outs], sp)
    torch.cuda.synchronize()
    return tuple(None if t is None else _down(t, s, dt) for (t, _), s, dt in zip(outs, sizes, dts))


def get_dev_list(hs, queries, cand=None, lead=0, shift=0):
    keys, offs = offsets_batch(queries, lead)
    return get_dev(hs, keys, offs, 0, len(queries), cand, shift)


def get_host(hs, queries, filters=None):
    from velarixdb_amd._lib import call
    keys, offs = offsets_batch(queries)
    n = len(queries)
    out = (np.full(n, 9, np.uint8), np.full(n, 9, np.uint32), np.full(n, 9, np.uint32), np.full(n, 9, np.uint64))
    fh = handles([f._h for f in filters]) if filters is not None else None
    call("vbf_table_get_host", keys.ctypes.data, offs.ctypes.data, 0, n, len(hs), handles(hs), fh,
         *[o.ctypes.data for o in out])
    return out


def same(got, want):
    for g, w, what in zip(got, want, ("found", "table_idx", "val_offsets", "created_ms")):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, "%s differs at %d of %d queries, first %d: got %d want %d" % (
            what, bad.size, g.size, bad[0], g[bad[0]], w[bad[0]])


def variants(keys):
    """Every key, each with a 0x00 appended, each with its last byte dropped."""
    return list(keys) + [k + b"\0" for k in keys] + [k[:-1] for k in keys]


# ---- 1. the reference's fixtures ------------------------------------------------------------

def test_fixtures_dev_and_host_with_filters(vbf, ora):
    files = [read_fixture(n) for n in NAMES]
    with Tables(files) as T:
        queries = []
        for s in T.ref:
            queries += variants(keys_of(s))
        queries += [b"zz%05d" % i for i in range(5000)]
        want = ref.search_many(queries, T.ref)
        assert int((want[0] == 1).sum()) >= 19908
        got = get_dev_list(T.h, queries)
        same(got, want)
        filters = []
        for (d, i), s in zip(files, T.ref):
            f = vbf.BloomFilter(0.01, len(s.fields))
            assert f.rebuild_from_sst(d, i) == len(s.fields)
            filters.append(f)
        got_f = get_host(T.h, queries, filters)
        same(got_f, want)
        same(got_f, got)
        same(get_host(T.h, queries), want)


def test_python_module(vbf, ora):
    """Table / get_many / ranges_from_tables: the same answers through the package."""
    from velarixdb_amd import Table, get_many
    from velarixdb_amd.key_range import candidates, ranges_from_tables
    names = NAMES[:3]
    tabs = [Table.open_dir(os.path.join(SST, n)) for n in names]
    refs = [ref.Sst(*read_fixture(n)) for n in names]
    try:
        assert [t.entries for t in tabs] == [len(s.fields) for s in refs]
        assert [t.blocks for t in tabs] == [len(s.ikeys) for s in refs]
        for t, s in zip(tabs, refs):
            assert t.key_range() == (min(s.starts), s.ikeys[-1]) and t.device == 0
        queries = variants(keys_of(refs[0])[::7]) + keys_of(refs[2])[::5] + [b"zz%05d" % i for i in range(300)]
        want = ref.search_many(queries, refs)
        r = get_many(queries, tabs)
        same((r.found, r.table, r.val_offsets, r.created_ms), want)
        filters = []
        for n, s in zip(names, refs):
            f = vbf.BloomFilter(0.01, len(s.fields))
            f.rebuild_from_sst(*read_fixture(n))
            filters.append(f)
        r = get_many(queries, tabs, filters)
        same((r.found, r.table, r.val_offsets, r.created_ms), want)
        c = candidates(queries, ranges_from_tables(tabs, filters))
        assert c[np.arange(len(queries)), np.minimum(want[1], 2)][want[0] != 0].all()  # no false negatives
    finally:
        for t in tabs:
            t.close()


# ---- 2. adversarial ordering ----------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def universe_files(ora):
    """The ordering universe dealt into three overlapping tables (each key in two of them), with
    created_at values that tie between tables for some keys and not for others."""
    uni = kt.ordered_universe()
    files = []
    for t in range(3):
        items = [(k, (j * 31 + t) & 0xFFFFFFFF, T0 + (j * 7 + t * (j % 3)) % 5, (j + t) % 11 == 0)
                 for j, k in enumerate(uni) if j % 3 != t]
        files.append(write(ora, items))
    return uni, files


def test_adversarial_ordering(vbf, ora):
    uni, files = universe_files(ora)
    with Tables(files) as T:
        assert sum(len(s.ikeys) for s in T.ref) > 6  # several blocks per table
        queries = variants(uni)
        want = ref.search_many(queries, T.ref)
        assert (want[0] == 1).any() and (want[0] == 2).any() and (want[0] == 0).any()
        same(get_dev_list(T.h, queries), want)
        same(get_host(T.h, queries), want)


# ---- 3. block geometry ----------------------------------------------------------------------

def counters(n, length, prefix=b""):
    return [prefix + j.to_bytes(length - len(prefix), "big") for j in range(1, n + 1)]


def geometry_files(ora):
    return {
        "full": simple(ora, counters(128 * 3 + 5, 15, b"f"), 1),      # 128 entries x 32 bytes = 4096
        "short": simple(ora, counters(117 * 3 + 5, 18, b"s"), 2),     # 117 entries x 35 bytes = 4095
        "mixed": simple(ora, [b"m" + bytes([j >> 8, j & 255]) * (1 + j % 9) for j in range(700)], 3),
        "huge": simple(ora, [b"h" + bytes([j]) * 4078 for j in range(1, 6)], 4),  # 4079-byte keys
        "one": simple(ora, [b"one"], 5),
        "block": simple(ora, counters(10, 9, b"b"), 6),
        "empty_key": simple(ora, [b"", b"\0", b"\0\0", b"e1", b"e2"], 7),
    }


def edge_queries(s):
    """First and last key of every block, between blocks, below the smallest, above the biggest."""
    ks = sorted(s.starts)
    q = [ks[0][:-1], ks[0], ks[-1], ks[-1] + b"\0", ks[-1][:-1] + b"\xff\xff", b"\xff" * 9]
    pos = {k: p[0] for k, p in s.starts.items()}
    for b, off in enumerate(s.ioffs):
        first = next(k for k in ks if pos[k] == off)
        last = s.ikeys[b]
        q += [first, last, last + b"\0", last + b"\0\0\0\0\0\0\0\0\0", first[:-1]]
    return q


def test_block_geometry(vbf, ora):
    files = geometry_files(ora)
    with Tables(list(files.values())) as T:
        by = dict(zip(files, zip(T.h, T.ref)))
        sizes = lambda s: np.diff(s.ioffs + [len(s.data)]).tolist()
        assert set(sizes(by["full"][1])[:-1]) == {4096} and set(sizes(by["short"][1])[:-1]) == {4095}
        assert sizes(by["huge"][1]) == [4096] * 5 and sizes(by["one"][1]) == [20] and len(by["block"][1].ioffs) == 1
        everything = []
        for name, (h, s) in by.items():
            queries = variants(keys_of(s)) + edge_queries(s)
            everything += queries
            same(get_dev_list([h], queries), ref.search_many(queries, [s]))
        # a 4080-byte query that agrees with a 4079-byte key on all its bytes, and a 64 KiB one
        everything += [b"h" + bytes([2]) * 4079, b"h" + bytes([2]) * 65535, b"f" * 4080]
        want = ref.search_many(everything, T.ref)
        assert not want[0][-3:].any()
        same(get_dev_list(T.h, everything), want)
        same(get_host(T.h, everything), want)


# ---- 4. the fold ----------------------------------------------------------------------------

def fold_files(ora):
    per = [{}, {}, {}]

    def put(key, *cells):  # cells: per table (created, tombstone byte) or None
        for t, c in enumerate(cells):
            if c is not None:
                per[t][key] = c

    put(b"tie", (T0, 0), (T0, 0), (T0, 0))
    put(b"tie-late", None, (T0 + 3, 0), (T0 + 3, 1))
    put(b"newer", (T0 + 5, 0), (T0 + 6, 0), (T0 + 9, 0))
    put(b"tomb", (T0 + 5, 0), (T0 + 9, 1), (T0 + 3, 0))
    put(b"tomb2", (T0 + 5, 0), (T0 + 9, 2), (T0 + 3, 0))
    put(b"tomb255", (T0 + 5, 1), (T0 + 9, 255), None)
    put(b"zero-only", None, (0, 0), None)
    put(b"zero-plus", (0, 0), None, (4, 0))
    put(b"zero-all", (0, 1), (0, 0), (0, 0))
    put(b"big-time", (2**63, 0), (2**64 - 1, 0), (2**63 + 1, 1))
    for j in range(40):
        put(b"fill%02d" % j, (T0 + j, 0), (T0 + 40 - j, j % 2), (T0 + 20, 0) if j % 3 else None)
    return [write(ora, [(k, 1000 * t + j, c, tb) for j, (k, (c, tb)) in enumerate(sorted(d.items()))])
            for t, d in enumerate(per)]


def test_the_fold(vbf, ora):
    files = fold_files(ora)
    with Tables(files) as T:
        queries = variants(keys_of(T.ref[0]) + keys_of(T.ref[1]))
        at = {q: j for j, q in enumerate(queries)}
        for perm in itertools.permutations(range(3)):
            hs, rs = [T.h[p] for p in perm], [T.ref[p] for p in perm]
            want = ref.search_many(queries, rs)
            got = get_dev_list(hs, queries)
            same(got, want)
            found, idx, val, cr = got
            first = lambda *tables: min(perm.index(t) for t in tables)
            assert (found[at[b"tie"]], idx[at[b"tie"]]) == (1, 0)  # the first listed, whichever it is
            assert val[at[b"tie"]] // 1000 == perm[0]
            assert idx[at[b"tie-late"]] == first(1, 2) and found[at[b"tie-late"]] == (1 if perm.index(1) < perm.index(2) else 2)
            assert (found[at[b"newer"]], idx[at[b"newer"]], cr[at[b"newer"]]) == (1, perm.index(2), T0 + 9)
            assert (found[at[b"tomb"]], idx[at[b"tomb"]]) == (2, perm.index(1))
            assert (found[at[b"tomb2"]], idx[at[b"tomb2"]]) == (1, perm.index(1))  # byte 2 is live
            assert found[at[b"tomb255"]] == 1
            assert (found[at[b"zero-only"]], idx[at[b"zero-only"]], val[at[b"zero-only"]]) == (0, ref.NO_TABLE, 0)
            assert (found[at[b"zero-plus"]], idx[at[b"zero-plus"]], cr[at[b"zero-plus"]]) == (1, perm.index(2), 4)
            assert found[at[b"zero-all"]] == 0
            assert (found[at[b"big-time"]], cr[at[b"big-time"]]) == (1, 2**64 - 1)  # compared as u64


# ---- 5. query layouts -----------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def stride_files(ora):
    """Three tables of random keys of the test's four strides (some in two tables) and a few others."""
    rng = np.random.default_rng(0x7AB1E)
    keys = {L: sorted({rng.integers(0, 256, L, dtype=np.uint8).tobytes() for _ in range(150 if L > 1 else 90)})
            for L in (1, 5, 16, 33)}
    allk = [k for L in keys for k in keys[L]] + [b"", b"odd", b"x" * 40]
    files = [simple(ora, [k for j, k in enumerate(allk) if (j + t) % 3], 10 + t) for t in range(3)]
    return keys, files


@pytest.mark.parametrize("shift", [1, 3, 7])
def test_offsets_with_a_lead_and_a_misaligned_base(vbf, ora, shift):
    uni, files = universe_files(ora)
    with Tables(files) as T:
        queries = variants(uni[shift::5])
        want = ref.search_many(queries, T.ref)
        same(get_dev_list(T.h, queries, lead=29 + shift, shift=shift), want)


@pytest.mark.parametrize("stride", [1, 5, 16, 33])
def test_fixed_strides(vbf, ora, stride):
    keys, files = stride_files(ora)
    rng = np.random.default_rng(stride)
    with Tables(files) as T:
        rows = keys[stride] + [rng.integers(0, 256, stride, dtype=np.uint8).tobytes() for _ in range(300)]
        if stride > 1:
            rows += [k[:-1] + bytes([k[-1] ^ 1]) for k in keys[stride]]
        want = ref.search_many(rows, T.ref)
        assert (want[0] != 0).sum() >= len(keys[stride]) * 0.6 and (want[0] == 0).any()
        buf = np.frombuffer(b"".join(rows), np.uint8)
        for shift in (0, 1):
            same(get_dev(T.h, buf, None, stride, len(rows), shift=shift), want)
        out = [np.zeros(len(rows), d) for d in (np.uint8, np.uint32, np.uint32, np.uint64)]
        from velarixdb_amd._lib import call
        call("vbf_table_get_host", buf.ctypes.data, None, stride, len(rows), 3, handles(T.h), None,
             *[o.ctypes.data for o in out])
        same(out, want)


@pytest.mark.parametrize("stride", [4080, 65536])
def test_queries_longer_than_any_key(vbf, ora, stride):
    files = [simple(ora, [b"h" + bytes([j]) * 4078 for j in range(1, 4)], 1), simple(ora, [b"a", b"h", b"zz"], 2)]
    with Tables(files) as T:
        rows = [(b"h" + bytes([j]) * stride)[:stride] for j in (0, 1, 2, 3, 4)] + [b"\0" * stride, b"\xff" * stride]
        got = get_dev(T.h, np.frombuffer(b"".join(rows), np.uint8), None, stride, len(rows))
        same(got, ref.search_many(rows, T.ref))
        assert not got[0].any() and (got[1] == ref.NO_TABLE).all()


def test_cand_matrix_with_random_zeros(vbf, ora):
    uni, files = universe_files(ora)
    with Tables(files) as T:
        queries = variants(uni[::3])
        cand = np.random.default_rng(5).integers(0, 3, (len(queries), 3), dtype=np.uint8)  # a third zeros
        cand[cand == 2] = 0xFF
        want = ref.search_many(queries, T.ref, cand != 0)
        full = ref.search_many(queries, T.ref)
        assert (want[1] != full[1]).any()
        same(get_dev_list(T.h, queries, cand=cand), want)
        same(get_dev_list(T.h, queries, cand=np.zeros_like(cand)), ref.search_many(queries, []))
        same(get_dev_list(T.h, queries, cand=np.ones_like(cand)), full)


# ---- 6. open_dev on the encoder's outputs ---------------------------------------------------

def test_open_dev_on_the_encoders_outputs(vbf, ora):
    import torch
    from velarixdb_amd._lib import call, lib
    uni = kt.ordered_universe()
    n = len(uni)
    keys, offs = offsets_batch(uni)
    val = (np.arange(n, dtype=np.uint32) * 2654435761).astype(np.uint32)
    cr = (T0 + np.arange(n)).astype(np.int64)
    tb = (np.arange(n) % 7 == 0).astype(np.uint8)
    keep = [_up(a) for a in (keys, offs, val, cr, tb)]
    ins = [p for _, p in keep]
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dl, il, nb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    S = (ctypes.byref(dl), ctypes.byref(il), ctypes.byref(nb))
    call("vbf_sst_encode_dev", ins[0], ins[1], 0, n, ins[2], ins[3], ins[4], None, 0, S[0], None, 0, S[1], None, 0,
         S[2], sp)
    td = torch.zeros(dl.value, dtype=torch.uint8, device="cuda:0")
    ti = torch.zeros(il.value, dtype=torch.uint8, device="cuda:0")
    tblk = torch.zeros(nb.value, dtype=torch.int32, device="cuda:0")
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    call("vbf_sst_encode_dev", ins[0], ins[1], 0, n, ins[2], ins[3], ins[4], P(td), dl.value, S[0], P(ti), il.value,
         S[1], P(tblk), nb.value, S[2], sp)
    h = ctypes.c_void_p()
    call("vbf_table_open_dev", P(td), dl.value, P(ti), il.value, P(tblk), nb.value, sp, ctypes.byref(h))
    data, index = td.cpu().numpy().tobytes(), ti.cpu().numpy().tobytes()
    h2 = open_host(data, index)
    try:
        assert lib.vbf_table_entries(h) == n and lib.vbf_table_blocks(h) == nb.value > 3
        s = ref.Sst(data, index)
        queries = variants(uni)
        want = ref.search_many(queries, [s])
        found, idx, v, c = get_dev_list([h], queries)
        same((found, idx, v, c), want)
        assert (found[:n] == np.where(tb, 2, 1)).all() and (v[:n] == val).all() and (c[:n] == cr.view(np.uint64)).all()
        same(get_dev_list([h2], queries), want)
        for hh in (h, h2):
            sl, bl = ctypes.c_uint64(), ctypes.c_uint64()
            call("vbf_table_key_range", hh, None, 0, ctypes.byref(sl), None, 0, ctypes.byref(bl))
            assert (sl.value, bl.value) == (len(uni[0]), len(uni[-1]))
            small, big = np.full(sl.value + 4, GUARD, np.uint8), np.full(bl.value + 4, GUARD, np.uint8)
            call("vbf_table_key_range", hh, small.ctypes.data, sl.value, ctypes.byref(sl), big.ctypes.data, bl.value,
                 ctypes.byref(bl))
            assert small[:sl.value].tobytes() == uni[0] and big[:bl.value].tobytes() == uni[-1]
            assert (small[sl.value:] == GUARD).all() and (big[bl.value:] == GUARD).all()
            assert lib.vbf_table_key_range(hh, small.ctypes.data, 0, ctypes.byref(sl), big.ctypes.data, 1,
                                           ctypes.byref(bl)) == -1
        # two handles borrowing the same buffers: freeing one leaves the other usable
        h3 = ctypes.c_void_p()
        call("vbf_table_open_dev", P(td), dl.value, P(ti), il.value, P(tblk), nb.value, sp, ctypes.byref(h3))
        lib.vbf_table_free(h3)
        same(get_dev_list([h], queries[:500]), [w[:500] for w in want])
    finally:
        lib.vbf_table_free(h)
        lib.vbf_table_free(h2)


# ---- 7. rejected files ----------------------------------------------------------------------

def open_dev_bytes(data, index, blocks, expect):
    import torch
    from velarixdb_amd._lib import lib
    keep = [_up(_np(data)), _up(_np(index)), _up(np.asarray(blocks, np.uint32))]
    h = ctypes.c_void_p()
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.vbf_table_open_dev(keep[0][1], len(data), keep[1][1], len(index), keep[2][1], len(blocks), sp,
                                ctypes.byref(h))
    msg = lib.vbf_last_error()
    assert rc == expect, msg
    torch.cuda.synchronize()  # no device error left behind
    return h, keep, msg


def test_rejected_files(vbf, ora):
    from velarixdb_amd._lib import VBF_EINVAL, lib
    base = [b"r" + bytes([j >> 8, j & 255]) * (2 + j % 7) for j in range(900)]
    items = [(k, j, T0 + j, 0) for j, k in enumerate(sorted(base))]
    good = write(ora, items)
    blocks = ora.sst_index_blocks(_np(good[1]))
    assert blocks.size >= 4
    s = ref.Sst(*good)

    def swapped():  # two adjacent keys change places; the writer lays the file out as usual
        it = list(items)
        it[400], it[401] = (it[401][0],) + it[400][1:], (it[400][0],) + it[401][1:]
        return write(ora, it)

    def duplicated():
        it = list(items)
        it[401] = (it[400][0],) + it[401][1:]
        return write(ora, it)

    def index_key_flipped():
        i = bytearray(good[1])
        second = 8 + len(s.ikeys[0])
        i[second + 4 + 1] ^= 0x40
        return good[0], bytes(i)

    def index_offset_moved():
        i = bytearray(good[1])
        at = 8 + len(s.ikeys[0]) + 4 + len(s.ikeys[1])
        struct.pack_into("<I", i, at, s.ioffs[1] + 5)
        return good[0], bytes(i)

    dense = b"".join(struct.pack("<IBIQB", 1, j % 256, j, T0 + j, 0) for j in range(300))
    cases = {
        "swapped": swapped(), "duplicated": duplicated(), "index key flipped": index_key_flipped(),
        "index offset moved": index_offset_moved(), "data truncated": (good[0][:-1], good[1]),
        "index truncated": (good[0], good[1][:-1]),
        "300 entries in a block": (dense, struct.pack("<IBI", 1, 299 % 256, 0)),
    }
    for name, (d, i) in cases.items():
        assert (d, i) != good, name
        open_host(d, i, expect=VBF_EINVAL)
        assert lib.vbf_last_error() != b"", name
        # the device entry point, with block starts that are right wherever index.db can still be read
        blk = [0] if name.startswith("300") else blocks if "index" in name else ora.sst_index_blocks(_np(i))
        h, _, msg = open_dev_bytes(d, i, blk, VBF_EINVAL)
        assert not h.value and msg, name
    # a valid open and get on the same stream afterwards
    h, keep, _ = open_dev_bytes(good[0], good[1], blocks, 0)
    try:
        queries = variants(sorted(base))
        same(get_dev_list([h], queries), ref.search_many(queries, [s]))
    finally:
        lib.vbf_table_free(h)


# ---- 8. empty and degenerate ----------------------------------------------------------------

def test_empty_and_degenerate(vbf, ora):
    import torch
    from velarixdb_amd._lib import VBF_EINVAL, lib
    uni, files = universe_files(ora)
    with Tables([files[0], (b"", b""), files[1]]) as T:
        assert lib.vbf_table_entries(T.h[1]) == 0 and lib.vbf_table_blocks(T.h[1]) == 0
        sl, bl = ctypes.c_uint64(9), ctypes.c_uint64(9)
        assert lib.vbf_table_key_range(T.h[1], None, 0, ctypes.byref(sl), None, 0, ctypes.byref(bl)) == 0
        assert (sl.value, bl.value) == (0, 0)
        queries = variants(uni[::4])
        want = ref.search_many(queries, T.ref)
        assert 1 not in want[1] and 2 in want[1]
        same(get_dev_list(T.h, queries), want)
        same(get_host(T.h, queries), want)
        same(get_dev_list([T.h[1]], queries), ref.search_many(queries, []))
        # nsst == 0: every output zero-filled; n == 0: nothing touched
        keys, offs = offsets_batch(queries)
        zero = get_dev([], keys, offs, 0, len(queries))
        assert all(not z.any() for z in zero)
        assert all(z.size == 0 for z in get_dev(T.h, keys, offs, 0, 0))
        # any output may be NULL
        for drop in range(4):
            mask = tuple(int(i != drop) for i in range(4))
            got = get_dev(T.h, keys, offs, 0, len(queries), want=mask)
            assert got[drop] is None
            for g, w in zip(got, want):
                assert g is None or np.array_equal(g, w)
        got = get_dev(T.h, keys, offs, 0, len(queries), want=(0, 0, 0, 0))
        assert got == (None, None, None, None)
        # index bytes for an empty data.db
        open_host(b"", struct.pack("<IBI", 1, 7, 0), expect=VBF_EINVAL)
    torch.cuda.synchronize()
