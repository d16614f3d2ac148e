"""GPU parity for the batched range scans over open SST tables (vbf_table_scan_*).

Checker: tests/sst_scan_ref.py (the keys inside the bounds by bytes comparison, each decided by the
lookup checker's fold; pinned by tests/test_sst_scan_ref.py).  Every comparison is exact equality on
all seven output arrays, through _dev (torch buffers with guard bytes around every output) and
_host.  Tables are written with the oracle's encoder."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import key_torture as kt
import scan_cases as sc
import sst_get_ref as ref
import sst_scan_ref as scan_ref

pytestmark = pytest.mark.gpu
GUARD, PAD = 0xA5, 16
T0 = sc.T0
KEEP, EXCL = 1, 2
NAMES7 = ("range_off", "keys", "key_off", "table_idx", "val_offsets", "created_ms", "tombstones")
DTYPES = (np.uint64, np.uint8, np.uint64, np.uint32, np.uint32, np.uint64, np.uint8)


# ---- tables -------------------------------------------------------------------------------

def _np(b):
    return np.frombuffer(b, np.uint8)


def open_host(data, index):
    from velarixdb_amd._lib import lib
    d, i = _np(data), _np(index)
    h = ctypes.c_void_p()
    rc = lib.vbf_table_open_host(d.ctypes.data if d.size else None, d.size, i.ctypes.data if i.size else None,
                                 i.size, 0, ctypes.byref(h))
    assert rc == 0 and h.value, lib.vbf_last_error()
    return h


class Tables:
    """Handles opened with vbf_table_open_host for [(data, index), ...], freed on exit, next to the
    checker's parse of the same bytes."""

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


def handles(hs):
    return (ctypes.c_void_p * max(len(hs), 1))(*[h.value for h in hs])


def simple(ora, keys, salt=0):
    """A table of `keys` (sorted here) with distinct fields derived from the position and `salt`."""
    return sc.write(ora, [(k, (j * 2654435761 + salt) & 0xFFFFFFFF, T0 + salt * 100003 + j, j % 5 == 0)
                          for j, k in enumerate(sorted(keys))])


# ---- calls --------------------------------------------------------------------------------

def pack_bounds(ranges, lead=0):
    """(bytes with `lead` filler bytes in front and one behind, u64 offsets starting at `lead`)"""
    flat = [b for pair in ranges for b in pair]
    offs = np.concatenate([[0], np.cumsum([len(b) for b in flat])]).astype(np.uint64) + np.uint64(lead)
    return np.frombuffer(b"\xEE" * lead + b"".join(flat) + b"\xEE", np.uint8), offs


def sizes_of(nr, n, kb):
    return ((nr + 1) * 8, kb, (n + 1) * 8, 4 * n, 4 * n, 8 * n, n)


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


def scan_dev(hs, ranges, flags=0, lead=0, shift=0, want=(1,) * 7, cut=(0, 0)):
    """vbf_table_scan_dev: a size query, then the filling call into outputs between guard bytes;
    want[i] == 0 passes NULL for output i (None comes back).  cut = (entries, key bytes) taken off
    the two capacities: the call must then fail and leave every output as it was.
    -> (seven arrays, (n_out, key_bytes))"""
    import torch
    from velarixdb_amd._lib import VBF_EINVAL, lib
    nr = len(ranges)
    b, off = pack_bounds(ranges, lead)
    tb, pb = _up(b, shift)
    to, po = _up(off)
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n, kb = ctypes.c_uint64(77), ctypes.c_uint64(77)
    head = (pb, po, nr, len(hs), handles(hs), flags)
    rc = lib.vbf_table_scan_dev(*head, None, None, 0, None, None, None, None, None, 0, ctypes.byref(n),
                                ctypes.byref(kb), sp)
    assert rc == 0, lib.vbf_last_error()
    n0, kb0 = n.value, kb.value
    sz = sizes_of(nr, n0, kb0)
    outs = [_out(s) if w else (None, None) for s, w in zip(sz, want)]
    p = [q for _, q in outs]
    n, kb = ctypes.c_uint64(77), ctypes.c_uint64(77)
    rc = lib.vbf_table_scan_dev(*head, p[0], p[1], kb0 - cut[1], p[2], p[3], p[4], p[5], p[6], n0 - cut[0],
                                ctypes.byref(n), ctypes.byref(kb), sp)
    torch.cuda.synchronize()
    assert (n.value, kb.value) == (n0, kb0), "the size query and the filling call disagree"
    if cut != (0, 0):
        assert rc == VBF_EINVAL and b"_cap" in lib.vbf_last_error()
        for (t, _), s in zip(outs, sz):
            assert t is None or (t.cpu().numpy() == GUARD).all(), "an output was written despite a small capacity"
        return None, (n0, kb0)
    assert rc == 0, lib.vbf_last_error()
    return tuple(None if t is None else _down(t, s, dt) for (t, _), s, dt in zip(outs, sz, DTYPES)), (n0, kb0)


def scan_host(hs, ranges, flags=0, lead=0, want=(1,) * 7, cut=(0, 0)):
    """The same through vbf_table_scan_host, on numpy buffers with guard bytes."""
    from velarixdb_amd._lib import VBF_EINVAL, lib
    nr = len(ranges)
    b, off = pack_bounds(ranges, lead)
    n, kb = ctypes.c_uint64(77), ctypes.c_uint64(77)
    head = (b.ctypes.data, off.ctypes.data, nr, len(hs), handles(hs), flags)
    rc = lib.vbf_table_scan_host(*head, None, None, 0, None, None, None, None, None, 0, ctypes.byref(n),
                                 ctypes.byref(kb))
    assert rc == 0, lib.vbf_last_error()
    n0, kb0 = n.value, kb.value
    sz = sizes_of(nr, n0, kb0)
    outs = [np.full(PAD + s + PAD, GUARD, np.uint8) if w else None for s, w in zip(sz, want)]
    p = [None if o is None else o.ctypes.data + PAD for o in outs]
    n, kb = ctypes.c_uint64(77), ctypes.c_uint64(77)
    rc = lib.vbf_table_scan_host(*head, p[0], p[1], kb0 - cut[1], p[2], p[3], p[4], p[5], p[6], n0 - cut[0],
                                 ctypes.byref(n), ctypes.byref(kb))
    assert (n.value, kb.value) == (n0, kb0), "the size query and the filling call disagree"
    if cut != (0, 0):
        assert rc == VBF_EINVAL and b"_cap" in lib.vbf_last_error()
        assert all(o is None or (o == GUARD).all() for o in outs), "an output was written despite a small capacity"
        return None, (n0, kb0)
    assert rc == 0, lib.vbf_last_error()
    got = []
    for o, s, dt in zip(outs, sz, DTYPES):
        if o is not None:
            assert (o[:PAD] == GUARD).all() and (o[PAD + s:] == GUARD).all(), "wrote outside the output"
        got.append(None if o is None else o[PAD:PAD + s].copy().view(dt))
    return tuple(got), (n0, kb0)


def same(got, want):
    for g, w, what in zip(got, want, NAMES7):
        assert g.size == w.size, "%s holds %d items, the checker %d" % (what, g.size, w.size)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, "%s differs at %d of %d items, first %d: got %d want %d" % (
            what, bad.size, g.size, bad[0], g[bad[0]], w[bad[0]])


def both(T, ranges, flags, hs=None, rs=None, **kw):
    """_dev and _host against the checker; -> the checker's arrays."""
    hs = T.h if hs is None else hs
    rs = T.ref if rs is None else rs
    want = scan_ref.scan_many(ranges, rs, flags)
    got, (n, kb) = scan_dev(hs, ranges, flags, **kw)
    same(got, want)
    assert (n, kb) == (want[3].size, want[1].size)
    same(scan_host(hs, ranges, flags)[0], want)
    return want


# ---- 1. the reference's fixtures ------------------------------------------------------------

def fixture_ranges(refs, count=50):
    keys = sorted(set().union(*[s.starts.keys() for s in refs]))
    rng = np.random.default_rng(0xF1C5)
    ranges = [sc.FULL]
    for _ in range(count):
        i, n = int(rng.integers(0, len(keys))), int(rng.integers(0, 300))
        ranges.append((keys[i], keys[min(i + n, len(keys) - 1)]))
    return ranges


def test_fixtures_full_range_and_ranges_from_their_keys(vbf, ora):
    files = [sc.read_fixture(n) for n in sc.NAMES]
    with Tables(files) as T:
        ranges = fixture_ranges(T.ref)
        for flags in (0, KEEP, EXCL, KEEP | EXCL):
            want = both(T, ranges, flags)
            assert want[0][1] == 19908  # the full range lists every distinct key of the seven tables


def test_python_module(vbf, ora):
    from velarixdb_amd import Table, scan_many
    names = sc.NAMES[:3]
    tabs = [Table.open_dir(os.path.join(sc.SST, n)) for n in names]
    refs = [ref.Sst(*sc.read_fixture(n)) for n in names]
    try:
        ranges = fixture_ranges(refs, 20)
        for keep, excl in itertools.product((False, True), repeat=2):
            want = scan_ref.scan_many(ranges, refs, (KEEP if keep else 0) | (EXCL if excl else 0))
            r = scan_many(ranges, tabs, keep_tombstones=keep, end_exclusive=excl)
            same((r.range_off, r.keys, r.key_off, r.table, r.val_offsets, r.created_ms, r.tombstones), want)
        for j in (0, 3, len(ranges) - 1):
            lo, hi = ranges[j]
            assert list(r.range(j)) == scan_ref.scan(lo, hi, refs, KEEP | EXCL)
        empty = scan_many([], tabs)
        assert empty.range_off.tolist() == [0] and empty.key_off.tolist() == [0] and empty.table.size == 0
    finally:
        for t in tabs:
            t.close()


# ---- 2. block geometry ----------------------------------------------------------------------

def counters(n, length, prefix=b""):
    return [prefix + j.to_bytes(length - len(prefix), "big") for j in range(1, n + 1)]


def edge_bounds(s):
    """Every block's first and last key, the keys just before and after each block edge, a bound
    between two keys, one below the first key and two above the last."""
    ks = sorted(s.starts)
    at = {k: j for j, k in enumerate(ks)}
    out = [ks[0][:-1], ks[0], ks[-1], ks[-1] + b"\0", b"\xff" * 9, ks[len(ks) // 2] + b"\0"]
    for last in s.ikeys:
        j = at[last]
        out += [ks[j], ks[max(j - 1, 0)], ks[min(j + 1, len(ks) - 1)], ks[min(j + 2, len(ks) - 1)], last + b"\0"]
    return sorted(set(out))


@pytest.mark.parametrize("kind", ["uniform", "mixed"])
def test_block_geometry(vbf, ora, kind):
    if kind == "uniform":  # 128 entries x 32 bytes = 4096: entry starts computed at open
        big = simple(ora, counters(128 * 2 + 40, 15, b"f"), 1)
    else:                  # mixed key lengths: entry starts from the walk
        big = simple(ora, [b"m" + bytes([j >> 8, j & 255]) * (1 + j % 9) for j in range(400)], 3)
    one = simple(ora, [b"f" + (130).to_bytes(14, "big") if kind == "uniform" else b"m\x00\x63"], 5)
    with Tables([big, one]) as T:
        assert len(T.ref[0].ikeys) == 3 and len(T.ref[1].fields) == 1
        assert set(T.ref[1].starts) <= set(T.ref[0].starts)
        bnd = edge_bounds(T.ref[0])
        ranges = [(lo, hi) for lo in bnd for hi in bnd]  # inside one block, across edges, all blocks, lo > hi
        for flags in (0, KEEP, EXCL, KEEP | EXCL):
            want = both(T, ranges, flags)
        assert want[0][-1] > len(ranges)
        # above the last key the index step finds no record: the rank is `entries`, nothing is listed
        top = scan_ref.scan_many([(b"\xff" * 9, b"\xff" * 10), (bnd[0], b"\xff" * 9)], T.ref, KEEP)
        assert top[0].tolist() == [0, 0, len(T.ref[0].fields)]  # table 1's single key is also in table 0
        same(scan_dev(T.h, [(b"\xff" * 9, b"\xff" * 10), (bnd[0], b"\xff" * 9)], KEEP)[0], top)
        # each table alone
        for j in (0, 1):
            both(T, ranges[::7], KEEP, hs=[T.h[j]], rs=[T.ref[j]])


# ---- 3. key order edge cases ----------------------------------------------------------------

def test_key_order_edge_cases(vbf, ora):
    rng = np.random.default_rng(0x0DE5)
    keys = {b"a", b"a\0", b"a\0\0", b"a\0\0\0\0\0\0\0", b"a\0\0\0\0\0\0\0\0", b"a\x01", b"b"}
    for L in (0, 1, 7, 8, 9, 15, 16, 17, 33):
        assert L in kt.EDGE
        keys |= {b"\0" * L, b"\xff" * L, b"a" * L, rng.bytes(L), b"a" * L + b"\0"}
    keys |= set(kt.ordered_universe()[::11])
    keys = sorted(keys)
    files = [sc.write(ora, [(k, 100 * t + j, T0 + (j * 7 + t) % 5, (j + t) % 6 == 0)
                            for j, k in enumerate(keys) if j % 3 != t]) for t in range(3)]
    with Tables(files) as T:
        bnd = [k for k in keys if len(k) in (0, 1, 2, 3, 7, 8, 9, 10, 15, 16, 17, 18, 33, 34)][::2]
        bnd += [b"a", b"a\0", b"a\0\0", b"", b"\xff" * 34]
        ranges = [(lo, hi) for lo in bnd for hi in bnd[::3]]
        for flags in (0, KEEP, EXCL, KEEP | EXCL):
            want = both(T, ranges, flags)
        assert want[4].size > len(ranges) and (want[6] == 1).any()
        # the prefix chain, literally: a < a\0 < a\0\0
        rows = scan_ref.scan(b"a", b"a\0\0", T.ref, KEEP)
        assert [r[0] for r in rows] == [b"a", b"a\0", b"a\0\0"]
        assert [r[0] for r in scan_ref.scan(b"a", b"a\0\0", T.ref, KEEP | EXCL)] == [b"a", b"a\0"]


# ---- 4. the fold ----------------------------------------------------------------------------

def fold_files(ora):
    per = [{}, {}, {}, {}]

    def put(key, *cells):  # cells: per table (created, tombstone byte) or None
        for t, c in enumerate(cells):
            if c is not None:
                per[t][key] = c

    put(b"newer", (T0 + 5, 0), (T0 + 6, 0), (T0 + 9, 0), (T0 + 7, 0))   # strictly newer in a later table
    put(b"tie", (T0, 0), (T0, 0), None, (T0, 0))                         # the earlier table wins
    put(b"tie-tomb", None, (T0 + 3, 0), (T0 + 3, 1), None)               # live or tombstone by the order
    put(b"zero-only", None, (0, 0), None, None)                          # absent
    put(b"zero-all", (0, 1), (0, 0), (0, 0), None)                       # absent
    put(b"zero-plus", (0, 0), None, (4, 0), None)                        # the live copy
    put(b"tomb-new", (T0 + 5, 0), (T0 + 9, 1), (T0 + 3, 0), None)        # a tombstone hides the live copies
    put(b"tomb-old", (T0 + 5, 1), (T0 + 9, 0), None, (T0 + 1, 1))        # the live copy is newer
    put(b"big-time", (2**63, 0), (2**64 - 1, 0), (2**63 + 1, 1), None)   # compared as u64
    for j in range(40):
        put(b"fill%02d" % j, (T0 + j, 0), (T0 + 40 - j, j % 2), (T0 + 20, 0) if j % 3 else None,
            (T0 + 20, 1) if j % 4 == 0 else None)
    return [sc.write(ora, [(k, 1000 * t + j, c, tb) for j, (k, (c, tb)) in enumerate(sorted(d.items()))])
            for t, d in enumerate(per)]


def test_the_fold(vbf, ora):
    files = fold_files(ora)
    with Tables(files) as T:
        keys = sorted(set().union(*[s.starts.keys() for s in T.ref]))
        ranges = [sc.FULL, (b"newer", b"tomb-old"), (b"tie", b"tie-tomb"), (b"zero-all", b"zero-plus")]
        ranges += [(k, k) for k in keys if not k.startswith(b"fill")]
        for perm in itertools.permutations(range(4)):
            hs, rs = [T.h[p] for p in perm], [T.ref[p] for p in perm]
            plain = scan_ref.scan_many(ranges, rs, 0)
            kept = scan_ref.scan_many(ranges, rs, KEEP)
            same(scan_dev(hs, ranges, 0)[0], plain)
            same(scan_dev(hs, ranges, KEEP)[0], kept)
            rows = {r[0]: r for r in scan_ref.scan(*sc.FULL, rs, KEEP)}
            first = lambda *tables: min(perm.index(t) for t in tables)
            assert rows[b"newer"][1:] == (perm.index(2), 2000 + rows[b"newer"][2] % 1000, T0 + 9, 0)
            assert rows[b"tie"][1] == first(0, 1, 3) and rows[b"tie"][2] // 1000 == perm[first(0, 1, 3)]
            assert rows[b"tie-tomb"][1] == first(1, 2) and rows[b"tie-tomb"][4] == (perm.index(2) < perm.index(1))
            assert b"zero-only" not in rows and b"zero-all" not in rows
            assert rows[b"zero-plus"][1:] == (perm.index(2), rows[b"zero-plus"][2], 4, 0)
            assert rows[b"tomb-new"][1:] == (perm.index(1), rows[b"tomb-new"][2], T0 + 9, 1)
            assert rows[b"tomb-old"][1:] == (perm.index(1), rows[b"tomb-old"][2], T0 + 9, 0)
            assert rows[b"big-time"][3] == 2**64 - 1 and rows[b"big-time"][4] == 0
            plain_keys = {r[0] for r in scan_ref.scan(*sc.FULL, rs, 0)}
            assert b"tomb-new" not in plain_keys and b"tomb-old" in plain_keys
        # the permutation changes the tie's winner, exactly as the checker says (compared above)
        same(scan_host(T.h, ranges, KEEP)[0], scan_ref.scan_many(ranges, T.ref, KEEP))
        same(scan_host(T.h[::-1], ranges, 0)[0], scan_ref.scan_many(ranges, T.ref[::-1], 0))


# ---- 5. consistency with the lookups --------------------------------------------------------

def test_consistency_with_the_lookups(vbf, ora):
    from velarixdb_amd._lib import call
    rng = np.random.default_rng(0xC0515)
    shared = [rng.bytes(int(rng.integers(1, 24))) for _ in range(600)]
    files = []
    for t in range(3):
        own = [rng.bytes(int(rng.integers(1, 24))) for _ in range(1400)]
        ks = sorted(set(own + shared))
        files.append(sc.write(ora, [(k, int(rng.integers(0, 2**32)), int(rng.choice([0, T0, T0 + 1, T0 + 2, T0 + 3])),
                                     int(rng.integers(0, 4) == 0)) for k in ks]))
    with Tables(files) as T:
        union = sorted(set().union(*[s.starts.keys() for s in T.ref]))
        ranges = []
        for _ in range(200):
            i, n = int(rng.integers(0, len(union))), int(rng.integers(0, 80))
            ranges.append((union[i], union[min(i + n, len(union) - 1)]))
        # one lookup of every key of the union, through the library
        offs = np.concatenate([[0], np.cumsum([len(k) for k in union])]).astype(np.uint64)
        kb = np.frombuffer(b"".join(union) + b"\0", np.uint8)
        n = len(union)
        found, idx, val, cr = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint64)
        call("vbf_table_get_host", kb.ctypes.data, offs.ctypes.data, 0, n, 3, handles(T.h), None, found.ctypes.data,
             idx.ctypes.data, val.ctypes.data, cr.ctypes.data)
        at = {k: j for j, k in enumerate(union)}
        assert (found == 0).any() and (found == 1).any() and (found == 2).any()
        for flags in (0, KEEP):
            (range_off, keys, key_off, table, vo, created, tomb), _ = scan_host(T.h, ranges, flags)
            kbytes = keys.tobytes()
            for r, (lo, hi) in enumerate(ranges):
                listed = {}
                for i in range(int(range_off[r]), int(range_off[r + 1])):
                    listed[kbytes[int(key_off[i]):int(key_off[i + 1])]] = i
                assert list(listed) == sorted(listed) and len(listed) == range_off[r + 1] - range_off[r]
                for k in union[at[lo]:at[hi] + 1]:
                    j = at[k]
                    if k in listed:
                        i = listed[k]
                        assert (found[j], idx[j], val[j], cr[j]) == (2 if tomb[i] else 1, table[i], vo[i], created[i])
                    else:
                        assert found[j] == 0 or (found[j] == 2 and not flags)
                assert set(listed) <= set(union[at[lo]:at[hi] + 1])
        both(T, ranges, KEEP | EXCL)


# ---- 6. degenerate cases --------------------------------------------------------------------

def test_degenerate_cases(vbf, ora):
    import torch
    a = simple(ora, counters(300, 6, b"d"), 1)
    b = simple(ora, counters(50, 6, b"d")[::2] + [b"e1", b"e2"], 2)
    with Tables([a, (b"", b""), b]) as T:
        ks = sorted(T.ref[0].starts)
        present, absent = ks[17], ks[17] + b"\0"
        ranges = [(ks[40], ks[10]),                       # lo > hi
                  (present, present), (absent, absent),   # lo == hi, present and absent
                  (ks[5], ks[30]), (ks[5], ks[30]),       # identical ranges: the outputs repeat
                  (ks[20], ks[60]), (b"", ks[3]), (b"e", b"f")]
        for flags in (0, KEEP, EXCL, KEEP | EXCL):
            want = both(T, ranges, flags)
            sizes = np.diff(want[0]).tolist()
            assert sizes[0] == 0 and sizes[2] == 0 and sizes[3] == sizes[4] > 0
            if flags & EXCL:
                assert sizes[1] == 0
        assert np.diff(both(T, ranges, KEEP)[0])[1] == 1
        # an empty table among the tables was scanned above; only empty tables, one range and one table
        for hs, rs in (([T.h[1]], [T.ref[1]]), ([T.h[1], T.h[1]], [T.ref[1]] * 2), ([T.h[0]], [T.ref[0]])):
            both(T, ranges, KEEP, hs=hs, rs=rs)
            both(T, ranges[3:4], KEEP, hs=hs, rs=rs)
        # no table at all: empty ranges
        got, (n, kb) = scan_dev([], ranges, KEEP)
        same(got, scan_ref.scan_many(ranges, [], KEEP))
        assert (n, kb) == (0, 0)
        same(scan_host([], ranges, KEEP)[0], scan_ref.scan_many(ranges, [], KEEP))
        # bounds_off[0] != 0 and bounds at a misaligned base address
        want = scan_ref.scan_many(ranges, T.ref, KEEP)
        for lead, shift in ((29, 0), (0, 1), (13, 3), (5, 7)):
            same(scan_dev(T.h, ranges, KEEP, lead=lead, shift=shift)[0], want)
        same(scan_host(T.h, ranges, KEEP, lead=29)[0], want)
    torch.cuda.synchronize()


def test_descending_bounds_off_on_the_device(vbf, ora):
    """_dev cannot see its bounds_off on the host: the first pass reports a descending pair."""
    import torch
    from velarixdb_amd._lib import VBF_EINVAL, lib
    with Tables([simple(ora, counters(20, 4, b"x"), 1)]) as T:
        tb, pb = _up(_np(b"abcdef"))
        to, po = _up(np.array([0, 2, 1, 3, 6], np.uint64))
        n, kb = ctypes.c_uint64(7), ctypes.c_uint64(7)
        sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = lib.vbf_table_scan_dev(pb, po, 2, 1, handles(T.h), 0, None, None, 0, None, None, None, None, None, 0,
                                    ctypes.byref(n), ctypes.byref(kb), sp)
        assert rc == VBF_EINVAL and b"bounds_off" in lib.vbf_last_error() and (n.value, kb.value) == (0, 0)
        torch.cuda.synchronize()
        both(T, [(b"", b"y")], 0)  # the stream and the workspaces are fine afterwards


def test_too_many_candidates(vbf, ora):
    """The candidate limit of 2^31 - 1, reached with many copies of one range over a small table:
    the bounds pass counts them, nothing is allocated for them."""
    from velarixdb_amd._lib import VBF_EINVAL, lib
    entries = 20_000
    with Tables([simple(ora, counters(entries, 6, b"t"), 1)]) as T:
        nr = 2**31 // entries + 1
        assert nr * entries > 2**31 - 1 >= (nr - 2) * entries
        bounds = np.frombuffer(b"\xff" * nr, np.uint8)  # lo_r empty, hi_r = ff: every entry, nr times
        off = np.repeat(np.arange(nr + 1, dtype=np.uint64), 2)[:2 * nr + 1]
        assert off[0] == off[1] == 0 and off[2] == 1 and off[-1] == nr
        n, kb = ctypes.c_uint64(7), ctypes.c_uint64(7)
        rc = lib.vbf_table_scan_host(bounds.ctypes.data, off.ctypes.data, nr, 1, handles(T.h), 0, None, None, 0,
                                     None, None, None, None, None, 0, ctypes.byref(n), ctypes.byref(kb))
        assert rc == VBF_EINVAL and b"too many entries" in lib.vbf_last_error()
        assert (n.value, kb.value) == (0, 0)
        both(T, [(b"", b"\xff")] * 3, KEEP)  # three copies are fine


# ---- 7. the sizing protocol -----------------------------------------------------------------

def test_sizing_protocol(vbf, ora):
    files = [simple(ora, counters(500, 7, b"s"), 1), simple(ora, counters(200, 9, b"s"), 2)]
    with Tables(files) as T:
        ks = sorted(T.ref[0].starts)
        ranges = [(ks[10], ks[200]), (b"", b"\xff"), (ks[499], ks[499])]
        want = scan_ref.scan_many(ranges, T.ref, KEEP)
        assert want[3].size > 700
        for fn in (scan_dev, scan_host):
            got, (n, kb) = fn(T.h, ranges, KEEP)  # asserts size query == filled call
            same(got, want)
            # one entry or one key byte too few: VBF_EINVAL, the sizes written, no output touched
            for cut in ((1, 0), (0, 1), (1, 1)):
                assert fn(T.h, ranges, KEEP, cut=cut) == (None, (n, kb))
            # entries_cap does not bind when no per-entry array is given, nor keys_cap without keys
            got, _ = fn(T.h, ranges, KEEP, want=(1, 1, 0, 0, 0, 0, 0), cut=(0, 0))
            same((got[0], got[1]), (want[0], want[1]))
            # each output may be NULL on its own
            for drop in range(7):
                mask = tuple(int(i != drop) for i in range(7))
                got, _ = fn(T.h, ranges, KEEP, want=mask)
                assert got[drop] is None
                for g, w, what in zip(got, want, NAMES7):
                    assert g is None or np.array_equal(g, w), what
            for keep_only in range(7):
                mask = tuple(int(i == keep_only) for i in range(7))
                got, _ = fn(T.h, ranges, KEEP, want=mask)
                assert np.array_equal(got[keep_only], want[keep_only]), NAMES7[keep_only]


def test_capacities_bind_only_the_arrays_they_size(vbf, ora):
    """range_off alone is written with entries_cap = keys_cap = 0."""
    from velarixdb_amd._lib import lib
    with Tables([simple(ora, counters(100, 5, b"c"), 1)]) as T:
        ranges = [(b"", b"\xff"), (b"c", b"c\xff")]
        want = scan_ref.scan_many(ranges, T.ref, 0)
        b, off = pack_bounds(ranges)
        n, kb = ctypes.c_uint64(), ctypes.c_uint64()
        range_off = np.full(3, 9, np.uint64)
        rc = lib.vbf_table_scan_host(b.ctypes.data, off.ctypes.data, 2, 1, handles(T.h), 0, range_off.ctypes.data,
                                     None, 0, None, None, None, None, None, 0, ctypes.byref(n), ctypes.byref(kb))
        assert rc == 0, lib.vbf_last_error()
        assert np.array_equal(range_off, want[0]) and (n.value, kb.value) == (want[3].size, want[1].size)


# ---- 8. open on the encoder's outputs -------------------------------------------------------

def test_open_dev_on_the_encoders_outputs(vbf, ora):
    import torch
    from velarixdb_amd._lib import call, lib
    uni = kt.ordered_universe()
    n = len(uni)
    offs = np.concatenate([[0], np.cumsum([len(k) for k in uni])]).astype(np.uint64)
    keys = np.frombuffer(b"".join(uni) + b"\xEE", np.uint8)
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
    try:
        assert lib.vbf_table_entries(h) == n and lib.vbf_table_blocks(h) > 3
        s = ref.Sst(td.cpu().numpy().tobytes(), ti.cpu().numpy().tobytes())
        ranges = [(b"", b"\xff" * 40)] + [(uni[i], uni[min(i + 90, n - 1)]) for i in range(0, n, 53)]
        for flags in (0, KEEP | EXCL, KEEP):
            want = scan_ref.scan_many(ranges, [s], flags)
            got, _ = scan_dev([h], ranges, flags)
            same(got, want)
        assert got[0][1] == n and np.array_equal(got[6][:n], tb) and np.array_equal(got[4][:n], val)
    finally:
        lib.vbf_table_free(h)
