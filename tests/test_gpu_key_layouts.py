"""The key-bytes axis on the GPU: every kernel that reads key bytes, on the torture batches of
tests/key_torture.py -- key lengths 0..4 097 B and 65 535 / 65 536 / 70 001 B interleaved (the
SipHash length byte wraps at 240 / 248 B, the length-order sort clamps at 248 B), placed at a
nonzero first offset and behind a device pointer that is not 8-byte aligned; odd fixed strides
and misaligned 8 / 16 / 24 / 32-byte rows; and keys that tie in their first 8 bytes through the
byte-order compares of the multi-SST probe and the compaction merge.

Every comparison is exact: whole word arrays (the set bits' indices where m > 1e8), whole answer
arrays, whole id lists, against the oracle (bf.rs:84-105, sized.rs:170-320) and Python's bytes
order (= Rust `Ord for [u8]`)."""
import contextlib
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import key_torture as kt
from test_gpu_compaction import _arena, _gpu_merge
from test_gpu_parity import ATOMIC, DEV, PARTITIONED, _dev, _ptr, _stream, dev_batch

pytestmark = pytest.mark.gpu

SEED, N = 0x5EED7001, 20_011
SAT = 4_294_967_295
LEADS = (1, 3, 4, 7, 4093)
SHIFTS = tuple(range(1, 8))
FULL = [("lead", 0)] + [("lead", x) for x in LEADS] + [("shift", x) for x in SHIFTS]


def _short(i):
    """lead 0, one lead and one shift (rotating with the case number)"""
    return [("lead", 0), ("lead", LEADS[i % len(LEADS)]), ("shift", SHIFTS[i % len(SHIFTS)])]


@contextlib.contextmanager
def _env(**kv):
    """environment the library reads per call, restored afterwards"""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _host_batch(keys, lp, lead=0):
    from velarixdb_amd.keys import HostBatch
    data, off = kt.pack_lead(keys, lead)
    return HostBatch(data, off, 0, len(keys), lp)


@functools.lru_cache(maxsize=None)
def _keys(kind):
    pos = kt.torture_keys(SEED, N)
    return pos if kind == "pos" else pos + kt.torture_negative_keys(SEED, N)


def _place(b, shift=0):
    """HostBatch -> (keys, offsets) on the device; shift > 0: the keys' base pointer is `shift`
    bytes into an allocation (a view), offsets unchanged"""
    if shift == 0:
        return dev_batch(b)
    buf = torch.full((b.data.size + shift,), 0x5A, dtype=torch.uint8, device=DEV)
    buf[shift:] = torch.from_numpy(b.data).to(DEV)
    keys = buf[shift:]
    assert keys.data_ptr() % 8 == shift % 8
    offs = _dev(b.offsets.view(np.int64)) if b.offsets is not None else None
    return keys, offs


def _placed(kind, lp, how, x):
    """the torture batch `kind` placed `how`: -> (HostBatch, keys_t, offs_t)"""
    b = _host_batch(_keys(kind), lp, x if how == "lead" else 0)
    return (b,) + tuple(_place(b, x if how == "shift" else 0))


def d_hashes(vbf, keys, offs, b, k):
    out = torch.zeros(b.n * k, dtype=torch.int64, device=DEV)
    vbf._lib.call("vbf_hashes_dev", _ptr(keys), _ptr(offs), b.stride, b.n, b.len_prefix, k, _ptr(out), _stream())
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64).reshape(b.n, k)


def d_build(vbf, keys, offs, b, m, k, strategy, words=None):
    """-> the words tensor (int32) after the build"""
    w = words if words is not None else torch.zeros((m + 31) // 32, dtype=torch.int32, device=DEV)
    vbf._lib.call("vbf_build_dev_ex", _ptr(keys), _ptr(offs), b.stride, b.n, b.len_prefix, m, k, _ptr(w), strategy,
                  _stream())
    torch.cuda.synchronize()
    return w


def d_probe(vbf, keys, offs, b, m, k, words, strategy):
    """-> (answers, count) of vbf_probe_dev_ex / vbf_probe_count_dev_ex"""
    out = torch.full((b.n,), 7, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    vbf._lib.call("vbf_probe_dev_ex", _ptr(keys), _ptr(offs), b.stride, b.n, b.len_prefix, m, k, _ptr(words),
                  _ptr(out), strategy, _stream())
    vbf._lib.call("vbf_probe_count_dev_ex", _ptr(keys), _ptr(offs), b.stride, b.n, b.len_prefix, m, k, _ptr(words),
                  _ptr(cnt), strategy, _stream())
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(cnt.item())


def _set_bits(w):
    """the set bits' indices of a device word tensor, ascending (the nonzero words come back)"""
    nz = torch.nonzero(w).flatten()
    val = w[nz].cpu().numpy().view(np.uint32)
    bits = np.unpackbits(val.view(np.uint8), bitorder="little").reshape(-1, 32).astype(bool)
    return (nz.cpu().numpy().astype(np.uint64)[:, None] * np.uint64(32) + np.arange(32, dtype=np.uint64))[bits]


def _check_words(w, want, m, note):
    if m > 100_000_000:  # want = the set bits' indices
        assert np.array_equal(_set_bits(w), want), note
    else:
        assert np.array_equal(w.cpu().numpy().view(np.uint32), want), note


def _want_words(ora, b, m, k):
    if m > 100_000_000:
        return np.unique((ora.hashes(b, k) % np.uint64(m)).ravel())
    return ora.build_words(b, m, k, threads=8)


# ---------------------------------------------------------------------------------------------
# a. hashes
@pytest.mark.parametrize("lp", [1, 0])
def test_hashes_torture_every_placement(vbf, ora, lp):
    """vbf_hashes_dev (k_keys<Op::Hashes>, calculate_hash bf.rs:222-227) at every placement."""
    want = ora.hashes(_host_batch(_keys("pos"), lp), 3)
    for how, x in FULL:
        b, keys, offs = _placed("pos", lp, how, x)
        got = d_hashes(vbf, keys, offs, b, 3)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (how, x, bad[:5], [len(_keys("pos")[j]) for j in bad[:5]])


# ---------------------------------------------------------------------------------------------
# b. build
BUILD_CASES = [
    (1_000_003, 10, 1), (3_800_017, 19, 1),             # compiled k, staged keys
    (SAT, 4, 1), (SAT, 9, 1),                           # SAT kernels on the offsets layout
    (2_000_003, 7, 1), (2_000_003, 23, 1), (2_300_000_023, 14, 1),  # classes 8, 24; 16 with Barrett
    (2_000_003, 10, 0), (2_000_003, 14, 0),             # no length prefix: main kernel, runtime-k class
]


@pytest.mark.parametrize("strategy", [ATOMIC, PARTITIONED])
@pytest.mark.parametrize("case", range(len(BUILD_CASES)))
def test_build_torture_matches_oracle(vbf, ora, case, strategy):
    """vbf_build_dev_ex (set, bf.rs:84-92) of the torture batch: the atomic kernel and the
    partitioned build's tile pack (length order, staged (begin - base, length) pairs, the head
    prefetch) with zero-length and bucket-31 keys, a nonzero first offset, a shifted base pointer."""
    m, k, lp = BUILD_CASES[case]
    want = _want_words(ora, _host_batch(_keys("pos"), lp), m, k)
    w = torch.zeros((m + 31) // 32, dtype=torch.int32, device=DEV)
    for how, x in (FULL if case == 0 else _short(case)):
        b, keys, offs = _placed("pos", lp, how, x)
        w.zero_()
        d_build(vbf, keys, offs, b, m, k, strategy, w)
        _check_words(w, want, m, (how, x))


def test_fresh_build_torture_into_garbage(vbf, ora):
    """VBF_BUILD_FRESH: the partitioned build of the torture batch (first offset 3) into words full
    of garbage is the oracle's filter of the keys alone."""
    from velarixdb_amd._lib import VBF_BUILD_FRESH
    m, k = 40_000_003, 10
    want = _want_words(ora, _host_batch(_keys("pos"), 1), m, k)
    b, keys, offs = _placed("pos", 1, "lead", 3)
    w = torch.randint(-2**31, 2**31 - 1, ((m + 31) // 32,), dtype=torch.int32, device=DEV)
    d_build(vbf, keys, offs, b, m, k, PARTITIONED | VBF_BUILD_FRESH, w)
    _check_words(w, want, m, "fresh")


# ---------------------------------------------------------------------------------------------
# c. probe
PROBE_CASES = [(1_000_000_007, 10, 1), (1_900_000_003, 19, 1), (300_000_007, 14, 1), (SAT, 4, 1), (300_000_007, 10, 0)]
PROBE_VARIANTS = [(1, {}), (2, {}), (2, {"VBF_PROBE_PU": 0}), (2, {"VBF_PROBE_PU": 0, "VBF_PROBE_GP": 0})]


@pytest.mark.parametrize("case", range(len(PROBE_CASES)))
def test_probe_torture_matches_oracle(vbf, ora, case):
    """contains (bf.rs:95-105) of positives + negatives against a filter of the positives: the
    gather probe and the three partitioned pipelines (round 6 on the build's image, whose slot ->
    key map sees bucket-31 and zero-length keys here; the round-4 position table; round 3)."""
    m, k, lp = PROBE_CASES[case]
    words = ora.build_words(_host_batch(_keys("pos"), lp), m, k, threads=8)
    want = ora.probe(_host_batch(_keys("both"), lp), m, k, words, threads=8)
    assert want[:N].all() and not want.all()
    wd = _dev(words.view(np.int32))
    del words
    for how, x in (FULL if case == 0 else _short(case)):
        b, keys, offs = _placed("both", lp, how, x)
        for strategy, env in PROBE_VARIANTS:
            with _env(**env):
                got, cnt = d_probe(vbf, keys, offs, b, m, k, wd, strategy)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (how, x, strategy, env, bad[:5], [len(_keys("both")[j]) for j in bad[:5]])
            assert cnt == int(want.sum()), (how, x, strategy, env)


# ---------------------------------------------------------------------------------------------
# d. strides
def _stride_check(vbf, ora, L, shift, rows=None):
    """hashes, builds and probes of STRIDE_ROWS rows of L bytes at a base pointer shifted by `shift`"""
    from velarixdb_amd.keys import HostBatch
    rows = kt.stride_rows(L) if rows is None else rows
    neg = kt.stride_rows(L, seed=0x57D2)
    for lp in (1, 0):
        b = HostBatch(rows, None, L, kt.STRIDE_ROWS, lp)
        keys, offs = _place(b, shift)
        assert np.array_equal(d_hashes(vbf, keys, offs, b, 3), ora.hashes(b, 3)), (L, shift, lp)
    b = HostBatch(rows, None, L, kt.STRIDE_ROWS, 1)
    keys, offs = _place(b, shift)
    pb = HostBatch(np.concatenate([rows, neg]), None, L, 2 * kt.STRIDE_ROWS, 1)
    pkeys, poffs = _place(pb, shift)
    m = 1_000_003
    for k in (10, 7):
        want = ora.build_words(b, m, k)
        for strategy in ((PARTITIONED, ATOMIC) if shift else (PARTITIONED,)):
            w = d_build(vbf, keys, offs, b, m, k, strategy)
            assert np.array_equal(w.cpu().numpy().view(np.uint32), want), (L, shift, k, strategy)
        wp = ora.probe(pb, m, k, want)
        for strategy in ((2, 1) if shift else (2,)):
            got, cnt = d_probe(vbf, pkeys, poffs, pb, m, k, w, strategy)
            assert np.array_equal(got, wp) and cnt == int(wp.sum()), (L, shift, k, strategy)
        assert wp[: kt.STRIDE_ROWS].all()


@pytest.mark.parametrize("L", kt.STRIDES)
def test_stride_batches_match_oracle(vbf, ora, L):
    """Fixed strides that are no multiple of 8, around 8 / 16 / 32 / 64 / 256 and single bytes: the
    runtime-stride kernels (hashes, partitioned build and probe at k = 10 and k = 7)."""
    batches = dict(kt.stride_batches())
    assert list(batches) == list(kt.STRIDES) and batches[L].size == kt.STRIDE_ROWS * L
    _stride_check(vbf, ora, L, 0, batches[L])


@pytest.mark.parametrize("L", [16, 32, 8, 24])
def test_misaligned_fixed_rows_fall_back(vbf, ora, L):
    """Rows of 16 / 32 / 8 / 24 bytes whose device pointer is 1, 4 and 8 bytes off: pick_fmt
    (keyhash.hpp) must not take the aligned vector-load kernels; the results equal the oracle."""
    for shift in (1, 4, 8):
        _stride_check(vbf, ora, L, shift)


# ---------------------------------------------------------------------------------------------
# e. multi-probe
A8 = b"a" * 8
STEM = kt.D_STEMS[0]
MULTI_BOUNDS = [
    (b"", b"\xaa" * 7),                                   # the empty key as smallest
    (b"a" * 15 + b"\x01\x07", b"a" * 15 + b"\x01\x07"),   # smallest == biggest
    (b"\xaa" * 5, b"\xaa" * 20),                          # a bound that is a prefix of another bound
    (b"k", b"k\x00\x00\x00"),                             # ties in the zero-padded 8-byte prefix
    (b"k\x00\x00", b"k" + b"\x00" * 9),
    (A8 + b"\x00\x11", A8 + b"\x01\x90"),                 # first difference in the second word
    (b"a" * 16 + b"\x00\x00", b"a" * 22 + b"\x02\x57"),
    (STEM, STEM + b"\x80"),                               # the last byte straddles the sign bit
    (STEM + b"\x7f", STEM + b"\xff\x00"),
    (b"", b"\xff" * 17),                                  # every key but the longer all-0xFF ones
    (b"\x40", b"\xc0\x00"),                               # half of the torture keys
]
MULTI_SPECS = [(2_400_011, 10), (2_400_011, 10), (500_009, 19), (2_400_011, 10), (2_400_011, 10), (2_400_011, 10),
               (95_003, 7), (2_400_011, 10), (2_400_011, 10), (500_009, 19), (2_400_011, 10)]


def test_multi_probe_adversarial_bounds(vbf, ora):
    """vbf_multi_probe_dev / _host (range.rs:118,136): 8 filters of one (m, k) and 3 others, key
    ranges whose bounds tie in their first 8 bytes, are prefixes of each other, are equal, or
    empty; queries = every bound, every bound minus its last byte, every bound plus 0x00, the
    ordering universe and the torture batch.  The one-lane-per-key kernel (VBF_MULTI=1), the interleaved groups (VBF_MULTI=2)
    with the round-4 and round-3 pipelines, the host API at the full batch and at 200 keys (the
    host mirror's CPU compare)."""
    from velarixdb_amd.key_range import SstRange, candidates
    from velarixdb_amd.keys import pack
    uni, tort = kt.ordered_universe(), _keys("pos")
    S = len(MULTI_SPECS)
    assert S == len(MULTI_BOUNDS) and all(lo <= hi for lo, hi in MULTI_BOUNDS)
    bound_keys = [x for lo_hi in MULTI_BOUNDS for x in lo_hi]
    q = bound_keys + [x[:-1] for x in bound_keys] + [x + b"\x00" for x in bound_keys] + uni + tort
    qb = _host_batch(q, 1, lead=3)
    ranges, contains = [], []
    for s, ((m, k), (lo, hi)) in enumerate(zip(MULTI_SPECS, MULTI_BOUNDS)):
        ks = uni[s::S] + tort[s * 1800:(s + 1) * 1800] + [lo, hi]
        f = vbf.BloomFilter.sized(m, k)
        f.set_many(pack(ks))
        ranges.append(SstRange(lo, hi, f))
        contains.append(ora.probe(qb, m, k, ora.build_words(pack(ks), m, k), threads=8).astype(bool))
    inr = np.array([[lo <= x <= hi for lo, hi in MULTI_BOUNDS] for x in q])
    want = inr & np.stack(contains, axis=1)
    assert want[: len(bound_keys)].any() and inr[:, 1].sum() == 3  # smallest == biggest: that key alone (both bounds and the universe's copy)
    keys, offs = _place(qb)
    handles = (ctypes.c_void_p * S)(*[r.filter._h.value for r in ranges])
    bounds = np.frombuffer(b"".join(bound_keys), np.uint8)
    boff = np.concatenate([[0], np.cumsum([len(x) for x in bound_keys])]).astype(np.uint64)
    for multi in (1, 2):
        for gp in (0, 1):
            out = torch.full((qb.n * S,), 7, dtype=torch.uint8, device=DEV)
            with _env(VBF_MULTI=multi, VBF_MULTI_GP=gp):
                vbf._lib.call("vbf_multi_probe_dev", _ptr(keys), _ptr(offs), 0, qb.n, 1, S, handles,
                              bounds.ctypes.data, boff.ctypes.data, _ptr(out), _stream())
                torch.cuda.synchronize()
            got = out.view(qb.n, S).cpu().numpy().astype(bool)
            bad = np.argwhere(got != want)
            assert bad.size == 0, (multi, gp, [(q[j][:24], s_) for j, s_ in bad[:5]])
    assert np.array_equal(candidates(qb, ranges), want)               # host API, the full batch on the GPU
    assert np.array_equal(candidates(q[:200], ranges), want[:200])    # <= 256 keys: the host mirror


# ---------------------------------------------------------------------------------------------
# f. compaction
def _compaction_pool():
    """the ordering universe plus a few long torture keys (a 4 097-byte key among them)"""
    tort = _keys("pos")
    longer = [x for x in tort if 239 <= len(x) <= 4097][:60] + [next(x for x in tort if len(x) == 4097)]
    return sorted(set(kt.ordered_universe() + longer))


def _tables(rng, pool, nruns, per_run=3000):
    """about per_run keys per table; every table holds the empty key and the 4 097-byte key"""
    forced = [i for i, x in enumerate(pool) if len(x) in (0, 4097)]
    runs = []
    for _ in range(nruns):
        pick = np.unique(np.concatenate([rng.choice(len(pool), size=per_run, replace=False), forced]))
        cr = rng.integers(1000, 1030, size=pick.size)  # many time ties
        tb = (rng.random(pick.size) < 0.25).astype(np.uint8)
        runs.append(([pool[i] for i in pick], cr, tb))
    return runs


def _start_map(rng, pool):
    """present keys and near-misses: a present key +- 0x00, a present key minus its last byte"""
    start = {}
    for i in rng.choice(len(pool), size=len(pool) // 6, replace=False):
        x = pool[i]
        for y in ((x,), (x, x + b"\x00"), (x, x[:-1]), (x + b"\x00", x[:-1]))[i % 4]:
            start[y] = int(rng.integers(995, 1035))
    return start


def _merge_dev(vbf, keys, offs, cr, tb, ro, tmap, use_ttl, ettl, tttl, now):
    """vbf_compact_merge_dev with upd_ids / upd_time -> (ids, the new map, device arena)"""
    T = lambda a: torch.from_numpy(np.array(a).view(np.int64) if a.dtype == np.uint64 else np.array(a)).to(DEV)
    mk = sorted(tmap)
    mkeys = np.frombuffer(b"".join(mk) or b"\0", np.uint8)
    moff = np.concatenate([[0], np.cumsum([len(x) for x in mk])]).astype(np.uint64)
    mt = np.asarray([tmap[x] for x in mk], np.int64)
    total = int(ro[-1])
    dk, do, dc, dt = T(keys), T(offs), T(cr), T(tb)
    dmk, dmo, dmt = T(mkeys), T(moff), T(mt if mk else np.zeros(1, np.int64))
    ids = torch.zeros(total, dtype=torch.int32, device=DEV)
    ui = torch.zeros(total, dtype=torch.int32, device=DEV)
    ut = torch.zeros(total, dtype=torch.int64, device=DEV)
    n, nu = ctypes.c_uint64(), ctypes.c_uint64()
    vbf._lib.call("vbf_compact_merge_dev", _ptr(dk), _ptr(do), _ptr(dc), _ptr(dt), ro.ctypes.data, ro.size - 1,
                  _ptr(dmk) if mk else None, _ptr(dmo) if mk else None, _ptr(dmt) if mk else None, len(mk),
                  int(use_ttl), ettl, tttl, now, _ptr(ids), ctypes.byref(n), _ptr(ui), _ptr(ut), ctypes.byref(nu),
                  _stream())
    torch.cuda.synchronize()
    new = dict(tmap)
    for e, t in zip(ui[: nu.value].cpu().numpy().view(np.uint32).tolist(), ut[: nu.value].cpu().tolist()):
        new[keys[int(offs[e]):int(offs[e + 1])].tobytes()] = t
    return ids[: n.value], new, (dk, do, dc, dt)


@pytest.mark.parametrize("nruns,use_ttl", [(2, False), (5, True), (8, False)])
def test_compaction_prefix_ties_match_fold(vbf, ora, nruns, use_ttl):
    """vbf_compact_merge_host / _dev (sized.rs:170-320) over tables drawn from the ordering
    universe: distinct keys that share their first 8 bytes (cmp_keys' word loop returns after an
    equal word, its tail loop runs after a word), keys that tie in the zero-padded prefix (k_fold's
    grouping, the tombstone map's binary search), pairs longer than one 2 048-entry merge tile.
    Then vbf_gather_entries_dev on the merged ids with every optional array."""
    rng = np.random.default_rng(100 + nruns)
    pool = _compaction_pool()
    assert b"" in pool and max(len(x) for x in pool) == 4097
    keys, offs, cr, tb, ro = _arena(_tables(rng, pool, nruns))
    start = _start_map(rng, pool)
    pset = set(pool)
    assert any(x not in pset for x in start) and any(x in pset for x in start)
    now, ettl, tttl = 1040, 20, 25  # some entries and tombstones expire
    m = ora.TombstoneMap(start)
    want = ora.compact_merge(keys, offs, cr, tb, ro, use_ttl, ettl, tttl, now, m)
    want_map = m.items()
    merged = [keys[offs[i]:offs[i + 1]].tobytes() for i in want]
    assert merged == sorted(set(merged))  # strictly increasing in Python bytes order
    got, new = _gpu_merge(keys, offs, cr, tb, ro, start, use_ttl, ettl, tttl, now)
    assert got.tolist() == want.tolist() and new == want_map
    ids, new, (dk, do, dc, dt) = _merge_dev(vbf, keys, offs, cr, tb, ro, start, use_ttl, ettl, tttl, now)
    assert ids.cpu().numpy().view(np.uint32).tolist() == want.tolist() and new == want_map
    # gather: the merged ids and, whatever the merge kept, every entry holding the empty key or the
    # 4 097-byte key; created_ms, tombstones and val_offsets all passed
    from velarixdb_amd._lib import VBF_EINVAL
    total = int(ro[-1])
    all_lens = np.diff(offs).astype(np.int64)
    extra = np.flatnonzero((all_lens == 0) | (all_lens == 4097)).astype(np.uint32)
    assert extra.size >= 2 * nruns and set(all_lens[extra].tolist()) == {0, 4097}
    w64 = np.concatenate([want, extra]).astype(np.int64)
    ids = torch.from_numpy(w64.astype(np.int32)).to(DEV)
    n = w64.size
    val = np.random.default_rng(5).integers(0, 2**32, total, dtype=np.uint64).astype(np.uint32)
    dv = torch.from_numpy(val.view(np.int32)).to(DEV)
    lens = all_lens[w64]
    wkeys = b"".join(keys[offs[i]:offs[i + 1]].tobytes() for i in w64)
    ok_ = torch.full((len(wkeys) + 8,), 0x5A, dtype=torch.uint8, device=DEV)
    oo = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    oc = torch.zeros(n, dtype=torch.int64, device=DEV)
    ot = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
    ov = torch.zeros(n, dtype=torch.int32, device=DEV)
    kb = ctypes.c_uint64()
    vbf._lib.call("vbf_gather_entries_dev", _ptr(dk), _ptr(do), _ptr(dc), _ptr(dt), _ptr(dv), _ptr(ids), n, _ptr(ok_),
                  len(wkeys), _ptr(oo), _ptr(oc), _ptr(ot), _ptr(ov), ctypes.byref(kb), _stream())
    torch.cuda.synchronize()
    assert kb.value == len(wkeys)
    assert ok_[: len(wkeys)].cpu().numpy().tobytes() == wkeys and bool((ok_[len(wkeys):] == 0x5A).all())
    assert np.array_equal(oo.cpu().numpy(), np.concatenate([[0], np.cumsum(lens)]))
    assert np.array_equal(oc.cpu().numpy(), cr[w64]) and np.array_equal(ot.cpu().numpy(), tb[w64])
    assert np.array_equal(ov.cpu().numpy().view(np.uint32), val[w64])
    kb.value = 0
    with pytest.raises(vbf.VbfError) as ei:  # one byte short
        vbf._lib.call("vbf_gather_entries_dev", _ptr(dk), _ptr(do), _ptr(dc), _ptr(dt), _ptr(dv), _ptr(ids), n,
                      _ptr(ok_), len(wkeys) - 1, _ptr(oo), _ptr(oc), _ptr(ot), _ptr(ov), ctypes.byref(kb), _stream())
    assert ei.value.code == VBF_EINVAL and kb.value == len(wkeys)


def test_prefix_tie_swap_rejected(vbf):
    """A table sorted except for one pair of neighbours that tie in the zero-padded 8-byte prefix
    ("k\\0" before "k") is not a SkipMap: rejected by the host and the device entry points."""
    pool = _compaction_pool()
    i = pool.index(b"k")
    assert pool[i + 1] == b"k\x00" and pool[i + 2] == b"k\x00\x00"
    for a in (i, i + 1):
        ks = list(pool)
        ks[a], ks[a + 1] = ks[a + 1], ks[a]
        n = len(ks)
        runs = [(pool, np.arange(n), np.zeros(n, np.uint8)), (ks, np.arange(n), np.zeros(n, np.uint8))]
        keys, offs, cr, tb, ro = _arena(runs)
        with pytest.raises(vbf.VbfError, match="strictly increasing"):
            _gpu_merge(keys, offs, cr, tb, ro, {}, False, 0, 0, 0)
        with pytest.raises(vbf.VbfError, match="strictly increasing"):
            _merge_dev(vbf, keys, offs, cr, tb, ro, {}, False, 0, 0, 0)
