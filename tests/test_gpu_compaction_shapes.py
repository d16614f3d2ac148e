"""GPU parity for the compaction merge on the buckets of compaction_cases.py: empty, uneven and
tile-edge tables (the host-built level geometry, k_merge_split / k_merge_tile's partial tiles and
zero-tile pairs, run_of and k_check_sorted over repeated run_off values), real-epoch and extreme
times (every i64 time and u64 TTL through the argument struct and the ctypes layer) and the shapes
of the tombstone map.  Every case goes through vbf_compact_merge_host, vbf_compact_merge_dev on a
side stream with and without the update arrays, and SizedTierMerger.merge_ids; some go on to files
through merge_bucket_sst.

Oracle: oracle.compact_merge, the literal fold (pinned on these cases by test_compaction_cases.py).
Ids, map and file bytes are compared for exact equality.  At the extreme times `created + ttl`
wraps in u64 in oracle and kernel alike (compaction_cases.py): the two are compared with each
other, with no claim about the Rust reference there."""
import ctypes
import functools

import numpy as np
import pytest

import compaction_cases as cc
from test_gpu_compaction import _arena

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 7


@functools.lru_cache(maxsize=None)
def _bucket(name):
    """The case as arrays, built once and never written: (case, arena, sorted map arrays)."""
    case = cc.CASES[name]()
    arena = _arena(case[0])
    mk = sorted(case[1])
    mkeys = np.frombuffer(b"".join(mk) or b"\0", np.uint8)
    moff = np.concatenate([[0], np.cumsum([len(k) for k in mk])]).astype(np.uint64)
    mtime = np.asarray([case[1][k] for k in mk], np.int64)
    for a in arena + (mkeys, moff, mtime):
        a.flags.writeable = False
    return case, arena, (mk, mkeys, moff, mtime)


_WANT = {}


def _want(ora, name):
    """The oracle's (ids, new map) for the case, computed once."""
    if name not in _WANT:
        (runs, start, use_ttl, ettl, tttl, now), (keys, offs, cr, tb, ro), _ = _bucket(name)
        m = ora.TombstoneMap(start)
        ids = ora.compact_merge(keys, offs, cr, tb, ro, use_ttl, ettl, tttl, now, m)
        _WANT[name] = (ids.tolist(), m.items())
    return _WANT[name]


def _apply(start, keys, offs, upd_ids, upd_time):
    new = dict(start)
    for e, t in zip(upd_ids, upd_time):
        new[keys[int(offs[e]):int(offs[e + 1])].tobytes()] = t
    return new


def _host_merge(name):
    from velarixdb_amd._lib import call
    (runs, start, use_ttl, ettl, tttl, now), (keys, offs, cr, tb, ro), (mk, mkeys, moff, mtime) = _bucket(name)
    total = int(ro[-1])
    ids, ui, ut = (np.zeros(max(total, 1), d) for d in (np.uint32, np.uint32, np.int64))
    n, nu = ctypes.c_uint64(POISON), ctypes.c_uint64(POISON)
    P = lambda a: a.ctypes.data if a.size else None
    call("vbf_compact_merge_host", P(keys) if int(offs[-1]) else None, P(offs), P(cr), P(tb), ro.ctypes.data,
         ro.size - 1, P(mkeys) if mk else None, P(moff) if mk else None, P(mtime), len(mk), int(use_ttl), ettl, tttl,
         now, ids.ctypes.data, ctypes.byref(n), ui.ctypes.data, ut.ctypes.data, ctypes.byref(nu), 0)
    return ids[:n.value].tolist(), _apply(start, keys, offs, ui[:nu.value].tolist(), ut[:nu.value].tolist())


_SIDE = []


def _side_stream():
    """one non-default stream for the whole module (the library keeps a workspace per stream)"""
    import torch
    if not _SIDE:
        _SIDE.append(torch.cuda.Stream(device=DEV))
    return _SIDE[0]


def _dev_merge(name, with_upd):
    """vbf_compact_merge_dev on the side stream -> (ids, new map or None, n_upd)"""
    import torch
    from velarixdb_amd._lib import call
    (runs, start, use_ttl, ettl, tttl, now), (keys, offs, cr, tb, ro), (mk, mkeys, moff, mtime) = _bucket(name)
    T = lambda a: torch.from_numpy(np.array(a).view(np.int64) if a.dtype == np.uint64 else np.array(a)).to(DEV)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None
    total = int(ro[-1])
    dk, do, dc, dt = T(keys), T(offs), T(cr), T(tb)
    dmk, dmo, dmt = T(mkeys), T(moff), T(mtime)
    ids = torch.full((total,), -1, dtype=torch.int32, device=DEV)
    ui = torch.full((total,), -1, dtype=torch.int32, device=DEV)
    ut = torch.zeros(total, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    n, nu = ctypes.c_uint64(POISON), ctypes.c_uint64(POISON)
    call("vbf_compact_merge_dev", ptr(dk) if int(offs[-1]) else None, ptr(do), ptr(dc), ptr(dt), ro.ctypes.data,
         ro.size - 1, ptr(dmk) if mk else None, ptr(dmo) if mk else None, ptr(dmt) if mk else None, len(mk),
         int(use_ttl), ettl, tttl, now, ptr(ids), ctypes.byref(n), ptr(ui) if with_upd else None,
         ptr(ut) if with_upd else None, ctypes.byref(nu), ctypes.c_void_p(_side_stream().cuda_stream))
    got = ids[: n.value].cpu().numpy().view(np.uint32).tolist()
    assert bool((ids[n.value:] == -1).all())  # nothing written past n_out
    if not with_upd:
        return got, None, nu.value
    new = _apply(start, keys, offs, ui[: nu.value].cpu().numpy().view(np.uint32).tolist(), ut[: nu.value].cpu().tolist())
    return got, new, nu.value


def _sst_tables(runs, val=None):
    from velarixdb_amd.sst import SstEntries
    tables, e0 = [], 0
    for ks, c, t in runs:
        n = len(ks)
        tables.append(SstEntries(np.frombuffer(b"".join(ks) or b"\0", np.uint8) if n else np.zeros(0, np.uint8),
                                 np.concatenate([[0], np.cumsum([len(x) for x in ks])]).astype(np.uint64),
                                 val[e0:e0 + n] if val is not None else np.zeros(n, np.uint32),
                                 c.astype(np.uint64), t.astype(bool)))
        e0 += n
    return tables


def _merger(name):
    from velarixdb_amd.compaction import CompactionConfig, SizedTierMerger
    (runs, start, use_ttl, ettl, tttl, now), _, _ = _bucket(name)
    mg = SizedTierMerger(CompactionConfig(use_ttl=use_ttl, entry_ttl_ms=ettl, tombstone_ttl_ms=tttl,
                                          filter_false_positive=0.01))
    mg.tombstones = dict(start)
    return mg


@pytest.mark.parametrize("name", list(cc.CASES))
def test_merge_host(vbf, ora, name):
    want, want_map = _want(ora, name)
    got, new = _host_merge(name)
    assert got == want
    assert new == want_map


@pytest.mark.parametrize("name", list(cc.CASES))
def test_merge_dev_side_stream(vbf, ora, name):
    want, want_map = _want(ora, name)
    got, new, nu = _dev_merge(name, True)
    assert got == want
    assert new == want_map
    assert nu == sum(1 for k, t in want_map.items() if _bucket(name)[0][1].get(k) != t)


@pytest.mark.parametrize("name", list(cc.CASES))
def test_merge_dev_without_update_arrays(vbf, ora, name):
    want, _ = _want(ora, name)
    got, _, nu = _dev_merge(name, False)
    assert got == want
    assert nu == 0


@pytest.mark.parametrize("name", list(cc.CASES))
def test_merger_merge_ids(vbf, ora, name):
    """SizedTierMerger.merge_ids from SstEntries; an empty table is an SstEntries of length 0."""
    want, want_map = _want(ora, name)
    (runs, start, use_ttl, ettl, tttl, now), (keys, offs, cr, tb, ro), _ = _bucket(name)
    mg = _merger(name)
    (akeys, aoffs, acr, atb, _, aro), got = mg.merge_ids(_sst_tables(runs), now_ms=now)
    assert np.array_equal(aoffs, offs) and np.array_equal(acr, cr) and np.array_equal(aro, ro)
    assert got.tolist() == want
    assert mg.tombstones == want_map


@pytest.mark.parametrize("name", cc.TO_FILES)
def test_merge_bucket_sst(vbf, ora, name):
    """The case through to data.db / index.db and the merged table's filter, byte-exact."""
    from test_gpu_compact_write import _oracle_files
    want, want_map = _want(ora, name)
    (runs, start, use_ttl, ettl, tttl, now), (keys, offs, cr, tb, ro), _ = _bucket(name)
    val = np.random.default_rng(9).integers(0, 2**32, size=int(ro[-1]), dtype=np.uint64).astype(np.uint32)
    ids = np.asarray(want, np.uint32)
    want_d, want_i, m, k, words = _oracle_files(ora, keys, offs, val, cr, tb, ids, 0.01)
    mg = _merger(name)
    data, index, bf, n = mg.merge_bucket_sst(_sst_tables(runs, val), now_ms=now)
    assert n == ids.size
    assert np.array_equal(data, want_d)
    assert np.array_equal(index, want_i)
    assert (bf.num_bits(), bf.no_of_hash_func, bf.num_elements()) == (m, k, n)
    assert np.array_equal(bf.words(), words)
    assert mg.tombstones == want_map


def test_geometry_cases_in_turn_on_one_stream(vbf, ora):
    """Large and small totals alternate on one stream, whose workspace only grows: what an earlier,
    larger merge left behind (ids, prefixes, keep / update flags, tile splits) must not show."""
    def total(name):
        return int(_bucket(name)[1][4][-1])
    by_size = sorted(cc.GEOMETRY, key=total)
    order = []
    while by_size:
        order.append(by_size.pop())
        if by_size:
            order.append(by_size.pop(0))
    assert total(order[0]) > 100 * max(total(order[1]), 1) and total(order[2]) > total(order[1])
    for name in order + order[:2]:
        want, want_map = _want(ora, name)
        got, new, _ = _dev_merge(name, True)
        assert got == want, name
        assert new == want_map, name
