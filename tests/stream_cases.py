"""Cases for calling the `_dev` entry points on a side stream while their inputs are still pending
(test_gpu_dev_streams.py).

include/vbf.h promises that a `_dev` call is queued on the caller's stream, reads its inputs and
writes its outputs in stream order, and shares nothing with another stream.  A test of that hands
the entry point buffers that still hold something else -- a decoy -- while the copy of the real
input waits on the stream behind a spinning kernel.  A library that reads an input too early, or
from another stream, then computes the decoy's answer.  That only shows if the decoy's answer is
well defined and different, which is what this module provides and test_stream_cases.py checks on
the CPU.

Generators only, seeded and deterministic, no GPU code.  A Case is

    call         the entry-point family ("table_get", "vlog_encode", ...)
    ident        a readable name of the inputs
    real         {name: numpy array}: every device input array
    decoy        {name: numpy array}: same names, same byte lengths, valid input, another answer
    want         the expected outputs for `real` (a tuple of numpy arrays, bytes and ints)
    sizes        {name: int}: what the entry point reports to the host for `real` ({} if nothing)
    decoy_want, decoy_sizes   the same for `decoy`
    meta         scalars and host-side arguments (n, stride, m, k, flags, run_off, ...)

Expectations come from the C oracle and the Python checkers (sst_get_ref, sst_scan_ref, vlog_ref,
vlog_walk_ref, memtable_ref) and from host_call_cases' tables; they are computed here, once, on one
thread.  The decoys are the shapes the suite already runs elsewhere: all-zero offsets (n empty keys),
all-zero keys, zero val_offsets / found / cand, another valid file of the same length.  None of them
sends a kernel out of range.

Three inputs have no decoy that changes the answer and are passed as themselves (still pending):
`blocks` of the SST decoder and of the rebuild (any other valid cut of the same file into as many
blocks decodes to the same entries), `blocks` of the table open (the files determine them, and a
decoy of the same three byte lengths has the same key lengths and so the same block starts), and
`offsets` / `map_off` of the compaction merge (its keys must stay strictly increasing per table, so
n empty keys are not valid input).  The data and the keys next to them do have decoys."""
import functools
import struct
from collections import namedtuple

import numpy as np

import host_call_cases as hc
import memtable_ref
import sst_get_ref as ref
import sst_scan_ref as scan_ref
import vlog_ref as vr
import vlog_walk_ref as wr

Case = namedtuple("Case", "call ident real decoy want sizes decoy_want decoy_sizes meta")

ATOMIC, PARTITIONED, FRESH = 1, 2, 0x100  # VBF_BUILD_* of include/vbf.h
SLICE = 16384                             # kVlogSlice: the value copy's workgroups own this many bytes
U64MAX = 2**64 - 1


def _zeros(real):
    return {k: np.zeros_like(v) for k, v in real.items()}


def _pack(keys):
    """-> (key bytes with one filler byte behind, u64 offsets from 0)"""
    offs = np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.uint64)
    return np.frombuffer(b"".join(keys) + b"\xEE", np.uint8).copy(), offs


def _case(call, ident, real, decoy, want, sizes, decoy_want, decoy_sizes, **meta):
    assert set(real) == set(decoy), (call, ident)
    for k in real:
        real[k] = np.ascontiguousarray(real[k])
        decoy[k] = np.ascontiguousarray(decoy[k])
        assert real[k].nbytes == decoy[k].nbytes and real[k].dtype == decoy[k].dtype, (call, ident, k)
        real[k].flags.writeable = decoy[k].flags.writeable = False
    return Case(call, ident, real, decoy, tuple(want), dict(sizes), tuple(decoy_want), dict(decoy_sizes), meta)


# ---- stateless: build, probe, hashes, or, fold, popcount ----------------------------------------

BUILD_N, BUILD_L, BUILD_M = 60_000, 16, 2_000_003  # RK_CASES' shape of test_gpu_parity.py
BUILDS = ((ATOMIC, 10), (PARTITIONED, 10), (PARTITIONED, 7), (ATOMIC | FRESH, 10), (PARTITIONED | FRESH, 10),
          (PARTITIONED | FRESH, 7))


@functools.lru_cache(maxsize=None)
def _build_keys(seed=0):
    from velarixdb_amd.keys import pack_fixed
    rng = np.random.default_rng(0xB111D + seed)
    return pack_fixed(rng.integers(0, 256, size=(BUILD_N, BUILD_L), dtype=np.uint8))


def _zero_keys(n=BUILD_N):
    from velarixdb_amd.keys import pack_fixed
    return pack_fixed(np.zeros((n, BUILD_L), np.uint8))


@functools.lru_cache(maxsize=None)
def build_case(ora, strategy, k, seed=0):
    """vbf_build_dev_ex.  Without FRESH the build ORs into `words`, an input like the keys: sparse
    random bits pending over zeros.  With FRESH the words are an output only and start as garbage."""
    b, nwords = _build_keys(seed), (BUILD_M + 31) // 32
    real, decoy = {"keys": b.data}, {"keys": np.zeros_like(b.data)}
    if strategy & FRESH:
        want, dwant = ora.build_words(b, BUILD_M, k), ora.build_words(_zero_keys(), BUILD_M, k)
    else:
        rng = np.random.default_rng(0x0A11 + k + seed)
        prior = (np.uint32(1) << rng.integers(0, 32, size=nwords).astype(np.uint32)).astype(np.uint32)
        prior[-1] &= np.uint32((1 << (BUILD_M % 32)) - 1)
        real["words"], decoy["words"] = prior, np.zeros_like(prior)
        want, dwant = ora.build_words(b, BUILD_M, k, prior.copy()), ora.build_words(_zero_keys(), BUILD_M, k)
    return _case("build", "s%#x/k%d/%d" % (strategy, k, seed), real, decoy, (want,), {}, (dwant,), {},
                 strategy=strategy, k=k, m=BUILD_M, n=BUILD_N, stride=BUILD_L, inout=("words",) * (not strategy & FRESH))


@functools.lru_cache(maxsize=None)
def probe_case(ora, strategy, k, count, seed=0):
    """vbf_probe_dev_ex / vbf_probe_count_dev_ex: the real filter holds the first half of the queries.
    The decoy filter is empty and the decoy keys are zeros: nothing is found.  The count entry point
    adds to a device counter, an input too: 1000 pending over 0."""
    from velarixdb_amd.keys import pack_fixed
    b = _build_keys(seed)
    held = BUILD_N // 2 - 4_099 * seed  # another share per seed: two threads' answers differ
    words = ora.build_words(pack_fixed(b.data.reshape(BUILD_N, BUILD_L)[:held]), BUILD_M, k)
    hits, dhits = ora.probe(b, BUILD_M, k, words), ora.probe(_zero_keys(), BUILD_M, k, np.zeros_like(words))
    real, decoy = {"keys": b.data, "words": words}, {"keys": np.zeros_like(b.data), "words": np.zeros_like(words)}
    if count:
        real["count"], decoy["count"] = np.array([1000], np.uint64), np.zeros(1, np.uint64)
        want, dwant = (np.array([1000 + int(hits.sum())], np.uint64),), (np.array([int(dhits.sum())], np.uint64),)
    else:
        want, dwant = (hits,), (dhits,)
    return _case("probe_count" if count else "probe", "s%d/k%d/%d" % (strategy, k, seed), real, decoy, want, {},
                 dwant, {}, strategy=strategy, k=k, m=BUILD_M, n=BUILD_N, stride=BUILD_L, inout=("count",) * count)


@functools.lru_cache(maxsize=None)
def var_batch(n=5_000, seed=0):
    """n keys of 0..40 bytes with offsets (a workgroup is 256 keys: twenty of them and a part)."""
    from velarixdb_amd.keys import pack_offsets
    rng = np.random.default_rng(0x4A54 + seed)
    offs = np.concatenate([[0], np.cumsum(rng.integers(0, 41, size=n))]).astype(np.uint64)
    return pack_offsets(rng.integers(0, 256, size=int(offs[-1]) + 1, dtype=np.uint8), offs)


def _empty_batch(b):
    from velarixdb_amd.keys import pack_offsets
    return pack_offsets(np.zeros_like(b.data), np.zeros_like(b.offsets))


@functools.lru_cache(maxsize=None)
def hashes_case(ora, k=5):
    b = var_batch()
    e = _empty_batch(b)
    return _case("hashes", "k%d" % k, {"keys": b.data, "offsets": b.offsets}, {"keys": e.data, "offsets": e.offsets},
                 (ora.hashes(b, k),), {}, (ora.hashes(e, k),), {}, k=k, n=b.n)


GEN_SEED, GEN_BASE, GEN_N, GEN_L = 0x5EED0003, 500, 3_000, 16


@functools.lru_cache(maxsize=None)
def gen_var_case(ora):
    """vbf_gen_var_dev writes key j at offsets[j]; with the decoy's zero offsets it writes nothing."""
    lens = ora.gen_var_lengths(GEN_SEED, GEN_BASE, GEN_N)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return _case("gen_var", "%d" % GEN_N, {"offsets": offs}, {"offsets": np.zeros_like(offs)},
                 (ora.gen_var(GEN_SEED, GEN_BASE, offs),), {}, (np.zeros(0, np.uint8),), {}, n=GEN_N)


OR_WORDS, FOLD_PARTS, FOLD_STRIDE = 62_501, 3, 62_504  # ceil(2 000 003 / 32) words; a stride of whole 16 bytes


@functools.lru_cache(maxsize=None)
def or_cases():
    """vbf_or_words_dev, vbf_or_fold_dev and vbf_popcount_dev over random words; the decoys are zeros.
    The expectations are numpy's | and bit count: the operations' own definitions in vbf.h."""
    rng = np.random.default_rng(0x0F01D)
    w = lambda n: rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    ones = lambda a: int(np.unpackbits(a.view(np.uint8)).sum())
    z = lambda n: np.zeros(n, np.uint32)
    dst, src = w(OR_WORDS) & w(OR_WORDS), w(OR_WORDS) & w(OR_WORDS)
    parts = w(FOLD_PARTS * FOLD_STRIDE) & w(FOLD_PARTS * FOLD_STRIDE) & w(FOLD_PARTS * FOLD_STRIDE)
    fold = np.bitwise_or.reduce(parts.reshape(FOLD_PARTS, FOLD_STRIDE)[:, :OR_WORDS], axis=0)
    cnt, zc = np.array([77], np.uint64), np.zeros(1, np.uint64)
    return [
        _case("or_words", "62501", {"dst": dst, "src": src}, {"dst": z(OR_WORDS), "src": z(OR_WORDS)},
              (dst | src,), {}, (z(OR_WORDS),), {}, nwords=OR_WORDS, inout=("dst",)),
        _case("or_fold", "3x62501", {"src": parts}, {"src": np.zeros_like(parts)}, (fold,), {}, (z(OR_WORDS),), {},
              nwords=OR_WORDS, nparts=FOLD_PARTS, part_stride=FOLD_STRIDE),
        _case("popcount", "62501", {"words": src, "count": cnt}, {"words": z(OR_WORDS), "count": zc},
              (np.array([77 + ones(src)], np.uint64),), {}, (zc,), {}, nwords=OR_WORDS, inout=("count",)),
    ]


def probe_want(ora, which, queries):
    """hc.probe_case's expectation for any query list over probe set `which`."""
    batch = hc._pack(queries)
    cols = []
    for keys, m, k, words, lo, hi in hc.probe_set(ora, which):
        inside = np.asarray([lo <= q <= hi for q in queries])
        cols.append(inside & ora.probe(batch, m, k, words).astype(bool))
    return np.stack(cols, axis=1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def multi_probe_case(ora, n=5_000):
    """vbf_multi_probe_dev over hc.probe_set(0)'s three filters with their key ranges as bounds (host
    arrays); the keys and their offsets are pending.  n empty keys lie below every range."""
    queries, want = hc.probe_case(ora, 0, n, 0)
    assert np.array_equal(want, probe_want(ora, 0, queries))
    keys, offs = _pack(queries)
    real = {"keys": keys, "offsets": offs}
    return _case("multi_probe", "set0/%d" % n, real, _zeros(real), (want,), {}, (probe_want(ora, 0, [b""] * n),), {},
                 n=n, which=0)


# ---- SST: decode, encode, rebuild, gather, merge -----------------------------------------------

STREAM_SST_SIZES = tuple(s for s in hc.SST_SIZES if s != 40_000)


def merged_pairs(data, blocks):
    """Another valid data.db of the same length and the same blocks with fewer entries: wherever two
    neighbours share a block, the first one's key_len is raised by 17 + the second's key_len, so the
    second entry becomes the tail of the first one's key and the first takes over its fields."""
    out = np.array(data, np.uint8)
    raw = out.tobytes()
    ends = list(map(int, blocks[1:])) + [len(raw)]
    for start, end in zip(map(int, blocks), ends):
        p = start
        while p < end:
            k0 = struct.unpack_from("<I", raw, p)[0]
            q = p + k0 + 17
            if q < end:
                k1 = struct.unpack_from("<I", raw, q)[0]
                if k0 + 17 + k1 <= 4079:
                    out[p:p + 4] = np.frombuffer(struct.pack("<I", k0 + 17 + k1), np.uint8)
                    p = q + k1 + 17
                    continue
            p = q
    return out


@functools.lru_cache(maxsize=None)
def decode_case(ora, size, thread=0):
    """vbf_sst_decode_dev: the count-only call, then the full decode."""
    _, (data, _, blocks) = hc.sst_table(ora, thread, size)
    other = merged_pairs(data, blocks)
    want, dwant = ora.sst_decode(data), ora.sst_decode(other)
    n, dn = want[1].size - 1, dwant[1].size - 1
    return _case("decode", "t%d/%s" % (thread, size), {"data": data, "blocks": blocks},
                 {"data": other, "blocks": blocks.copy()}, want, {"n_out": n}, dwant, {"n_out": dn}, n=n)


def _files(ora, keys, offs, val, cr, tb):
    data, index = ora.sst_write(keys, offs, val, cr.view(np.uint64), tb)
    return data, index, ora.sst_index_blocks(index)


@functools.lru_cache(maxsize=None)
def encode_case(ora, size, thread=0):
    """vbf_sst_encode_dev, the offsets path: the size query, then the fill.  The decoy is n empty keys
    with zero fields: 17 bytes an entry."""
    (keys, offs, val, cr, tb), files = hc.sst_table(ora, thread, size)
    n = offs.size - 1
    real = {"keys": np.concatenate([keys, np.zeros(1, np.uint8)]), "offsets": offs, "val": val, "created": cr, "tomb": tb}
    decoy = _zeros(real)
    dfiles = _files(ora, decoy["keys"], decoy["offsets"], decoy["val"], decoy["created"], decoy["tomb"])
    sz = lambda f: {"data_len": f[0].size, "index_len": f[1].size, "nblocks": f[2].size}
    return _case("encode", "t%d/%s" % (thread, size), real, decoy, files, sz(files), dfiles, sz(dfiles), n=n, stride=0)


@functools.lru_cache(maxsize=None)
def encode_fixed_case(ora, n=5_000, L=16):
    """The fixed-stride path: no offsets, closed-form sizes (the same for any keys: the one case whose
    reported sizes cannot differ), no synchronisation."""
    rng = np.random.default_rng(0xF17ED)
    real = {"keys": rng.integers(0, 256, size=n * L, dtype=np.uint8),
            "val": rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32),
            "created": rng.integers(-2**63, 2**63 - 1, size=n, dtype=np.int64),
            "tomb": rng.integers(0, 2, size=n, dtype=np.uint8)}
    decoy = _zeros(real)
    offs = np.arange(n + 1, dtype=np.uint64) * L
    f = _files(ora, real["keys"], offs, real["val"], real["created"], real["tomb"])
    d = _files(ora, decoy["keys"], offs, decoy["val"], decoy["created"], decoy["tomb"])
    sz = lambda f: {"data_len": f[0].size, "index_len": f[1].size, "nblocks": f[2].size}
    return _case("encode", "fixed/%dx%d" % (n, L), real, decoy, f, sz(f), d, sz(d), n=n, stride=L, sizes_fixed=True)


@functools.lru_cache(maxsize=None)
def rebuild_case(ora, size=5_000, thread=0):
    """vbf_filter_rebuild_from_sst_dev into BloomFilter::new(P, n): (n_out, words)."""
    from velarixdb_amd.keys import pack_offsets
    _, (data, _, blocks) = hc.sst_table(ora, thread, size)
    other = merged_pairs(data, blocks)
    n = ora.sst_decode(data)[1].size - 1
    m = ora.num_bits(n, hc.P)
    k = ora.num_hash(m, n)

    def built(d):
        keys, offs, *_ = ora.sst_decode(d)
        return offs.size - 1, ora.build_words(pack_offsets(keys, offs), m, k)
    (wn, ww), (dn, dw) = built(data), built(other)
    return _case("rebuild", "t%d/%s" % (thread, size), {"data": data, "blocks": blocks},
                 {"data": other, "blocks": blocks.copy()}, (ww,), {"n_out": wn}, (dw,), {"n_out": dn}, m=m, k=k, n=n)


def gather_want(a, ids):
    """ids -> the build's key layout, as vbf.h words vbf_gather_entries_dev: numpy indexing."""
    keys, offs, val, cr, tb = a["keys"], a["offsets"], a["val"], a["created"], a["tomb"]
    parts = [keys[int(offs[i]):int(offs[i + 1])] for i in ids]
    out_off = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)
    return (np.concatenate(parts + [np.zeros(0, np.uint8)]), out_off, cr[ids], tb[ids], val[ids]), int(out_off[-1])


@functools.lru_cache(maxsize=None)
def gather_case(ora, size=5_000, n=3_001):
    (keys, offs, val, cr, tb), _ = hc.sst_table(ora, 0, size)
    ids = np.random.default_rng(0x6A7).integers(0, size, size=n).astype(np.uint32)
    real = {"keys": np.concatenate([keys, np.zeros(1, np.uint8)]), "offsets": offs, "val": val, "created": cr,
            "tomb": tb, "ids": ids}
    decoy = _zeros(real)
    (want, kb), (dwant, dkb) = gather_want(real, ids), gather_want(decoy, decoy["ids"])
    return _case("gather", "%d of %d" % (n, size), real, decoy, want, {"key_bytes": kb}, dwant, {"key_bytes": dkb}, n=n)


@functools.lru_cache(maxsize=None)
def merge_case(ora, name="sizes_6000_1_1_1_3"):
    """vbf_compact_merge_dev with every device array pending: want = (ids, the new tombstone map).
    The decoy keeps the 8-byte key layout: table r holds the keys b'%08d' % 0, 1, 2, ... (strictly
    increasing, as the entry point demands), the map holds counters too, the times are reversed and
    the tombstones flipped."""
    from test_gpu_compaction_shapes import _bucket
    (runs, start, use_ttl, ettl, tttl, now), (keys, offs, cr, tb, ro), (mk, mkeys, moff, mtime) = _bucket(name)
    assert set(np.diff(offs).tolist()) == {8} and set(np.diff(moff).tolist()) == {8}
    dkeys = np.frombuffer(b"".join(b"%08d" % j for a, b in zip(ro[:-1], ro[1:]) for j in range(int(b - a))), np.uint8)
    dmk = [b"%08d" % j for j in range(len(mk))]
    real = {"keys": keys, "offsets": offs, "created": cr, "tomb": tb, "map_keys": mkeys, "map_off": moff, "map_time": mtime}
    decoy = {"keys": dkeys, "offsets": offs.copy(), "created": cr[::-1].copy(), "tomb": (1 - tb).astype(np.uint8),
             "map_keys": np.frombuffer(b"".join(dmk), np.uint8), "map_off": moff.copy(), "map_time": mtime[::-1].copy()}

    def merged(a, start_map):
        m = ora.TombstoneMap(start_map)
        ids = ora.compact_merge(a["keys"], a["offsets"], a["created"], a["tomb"], ro, use_ttl, ettl, tttl, now, m)
        return (np.asarray(ids, np.uint32), m.items()), {"n_out": len(ids)}
    dstart = dict(zip(dmk, decoy["map_time"].tolist()))
    (want, sz), (dwant, dsz) = merged(real, start), merged(decoy, dstart)
    return _case("merge", name, real, decoy, want, sz, dwant, dsz, name=name, run_off=ro, start=start, decoy_start=dstart,
                 map_n=len(mk), ttl=(int(use_ttl), ettl, tttl, now), total=int(ro[-1]))


# ---- tables: open, get, scan --------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def open_case(ora, i):
    """vbf_table_open_dev on pending data / index / blocks.  The decoy is a table of as many keys of the
    same lengths under another prefix: the same three byte lengths, another key range, other fields."""
    n = hc.FLUSH_SIZES[i]
    files = [hc.counter_table(ora, n, salt + i) for salt in (20, 30)]
    arrs = [{"data": np.frombuffer(d, np.uint8), "index": np.frombuffer(x, np.uint8),
             "blocks": ora.sst_index_blocks(np.frombuffer(x, np.uint8))} for d, x in files]
    (want, dwant) = [hc.open_want(d, x) for d, x in files]
    return _case("open", "table%d/%d" % (i, n), arrs[0], arrs[1], want, {}, dwant, {}, n=n)


def _first_differing(make):
    """make(thread) -> (real stuff, want, decoy want); the first thread seed whose answers differ (a
    batch of one key may well be a miss, which is the decoy's answer too)."""
    for thread in range(32):
        got = make(thread)
        if hc.blob(got[1]) != hc.blob(got[2]):
            return thread, got
    raise AssertionError("no seed gives a real answer that differs from the decoy's")


@functools.lru_cache(maxsize=None)
def get_case(ora, n, with_cand, first_thread=0):
    """vbf_table_get_dev over hc.read_tables' three tables (open before the call: the handles are no
    device input of the caller's).  Pending: keys, offsets and, with_cand, a candidate matrix with a
    third of its entries zero.  Decoy: n empty keys and no candidates."""
    parsed = hc.read_tables(ora)[2]

    def make(thread):
        queries, want = hc.get_case(ora, first_thread + thread, n)
        if not with_cand:
            return (queries, None), want, ref.search_many([b""] * n, parsed)
        cand = np.random.default_rng(0xCA4D + n).integers(0, 3, size=(n, 3)).astype(np.uint8) * 127
        return ((queries, cand), ref.search_many(queries, parsed, cand != 0),
                ref.search_many([b""] * n, parsed, np.zeros((n, 3), bool)))
    thread, ((queries, cand), want, dwant) = _first_differing(make)
    keys, offs = _pack(queries)
    real = {"keys": keys, "offsets": offs}
    if with_cand:
        real["cand"] = cand.reshape(-1)
    return _case("table_get", "t%d/%d%s" % (first_thread + thread, n, "/cand" if with_cand else ""), real, _zeros(real),
                 want, {}, dwant, {}, n=n)


@functools.lru_cache(maxsize=None)
def scan_case(ora, nranges, flags, thread=0):
    """vbf_table_scan_dev over the same tables: the size query, then the fill.  Decoy: every range is
    (b"", b"")."""
    parsed = hc.read_tables(ora)[2]
    ranges, want = hc.scan_case(ora, thread, nranges, flags)
    bounds, boff = _pack([b for pair in ranges for b in pair])
    real = {"bounds": bounds, "bounds_off": boff}
    dwant = scan_ref.scan_many([(b"", b"")] * nranges, parsed, flags)
    sz = lambda w: {"n_out": int(w[0][-1]), "key_bytes": int(w[1].size)}
    return _case("table_scan", "t%d/%dx%d" % (thread, nranges, flags), real, _zeros(real), want, sz(want), dwant,
                 sz(dwant), nranges=nranges, flags=flags)


# ---- value log: get, encode, walk ---------------------------------------------------------------

VLOG_BASE = 1000
VLOG_VALUE_LENGTHS = (0, 1, 33, 700, SLICE - 1, SLICE, SLICE + 1, 40_000)
VLOG_KEY_LENGTHS = (0, 1, 5, 17, 40)


@functools.lru_cache(maxsize=None)
def vlog_entries(seed=0, rounds=3):
    """[(key, value, created, tombstone)]: every value length above `rounds` times over, the key
    lengths in rotation, every fifth entry a tombstone."""
    rng = np.random.default_rng(0x7106 + seed)
    lens = [VLOG_VALUE_LENGTHS[(j + seed) % len(VLOG_VALUE_LENGTHS)] for j in range(rounds * len(VLOG_VALUE_LENGTHS))]
    return [(rng.bytes(VLOG_KEY_LENGTHS[j % len(VLOG_KEY_LENGTHS)]), rng.bytes(vl), 1_720_785_462_000 + j, int(j % 5 == 4))
            for j, vl in enumerate(lens)]


@functools.lru_cache(maxsize=None)
def vlog_get_case(with_keys, seed=0, rounds=3):
    """vbf_vlog_get_dev over a log that vbf_vlog_open_dev borrowed while its bytes were pending: the
    size query, then the fill.  Items: every entry in a shuffled order, six of them twice, the end of
    the log and an offset below the window.  Decoys: a log of the same entries with every value's bytes
    reversed; val_offsets 0 (below the window's base: BAD); found 0 (every item skipped); n empty
    keys (a mismatch wherever the entry's key is not empty)."""
    entries = vlog_entries(seed, rounds)
    log, offs = vr.encode(entries, VLOG_BASE)
    other, _ = vr.encode([(k, v[::-1], c + 1, t) for k, v, c, t in entries], VLOG_BASE)
    rng = np.random.default_rng(0x6E7 + seed)
    order = rng.permutation(len(entries)).tolist() + rng.integers(0, len(entries), size=6).tolist()
    vo = np.array([offs[i] for i in order] + [VLOG_BASE + len(log), VLOG_BASE - 1], np.uint32)
    n = vo.size
    found = np.ones(n, np.uint8)
    found[[3, 11]] = (0, 2)
    qkeys = [entries[i][0] for i in order] + [b"x", b"y"]
    qkeys[5] = qkeys[5] + b"!"  # one mismatch
    real = {"log": np.frombuffer(log, np.uint8), "val_offsets": vo, "found": found}
    if with_keys:
        real["keys"], real["offsets"] = _pack(qkeys)
    decoy = _zeros(real)
    decoy["log"] = np.frombuffer(other, np.uint8)
    want = vr.get_many(log, vo, VLOG_BASE, found, qkeys if with_keys else None)
    dwant = vr.get_many(other, decoy["val_offsets"], VLOG_BASE, decoy["found"], [b""] * n if with_keys else None)
    sz = lambda w: {"value_bytes": int(w[2][-1])}
    return _case("vlog_get", "seed%d/%d%s" % (seed, n, "/keys" if with_keys else ""), real, decoy, want, sz(want),
                 dwant, sz(dwant), n=n, base=VLOG_BASE)


@functools.lru_cache(maxsize=None)
def vlog_encode_case(seed=0, rounds=3):
    """vbf_vlog_encode_dev: the size query, then the fill.  Decoy: n empty keys with empty values and
    zero fields, 17 bytes an entry."""
    entries = vlog_entries(seed, rounds)
    n = len(entries)
    real = {}
    real["keys"], real["offsets"] = _pack([k for k, *_ in entries])
    real["values"], real["value_off"] = _pack([v for _, v, *_ in entries])
    real["created"] = np.array([c for *_, c, _ in entries], np.int64)
    real["tomb"] = np.array([t for *_, t in entries], np.uint8)
    (log, offs), (dlog, doffs) = vr.encode(entries, VLOG_BASE), vr.encode([(b"", b"", 0, 0)] * n, VLOG_BASE)
    arr = lambda b, o: (np.frombuffer(b, np.uint8), np.array(o, np.uint32))
    return _case("vlog_encode", "seed%d/%d" % (seed, n), real, _zeros(real), arr(log, offs), {"out_len": len(log)},
                 arr(dlog, doffs), {"out_len": len(dlog)}, n=n, base=VLOG_BASE)


@functools.lru_cache(maxsize=None)
def vlog_walk_case():
    """vbf_vlog_walk_dev over two 8 MiB segments and a little (test_two_segments_and_a_little's log),
    borrowed while pending.  Decoy: the same bytes with the first entry's val_len raised over the
    second entry, one entry fewer and every size different."""
    from test_gpu_vlog_walk import SEGMENT, TILE, Builder
    b = Builder(0x5E6)
    b.add(7, 100)
    for _ in range(4):
        b.add(3, SEGMENT // 2 + 12345)
        b.add(0, 0)
        b.add(9, 700)
    b.reach(b.pos // TILE * TILE + TILE + 40)
    log = b.log()
    assert 2 * SEGMENT < len(log) < 2 * SEGMENT + SEGMENT // 4
    (k0, v0, *_), (k1, v1, *_) = b.entries[:2]
    other = bytearray(log)
    struct.pack_into("<I", other, 4, len(v0) + 17 + len(k1) + len(v1))
    other = bytes(other)

    def walked(raw):
        entries, end, stop = wr.walk(raw, 0, U64MAX, 0)
        a = wr.arrays(entries, end)
        return a, {"n_out": len(entries), "key_bytes": a[2].size, "value_bytes": a[4].size, "end_off": end, "stop": stop}
    (want, sz), (dwant, dsz) = walked(log), walked(other)
    return _case("vlog_walk", "two segments", {"log": np.frombuffer(log, np.uint8)}, {"log": np.frombuffer(other, np.uint8)},
                 want, sz, dwant, dsz, start=0, budget=U64MAX)


# ---- memtable: sort, filter insert --------------------------------------------------------------

MEMTABLE_N = 2049  # one past the sort's tile


@functools.lru_cache(maxsize=None)
def memtable_puts(n=MEMTABLE_N, seed=0):
    """n puts of 1..24-byte keys from a universe of n / 4 (test_gpu_memtable._dup_keys)."""
    rng = np.random.default_rng([0x3E37, n, seed])
    uni = [rng.bytes(int(L)) for L in rng.integers(1, 25, max(1, n // 4))]
    return [uni[i] for i in rng.integers(0, len(uni), n)]


@functools.lru_cache(maxsize=None)
def sort_case(n=MEMTABLE_N, seed=0):
    """vbf_memtable_sort_dev.  Decoy: n empty keys, one distinct key held by the last put."""
    puts = memtable_puts(n, seed)
    real = {}
    real["keys"], real["offsets"] = _pack(puts)
    want, dwant = memtable_ref.sort_ids(puts), memtable_ref.sort_ids([b""] * n)
    return _case("sort", "seed%d/%d" % (seed, n), real, _zeros(real), (want,), {"n_out": want.size}, (dwant,),
                 {"n_out": dwant.size}, n=n)


@functools.lru_cache(maxsize=None)
def insert_case(ora, n=MEMTABLE_N, k=7):
    """vbf_filter_insert_dev into an empty device filter of m bits: (words, elements) and n_new."""
    from velarixdb_amd.keys import pack_offsets
    puts = memtable_puts(n)
    real = {}
    real["keys"], real["offsets"] = _pack(puts)
    decoy = _zeros(real)
    m = ora.num_bits(n, 1e-3)

    def model(a):
        f, fresh = memtable_ref.insert_model(ora, pack_offsets(a["keys"], a["offsets"]), m, k)
        return (f.words(),), {"n_new": fresh}
    (want, sz), (dwant, dsz) = model(real), model(decoy)
    return _case("insert", "%d/k%d" % (n, k), real, decoy, want, sz, dwant, dsz, n=n, m=m, k=k)


# ---- every case of the single-stream test, by family --------------------------------------------

def stateless_cases(ora):
    out = [build_case(ora, s, k) for s, k in BUILDS]
    out += [probe_case(ora, s, 10, count) for count in (False, True) for s in (ATOMIC, PARTITIONED)]
    return out + [hashes_case(ora), gen_var_case(ora)] + or_cases() + [multi_probe_case(ora)]


def sst_cases(ora):
    out = [decode_case(ora, s) for s in STREAM_SST_SIZES if s != 1]  # one entry has no neighbour to merge with
    # the table of one entry: the first seed whose entry has a key, a tombstone and fields that are not zero
    one = next(t for t in range(64) if all(a.any() for a in hc.sst_table(ora, t, 1)[0]))
    out += [encode_case(ora, s, one if s == 1 else 0) for s in STREAM_SST_SIZES] + [encode_fixed_case(ora)]
    return out + [rebuild_case(ora), gather_case(ora), merge_case(ora)]


def table_cases(ora):
    out = [open_case(ora, i) for i in range(len(hc.FLUSH_SIZES))]
    out += [get_case(ora, n, c) for n in hc.GET_SIZES for c in (False, True)]
    return out + [scan_case(ora, *s) for s in hc.SCAN_SHAPES]


def vlog_cases(ora):
    return [vlog_get_case(False), vlog_get_case(True), vlog_encode_case(), vlog_walk_case()]


def memtable_cases(ora):
    return [sort_case(), insert_case(ora)]


FAMILIES = {"stateless": stateless_cases, "sst": sst_cases, "tables": table_cases, "vlog": vlog_cases,
            "memtable": memtable_cases}


# ---- different streams from different threads ---------------------------------------------------

STREAM_THREADS = 3
STREAM_ROUNDS = 8


def thread_jobs(ora, family, threads=STREAM_THREADS, rounds=STREAM_ROUNDS):
    """One list of cases per thread, `rounds` long, the sizes in hc.rotation's order: in every round
    the threads ask their streams' workspaces for different sizes, with inputs of their own."""
    if family == "tables":
        def per(t):
            gets = [get_case(ora, n, False, 4 + 8 * t) for n in hc.GET_SIZES]
            scans = [scan_case(ora, *s, thread=4 + t) for s in hc.SCAN_SHAPES]
            return [c for pair in zip(gets, scans) for c in pair]
    elif family == "sst":
        def per(t):
            return [c for s in STREAM_SST_SIZES for c in (encode_case(ora, s, t), decode_case(ora, s if s != 1 else 300, t))]
    elif family == "vlog":
        def per(t):
            return [c for r in (3, 1, 2) for c in (vlog_get_case(True, 10 * t + r, r), vlog_encode_case(10 * t + r, r))]
    elif family == "memtable":
        def per(t):
            return [sort_case(n, t) for n in (MEMTABLE_N, 300, 6_145, 1)]
    elif family == "build_probe":
        def per(t):
            return [c for k in (10, 7) for c in (build_case(ora, PARTITIONED, k, 1 + t), probe_case(ora, PARTITIONED, k, False, 1 + t))]
    else:
        raise KeyError(family)
    # the lists pair two entry points, so a step of two keeps the threads of a round in one of them
    step = 1 if family == "memtable" else 2
    return [hc.rotation(per(t), step * t, rounds) for t in range(threads)]


THREAD_FAMILIES = ("tables", "sst", "vlog", "memtable", "build_probe")
