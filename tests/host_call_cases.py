"""Jobs for calling the host entry points from several threads at once (test_gpu_host_threads.py).

Every `_host` entry point stages into workspaces cached on the device's shared stream; two callers
inside one of them at the same time would read each other's staged keys, offsets or descriptors
unless the library serialises them.  A test of that needs, per thread, a list of calls whose right
answers are known before any thread starts and differ from every other thread's, so that an answer
computed from a neighbour's inputs cannot pass.

Generators only, seeded and deterministic, no GPU code.  A Job is (call, ident, args, want, size):
the entry-point family, a readable name of its inputs, the inputs, the expected outputs (numpy
arrays, bytes and ints, compared byte for byte through `blob`) and the number of entries, keys or
ranges that sets its workspace sizes.  Expectations come from the C oracle and the Python checkers
(sst_get_ref, sst_scan_ref) and are computed here, on one thread: the oracle is not assumed
re-entrant from Python threads.

`<family>_jobs(ora)` returns one job list per thread, ROUNDS long.  Thread t takes the family's
cases in the order `rotation` gives, so in every round the threads ask the same workspace slots for
different sizes, and one thread asks for small, large, small.

test_host_call_cases.py checks on the CPU that the expectations are not trivial and that the jobs
of one round really differ."""
import functools
import hashlib
from collections import namedtuple

import numpy as np

import compaction_cases as cc
import sst_get_ref as ref
import sst_scan_ref as scan_ref

Job = namedtuple("Job", "call ident args want size")

THREADS = 4
ROUNDS = 24  # per thread; each thread's calls take a millisecond or so, so a run lasts tens of milliseconds
KEEP, EXCL = scan_ref.KEEP_TOMBSTONES, scan_ref.END_EXCLUSIVE


def rotation(cases, thread, rounds=ROUNDS):
    """cases[(r + thread) % len(cases)] for every round: with at least as many cases as threads, no two
    threads hold the same case in one round."""
    return [cases[(r + thread) % len(cases)] for r in range(rounds)]


def blob(x):
    """The bytes an output is compared by.  Arrays keep their dtype in it, so a u32 answer cannot
    equal a u64 one of the same values."""
    if isinstance(x, np.ndarray):
        return x.dtype.str.encode() + b"|" + np.ascontiguousarray(x).tobytes()
    if isinstance(x, (bytes, bytearray)):
        return b"b|" + bytes(x)
    if isinstance(x, (bool, np.bool_, int, np.integer)):
        return b"i|%d" % int(x)
    if isinstance(x, str):
        return b"s|" + x.encode()
    if isinstance(x, dict):
        return b"{" + b",".join(blob(k) + b":" + blob(v) for k, v in sorted(x.items())) + b"}"
    if isinstance(x, (tuple, list)):
        return b"(" + b",".join(b"%d:" % len(b) + b for b in map(blob, x)) + b")"
    if x is None:
        return b"n|"
    raise TypeError("no byte form for %r" % type(x))


_PRINTS = {}


def fingerprint(x):
    """sha256 of blob(x), kept per object: the jobs repeat over the rounds."""
    if id(x) not in _PRINTS:
        _PRINTS[id(x)] = (x, hashlib.sha256(blob(x)).hexdigest())  # x kept alive, so its id stays its own
    return _PRINTS[id(x)][1]


# ---- encode / decode ----------------------------------------------------------------------------

# small, large, small: the order one thread meets them in
SST_SIZES = (1, 40_000, 300, 5_000, "block")
BLOCK_LENS = (4079, 4000, 1, 0)  # a block filled to 4096 bytes, then one that just does not fit


@functools.lru_cache(maxsize=None)
def sst_table(ora, thread, size):
    """A random table (test_gpu_sst_encode._table) and the oracle's files for it:
    (keys, offs, val, created i64, tomb), (data, index, blocks)."""
    from test_gpu_sst_encode import _table
    seed = 0x51000 + 97 * thread + SST_SIZES.index(size)
    lens = BLOCK_LENS if size == "block" else np.random.default_rng(seed).integers(0, 71, size=size)
    keys, offs, val, cr, tb = _table(seed, lens)
    data, index = ora.sst_write(keys, offs, val, cr.view(np.uint64), tb)
    out = (keys, offs, val, cr, tb), (data, index, ora.sst_index_blocks(index))
    for a in out[0] + out[1]:
        a.flags.writeable = False
    return out


def encode_jobs(ora, threads=THREADS):
    """vbf_sst_encode_host: args as encode_host of test_gpu_sst_encode.py takes them (stride 0)."""
    def job(t, size):
        arrays, files = sst_table(ora, t, size)
        return Job("encode", "t%d/%s" % (t, size), arrays, files, arrays[1].size - 1)
    return [rotation([job(t, s) for s in SST_SIZES], t) for t in range(threads)]


def decode_jobs(ora, threads=THREADS):
    """vbf_sst_decode_host on the same files: (data, index) -> keys, offsets, val, created u64, tomb."""
    def job(t, size):
        arrays, (data, index, _) = sst_table(ora, t, size)
        keys, offs, val, cr, tb = ora.sst_decode(data)
        assert np.array_equal(offs, arrays[1]) and np.array_equal(val, arrays[2])  # the oracle inverts itself
        return Job("decode", "t%d/%s" % (t, size), (data, index), (keys, offs, val, cr, tb), offs.size - 1)
    return [rotation([job(t, s) for s in SST_SIZES], t) for t in range(threads)]


# ---- tables: get, scan, open --------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def read_tables(ora):
    """The three overlapping tables of the ordering universe (test_gpu_table_get.universe_files) ->
    (universe, [(data, index)], the checker's parses, the query pool)."""
    from test_gpu_table_get import universe_files, variants
    uni, files = universe_files(ora)
    pool = sorted(set(variants(uni)) | {b"zz%05d" % i for i in range(3000)})
    return uni, files, [ref.Sst(d, i) for d, i in files], pool


_SEARCH = {}


def _search(ora, key):
    """The lookup checker's answer for one key over the read tables, computed once per key."""
    if key not in _SEARCH:
        _SEARCH[key] = ref.search(key, read_tables(ora)[2])
    return _SEARCH[key]


GET_SIZES = (1, 20_000, 257, 4_099)  # one key, many blocks of threads, one past a block, an odd middle


@functools.lru_cache(maxsize=None)
def get_case(ora, thread, n):
    pool = read_tables(ora)[3]
    rng = np.random.default_rng(0x6E7000 + 131 * thread + n)
    queries = [pool[i] for i in rng.integers(0, len(pool), size=n)]
    rows = [_search(ora, q) for q in queries]
    want = tuple(np.asarray([r[c] for r in rows], dt) for c, dt in enumerate((np.uint8, np.uint32, np.uint32, np.uint64)))
    return queries, want


def get_jobs(ora, threads=THREADS, with_filters=False, rounds=ROUNDS, first_thread=0):
    """vbf_table_get_host over the three read tables; filters only prune, so the same answers."""
    call = "get_filtered" if with_filters else "get"

    def job(t, n):
        queries, want = get_case(ora, t, n)
        return Job(call, "t%d/%d" % (t, n), (queries,), want, n)
    return [[job(t, n) for n in rotation(GET_SIZES, t, rounds)] for t in range(first_thread, first_thread + threads)]


# (ranges, flags): both flags off, each alone, both on; narrow ranges in the large batches, so the
# outputs stay a few thousand entries, and one wide range in the batch of one
SCAN_SHAPES = ((1, KEEP), (400, 0), (7, EXCL), (64, KEEP | EXCL))


@functools.lru_cache(maxsize=None)
def scan_case(ora, thread, nranges, flags):
    uni, _, parsed, _ = read_tables(ora)
    rng = np.random.default_rng(0x5CA000 + 137 * thread + nranges)
    ranges = []
    for _ in range(nranges):
        a = int(rng.integers(0, len(uni) - 1))
        b = min(len(uni) - 1, a + int(rng.integers(1, 1500 if nranges == 1 else 40)))
        lo, hi = uni[a], uni[b]
        ranges.append((lo, hi) if rng.random() < 0.8 else (lo[:-1] if lo else lo, hi + b"\0"))  # bounds that are no key
    return ranges, scan_ref.scan_many(ranges, parsed, flags)


def scan_jobs(ora, threads=THREADS, rounds=ROUNDS, first_thread=0):
    """vbf_table_scan_host (size query, then fill) over the three read tables."""
    def job(t, shape):
        ranges, want = scan_case(ora, t, *shape)
        return Job("scan", "t%d/%dx%d" % (t, shape[0], shape[1]), (ranges, shape[1]), want, shape[0])
    return [[job(t, s) for s in rotation(SCAN_SHAPES, t, rounds)] for t in range(first_thread, first_thread + threads)]


def counter_table(ora, n, salt):
    """n keys b'c<salt>-%08d' in a table of their own (test_gpu_table_get.simple)."""
    from test_gpu_table_get import simple
    return simple(ora, [b"c%d-%08d" % (salt, i) for i in range(n)], salt)


@functools.lru_cache(maxsize=None)
def open_files(ora):
    """Six tables of different sizes: the three read tables and three of 1, 300 and 5 000 keys."""
    files = list(read_tables(ora)[1]) + [counter_table(ora, n, s) for s, n in enumerate((1, 300, 5_000), 1)]
    return [files[i] for i in (3, 0, 4, 5, 1, 2)]  # small, large, small


def open_want(data, index):
    """(entries, blocks, smallest key, biggest key) from the checker's parse."""
    s = ref.Sst(data, index)
    return len(s.fields), len(s.ikeys), min(s.starts), s.ikeys[-1]


def open_jobs(ora, threads=THREADS):
    """vbf_table_open_host: entries, blocks and key_range of the handle against the parse."""
    jobs = [Job("open", "file%d" % i, f, open_want(*f), len(f[0])) for i, f in enumerate(open_files(ora))]
    return [rotation(jobs, t) for t in range(threads)]


# ---- compaction ---------------------------------------------------------------------------------

# one small and one large geometry case, two of the cases that go through to files
MERGE_CASES = ("sizes_0_5_0_7_0", "sizes_6000_1_1_1_3", cc.TO_FILES[0], "every_key_in_every_table")


@functools.lru_cache(maxsize=None)
def merge_case(ora, name):
    """(oracle ids, new map, val offsets, oracle files (data, index, m, k, words)) for a case of
    compaction_cases.py, as test_gpu_compaction_shapes.py computes them."""
    from test_gpu_compact_write import _oracle_files
    from test_gpu_compaction_shapes import _bucket
    (runs, start, use_ttl, ettl, tttl, now), (keys, offs, cr, tb, ro), _ = _bucket(name)
    m = ora.TombstoneMap(start)
    ids = ora.compact_merge(keys, offs, cr, tb, ro, use_ttl, ettl, tttl, now, m)
    val = np.random.default_rng(9).integers(0, 2**32, size=int(ro[-1]), dtype=np.uint64).astype(np.uint32)
    return ids.tolist(), m.items(), val, _oracle_files(ora, keys, offs, val, cr, tb, ids, 0.01)


def merge_jobs(ora, threads=THREADS, rounds=ROUNDS):
    """vbf_compact_merge_host through _host_merge of test_gpu_compaction_shapes.py: (ids, new map)."""
    def job(name):
        ids, new, _, _ = merge_case(ora, name)
        total = sum(len(ks) for ks, _, _ in cc.CASES[name]()[0])
        return Job("merge", name, (name,), (np.asarray(ids, np.uint32), new), total)
    jobs = [job(n) for n in MERGE_CASES]
    return [rotation(jobs, t, rounds) for t in range(threads)]


def write_jobs(ora, threads=THREADS, rounds=ROUNDS):
    """vbf_compact_write_host through SizedTierMerger.merge_bucket_sst: data.db, index.db, the merged
    table's filter (m, k, n, words), the entry count and the new map."""
    def job(name):
        ids, new, val, (data, index, m, k, words) = merge_case(ora, name)
        total = sum(len(ks) for ks, _, _ in cc.CASES[name]()[0])
        return Job("write", name, (name, val), (data, index, m, k, words, len(ids), new), total)
    jobs = [job(n) for n in MERGE_CASES]
    return [rotation(jobs, t, rounds) for t in range(threads)]


# ---- multi-probe and rebuild --------------------------------------------------------------------

P = 0.01
PROBE_BATCHES = (300, 5_000)  # both above the 256-key mirror limit: the device path


def _pack(keys):
    from velarixdb_amd.keys import pack
    return pack(keys)


@functools.lru_cache(maxsize=None)
def probe_set(ora, which):
    """Three filters over overlapping slices of a key universe of their own ('a...' or 'b...', so the
    two sets are disjoint): [(keys, m, k, oracle words, smallest, biggest)]."""
    uni = [b"%c%06d" % (b"ab"[which], 3 * i) for i in range(4_000)]
    out = []
    for j in range(3):
        keys = uni[j * 1000 + 100 * which:j * 1000 + 1_700 + 300 * which]
        m = ora.num_bits(len(keys), P)
        k = ora.num_hash(m, len(keys))
        out.append((keys, m, k, ora.build_words(_pack(keys), m, k), keys[0], keys[-1]))
    return out


@functools.lru_cache(maxsize=None)
def probe_case(ora, which, n, seed):
    """n queries (members, near misses inside the ranges, keys of the other set) and
    candidates() = in range and filter.contains, [n, 3] as u8."""
    rng = np.random.default_rng(0x3B0000 + seed)
    c = b"ab"[which]
    queries = []
    for i, r in zip(rng.integers(0, 12_000, size=n).tolist(), rng.random(n).tolist()):
        queries.append(b"%c%06d" % (c, i) if r < 0.9 else b"%c%06d" % (b"ab"[1 - which], i))
    batch = _pack(queries)
    cols = []
    for keys, m, k, words, lo, hi in probe_set(ora, which):
        inside = np.asarray([lo <= q <= hi for q in queries])
        cols.append(inside & ora.probe(batch, m, k, words).astype(bool))
    return queries, np.stack(cols, axis=1).astype(np.uint8)


def probe_jobs(ora, threads=THREADS, rounds=ROUNDS):
    """vbf_multi_probe_host through key_range.candidates: thread t takes the four (set, batch)
    combinations in turn, with queries of its own."""
    combos = [(0, 300), (0, 5_000), (1, 300), (1, 5_000)]

    def job(t, which, n):
        queries, want = probe_case(ora, which, n, 10 * t + which)
        return Job("probe", "t%d/set%d/%d" % (t, which, n), (which, queries), (want,), n)
    return [[job(t, *c) for c in rotation(combos, t, rounds)] for t in range(threads)]


REBUILD_SIZES = (17, 20_000, 200, 3_000)


@functools.lru_cache(maxsize=None)
def rebuild_case(ora, i):
    """SST i (data, index) and the filter BloomFilter::new(P, n) rebuilt from it: (m, k, words)."""
    n = REBUILD_SIZES[i]
    data, index = counter_table(ora, n, 10 + i)
    keys, offs, *_ = ora.sst_decode(np.frombuffer(data, np.uint8))
    m = ora.num_bits(n, P)
    k = ora.num_hash(m, n)
    from velarixdb_amd.keys import pack_offsets
    return (data, index), (n, m, k, ora.build_words(pack_offsets(keys, offs), m, k))


def rebuild_jobs(ora, threads=THREADS, rounds=ROUNDS):
    """vbf_filter_rebuild_from_sst_host: thread t rebuilds filter (t, i) from SST i, the SSTs in
    turn.  ORing the same keys in again leaves the words as they are, so every round expects the
    oracle's words; the returned entry count is the SST's every time."""
    def job(t, i):
        files, (n, m, k, words) = rebuild_case(ora, i)
        return Job("rebuild", "t%d/sst%d" % (t, i), (t, i) + files, (n, m, k, words), n)
    return [[job(t, i) for i in rotation(range(len(REBUILD_SIZES)), t, rounds)] for t in range(threads)]


P_BUILD = 1e-4                     # k = 19
REBUILD_BUILD_SIZES = (240_000, 3_000)  # 4 560 000 bit indices, past the 2^22 at which AUTO builds partitioned; 57 000
BUILD_THREADS, BUILD_ROUNDS = 2, 12


@functools.lru_cache(maxsize=None)
def rebuild_build_case(ora, thread, i):
    """A table of thread `thread`'s own with REBUILD_BUILD_SIZES[i] entries and the filter
    BloomFilter::new(P_BUILD, n) rebuilt from it: (data, index), (n, m, k, words)."""
    from velarixdb_amd.keys import pack_offsets
    n = REBUILD_BUILD_SIZES[i]
    data, index = counter_table(ora, n, 40 + 10 * i + thread)
    keys, offs, *_ = ora.sst_decode(np.frombuffer(data, np.uint8))
    m = ora.num_bits(n, P_BUILD)
    k = ora.num_hash(m, n)
    return (data, index), (n, m, k, ora.build_words(pack_offsets(keys, offs), m, k, threads=8))


def rebuild_build_jobs(ora, threads=BUILD_THREADS, rounds=BUILD_ROUNDS):
    """vbf_filter_rebuild_from_sst_host where the build behind the decode is the partitioned one: the
    large and the small table alternate, thread 1 a round behind thread 0, so in every round one
    thread's rebuild takes the partitioned build's workspace and the other's the atomic build."""
    def job(t, i):
        files, want = rebuild_build_case(ora, t, i)
        return Job("rebuild_build", "t%d/sst%d" % (t, i), (t, i) + files, want, want[0])
    return [[job(t, i) for i in rotation(range(len(REBUILD_BUILD_SIZES)), t, rounds)] for t in range(threads)]


# ---- the one-shot build and probe (they take the staging lock, not the host-call lock) ----------

ONE_SHOT = ((1_000, 12), (60_000, 16), (257, 0), (9_000, 33))  # (keys, stride; 0 = lengths 0..40)


@functools.lru_cache(maxsize=None)
def one_shot_case(ora, i):
    """A key batch, (m, k), the oracle's words for it, and probe answers for a second batch that
    holds every other key of the first plus as many strangers."""
    from velarixdb_amd.keys import pack_fixed, pack_offsets
    n, stride = ONE_SHOT[i]
    rng = np.random.default_rng(0x0B5000 + i)

    def batch(n):
        if stride:
            return pack_fixed(rng.integers(0, 256, size=(n, stride), dtype=np.uint8))
        offs = np.concatenate([[0], np.cumsum(rng.integers(0, 41, size=n))]).astype(np.uint64)
        return pack_offsets(rng.integers(0, 256, size=int(offs[-1]), dtype=np.uint8), offs)
    keys, strangers = batch(n), batch(n // 2)
    m = ora.num_bits(n, P)
    k = ora.num_hash(m, n)
    words = ora.build_words(keys, m, k)
    if stride:
        half = keys.data.reshape(n, stride)[::2]
        q = pack_fixed(np.concatenate([half, strangers.data.reshape(-1, stride)]))
    else:
        lens = np.diff(keys.offsets)[::2].tolist() + np.diff(strangers.offsets).tolist()
        parts = [keys.data[int(keys.offsets[j]):int(keys.offsets[j + 1])] for j in range(0, n, 2)] + [strangers.data]
        q = pack_offsets(np.concatenate(parts), np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64))
    return keys, q, m, k, words, ora.probe(q, m, k, words)


def build_host_jobs(ora, rounds=ROUNDS):
    """vbf_build_host into a zeroed private word array -> the oracle's words."""
    def job(i):
        keys, _, m, k, words, _ = one_shot_case(ora, i)
        return Job("build_host", "batch%d" % i, (keys, m, k), (words,), keys.n)
    return rotation([job(i) for i in range(len(ONE_SHOT))], 0, rounds)


def probe_host_jobs(ora, rounds=ROUNDS):
    """vbf_probe_host on the oracle's words -> the oracle's answers."""
    def job(i):
        _, q, m, k, words, hits = one_shot_case(ora, i)
        return Job("probe_host", "batch%d" % i, (q, m, k, words), (hits,), q.n)
    return rotation([job(i) for i in range(len(ONE_SHOT))], 1, rounds)


# ---- flush: encode, then open the encoder's own output -----------------------------------------

FLUSH_SIZES = (1, 12_000, 300, 2_500)


@functools.lru_cache(maxsize=None)
def flush_case(ora, i):
    """A sorted table as the flush hands it over (keys, offs, val, created u64, tomb) -> its files and
    what opening them reports."""
    n = FLUSH_SIZES[i]
    data, index = counter_table(ora, n, 20 + i)
    keys, offs, val, cr, tb = ora.sst_decode(np.frombuffer(data, np.uint8))
    return (keys, offs, val, cr, tb), (np.frombuffer(data, np.uint8), np.frombuffer(index, np.uint8)) + \
        open_want(data, index)


def flush_jobs(ora, rounds=ROUNDS):
    """sst.write_entries (vbf_sst_encode_host), then Table.open of the bytes it returned."""
    def job(i):
        arrays, want = flush_case(ora, i)
        return Job("flush", "table%d" % i, arrays, want, arrays[1].size - 1)
    return rotation([job(i) for i in range(len(FLUSH_SIZES))], 0, rounds)


# ---- lock order: one filter written, probed, read through and rebuilt at once ------------------

@functools.lru_cache(maxsize=None)
def lock_order_case(ora):
    """Table T = the first read table, filter F sized for T's keys and everything set later.
    -> dict: files of T, T's keys, the batches thread 1 sets into F (none of them a key of a read
    table), F's (m, k), F's words with T alone and with everything."""
    from velarixdb_amd.keys import pack_offsets
    _, files, parsed, _ = read_tables(ora)
    t_keys = sorted(parsed[0].starts)
    others = [[b"other-%02d-%05d" % (r, i) for i in range(4_000 + 37 * r)] for r in range(ROUNDS)]
    n = len(t_keys) + sum(len(b) for b in others)
    m = ora.num_bits(n, P)
    k = ora.num_hash(m, n)
    first = ora.build_words(_pack(t_keys), m, k)
    final = first.copy()
    for b in others:
        ora.build_words(_pack(b), m, k, final)
    keys, offs, *_ = ora.sst_decode(np.frombuffer(files[0][0], np.uint8))
    assert np.array_equal(ora.build_words(pack_offsets(keys, offs), m, k), first)  # a rebuild from T adds nothing
    return dict(files=files[0], t_keys=t_keys, others=others, n=n, m=m, k=k, first=first, final=final)


def lock_order_probe_jobs(ora, rounds=ROUNDS):
    """candidates() over the three read tables' ranges with F as the first table's filter.  F gains
    bits while the probes run: its column is bounded by F's words before and after (want[1], want[2]);
    the other two filters stand still and their columns are exact (want[0], F's column zeroed)."""
    _, files, parsed, pool = read_tables(ora)
    lo = lock_order_case(ora)
    rest = [rebuild_words(ora, i) for i in (1, 2)]
    bounds = [(min(s.starts), s.ikeys[-1]) for s in parsed]
    jobs = []
    for r, n in enumerate(rotation(PROBE_BATCHES, 0, rounds)):
        rng = np.random.default_rng(0x10C000 + r)
        queries = [pool[i] for i in rng.integers(0, len(pool), size=n)]
        batch = _pack(queries)
        inside = [np.asarray([a <= q <= b for q in queries]) for a, b in bounds]
        cols = [ins & ora.probe(batch, m, k, words).astype(bool)
                for ins, (m, k, words) in zip(inside, [(lo["m"], lo["k"], lo["first"])] + rest)]
        exact = np.stack(cols, axis=1).astype(np.uint8)
        after = (inside[0] & ora.probe(batch, lo["m"], lo["k"], lo["final"]).astype(bool)).astype(np.uint8)
        before = exact[:, 0].copy()
        exact[:, 0] = 0
        jobs.append(Job("lock_probe", "round%d/%d" % (r, n), (queries,), (exact, before, after), n))
    return jobs


@functools.lru_cache(maxsize=None)
def rebuild_words(ora, table):
    """(m, k, words) of BloomFilter::new(P, n) rebuilt from read table `table`."""
    from velarixdb_amd.keys import pack_offsets
    data = read_tables(ora)[1][table][0]
    keys, offs, *_ = ora.sst_decode(np.frombuffer(data, np.uint8))
    n = offs.size - 1
    m = ora.num_bits(n, P)
    k = ora.num_hash(m, n)
    return m, k, ora.build_words(pack_offsets(keys, offs), m, k)
