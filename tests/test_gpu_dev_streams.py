"""Where the `_dev` entry points run: on the caller's stream, in stream order, one stream apart from
another (the stream contract of include/vbf.h, "Threads" and the `_dev` entries).

Every other parity test hands the library torch's current stream, the legacy default stream, which
orders itself against every blocking stream, and synchronises the device around the call.  A copy,
memset or kernel queued on stream 0 instead of the caller's, a size read back before the pass that
produces it is ordered, or scratch shared by two streams would pass all of them.

Here every call is made on one side stream of torch's pool while its inputs are still pending.  The
buffers the call is given hold a decoy (stream_cases.py: valid input of the same length with another
answer, checked on the CPU by test_stream_cases.py); the copy of the real input is queued on the
side stream behind a kernel that spins for SLEEP_CYCLES.  Per call:

  1. real inputs staged, live inputs = decoys, outputs = 0xA5 guard bytes; torch.cuda.synchronize(),
     the last device-wide synchronisation before the call (one more stands before the buffers are
     reset, so that a size query's queued passes are over)
  2. on the side stream: the spin, live <- real for every input, an event `armed`; on the legacy
     stream a spin three times as long, which nothing of the side stream waits for: whatever the
     library queues on stream 0 instead of the caller's stays behind it until after step 7
  3. `armed` has not happened: the inputs are still decoys (else the test fails and says so)
  4. the call, with the side stream's handle, without synchronising; where the protocol has a size
     query and a filling call, each is armed this way
  5. the sizes and return codes that came back are the real inputs'
  6. on the side stream: a clone of every output, guard bytes included; then the side stream alone is
     synchronised
  7. the clones equal the expectation byte for byte, guard bytes untouched
  8. torch.cuda.synchronize(), and the outputs still equal their clones: no write landed later from
     another stream

torch's pool streams are created with hipStreamNonBlocking, so the legacy stream does not order
itself against them; test_side_stream_is_non_blocking asserts it through hipStreamGetFlags of the HIP
runtime this process has loaded, when ctypes can reach it, and otherwise this is the assumption.

The entry points that promise an asynchronous return (vbf.h: "Calls are asynchronous on that
stream") and document no synchronisation are called once to warm the stream's workspace and then
armed: `armed` must still be pending when they return.

SLEEP_CYCLES is test_gpu_async.py's constant, about 17 ms of spinning; step 3 guards it.

The last part runs different streams from different threads, one `_dev` family per test, each
thread's sizes rotating, thread 0's first job behind the spin so that its synchronising call blocks
while the others complete whole calls."""
import contextlib
import ctypes
import threading
import time
import traceback

import numpy as np
import pytest

import host_call_cases as hc
import stream_cases as sc
import vlog_ref as vr
from test_gpu_async import SLEEP_CYCLES
from test_gpu_vlog import GUARD, PAD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEGACY_CYCLES = 3 * SLEEP_CYCLES  # the legacy stream's spin outlasts the side stream's and the call
CAP = 120.0  # seconds after the common start at which a thread still alive counts as hung
U64 = ctypes.c_uint64


# ---- the harness --------------------------------------------------------------------------------

_SIDE = []


def side_stream():
    """One side stream for the whole module: the library keeps a workspace per stream."""
    import torch
    if not _SIDE:
        _SIDE.append(torch.cuda.Stream(device=DEV))
    return _SIDE[0]


def _loaded_hip():
    """The HIP runtime this process has already loaded, or None."""
    try:
        with open("/proc/self/maps") as f:
            paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
        return ctypes.CDLL(paths[0]) if paths else None
    except OSError:
        return None


_STAGED = {}


def staged(case):
    """The case's real inputs and decoys as device tensors, uploaded once (on the legacy stream; the
    callers synchronise the device before they use them)."""
    import torch
    if id(case) not in _STAGED:
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)
        _STAGED[id(case)] = (case, {k: up(v) for k, v in case.real.items()}, {k: up(v) for k, v in case.decoy.items()})
    return _STAGED[id(case)][1:]


class Rig:
    """The buffers of one case on one stream.  threaded: a caller of the thread tests -- everything,
    the guard fill included, is queued on the thread's own stream, the inputs are copied without a
    decoy phase and nothing synchronises the device."""

    def __init__(self, side, case, threaded=False, spin=True):
        import torch
        self.torch, self.side, self.case, self.threaded, self.spin = torch, side, case, threaded, spin
        self.sp = ctypes.c_void_p(side.cuda_stream)
        self.real, self.decoy = staged(case)
        self.outs, self.live, self.sizes, self.cleanup, self.armed = {}, {}, {}, [], None
        with self.ctx():
            for name, t in self.real.items():
                if name in case.meta.get("inout", ()):
                    self.out(name, t.numel(), want=0)
                    self.live[name] = self.outs[name][0][PAD:PAD + t.numel()]
                else:
                    self.live[name] = torch.empty_like(t)

    def ctx(self):
        return self.torch.cuda.stream(self.side) if self.threaded else contextlib.nullcontext()

    def p(self, name):
        t = self.live.get(name)
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    def out(self, name, nbytes, want=None, rest="exact"):
        """An output of nbytes between guard bytes -> its pointer.  want: the index in case.want it is
        compared with.  rest: what lies behind the expected bytes when they are fewer than nbytes --
        "exact" (there are none), "guard" (untouched) or "any" (unspecified by vbf.h)."""
        with self.ctx():
            t = self.torch.full((PAD + nbytes + PAD,), GUARD, dtype=self.torch.uint8, device=DEV)
        self.outs[name] = (t, nbytes, want, rest)
        return ctypes.c_void_p(t.data_ptr() + PAD)

    def arm(self, spin=None):
        """Steps 1 to 3."""
        torch = self.torch
        spin = self.spin if spin is None else spin
        if not self.threaded:
            torch.cuda.synchronize()  # an earlier call's queued passes are over before the buffers are reset
            for t, *_ in self.outs.values():
                t.fill_(GUARD)
            for name, t in self.live.items():
                t.copy_(self.decoy[name])
            torch.cuda.synchronize()
            if spin:
                torch.cuda._sleep(LEGACY_CYCLES)
        with torch.cuda.stream(self.side):
            if spin:
                torch.cuda._sleep(SLEEP_CYCLES)
            for name, t in self.live.items():
                t.copy_(self.real[name], non_blocking=True)
            self.armed = torch.cuda.Event()
            self.armed.record()
        if spin:
            assert not self.armed.query(), \
                "the spin of %d cycles was over before the call: the inputs are no decoys any more" % SLEEP_CYCLES

    def launch(self, fn, asynchronous=False):
        """Steps 1 to 4 for one call -> its return code.  asynchronous: the entry point documents no
        synchronisation -- warmed with one call first, it must return while the spin still runs."""
        if asynchronous and not self.threaded:
            self.arm(spin=False)
            assert fn() == 0, self.error()
        self.arm()
        rc = fn()
        if asynchronous and self.spin and not self.threaded:
            assert not self.armed.query(), "%s waited for the stream" % self.case.call
        return rc

    def error(self):
        from velarixdb_amd._lib import lib
        return "%s %s: %s" % (self.case.call, self.case.ident, lib.vbf_last_error().decode(errors="replace"))

    def collect(self, tail=()):
        """Steps 6 to 8 -> (the outputs in case.want's order, then `tail`; the reported sizes; the
        outputs that changed after step 6).  tail: a callable from the outputs' host copies to further
        values, or the values."""
        torch = self.torch
        with torch.cuda.stream(self.side):
            snaps = {name: t.clone() for name, (t, *_) in self.outs.items()}
            host = {name: s.cpu().numpy() for name, s in snaps.items()}
        self.side.synchronize()
        got, bodies = {}, {}
        for name, (t, nbytes, want, rest) in self.outs.items():
            h = host[name]
            assert (h[:PAD] == GUARD).all() and (h[PAD + nbytes:] == GUARD).all(), \
                "%s %s: wrote outside %s" % (self.case.call, self.case.ident, name)
            bodies[name] = h[PAD:PAD + nbytes]
            if want is None:
                continue
            w = self.case.want[want]
            assert w.nbytes <= nbytes and (rest != "exact" or w.nbytes == nbytes), (name, w.nbytes, nbytes)
            if rest == "guard":
                assert (bodies[name][w.nbytes:] == GUARD).all(), "%s: written past the reported size" % name
            got[want] = bodies[name][:w.nbytes].copy().view(w.dtype).reshape(w.shape)
        late = []
        if not self.threaded:
            torch.cuda.synchronize()
            late = [name for name, (t, *_) in self.outs.items() if not torch.equal(t, snaps[name])]
        for fn in self.cleanup:
            fn()
        tail = tail(bodies) if callable(tail) else tail
        return tuple(got[i] for i in sorted(got)) + tuple(tail), dict(self.sizes), late


def verify(case, result):
    """Steps 5, 7 and 8 on what Rig.collect returned."""
    got, sizes, late = result
    where = "%s %s" % (case.call, case.ident)
    assert sizes == case.sizes, "%s: reported %r, the real input's sizes are %r (the decoy's %r)" % (
        where, sizes, case.sizes, case.decoy_sizes)
    assert len(got) == len(case.want), where
    for i, (g, w) in enumerate(zip(got, case.want)):
        if hc.blob(g) != hc.blob(w):
            detail = ""
            if isinstance(g, np.ndarray) and isinstance(w, np.ndarray) and g.shape == w.shape:
                bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
                detail = ": %d of %d items differ, first at %d" % (bad.size, g.size, bad[0] if bad.size else -1)
            if i < len(case.decoy_want) and hc.blob(g) == hc.blob(case.decoy_want[i]):
                detail += " -- it is the decoy's answer: an input was read before its copy"
            if late:
                detail += " -- %s changed after the caller's stream was drained" % ", ".join(late)
            raise AssertionError("%s: output %d differs from the expectation%s" % (where, i, detail))
    assert not late, "%s: %s changed after the caller's stream was drained: a write from another stream" % (
        where, ", ".join(late))


# ---- what the calls run on ----------------------------------------------------------------------

class Ctx:
    """Handles shared by the cases: the three read tables open on the device, the probe set's filters."""

    def __init__(self, vbf, ora):
        from test_gpu_table_get import handles, open_host
        self.vbf, self.ora = vbf, ora
        self.tables = [open_host(d, i) for d, i in hc.read_tables(ora)[1]]
        self.table_handles = handles(self.tables)
        self.filters, lo_hi = [], []
        for keys, m, k, words, lo, hi in hc.probe_set(ora, 0):
            f = vbf.BloomFilter.sized(m, k, hc.P)
            f.set_many(keys)
            assert np.array_equal(f.words(), words)
            self.filters.append(f)
            lo_hi += [lo, hi]
        self.filter_handles = handles([f._h for f in self.filters])
        self.bounds, self.bounds_off = sc._pack(lo_hi)

    def close(self):
        from velarixdb_amd._lib import lib
        for h in self.tables:
            lib.vbf_table_free(h)


@pytest.fixture(scope="module")
def ctx(vbf, ora):
    import torch
    c = Ctx(vbf, ora)
    yield c
    torch.cuda.synchronize()
    c.close()
    _STAGED.clear()


def _lib():
    from velarixdb_amd._lib import lib
    return lib


# ---- the entry points ---------------------------------------------------------------------------
# run_<call>(rig, ctx) makes the calls of one case and returns rig.collect(...)

def run_build(rig, ctx):
    m = rig.case.meta
    pw = rig.p("words") if m["inout"] else rig.out("words", 4 * ((m["m"] + 31) // 32), want=0)
    rc = rig.launch(lambda: _lib().vbf_build_dev_ex(rig.p("keys"), None, m["stride"], m["n"], 1, m["m"], m["k"], pw,
                                                    m["strategy"], rig.sp), asynchronous=True)
    assert rc == 0, rig.error()
    return rig.collect()


def run_probe(rig, ctx):
    m = rig.case.meta
    count = rig.case.call == "probe_count"
    po = rig.p("count") if count else rig.out("out", m["n"], want=0)
    fn = _lib().vbf_probe_count_dev_ex if count else _lib().vbf_probe_dev_ex
    rc = rig.launch(lambda: fn(rig.p("keys"), None, m["stride"], m["n"], 1, m["m"], m["k"], rig.p("words"), po,
                               m["strategy"], rig.sp), asynchronous=True)
    assert rc == 0, rig.error()
    return rig.collect()


def run_hashes(rig, ctx):
    m = rig.case.meta
    po = rig.out("out", 8 * m["n"] * m["k"], want=0)
    rc = rig.launch(lambda: _lib().vbf_hashes_dev(rig.p("keys"), rig.p("offsets"), 0, m["n"], 1, m["k"], po, rig.sp),
                    asynchronous=True)
    assert rc == 0, rig.error()
    return rig.collect()


def run_gen_var(rig, ctx):
    po = rig.out("out", rig.case.want[0].nbytes, want=0)
    rc = rig.launch(lambda: _lib().vbf_gen_var_dev(sc.GEN_SEED, sc.GEN_BASE, sc.GEN_N, rig.p("offsets"), po, rig.sp),
                    asynchronous=True)
    assert rc == 0, rig.error()
    return rig.collect()


def run_or_words(rig, ctx):
    rc = rig.launch(lambda: _lib().vbf_or_words_dev(rig.p("dst"), rig.p("src"), rig.case.meta["nwords"], rig.sp),
                    asynchronous=True)
    assert rc == 0, rig.error()
    return rig.collect()


def run_or_fold(rig, ctx):
    m = rig.case.meta
    po = rig.out("dst", 4 * m["nwords"], want=0)
    rc = rig.launch(lambda: _lib().vbf_or_fold_dev(po, rig.p("src"), m["nwords"], m["nparts"], m["part_stride"], rig.sp),
                    asynchronous=True)
    assert rc == 0, rig.error()
    return rig.collect()


def run_popcount(rig, ctx):
    rc = rig.launch(lambda: _lib().vbf_popcount_dev(rig.p("words"), rig.case.meta["nwords"], rig.p("count"), rig.sp),
                    asynchronous=True)
    assert rc == 0, rig.error()
    return rig.collect()


def run_multi_probe(rig, ctx):
    n = rig.case.meta["n"]
    po = rig.out("out", 3 * n, want=0)
    # not asynchronous: the filter table and the bounds go up from pageable host memory, and the call
    # synchronises the stream once to be done with them (vbf.h says so since this test found it)
    rc = rig.launch(lambda: _lib().vbf_multi_probe_dev(rig.p("keys"), rig.p("offsets"), 0, n, 1, 3, ctx.filter_handles,
                                                       ctx.bounds.ctypes.data, ctx.bounds_off.ctypes.data, po, rig.sp))
    assert rc == 0, rig.error()
    return rig.collect()


def run_decode(rig, ctx):
    c = rig.case
    n, cnt = c.meta["n"], U64(77)
    head = (rig.p("data"), c.real["data"].size, rig.p("blocks"), c.real["blocks"].size)
    rc = rig.launch(lambda: _lib().vbf_sst_decode_dev(*head, None, 0, None, None, None, None, 0, ctypes.byref(cnt), rig.sp))
    assert rc == 0 and cnt.value == n, (rig.error(), cnt.value, n)
    sizes = (c.want[0].size, 8 * (n + 1), 4 * n, 8 * n, n)
    p = [rig.out(name, s, want=i) for i, (name, s) in enumerate(zip(("keys", "offsets", "val", "created", "tomb"), sizes))]
    cnt = U64(77)
    rc = rig.launch(lambda: _lib().vbf_sst_decode_dev(*head, p[0], sizes[0], p[1], p[2], p[3], p[4], n + 1,
                                                      ctypes.byref(cnt), rig.sp))
    assert rc == 0, rig.error()
    rig.sizes = {"n_out": cnt.value}
    return rig.collect()


def run_encode(rig, ctx):
    c = rig.case
    m, want = c.meta, c.sizes
    head = (rig.p("keys"), rig.p("offsets"), m["stride"], m["n"], rig.p("val"), rig.p("created"), rig.p("tomb"))
    s = [U64(77), U64(77), U64(77)]
    B = [ctypes.byref(x) for x in s]
    rc = rig.launch(lambda: _lib().vbf_sst_encode_dev(*head, None, 0, B[0], None, 0, B[1], None, 0, B[2], rig.sp))
    assert rc == 0, rig.error()
    query = dict(zip(("data_len", "index_len", "nblocks"), (x.value for x in s)))
    assert query == want, "%s %s: the size query reported %r, not %r" % (c.call, c.ident, query, want)
    pd = rig.out("data", want["data_len"], want=0)
    pi = rig.out("index", want["index_len"], want=1)
    pb = rig.out("blocks", 4 * want["nblocks"], want=2)
    rc = rig.launch(lambda: _lib().vbf_sst_encode_dev(*head, pd, want["data_len"], B[0], pi, want["index_len"], B[1], pb,
                                                      want["nblocks"], B[2], rig.sp))
    assert rc == 0, rig.error()
    rig.sizes = dict(zip(("data_len", "index_len", "nblocks"), (x.value for x in s)))
    return rig.collect()


def run_rebuild(rig, ctx):
    c = rig.case
    f = ctx.vbf.BloomFilter(hc.P, c.meta["n"])
    assert (f.num_bits(), f.no_of_hash_func) == (c.meta["m"], c.meta["k"])
    got = []
    rig.arm()
    got.append(f.rebuild_from_sst_dev(rig.p("data"), c.real["data"].size, rig.p("blocks"), c.real["blocks"].size, rig.sp))
    rig.sizes = {"n_out": got[0]}
    return rig.collect(lambda bodies: (f.words(),))  # a host call on the filter waits for its last operation


def run_gather(rig, ctx):
    c = rig.case
    n, kb = c.meta["n"], U64(77)
    sizes = (c.sizes["key_bytes"], 8 * (n + 1), 8 * n, n, 4 * n)
    p = [rig.out(name, s, want=i) for i, (name, s) in enumerate(zip(("keys", "offsets", "created", "tomb", "val"), sizes))]
    rc = rig.launch(lambda: _lib().vbf_gather_entries_dev(
        rig.p("keys"), rig.p("offsets"), rig.p("created"), rig.p("tomb"), rig.p("val"), rig.p("ids"), n, p[0], sizes[0],
        p[1], p[2], p[3], p[4], ctypes.byref(kb), rig.sp))
    assert rc == 0, rig.error()
    rig.sizes = {"key_bytes": kb.value}
    return rig.collect()


def run_merge(rig, ctx):
    from test_gpu_compaction_shapes import _apply
    c = rig.case
    m, total = c.meta, c.meta["total"]
    pi = rig.out("ids", 4 * total, want=0, rest="guard")
    pu, pt = rig.out("upd_ids", 4 * total), rig.out("upd_time", 8 * total)
    n, nu = U64(7), U64(7)
    rc = rig.launch(lambda: _lib().vbf_compact_merge_dev(
        rig.p("keys"), rig.p("offsets"), rig.p("created"), rig.p("tomb"), m["run_off"].ctypes.data, m["run_off"].size - 1,
        rig.p("map_keys"), rig.p("map_off"), rig.p("map_time"), m["map_n"], *m["ttl"], pi, ctypes.byref(n), pu, pt,
        ctypes.byref(nu), rig.sp))
    assert rc == 0, rig.error()
    rig.sizes = {"n_out": n.value}

    def new_map(bodies):
        ui, ut = bodies["upd_ids"].view(np.uint32)[:nu.value], bodies["upd_time"].view(np.int64)[:nu.value]
        return (_apply(m["start"], c.real["keys"], c.real["offsets"], ui.tolist(), ut.tolist()),)
    return rig.collect(new_map)


def _key_range(h):
    lib = _lib()
    sl, bl = U64(), U64()
    assert lib.vbf_table_key_range(h, None, 0, ctypes.byref(sl), None, 0, ctypes.byref(bl)) == 0
    s, b = ctypes.create_string_buffer(max(1, sl.value)), ctypes.create_string_buffer(max(1, bl.value))
    assert lib.vbf_table_key_range(h, s, sl.value, ctypes.byref(sl), b, bl.value, ctypes.byref(bl)) == 0
    return s.raw[:sl.value], b.raw[:bl.value]


def run_open(rig, ctx):
    c = rig.case
    h = ctypes.c_void_p()
    rc = rig.launch(lambda: _lib().vbf_table_open_dev(rig.p("data"), c.real["data"].size, rig.p("index"), c.real["index"].size,
                                                      rig.p("blocks"), c.real["blocks"].size, rig.sp, ctypes.byref(h)))
    assert rc == 0 and h.value, rig.error()
    rig.cleanup.append(lambda: _lib().vbf_table_free(h))
    tail = (_lib().vbf_table_entries(h), _lib().vbf_table_blocks(h)) + _key_range(h)
    return rig.collect(tail)


def run_table_get(rig, ctx):
    n = rig.case.meta["n"]
    p = [rig.out(name, s, want=i) for i, (name, s) in enumerate(zip(("found", "table_idx", "val", "created"),
                                                                    (n, 4 * n, 4 * n, 8 * n)))]
    rc = rig.launch(lambda: _lib().vbf_table_get_dev(rig.p("keys"), rig.p("offsets"), 0, n, 3, ctx.table_handles,
                                                     rig.p("cand"), *p, rig.sp))
    assert rc == 0, rig.error()
    return rig.collect()


def run_table_scan(rig, ctx):
    from test_gpu_table_scan import NAMES7, sizes_of
    c = rig.case
    m, want = c.meta, c.sizes
    head = (rig.p("bounds"), rig.p("bounds_off"), m["nranges"], 3, ctx.table_handles, m["flags"])
    n, kb = U64(77), U64(77)
    rc = rig.launch(lambda: _lib().vbf_table_scan_dev(*head, None, None, 0, None, None, None, None, None, 0,
                                                      ctypes.byref(n), ctypes.byref(kb), rig.sp))
    assert rc == 0, rig.error()
    query = {"n_out": n.value, "key_bytes": kb.value}
    assert query == want, "%s %s: the size query reported %r, not %r" % (c.call, c.ident, query, want)
    sz = sizes_of(m["nranges"], want["n_out"], want["key_bytes"])
    p = [rig.out(name, s, want=i) for i, (name, s) in enumerate(zip(NAMES7, sz))]
    rc = rig.launch(lambda: _lib().vbf_table_scan_dev(*head, p[0], p[1], want["key_bytes"], p[2], p[3], p[4], p[5], p[6],
                                                      want["n_out"], ctypes.byref(n), ctypes.byref(kb), rig.sp))
    assert rc == 0, rig.error()
    rig.sizes = {"n_out": n.value, "key_bytes": kb.value}
    return rig.collect()


def _open_vlog(rig):
    """vbf_vlog_open_dev borrows the live log while it still holds the decoy: open parses nothing."""
    c = rig.case
    h = ctypes.c_void_p()
    rc = _lib().vbf_vlog_open_dev(rig.p("log"), c.real["log"].size, c.meta.get("base", 0), ctypes.byref(h))
    assert rc == 0 and h.value, rig.error()
    rig.cleanup.append(lambda: _lib().vbf_vlog_free(h))
    return h


def run_vlog_get(rig, ctx):
    c = rig.case
    n, want = c.meta["n"], c.sizes["value_bytes"]
    h = _open_vlog(rig)
    head = (h, rig.p("val_offsets"), rig.p("found"), n, rig.p("keys"), rig.p("offsets"), 0)
    ps, po = rig.out("status", n, want=0), rig.out("value_off", 8 * (n + 1), want=2)
    vb = U64(77)
    rc = rig.launch(lambda: _lib().vbf_vlog_get_dev(*head, ps, None, 0, po, ctypes.byref(vb), rig.sp))
    assert rc == 0 and vb.value == want, (rig.error(), vb.value, want)
    pv = rig.out("values", want, want=1)
    vb = U64(77)
    rc = rig.launch(lambda: _lib().vbf_vlog_get_dev(*head, ps, pv, want, po, ctypes.byref(vb), rig.sp))
    assert rc == 0, rig.error()
    rig.sizes = {"value_bytes": vb.value}
    return rig.collect()


def run_vlog_encode(rig, ctx):
    c = rig.case
    n, want = c.meta["n"], c.sizes["out_len"]
    head = (rig.p("keys"), rig.p("offsets"), 0, n, rig.p("values"), rig.p("value_off"), rig.p("created"), rig.p("tomb"),
            c.meta["base"])
    ln = U64(77)
    rc = rig.launch(lambda: _lib().vbf_vlog_encode_dev(*head, None, 0, ctypes.byref(ln), None, rig.sp))
    assert rc == 0 and ln.value == want, (rig.error(), ln.value, want)
    po, pv = rig.out("out", want, want=0), rig.out("val_offsets", 4 * n, want=1)
    ln = U64(77)
    rc = rig.launch(lambda: _lib().vbf_vlog_encode_dev(*head, po, want, ctypes.byref(ln), pv, rig.sp))
    assert rc == 0, rig.error()
    rig.sizes = {"out_len": ln.value}
    return rig.collect()


def run_vlog_walk(rig, ctx):
    from test_gpu_vlog_walk import NAMES, _args, _scalars, _sizes
    c = rig.case
    h = _open_vlog(rig)
    names = ("n_out", "key_bytes", "value_bytes", "end_off", "stop")
    s = _scalars()
    rc = rig.launch(lambda: _lib().vbf_vlog_walk_dev(*_args(h, c.meta["start"], c.meta["budget"], [None] * 8, (0, 0, 0), s),
                                                     rig.sp))
    query = dict(zip(names, (x.value for x in s)))
    assert rc == 0 and query == c.sizes, (rig.error(), query, c.sizes)
    n, kb, vb = (c.sizes[x] for x in names[:3])
    p = [rig.out(name, size, want=i) for i, (name, size) in enumerate(zip(NAMES, _sizes(n, kb, vb)))]
    s = _scalars()
    rc = rig.launch(lambda: _lib().vbf_vlog_walk_dev(*_args(h, c.meta["start"], c.meta["budget"], p, (kb, vb, n), s), rig.sp))
    assert rc == 0, rig.error()
    rig.sizes = dict(zip(names, (x.value for x in s)))
    return rig.collect()


def run_sort(rig, ctx):
    n, cnt = rig.case.meta["n"], U64(77)
    po = rig.out("ids", 4 * n, want=0, rest="any")
    rc = rig.launch(lambda: _lib().vbf_memtable_sort_dev(rig.p("keys"), rig.p("offsets"), 0, n, po, ctypes.byref(cnt), rig.sp))
    assert rc == 0, rig.error()
    rig.sizes = {"n_out": cnt.value}
    return rig.collect()


def run_insert(rig, ctx):
    m = rig.case.meta
    f = ctx.vbf.BloomFilter.sized(m["m"], m["k"], 1e-3)
    fresh = U64(77)
    rc = rig.launch(lambda: _lib().vbf_filter_insert_dev(f._h, rig.p("keys"), rig.p("offsets"), 0, m["n"], 1,
                                                         ctypes.byref(fresh), rig.sp))
    assert rc == 0, rig.error()
    rig.sizes = {"n_new": fresh.value}
    return rig.collect(lambda bodies: (f.words(),))


RUN = {"build": run_build, "probe": run_probe, "probe_count": run_probe, "hashes": run_hashes, "gen_var": run_gen_var,
       "or_words": run_or_words, "or_fold": run_or_fold, "popcount": run_popcount, "multi_probe": run_multi_probe,
       "decode": run_decode, "encode": run_encode, "rebuild": run_rebuild, "gather": run_gather, "merge": run_merge,
       "open": run_open, "table_get": run_table_get, "table_scan": run_table_scan, "vlog_get": run_vlog_get,
       "vlog_encode": run_vlog_encode, "vlog_walk": run_vlog_walk, "sort": run_sort, "insert": run_insert}


# ---- 1. one stream, inputs pending --------------------------------------------------------------

def test_side_stream_is_non_blocking(vbf):
    hip = _loaded_hip()
    if hip is None or not hasattr(hip, "hipStreamGetFlags"):
        print("the loaded HIP runtime is not reachable: the side stream is assumed non-blocking")
        return  # the module docstring states the assumption
    flags = ctypes.c_uint(0xFFFF)
    rc = hip.hipStreamGetFlags(ctypes.c_void_p(side_stream().cuda_stream), ctypes.byref(flags))
    print("hipStreamGetFlags of the side stream: %#x" % flags.value)
    assert rc == 0 and flags.value & 1, "torch's side stream is a blocking one (flags %#x): nothing here proves anything" % flags.value


@pytest.mark.parametrize("family", list(sc.FAMILIES))
def test_inputs_pending_on_a_side_stream(ctx, family):
    t0 = time.perf_counter()
    cases = sc.FAMILIES[family](ctx.ora)
    for case in cases:
        verify(case, RUN[case.call](Rig(side_stream(), case), ctx))
    print("%s: %d cases in %.2f s" % (family, len(cases), time.perf_counter() - t0))


def test_gen_fixed_returns_before_the_stream(ctx):
    """vbf_gen_fixed_dev has no device input: its output must come after the spin, in stream order,
    and the call must not wait for it."""
    import torch
    side = side_stream()
    n, L = sc.GEN_N, sc.GEN_L
    out = torch.full((PAD + n * L + PAD,), GUARD, dtype=torch.uint8, device=DEV)
    sp, po = ctypes.c_void_p(side.cuda_stream), ctypes.c_void_p(out.data_ptr() + PAD)
    assert _lib().vbf_gen_fixed_dev(sc.GEN_SEED, sc.GEN_BASE, n, L, po, sp) == 0  # warms the stream
    side.synchronize()
    out.fill_(GUARD)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(SLEEP_CYCLES)
        armed = torch.cuda.Event()
        armed.record()
    assert not armed.query(), "the spin of %d cycles was over before the call" % SLEEP_CYCLES
    assert _lib().vbf_gen_fixed_dev(sc.GEN_SEED, sc.GEN_BASE, n, L, po, sp) == 0
    assert not armed.query(), "vbf_gen_fixed_dev waited for the stream"
    early = out.cpu().numpy()  # the legacy stream does not wait for a non-blocking one
    assert not armed.query() and (early == GUARD).all(), "written before the spin ended: not queued on the stream"
    with torch.cuda.stream(side):
        got = out.clone().cpu().numpy()
    side.synchronize()
    assert (got[:PAD] == GUARD).all() and (got[PAD + n * L:] == GUARD).all()
    assert np.array_equal(got[PAD:PAD + n * L], ctx.ora.gen_fixed(sc.GEN_SEED, sc.GEN_BASE, n, L))
    torch.cuda.synchronize()


# ---- 2. the chain -------------------------------------------------------------------------------

def test_put_then_get_chain_on_the_side_stream(ctx):
    """test_put_then_get_chain_on_one_stream of test_gpu_vlog.py on the side stream, the puts pending
    behind the spin: encode the log -> encode the SST from its val_offsets -> open both -> get ->
    fetch.  Nothing of the test's own synchronises between the first call and the end."""
    import torch
    from test_gpu_vlog import T0, _down, _out, _up, pack_keys
    call, lib = ctx.vbf._lib.call, _lib()
    side = side_stream()
    sp = ctypes.c_void_p(side.cuda_stream)
    rng = np.random.default_rng(0xC4A1)
    keys = sorted({rng.bytes(int(rng.integers(1, 40))) for _ in range(3000)})
    n = len(keys)
    values = [rng.bytes(int(rng.integers(0, 700))) for _ in range(n)]
    tomb = (np.arange(n) % 11 == 0).astype(np.uint8)
    created = (T0 + np.arange(n)).astype(np.int64)
    base = 4321
    kb, koff = pack_keys(keys)
    vb, voff = pack_keys(values)
    ask = keys[::2] + [k + b"\0absent" for k in keys[:100]]
    m = len(ask)
    qb, qoff = pack_keys(ask)
    real = [_up(a)[0] for a in (kb, koff, vb, voff, created, tomb, qb, qoff)]
    live = [torch.zeros_like(t) for t in real]  # decoys: empty keys, empty values, zero fields
    torch.cuda.synchronize()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    pk, pko, pv, pvo, pcr, ptb, pq, pqo = [P(t) for t in live]
    ht, hv = ctypes.c_void_p(), ctypes.c_void_p()
    with torch.cuda.stream(side):  # every buffer below is filled on the side stream too
        torch.cuda._sleep(SLEEP_CYCLES)
        for t, r in zip(live, real):
            t.copy_(r, non_blocking=True)
        armed = torch.cuda.Event()
        armed.record()
        assert not armed.query(), "the spin of %d cycles was over before the chain began" % SLEEP_CYCLES
        try:
            ln = ctypes.c_uint64()
            call("vbf_vlog_encode_dev", pk, pko, 0, n, pv, pvo, pcr, ptb, base, None, 0, ctypes.byref(ln), None, sp)
            t_log = torch.zeros(ln.value, dtype=torch.uint8, device=DEV)
            t_vo = torch.zeros(n, dtype=torch.int32, device=DEV)
            call("vbf_vlog_encode_dev", pk, pko, 0, n, pv, pvo, pcr, ptb, base, P(t_log), ln.value, ctypes.byref(ln),
                 P(t_vo), sp)
            dl, il, nb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
            S = (ctypes.byref(dl), ctypes.byref(il), ctypes.byref(nb))
            call("vbf_sst_encode_dev", pk, pko, 0, n, P(t_vo), pcr, ptb, None, 0, S[0], None, 0, S[1], None, 0, S[2], sp)
            td = torch.zeros(dl.value, dtype=torch.uint8, device=DEV)
            ti = torch.zeros(il.value, dtype=torch.uint8, device=DEV)
            tblk = torch.zeros(nb.value, dtype=torch.int32, device=DEV)
            call("vbf_sst_encode_dev", pk, pko, 0, n, P(t_vo), pcr, ptb, P(td), dl.value, S[0], P(ti), il.value, S[1],
                 P(tblk), nb.value, S[2], sp)
            call("vbf_table_open_dev", P(td), dl.value, P(ti), il.value, P(tblk), nb.value, sp, ctypes.byref(ht))
            call("vbf_vlog_open_dev", P(t_log), ln.value, base, ctypes.byref(hv))
            t_found = torch.zeros(m, dtype=torch.uint8, device=DEV)
            t_val = torch.zeros(m, dtype=torch.int32, device=DEV)
            th = (ctypes.c_void_p * 1)(ht.value)
            call("vbf_table_get_dev", pq, pqo, 0, m, 1, th, None, P(t_found), None, P(t_val), None, sp)
            ts, ps = _out(m)
            to, po = _out((m + 1) * 8)
            tot = ctypes.c_uint64()
            call("vbf_vlog_get_dev", hv, P(t_val), P(t_found), m, pq, pqo, 0, ps, None, 0, po, ctypes.byref(tot), sp)
            tv, pvv = _out(tot.value)
            call("vbf_vlog_get_dev", hv, P(t_val), P(t_found), m, pq, pqo, 0, ps, pvv, tot.value, po, ctypes.byref(tot), sp)
            side.synchronize()  # the one synchronisation of the chain
            status, voff_out = _down(ts, m, np.uint8), _down(to, (m + 1) * 8, np.uint64)
            vals = _down(tv, tot.value, np.uint8).tobytes()
            got_log, got_vo = t_log.cpu().numpy().tobytes(), t_vo.cpu().numpy().view(np.uint32).tolist()
        finally:
            side.synchronize()
            if ht.value:
                lib.vbf_table_free(ht)
            if hv.value:
                lib.vbf_vlog_free(hv)
    at = {k: j for j, k in enumerate(keys)}
    for j, k in enumerate(ask):
        got = vals[int(voff_out[j]):int(voff_out[j + 1])]
        if k not in at or tomb[at[k]]:
            assert status[j] == vr.SKIPPED and got == b""  # absent, or found == 2: the table says tombstone
        else:
            assert status[j] == vr.VALUE and got == values[at[k]], j
    want, woffs = vr.encode(list(zip(keys, values, created.tolist(), tomb.tolist())), base)
    assert got_log == want and got_vo == woffs
    torch.cuda.synchronize()


# ---- 3. different streams from different threads ------------------------------------------------

def run_stream_threads(per_thread, ctx):
    """One daemon thread and one side stream per case list, behind a barrier; thread 0's first case
    waits behind the spin.  Each thread synchronises only its own stream.  Joined with the cap, then
    checked on this thread: nobody hung, nobody raised, every pair overlapped, every output is right."""
    import torch
    n = len(per_thread)
    assert 2 <= n <= 4
    for jobs in per_thread:
        for case in jobs:
            staged(case)
    torch.cuda.synchronize()
    sides = [torch.cuda.Stream(device=DEV) for _ in range(n)]
    barrier = threading.Barrier(n + 1)
    state = [dict(at="the barrier", out=[], err=None, t0=None, t1=None, first=None) for _ in range(n)]

    def body(i):
        st = state[i]
        try:
            barrier.wait(CAP)
            st["t0"] = time.monotonic()
            for r, case in enumerate(per_thread[i]):
                st["at"] = "%s %s" % (case.call, case.ident)
                st["out"].append(RUN[case.call](Rig(sides[i], case, threaded=True, spin=(i == 0 and r == 0)), ctx))
                if r == 0:
                    st["first"] = time.monotonic()
            st["at"] = None
        except BaseException:
            st["err"] = traceback.format_exc()
        finally:
            st["t1"] = time.monotonic()

    threads = [threading.Thread(target=body, args=(i,), daemon=True, name="stream-%d" % i) for i in range(n)]
    for th in threads:
        th.start()
    barrier.wait(CAP)
    start = time.monotonic()
    for th in threads:
        th.join(max(0.0, start + CAP - time.monotonic()))
    hung = ["thread %d in %s" % (i, state[i]["at"]) for i, th in enumerate(threads) if th.is_alive()]
    if hung:
        pytest.exit("still inside a call %d s after the common start: %s" % (CAP, "; ".join(hung)), returncode=1)
    torch.cuda.synchronize()
    for i, st in enumerate(state):
        assert st["err"] is None, "thread %d raised in %s:\n%s" % (i, st["at"], st["err"])
    for a in range(n):
        for b in range(a + 1, n):
            shared = min(state[a]["t1"], state[b]["t1"]) - max(state[a]["t0"], state[b]["t0"])
            assert shared > 0, "threads %d and %d never ran at the same time" % (a, b)
    print("threads: %s" % ", ".join("%d cases in %.3f s" % (len(j), st["t1"] - st["t0"]) for j, st in zip(per_thread, state)))
    for jobs, st in zip(per_thread, state):
        assert len(st["out"]) == len(jobs)
        for case, got in zip(jobs, st["out"]):
            verify(case, got)


@pytest.mark.parametrize("family", sc.THREAD_FAMILIES)
def test_different_streams_from_different_threads(ctx, family):
    """tables: vbf_table_get_dev + vbf_table_scan_dev over shared open tables; sst: vbf_sst_encode_dev +
    vbf_sst_decode_dev; vlog: vbf_vlog_get_dev + vbf_vlog_encode_dev; memtable: vbf_memtable_sort_dev;
    build_probe: vbf_build_dev_ex(PARTITIONED) + vbf_probe_dev_ex(2), the kWsBuild and kWsProbe slots of
    each stream's workspace."""
    run_stream_threads(sc.thread_jobs(ctx.ora, family), ctx)
