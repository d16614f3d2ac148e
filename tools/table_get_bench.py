"""Table lookup timing, beside bench.py and with its conventions: a clock
settle, W untimed warm-up steps, then K steps timed with device events around each call.

  python tools/table_get_bench.py [--tables 8] [--entries 1000000] [--queries 4000000] [--steps 20] [--warmup 3]

One process, everything device-resident, one JSON line:
  T tables of N sorted 16-byte keys (two big-endian copies of a counter: table t holds the even
  values 2 (j T + t), so the tables are disjoint and sorted by construction), encoded with
  vbf_sst_encode_dev and opened with vbf_table_open_dev on those very buffers (open wall time, with
  its synchronisations, and the library's phase times);
  Q random queries over [0, 2 N T) -- about half of them hit -- through vbf_table_get_dev with
  cand = NULL, with cand from vbf_multi_probe_dev (the tables' filters and key ranges; the probe
  timed apart and together), gets/s each;
  the checker of tests/sst_get_ref.py (the reference's linear scans, in Python) on a few of the same
  queries for about --cpu-seconds: its gets/s, and the GPU's answers for them compared.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import velarixdb_amd as vbf  # noqa: E402
from velarixdb_amd._lib import call, lib, profile_read  # noqa: E402

from sst_write_bench import timed, vp  # noqa: E402


def be16(v):
    """int64 tensor -> [n, 16] bytes: the value big-endian, twice."""
    be = v.view(torch.uint8).view(-1, 8).flip(1)
    return torch.cat([be, be], dim=1).contiguous()


class DevTable:
    def __init__(self, t, T, N, dev, sp):
        j = torch.arange(N, device=dev, dtype=torch.int64)
        self.keys = be16(2 * (j * T + t)).reshape(-1)
        self.val = j.to(torch.int32)
        self.cr = 1720785462000 + j * T + t
        self.tb = (j % 97 == 0).to(torch.uint8)
        dl, il, nb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        S = (ctypes.byref(dl), ctypes.byref(il), ctypes.byref(nb))
        a = (vp(self.keys), None, 16, N, vp(self.val), vp(self.cr), vp(self.tb))
        call("vbf_sst_encode_dev", *a, None, 0, S[0], None, 0, S[1], None, 0, S[2], sp)
        self.data = torch.empty(dl.value, dtype=torch.uint8, device=dev)
        self.index = torch.empty(il.value, dtype=torch.uint8, device=dev)
        self.blocks = torch.empty(nb.value, dtype=torch.int32, device=dev)
        call("vbf_sst_encode_dev", *a, vp(self.data), dl.value, S[0], vp(self.index), il.value, S[1], vp(self.blocks),
             nb.value, S[2], sp)
        self.sp = sp
        self.h = None

    def open(self):
        h = ctypes.c_void_p()
        call("vbf_table_open_dev", vp(self.data), self.data.numel(), vp(self.index), self.index.numel(),
             vp(self.blocks), self.blocks.numel(), self.sp, ctypes.byref(h))
        return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, default=8)
    ap.add_argument("--entries", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=4_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-seconds", type=float, default=3.0)
    args = ap.parse_args()
    assert torch.cuda.is_available() and vbf.device_count() > 0, "needs an MI355X: there is no CPU path"
    dev = torch.device("cuda:0")
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    T, N, Q = args.tables, args.entries, args.queries
    tabs = [DevTable(t, T, N, dev, sp) for t in range(T)]
    res = {"workload": "%d tables x %d x 16B keys, %d queries" % (T, N, Q), "steps": args.steps,
           "warmup": args.warmup, "data_len": tabs[0].data.numel(), "nblocks": tabs[0].blocks.numel()}

    # open: wall time per table (two synchronisations and the key-range readback included)
    tabs[0].h = tabs[0].open()
    lib.vbf_table_free(tabs[0].h)
    torch.cuda.synchronize()
    lib.vbf_profile_enable(1)
    profile_read()
    walls = []
    for tb in tabs:
        t0 = time.perf_counter()
        tb.h = tb.open()
        walls.append((time.perf_counter() - t0) * 1e3)
    lib.vbf_profile_enable(0)
    res["open_ms_per_table"] = {"mean": round(sum(walls) / T, 3), "min": round(min(walls), 3), "max": round(max(walls), 3),
                                "phase_ms_per_launch": {p: round(ms / c, 4) for p, (ms, c) in profile_read().items() if c}}
    assert all(lib.vbf_table_entries(tb.h) == N for tb in tabs)
    handles = (ctypes.c_void_p * T)(*[tb.h.value for tb in tabs])

    g = torch.Generator(device=dev)
    g.manual_seed(11)
    qv = torch.randint(0, 2 * N * T, (Q,), device=dev, generator=g)
    qk = be16(qv).reshape(-1)
    found = torch.empty(Q, dtype=torch.uint8, device=dev)
    idx = torch.empty(Q, dtype=torch.int32, device=dev)
    val = torch.empty(Q, dtype=torch.int32, device=dev)
    cr = torch.empty(Q, dtype=torch.int64, device=dev)

    def get(cand=None):
        call("vbf_table_get_dev", vp(qk), None, 16, Q, T, handles, vp(cand), vp(found), vp(idx), vp(val), vp(cr), sp)

    r = timed(get, args.steps, args.warmup)
    r["gets_per_s"] = round(Q / r["ms_per_step"] * 1e3)
    res["get_all_tables"] = r
    torch.cuda.synchronize()
    hits = found != 0
    res["hit_fraction"] = round(float(hits.float().mean()), 4)
    want_idx = torch.where(qv % 2 == 0, (qv // 2) % T, torch.full_like(qv, -1)).to(torch.int32)
    assert torch.equal(idx, want_idx) and torch.equal(hits, qv % 2 == 0), "lookup answers differ from the construction"
    assert torch.equal(cr[hits], 1720785462000 + qv[hits] // 2)
    first = [t.clone() for t in (found, idx, val, cr)]

    # the same behind the filters: cand from vbf_multi_probe_dev with the tables' key ranges
    filters = []
    for tb in tabs:
        f = vbf.BloomFilter(0.01, N)
        f.set_dev(vp(tb.keys), None, 16, N, 1, sp)
        filters.append(f)
    fh = (ctypes.c_void_p * T)(*[f._h.value for f in filters])
    bounds, boff = b"", [0]
    for tb in tabs:
        sl, bl = ctypes.c_uint64(), ctypes.c_uint64()
        s, b = np.zeros(16, np.uint8), np.zeros(16, np.uint8)
        call("vbf_table_key_range", tb.h, s.ctypes.data, 16, ctypes.byref(sl), b.ctypes.data, 16, ctypes.byref(bl))
        for x in (s, b):
            bounds += x.tobytes()
            boff.append(len(bounds))
    bounds, boff = np.frombuffer(bounds, np.uint8), np.asarray(boff, np.uint64)
    cand = torch.empty(Q * T, dtype=torch.uint8, device=dev)

    def probe():
        call("vbf_multi_probe_dev", vp(qk), None, 16, Q, 1, T, fh, bounds.ctypes.data, boff.ctypes.data, vp(cand), sp)

    def both():
        probe()
        get(cand)

    res["multi_probe"] = timed(probe, args.steps, args.warmup)
    r = timed(lambda: get(cand), args.steps, args.warmup)
    r["gets_per_s"] = round(Q / r["ms_per_step"] * 1e3)
    res["get_with_cand"] = r
    r = timed(both, args.steps, args.warmup)
    r["gets_per_s"] = round(Q / r["ms_per_step"] * 1e3)
    res["probe_then_get"] = r
    torch.cuda.synchronize()
    res["cand_fraction"] = round(float((cand != 0).float().mean()), 4)
    assert all(torch.equal(a, b) for a, b in zip(first, (found, idx, val, cr))), "cand changed an answer"

    # the reference's scans in Python on a few of these queries
    import sst_get_ref as ref
    files = [(tb.data.cpu().numpy().tobytes(), tb.index.cpu().numpy().tobytes()) for tb in tabs]
    qh, hf, hi, hv, hc = (x.cpu().numpy() for x in (qk.view(-1, 16), found, idx, val, cr))
    t0, done = time.perf_counter(), 0
    while done < Q and (done < 2 or time.perf_counter() - t0 < args.cpu_seconds):
        w = ref.search(qh[done].tobytes(), files)
        got = (int(hf[done]), int(hi[done]) & 0xFFFFFFFF, int(hv[done]) & 0xFFFFFFFF, int(hc[done]))
        assert got == w, (done, got, w)
        done += 1
    dt = time.perf_counter() - t0
    res["python_checker"] = {"queries": done, "gets_per_s": round(done / dt, 2), "answers_equal": True}
    for tb in tabs:
        lib.vbf_table_free(tb.h)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
