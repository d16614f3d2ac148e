"""SST encoder timing, beside bench.py and with its conventions: a clock
settle, W untimed warm-up steps, then K steps timed with device events around each call
(every encode through offsets includes its one size readback, as every decode does its count).

  python tools/sst_write_bench.py [--keys 100000000] [--steps 20] [--warmup 3] [--no-compact]

One process, device-resident inputs, one JSON line per section:
  encode   100M x 16-byte keys through the offsets layout (the general path: segmentation + scan +
           index.db + data.db), the same through the fixed stride (closed-form blocks), and on the
           file the encoder just wrote: vbf_sst_decode_dev (the yardstick: the same bytes the
           other way) and a device-to-device copy of data_len bytes
  zipf     config 3's key lengths (8..128 bytes, Zipf 1.1), as many keys as keep data.db < 2^32
  compact  bench.py --compact's bucket (4 tables x keys/4, half of each also in another table):
           merge + gather + filter build, and the same with the three per-entry arrays gathered
           and the files encoded (the device part of vbf_compact_write_host); the difference is
           what the files cost.  Then one vbf_compact_write_host call from host arrays (wall time).
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

import torch  # noqa: E402

import velarixdb_amd as vbf  # noqa: E402
from velarixdb_amd import workloads as wl  # noqa: E402
from velarixdb_amd._lib import call, lib, profile_read  # noqa: E402


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def timed(step, steps, warmup):
    """bench.py's timed_steps for one GPU: ms per step (device events), library phase times."""
    t0 = time.perf_counter()
    while True:
        step()
        torch.cuda.synchronize()
        if time.perf_counter() - t0 > 0.3:
            break
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    lib.vbf_profile_enable(1)
    profile_read()
    evs = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    lib.vbf_profile_enable(0)
    ph = {p: round(ms / n, 4) for p, (ms, n) in profile_read().items() if n}
    ms = sorted(a.elapsed_time(b) for a, b in evs)
    return {"ms_per_step": round(sum(ms) / len(ms), 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
            "phase_ms_per_launch": ph}


class Encoder:
    """vbf_sst_encode_dev on device tensors, outputs sized by the all-NULL query."""

    def __init__(self, keys, offs, stride, n, val, cr, tb, sp):
        self.args = (vp(keys), vp(offs), stride, n, vp(val), vp(cr), vp(tb))
        self.sp = sp
        self.dl, self.il, self.nb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self.sizes = (ctypes.byref(self.dl), ctypes.byref(self.il), ctypes.byref(self.nb))
        call("vbf_sst_encode_dev", *self.args, None, 0, self.sizes[0], None, 0, self.sizes[1], None, 0, self.sizes[2], sp)
        dev = (keys if keys is not None else val).device
        self.data = torch.empty(self.dl.value, dtype=torch.uint8, device=dev)
        self.index = torch.empty(self.il.value, dtype=torch.uint8, device=dev)
        self.blocks = torch.empty(self.nb.value, dtype=torch.int32, device=dev)

    def __call__(self):
        call("vbf_sst_encode_dev", *self.args, vp(self.data), self.data.numel(), self.sizes[0], vp(self.index),
             self.index.numel(), self.sizes[1], vp(self.blocks), self.blocks.numel(), self.sizes[2], self.sp)


def per_entry_arrays(n, dev):
    j = torch.arange(n, device=dev, dtype=torch.int64)
    return j.to(torch.int32), 1720785462000 + j, (j % 97 == 0).to(torch.uint8)


def bench_encode(args, dev, sp):
    n, L = args.keys, 16
    keys = torch.empty(n * L, dtype=torch.uint8, device=dev)
    call("vbf_gen_fixed_dev", wl.SEED_CFG2, 0, n, L, vp(keys), sp)
    offs = torch.arange(n + 1, device=dev, dtype=torch.int64) * L
    val, cr, tb = per_entry_arrays(n, dev)
    general = Encoder(keys, offs, 0, n, val, cr, tb, sp)
    res = {"section": "encode", "workload": "%dM x 16B keys" % (n // 10**6), "steps": args.steps, "warmup": args.warmup}
    res["encode_offsets"] = timed(general, args.steps, args.warmup)
    fixed = Encoder(keys, None, L, n, val, cr, tb, sp)
    res["encode_stride"] = timed(fixed, args.steps, args.warmup)
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in ((general.data, fixed.data), (general.index, fixed.index),
                                              (general.blocks, fixed.blocks)))
    # the generator's data.db (the decoder benchmark's input) is this file too
    ref = torch.empty_like(general.data)
    refb = torch.empty_like(general.blocks)
    call("vbf_gen_sst_fixed_dev", wl.SEED_CFG2, 0, n, L, vp(ref), vp(refb), sp)
    torch.cuda.synchronize()
    res["outputs_equal_stride_path"] = bool(same)
    res["outputs_equal_generator"] = bool(torch.equal(ref, general.data) and torch.equal(refb, general.blocks))
    del ref, refb, fixed
    out_k = torch.empty(n * L, dtype=torch.uint8, device=dev)
    out_o = torch.empty(n + 1, dtype=torch.int64, device=dev)
    got = ctypes.c_uint64()
    data, blocks = general.data, general.blocks

    def decode():
        call("vbf_sst_decode_dev", vp(data), data.numel(), vp(blocks), blocks.numel(), vp(out_k), out_k.numel(),
             vp(out_o), None, None, None, n + 1, ctypes.byref(got), sp)

    res["decode_same_file"] = timed(decode, args.steps, args.warmup)
    assert got.value == n and torch.equal(out_k, keys)
    dst = torch.empty_like(data)
    res["d2d_copy_data_len"] = timed(lambda: dst.copy_(data), args.steps, args.warmup)
    res["data_len"], res["index_len"], res["nblocks"] = general.dl.value, general.il.value, general.nb.value
    res["encode_over_decode"] = round(res["encode_offsets"]["ms_per_step"] / res["decode_same_file"]["ms_per_step"], 3)
    return res


def bench_zipf(args, dev, sp):
    n = min(args.keys, 80_000_000)  # mean entry ~42.9 bytes: data.db must stay below 2^32
    off_h = wl.var_offsets(wl.SEED_CFG3, 0, n)
    offs = torch.from_numpy(off_h.view(np.int64)).to(dev)
    keys = torch.empty(int(off_h[-1]), dtype=torch.uint8, device=dev)
    call("vbf_gen_var_dev", wl.SEED_CFG3, 0, n, vp(offs), vp(keys), sp)
    val, cr, tb = per_entry_arrays(n, dev)
    enc = Encoder(keys, offs, 0, n, val, cr, tb, sp)
    res = {"section": "zipf", "workload": "%dM keys, config 3 lengths (8..128 B, Zipf 1.1), %.2f GB of keys"
           % (n // 10**6, off_h[-1] / 1e9), "steps": args.steps, "warmup": args.warmup}
    res["encode_offsets"] = timed(enc, args.steps, args.warmup)
    out_k = torch.empty_like(keys)
    out_o = torch.empty(n + 1, dtype=torch.int64, device=dev)
    got = ctypes.c_uint64()

    def decode():
        call("vbf_sst_decode_dev", vp(enc.data), enc.data.numel(), vp(enc.blocks), enc.blocks.numel(), vp(out_k),
             out_k.numel(), vp(out_o), None, None, None, n + 1, ctypes.byref(got), sp)

    res["decode_same_file"] = timed(decode, args.steps, args.warmup)
    assert got.value == n and torch.equal(out_k, keys) and torch.equal(out_o, offs)
    res["data_len"], res["index_len"], res["nblocks"] = enc.dl.value, enc.il.value, enc.nb.value
    return res


def bench_compact(args, dev, sp):
    nr, per, L = 4, args.keys // 4, 16
    j = torch.arange(per, device=dev, dtype=torch.int64)
    ks, crs, tbs = [], [], []
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    for r in range(nr):  # bench.py --compact's bucket
        v = 2 * j + (r % 2) + (per * (r // 2))
        be = v.view(torch.uint8).view(-1, 8).flip(1)
        ks.append(torch.cat([be, be], dim=1).reshape(-1))
        crs.append(torch.randint(0, 1 << 40, (per,), device=dev, generator=g))
        tbs.append((torch.rand(per, device=dev, generator=g) < 0.05).to(torch.uint8))
    keys, created, tomb = torch.cat(ks), torch.cat(crs), torch.cat(tbs)
    del ks, crs, tbs, j
    total = nr * per
    val = torch.arange(total, device=dev, dtype=torch.int32)
    offs = torch.arange(total + 1, device=dev, dtype=torch.int64) * L
    run_off = np.arange(nr + 1, dtype=np.uint64) * per
    ids = torch.empty(total, dtype=torch.int32, device=dev)
    mk = torch.empty(total * L, dtype=torch.uint8, device=dev)
    mo = torch.empty(total + 1, dtype=torch.int64, device=dev)
    mc = torch.empty(total, dtype=torch.int64, device=dev)
    mt = torch.empty(total, dtype=torch.uint8, device=dev)
    mv = torch.empty(total, dtype=torch.int32, device=dev)
    data = torch.empty(total * (L + 17), dtype=torch.uint8, device=dev)
    index = torch.empty(total * (L + 8), dtype=torch.uint8, device=dev)
    n, nu, kb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    dl, il, nb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()

    def merge():
        call("vbf_compact_merge_dev", vp(keys), vp(offs), vp(created), vp(tomb), run_off.ctypes.data, nr,
             None, None, None, 0, 0, 0, 10**15, 1 << 41, vp(ids), ctypes.byref(n), None, None, ctypes.byref(nu), sp)

    merge()
    bf = vbf.BloomFilter(1e-4, max(n.value, 1))

    def parent():  # what bench.py --compact times: merge + gather of the keys + build
        merge()
        call("vbf_gather_entries_dev", vp(keys), vp(offs), None, None, None, vp(ids), n.value, vp(mk), mk.numel(),
             vp(mo), None, None, None, ctypes.byref(kb), sp)
        bf.set_dev(vp(mk), None, L, n.value, 1, sp)

    def fused():  # vbf_compact_write_host's device part: every array gathered, the files, the build
        merge()
        call("vbf_gather_entries_dev", vp(keys), vp(offs), vp(created), vp(tomb), vp(val), vp(ids), n.value, vp(mk),
             mk.numel(), vp(mo), vp(mc), vp(mt), vp(mv), ctypes.byref(kb), sp)
        call("vbf_sst_encode_dev", vp(mk), vp(mo), 0, n.value, vp(mv), vp(mc), vp(mt), vp(data), data.numel(),
             ctypes.byref(dl), vp(index), index.numel(), ctypes.byref(il), None, 0, ctypes.byref(nb), sp)
        bf.set_dev(vp(mk), vp(mo), 0, n.value, 1, sp)

    res = {"section": "compact", "workload": "bucket of %d tables x %dM x 16B keys" % (nr, per // 10**6),
           "steps": args.steps, "warmup": args.warmup}
    res["merge_gather_build"] = timed(parent, args.steps, args.warmup)
    res["merge_gather_encode_build"] = timed(fused, args.steps, args.warmup)
    res["merged_entries"], res["data_len"], res["index_len"] = n.value, dl.value, il.value
    res["files_cost_ms"] = round(res["merge_gather_encode_build"]["ms_per_step"]
                                 - res["merge_gather_build"]["ms_per_step"], 4)
    # the host entry point once, arena in host memory (uploads and downloads included)
    hk, ho, hc, ht, hv = (x.cpu().numpy() for x in (keys, offs, created, tomb, val))
    del mk, mo, mc, mt, mv, data, index, ids
    torch.cuda.empty_cache()
    hd = np.empty(total * (L + 17), np.uint8)
    hi = np.empty(total * (L + 8), np.uint8)
    h = ctypes.c_void_p()
    lib.vbf_profile_enable(1)
    profile_read()
    walls = []
    for _ in range(2):
        t0 = time.perf_counter()
        call("vbf_compact_write_host", hk.ctypes.data, ho.ctypes.data, hc.ctypes.data, ht.ctypes.data,
             run_off.ctypes.data, nr, None, None, None, 0, 0, 0, 10**15, 1 << 41, hv.ctypes.data, 1e-4,
             ctypes.byref(h), hd.ctypes.data, hd.size, ctypes.byref(dl), hi.ctypes.data, hi.size, ctypes.byref(il),
             ctypes.byref(n), None, None, None, 0)
        walls.append(round((time.perf_counter() - t0) * 1e3, 1))
        lib.vbf_filter_free(h)
    lib.vbf_profile_enable(0)
    res["compact_write_host"] = {"wall_ms": walls, "merged_entries": n.value, "data_len": dl.value,
                                 "phase_ms_per_launch": {p: round(ms / c, 4) for p, (ms, c) in profile_read().items() if c}}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-compact", action="store_true")
    ap.add_argument("--no-zipf", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available() and vbf.device_count() > 0, "needs an MI355X: there is no CPU path"
    dev = torch.device("cuda:0")
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for section in (bench_encode, None if args.no_zipf else bench_zipf, None if args.no_compact else bench_compact):
        if section is None:
            continue
        print(json.dumps(section(args, dev, sp)), flush=True)
        torch.cuda.empty_cache()
        lib.vbf_release_workspaces()


if __name__ == "__main__":
    main()
