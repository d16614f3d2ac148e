"""The key-bytes axis on the CPU: the oracle pinned at the edge key lengths by a SipHash-1-3
written here with Python integers, and the library's host-resident filter (VBF_DEVICE_HOST: the
CPU SipHash of csrc/sip13.hpp) on the torture batches of tests/key_torture.py -- key lengths
0..4 097 B and 65 535 / 65 536 / 70 001 B interleaved, a nonzero first offset, both length-prefix
modes.  Every comparison is exact.  The GPU counterpart is tests/test_gpu_key_layouts.py."""
import os
import struct

import numpy as np
import pytest

import key_torture as kt
from conftest import ROOT

SEED = 0x5EED7001
MASK = (1 << 64) - 1


def _rotl(x, b):
    return ((x << b) | (x >> (64 - b))) & MASK


class PySip13:
    """SipHash-1-3 with a zero key (Aumasson & Bernstein; Rust's DefaultHasher), streaming, in
    arbitrary-precision ints.  Shares nothing with oracle.c or csrc/sip13.hpp."""

    def __init__(self):
        self.v = [0x736F6D6570736575, 0x646F72616E646F6D, 0x6C7967656E657261, 0x7465646279746573]
        self.tail = b""
        self.length = 0

    def copy(self):
        c = PySip13()
        c.v, c.tail, c.length = list(self.v), self.tail, self.length
        return c

    def _round(self):
        v0, v1, v2, v3 = self.v
        v0 = (v0 + v1) & MASK
        v1 = _rotl(v1, 13) ^ v0
        v0 = _rotl(v0, 32)
        v2 = (v2 + v3) & MASK
        v3 = _rotl(v3, 16) ^ v2
        v0 = (v0 + v3) & MASK
        v3 = _rotl(v3, 21) ^ v0
        v2 = (v2 + v1) & MASK
        v1 = _rotl(v1, 17) ^ v2
        v2 = _rotl(v2, 32)
        self.v = [v0, v1, v2, v3]

    def write(self, data):
        self.length += len(data)
        buf = self.tail + data
        full = len(buf) // 8 * 8
        for (m,) in struct.iter_unpack("<Q", buf[:full]):
            self.v[3] ^= m
            self._round()            # c = 1
            self.v[0] ^= m
        self.tail = buf[full:]
        return self

    def finish(self):
        s = self.copy()
        b = ((s.length & 0xFF) << 56) | int.from_bytes(s.tail, "little")
        s.v[3] ^= b
        s._round()
        s.v[0] ^= b
        s.v[2] ^= 0xFF
        for _ in range(3):           # d = 3
            s._round()
        return s.v[0] ^ s.v[1] ^ s.v[2] ^ s.v[3]


def py_hashes(key, lp, seeds):
    """calculate_hash (bf.rs:222-227): SipHash-1-3(LE64(len) || key || LE64(seed)), lp = 0 without the length"""
    pre = PySip13()
    if lp:
        pre.write(struct.pack("<Q", len(key)))
    pre.write(key)
    return [pre.copy().write(struct.pack("<Q", s)).finish() for s in seeds]


def test_py_siphash_known_vector():
    """The checker's checker: SipHash-1-3 of the empty message with a zero key (the golden set's
    first vector, tests/golden/siphash13_openssl.json)."""
    assert PySip13().finish() == 0xD1FBA762150C532C


def test_torture_batch_shape():
    """What the generators promise: the length mix, the long keys' places, lead bytes."""
    n = 20_011
    data, off = kt.torture_offsets_batch(SEED, n, lead=7)
    lens = np.diff(off).astype(np.int64)
    assert off[0] == 7 and (data[:7] == 0xA5).all() and off[-1] == data.size and lens.size == n
    assert (lens <= 41).sum() * 3 >= 2 * n and data.size < 12_000_000
    for L in kt.EDGE:
        assert (lens == L).sum() >= kt.EDGE_REPEATS, L
    assert lens[0] in kt.LONG and lens[-1] in kt.LONG and (np.isin(lens, kt.LONG)).sum() == 5
    assert set(lens[np.isin(lens, kt.LONG)].tolist()) == set(kt.LONG)
    keys = kt.torture_keys(SEED, n)
    have = set(keys)
    for L in kt.EDGE:
        assert b"\x00" * L in have and b"\xff" * L in have
    assert sum(1 for k in keys if len(k) and k[:-1] in have) >= len(kt.EDGE) - 1
    # interleaved: a 64-key window (one wave) holds short and long keys side by side
    win = lens[: n // 64 * 64].reshape(-1, 64)
    assert ((win.min(axis=1) <= 9) & (win.max(axis=1) >= 239)).mean() > 0.95
    d0, o0 = kt.torture_offsets_batch(SEED, n)
    assert np.array_equal(d0, data[7:]) and np.array_equal(o0 + np.uint64(7), off)  # deterministic
    uni = kt.ordered_universe()
    assert uni == sorted(set(uni)) and uni[0] == b"" and b"k\x00\x00" in uni


@pytest.mark.parametrize("lp", [1, 0])
def test_oracle_hashes_pinned_at_edge_lengths(ora, lp):
    """oracle.hashes against the pure-Python SipHash-1-3: one key of every EDGE length and the
    three long ones, seeds 0..18."""
    from velarixdb_amd.keys import HostBatch
    rng = np.random.default_rng(11 + lp)
    keys = [rng.bytes(L) for L in kt.EDGE + kt.LONG]
    data, off = kt.pack_lead(keys, lead=5)
    got = ora.hashes(HostBatch(data, off, 0, len(keys), lp), 19)
    for j, key in enumerate(keys):
        assert got[j].tolist() == py_hashes(key, lp, range(19)), len(key)
        assert ora.calc_hash(key, 18, lp) == int(got[j, 18])


def test_oracle_matches_openssl_at_wrap_lengths(ora):
    """The oracle against OpenSSL's SipHash-1-3 on messages of 230..270 B (the final block's
    length byte wraps at 256) and 4 090..4 100 B, when the openssl CLI with SIPHASH c-rounds /
    d-rounds parameters is present."""
    import random
    import shutil
    import subprocess
    import sys
    if not shutil.which("openssl"):
        pytest.skip("no openssl CLI")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from gen_openssl_pin import openssl_sip13
    try:
        openssl_sip13(b"probe")
    except (subprocess.CalledProcessError, ValueError):
        pytest.skip("openssl lacks SIPHASH c-rounds / d-rounds")
    rng = random.Random(20261019)
    for L in list(range(230, 271)) + list(range(4090, 4101)):
        msg = bytes(rng.randrange(256) for _ in range(L))
        want = openssl_sip13(msg)
        assert ora.siphash13(msg) == want == PySip13().write(msg).finish(), L


def _set_bits(words):
    """the set bits' indices of a word array, ascending"""
    nz = np.flatnonzero(words)
    bits = np.unpackbits(words[nz].view(np.uint8), bitorder="little").reshape(-1, 32).astype(bool)
    return (nz.astype(np.uint64)[:, None] * np.uint64(32) + np.arange(32, dtype=np.uint64))[bits]


@pytest.mark.parametrize("lp", [1, 0])
@pytest.mark.parametrize("m,k", [(1_000_003, 10), (9_815, 19), (4_294_967_295, 4)])
def test_host_filter_on_torture_batch(ora, m, k, lp):
    """A host-resident filter (the library's CPU SipHash, bf.rs:84-105): set_many of the torture
    batch gives the oracle's words, contains_many of positives + negatives the oracle's answers.
    lp = 1: an offsets batch whose first offset is 3; lp = 0: the keys as RawMessage."""
    from velarixdb_amd import HOST, BloomFilter
    from velarixdb_amd.keys import HostBatch, RawMessage, pack
    pos_keys, neg_keys = kt.torture_keys(SEED), kt.torture_negative_keys(SEED)
    if lp:
        pos = HostBatch(*kt.pack_lead(pos_keys, 3), 0, len(pos_keys), 1)
        both = HostBatch(*kt.pack_lead(pos_keys + neg_keys, 3), 0, len(pos_keys) + len(neg_keys), 1)
    else:
        pos = pack([RawMessage(x) for x in pos_keys])
        both = pack([RawMessage(x) for x in pos_keys + neg_keys])
        assert pos.len_prefix == 0 and pos.offsets is not None
    f = BloomFilter.sized(m, k, device=HOST)
    f.set_many(pos)
    assert f.no_of_elements == len(pos_keys)
    got = f.words()
    if m > 100_000_000:  # compare the set bits (512 MiB of words)
        assert np.array_equal(_set_bits(got), np.unique(ora.hashes(pos, k) % np.uint64(m)))
        want = got
    else:
        want = ora.build_words(pos, m, k)
        assert np.array_equal(got, want)
    ans = f.contains_many(both)
    assert np.array_equal(ans, ora.probe(both, m, k, want, threads=8).astype(bool))
    assert ans[: len(pos_keys)].all()
