"""Seeded, deterministic key batches for the key-bytes axis: edge lengths, interleaved lengths,
nonzero first offsets, odd strides and adversarial orderings.  Generators only -- the tests that
use them are tests/test_key_layouts_host.py (CPU) and tests/test_gpu_key_layouts.py (GPU).

Why these lengths.  SipHash's final block carries (message length & 0xff): with the 8-byte length
prefix and the 8-byte seed the byte wraps at a key of 240 B, without the prefix at 248 B.  The
partitioned build deals a tile's keys to lanes by min(len / 8, 31): every key of 248 B or more
shares the last bucket.  The absorb reads whole aligned 8-byte words and runs four blocks per
loop trip: lengths around every multiple of 8 up to 40, around 64 / 128 / 256 / 512 / 4096, and
the u16 boundary (65 535 / 65 536 / 70 001 B) are where it can go wrong.
"""
import functools

import numpy as np

EDGE = tuple(range(10)) + (15, 16, 17, 23, 24, 25, 31, 32, 33, 39, 40, 41, 63, 64, 65, 127, 128, 129,
                           239, 240, 241, 247, 248, 249, 255, 256, 257, 263, 264, 511, 512, 513,
                           4095, 4096, 4097)
LONG = (65_535, 65_536, 70_001)
SMALL = tuple(L for L in EDGE if L <= 41)
LARGE = tuple(L for L in EDGE if L > 41)
EDGE_REPEATS = 20       # every EDGE length occurs at least this often
SMALL_SHARE = 0.72      # of the freely drawn keys; keeps >= 2/3 of a batch at <= 41 B
STRIDES = (1, 2, 3, 5, 7, 9, 12, 15, 17, 20, 31, 33, 40, 48, 63, 64, 65, 100, 255, 256, 257)
STRIDE_ROWS = 6_000


def _long_slots(n):
    """index 0, index n - 1 and three interior indices, with the LONG lengths dealt round-robin"""
    idx = (0, n // 4, n // 2 + 1, (3 * n) // 4 + 2, n - 1)
    return {i: LONG[j % len(LONG)] for j, i in enumerate(idx)}


@functools.lru_cache(maxsize=8)
def _torture_keys(seed, n):
    """The batch as a tuple of bytes objects (cached: the same batch is placed in many ways)."""
    rng = np.random.default_rng([0x70C7, seed])
    slots = _long_slots(n)
    assert n >= 4 * len(EDGE) + EDGE_REPEATS * len(EDGE) + len(slots) + 100
    keys = []
    for L in EDGE:
        keys.append(b"\x00" * L)           # differ from their neighbours in length only
        keys.append(b"\xff" * L)
        r = rng.bytes(L)
        keys.append(r)                      # a truncation pair: the key and the key minus its last byte
        keys.append(r[:-1])
        keys.extend(rng.bytes(L) for _ in range(EDGE_REPEATS))
    free = n - len(slots) - len(keys)
    small = rng.random(free) < SMALL_SHARE
    lens = np.where(small, rng.choice(SMALL, free), rng.choice(LARGE, free))
    keys.extend(rng.bytes(int(L)) for L in lens)
    order = rng.permutation(len(keys))      # interleaved, not grouped
    keys = [keys[i] for i in order]
    for i in sorted(slots):                 # the long keys at their fixed places
        keys.insert(i, rng.bytes(slots[i]))
    assert len(keys) == n
    return tuple(keys)


def torture_keys(seed, n=20_011):
    return list(_torture_keys(seed, n))


def pack_lead(keys, lead=0):
    """keys -> (data, offsets) with `lead` bytes of 0xA5 first and offsets[0] = lead"""
    lens = np.fromiter((len(k) for k in keys), dtype=np.uint64, count=len(keys))
    offsets = np.empty(len(keys) + 1, dtype=np.uint64)
    offsets[0] = lead
    np.cumsum(lens, out=offsets[1:])
    offsets[1:] += np.uint64(lead)
    data = np.frombuffer(b"\xa5" * lead + b"".join(keys), dtype=np.uint8).copy()
    return data, offsets


def torture_offsets_batch(seed, n=20_011, lead=0):
    """(data, offsets): n keys with lengths from EDGE (each at least 20 times; at least two thirds of
    the keys at most 41 B), the LONG keys at index 0, n - 1 and three interior indices, an all-0x00
    key, an all-0xFF key and a truncation pair per EDGE length, lengths interleaved."""
    return pack_lead(_torture_keys(seed, n), lead)


@functools.lru_cache(maxsize=8)
def _negative_keys(seed, n):
    rng = np.random.default_rng([0x2E6A, seed])
    small = rng.random(n) < SMALL_SHARE
    lens = np.where(small, rng.choice(SMALL, n), rng.choice(LARGE, n))
    lens[0], lens[n - 1] = LONG[0], LONG[1]  # two long negatives of their own
    keys = [rng.bytes(int(L)) for L in lens]
    keys += [k + b"\x00" for k in _torture_keys(seed, n)]
    return tuple(keys)


def torture_negative_keys(seed, n=20_011):
    return list(_negative_keys(seed, n))


def torture_negatives(seed, n=20_011, lead=0):
    """(data, offsets): n keys of the same length mix and other bytes, then every key of
    torture_offsets_batch(seed, n) extended by one 0x00 byte (2n keys).  Not every one is absent
    from the positives (an all-0x00 key plus 0x00 is the next all-0x00 key): the oracle decides."""
    return pack_lead(_negative_keys(seed, n), lead)


def stride_rows(stride, rows=STRIDE_ROWS, seed=0x57D1):
    """rows x stride random bytes (one fixed-stride batch)"""
    return np.random.default_rng([seed, stride]).integers(0, 256, rows * stride, dtype=np.uint8)


@functools.lru_cache(maxsize=1)
def stride_batches():
    """((stride, uint8[STRIDE_ROWS * stride]), ...) for every stride of STRIDES"""
    return tuple((L, stride_rows(L)) for L in STRIDES)


D_STEMS = (b"stem-0123456789a", b"\x00" * 16, b"\xff" * 16, b"stem-012345678\x7f\x80")
D_TAILS = (b"", b"\x00", b"\x01", b"\x7f", b"\x80", b"\xff", b"\xff\x00")


@functools.lru_cache(maxsize=1)
def _universe():
    keys = set()
    for L in (6, 7, 8, 14, 15, 16, 22):     # A: long shared prefixes, first difference at every byte mod 8
        for i in range(600):
            keys.add(b"\x61" * L + bytes((i >> 8, i & 0xFF)))
    for i in range(41):                      # B: each a proper prefix of the next; the empty key
        keys.add(b"\xaa" * i)
    for i in range(21):                      # C: tie in the zero-padded 8-byte prefix
        keys.add(b"k" + b"\x00" * i)
    for stem in D_STEMS:                     # D: the last byte straddles the sign bit
        for tail in D_TAILS:
            keys.add(stem + tail)
    return tuple(sorted(keys))


def ordered_universe():
    """The adversarial ordering keys, sorted (Python bytes order = Rust `Ord for [u8]`), unique."""
    return list(_universe())
