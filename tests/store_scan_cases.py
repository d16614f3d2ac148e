"""Ranges for the whole-store scan tests over the worlds of tests/store_get_cases.py
(tests/test_store_scan_ref.py on the CPU pins what tests/test_gpu_store_scan.py relies on).
Generators only."""
import numpy as np

import store_get_cases as cases

MAIN = (300, 5000, (2049, 1, 4097))   # the main world: gc, active, read-only sizes
TRUTH = (40, 40, (40, 40, 40))        # every layer holds every row of the truth table it is named in
FULL = (b"", b"\xff" * 301)           # every key of every world and fixture lies inside
PRESENT = cases.ROW_KEYS["gc_live"]
ABSENT = cases.STEM + b"no-such-key"
STEM = cases.STEM

# One of each kind the bounds pass can get wrong; the flags apply to the whole call, so lo == hi on a
# present key is also the lo == hi case of END_EXCLUSIVE.
EDGES = [
    FULL,
    (PRESENT, PRESENT),                 # lo == hi on a present key
    (ABSENT, ABSENT),                   # lo == hi on an absent key
    (b"z", b"a"),                       # lo > hi
    (STEM + b"ro", STEM + b"gc"),       # lo > hi past the 8-byte prefix
    (b"", STEM + b"gc_log_none"),       # a zero-length lo
    (b"", b""),                         # the zero-length key alone
    (b"k\0", b"k\0\0"),                 # the trailing-zero family
    (b"k\0\0", b"k\0\0"),
    (b"k", b"k\0"),
    (b"k\0\0", b"k\0\0\0\0"),
    (STEM + b"a", STEM + b"h"),         # bounds that share 17 bytes with the keys next to them
    (STEM + b"gc", STEM + b"gc_log\xff"),
    (STEM + b"gc_log_bad_hi", STEM + b"gc_log_bad_lo"),
    (STEM + b"ro_time", STEM + b"sst_tomc"),
    (STEM[:-1] + b"#000100", STEM[:-1] + b"#000400\0\0"),
    (STEM[:8], STEM[:8] + b"\xff"),     # bounds of exactly the prefix length
]


def ranges(keys, count=300, seed=0x5CA9):
    """`count` ranges over the sorted key list `keys`: EDGES, every truth-table row's key as lo == hi,
    then random cuts of 0 .. 300 keys whose bounds are keys, keys + b"\\0" or shortened keys."""
    out = (EDGES + [(k, k) for k in cases.ROW_KEYS.values()])[:count]
    rng = np.random.default_rng(seed)
    while len(out) < count:
        i = int(rng.integers(0, len(keys)))
        j = min(len(keys) - 1, i + int(rng.integers(0, 300)))
        lo, hi = keys[i], keys[j]
        kind = int(rng.integers(0, 4))
        if kind == 1:
            lo, hi = lo + b"\0", hi + b"\0"
        elif kind == 2:
            lo, hi = lo[:-1], hi[:-1]
        out.append((lo, hi))
    return out
