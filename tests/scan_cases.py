"""Tables and ranges shared by the range-scan tests (tests/test_sst_scan_ref.py on the CPU,
tests/test_gpu_table_scan.py on the GPU).  Tables are written with the oracle's encoder."""
import os

import numpy as np

from conftest import GOLDEN

SST = os.path.join(GOLDEN, "sst_fixtures")
NAMES = sorted(os.listdir(SST))
T0 = 1720785462000
FULL = (b"", b"\xff" * 8)  # every fixture key and every generated key lies inside


def write(ora, items):
    """items: [(key, value offset, created_at ms, tombstone byte)] in file order -> (data, index)
    bytes as Table::write_to_file lays them out."""
    keys = np.frombuffer(b"".join(k for k, *_ in items) or b"\0", np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(k) for k, *_ in items])]).astype(np.uint64)
    data, index = ora.sst_write(keys, offs, np.array([v for _, v, _, _ in items], np.uint32),
                                np.array([c for _, _, c, _ in items], np.uint64),
                                np.array([t for *_, t in items], np.uint8))
    return data.tobytes(), index.tobytes()


def read_fixture(name):
    with open(os.path.join(SST, name, "data.db"), "rb") as f:
        data = f.read()
    with open(os.path.join(SST, name, "index.db"), "rb") as f:
        index = f.read()
    return data, index


# The hand-written case: three tables, (key, value offset, created_at, tombstone).
#   b  a tie between tables 0 and 1 (table 2 older)      c  only a time-0 copy: absent
#   d  a tombstone in table 2 over an older live entry   f  a time-0 copy beside a live one
#   g  a tombstone alone                                 a, e, h  one live copy each
HAND = (
    [(b"a", 1, 100, 0), (b"b", 2, 200, 0), (b"c", 3, 0, 0), (b"d", 4, 300, 0), (b"e", 5, 150, 0)],
    [(b"b", 12, 200, 0), (b"f", 15, 0, 0), (b"h", 17, 70, 0)],
    [(b"b", 22, 199, 0), (b"d", 24, 400, 1), (b"f", 25, 5, 0), (b"g", 26, 50, 1)],
)
# (lo, hi, flags, table order) -> the expected list, written out by hand
HAND_EXPECT = [
    (b"", b"\xff", 0, (0, 1, 2),
     [(b"a", 0, 1, 100, 0), (b"b", 0, 2, 200, 0), (b"e", 0, 5, 150, 0), (b"f", 2, 25, 5, 0), (b"h", 1, 17, 70, 0)]),
    (b"", b"\xff", 1, (0, 1, 2),
     [(b"a", 0, 1, 100, 0), (b"b", 0, 2, 200, 0), (b"d", 2, 24, 400, 1), (b"e", 0, 5, 150, 0), (b"f", 2, 25, 5, 0),
      (b"g", 2, 26, 50, 1), (b"h", 1, 17, 70, 0)]),
    (b"b", b"f", 0, (0, 1, 2), [(b"b", 0, 2, 200, 0), (b"e", 0, 5, 150, 0), (b"f", 2, 25, 5, 0)]),
    (b"b", b"f", 2, (0, 1, 2), [(b"b", 0, 2, 200, 0), (b"e", 0, 5, 150, 0)]),
    (b"b", b"f", 3, (0, 1, 2), [(b"b", 0, 2, 200, 0), (b"d", 2, 24, 400, 1), (b"e", 0, 5, 150, 0)]),
    # the tie goes to whichever of its two tables is listed first
    (b"", b"\xff", 0, (2, 1, 0),
     [(b"a", 2, 1, 100, 0), (b"b", 1, 12, 200, 0), (b"e", 2, 5, 150, 0), (b"f", 0, 25, 5, 0), (b"h", 1, 17, 70, 0)]),
    (b"c", b"d", 1, (0, 1), [(b"d", 0, 4, 300, 0)]),   # without table 2 the live d shows; c stays absent
    (b"c", b"c", 1, (0, 1, 2), []),
    (b"h", b"a", 1, (0, 1, 2), []),                    # lo > hi
    (b"e", b"e", 0, (0, 1, 2), [(b"e", 0, 5, 150, 0)]),
    (b"e", b"e", 2, (0, 1, 2), []),                    # lo == hi, exclusive
]


def hand_files(ora):
    return [write(ora, list(items)) for items in HAND]


def fold(copies):
    """The independent statement of the winner rule: copies = [(created, table, val, tomb)] in table
    order -> the winner, or None.  The winner starts at time 0; only a strictly newer copy replaces it."""
    best = None
    for c in copies:
        if c[0] > (best[0] if best else 0):
            best = c
    return best


def expected(holders, lo, hi, flags):
    """holders: {key: [(created, table, val, tomb), ...] in table order} -> the scan of [lo, hi]."""
    out = []
    for k in sorted(holders):
        if not (lo <= k and (k < hi if flags & 2 else k <= hi)):
            continue
        w = fold(holders[k])
        if w is None or (w[3] == 1 and not flags & 1):
            continue
        out.append((k, w[1], w[2], w[0], 1 if w[3] == 1 else 0))
    return out
