"""Pins the lookup checker (tests/sst_get_ref.py) on the reference's own seven fixture SSTs, and
the properties of those files that the GPU tests rely on (no GPU needed)."""
import functools
import os

import numpy as np

import sst_get_ref as ref
from conftest import GOLDEN

SST = os.path.join(GOLDEN, "sst_fixtures")
NAMES = sorted(os.listdir(SST))
SAMPLE = 37  # every SAMPLE-th query is also answered by the literal scans


def read(name):
    with open(os.path.join(SST, name, "data.db"), "rb") as f:
        data = f.read()
    with open(os.path.join(SST, name, "index.db"), "rb") as f:
        index = f.read()
    return data, index


@functools.lru_cache(maxsize=1)
def fixtures(ora):
    """[(data, index, Sst, [keys], val, created, tomb)] per fixture, decoded by the oracle."""
    out = []
    for name in NAMES:
        data, index = read(name)
        keys, offs, val, cr, tb = ora.sst_decode(np.frombuffer(data, np.uint8))
        kl = [keys[int(offs[j]):int(offs[j + 1])].tobytes() for j in range(offs.size - 1)]
        out.append((data, index, ref.Sst(data, index), kl, val, cr, tb))
    return out


def test_every_key_is_found_in_its_own_table(ora):
    for data, index, sst, keys, val, cr, tb in fixtures(ora):
        for j, k in enumerate(keys):
            want = (int(val[j]), int(cr[j]), bool(tb[j] == 1))
            assert sst.get(k) == want
            if j % SAMPLE == 0:
                assert ref.table_get(data, index, k) == want


def test_absent_keys_are_none(ora):
    zz = [b"zz%05d" % i for i in range(5000)]
    for data, index, sst, keys, *_ in fixtures(ora):
        have = set(keys)
        for j, q in enumerate([k + b"\0" for k in keys] + [k[:-1] for k in keys] + zz):
            assert q not in have
            assert sst.get(q) is None
            if j % (SAMPLE * 8) == 0:  # a miss scans to the end of the file
                assert ref.table_get(data, index, q) is None


def test_parsed_form_equals_the_scans_step_by_step(ora):
    data, index, sst, keys, *_ = fixtures(ora)[0]
    for q in keys[::SAMPLE] + [b"", b"\xff" * 40, keys[0][:-1], keys[-1] + b"\0"]:
        off = ref.get_from_index(index, q)
        assert sst.get_from_index(q) == off
        if off is not None:
            assert sst.find_entry(off, q) == ref.find_entry(data, off, q)
    assert ref.get_from_index(index, keys[-1] + b"\0") is None  # block_offset is never reassigned


def test_fold_returns_the_latest_holder(ora):
    fx = fixtures(ora)
    holders = {}
    for t, (_, _, _, keys, _, cr, _) in enumerate(fx):
        for j, k in enumerate(keys):
            holders.setdefault(k, []).append((t, int(cr[j])))
    assert len(holders) == 19908
    twice = {k: h for k, h in holders.items() if len(h) > 1}
    assert len(twice) == 1
    (key, h), = twice.items()
    # the one key that lives in more than one table lives in all seven, at seven different times
    assert len(h) == len(fx) and len({c for _, c in h}) == len(h)
    late = max(h, key=lambda x: x[1])
    ssts = [f[2] for f in fx]
    found, who, val, created = ref.search(key, ssts)
    assert (found, who, created) == (1, late[0], late[1])
    assert ref.search(key, [(f[0], f[1]) for f in fx]) == (found, who, val, created)  # the literal scans
    assert ref.search(key, ssts[::-1])[1] == len(fx) - 1 - late[0]
    second = sorted(h, key=lambda x: x[1])[-2]
    allowed = [t != late[0] for t in range(len(fx))]
    assert ref.search(key, ssts, allowed)[1] == second[0]
    assert ref.search(b"zz00000", ssts) == (0, ref.NO_TABLE, 0, 0)


def test_fixtures_pass_the_open_time_validation(ora):
    """Strictly increasing keys, index record b = (last key, start) of block b, blocks <= 4096 bytes,
    no tombstone and no created_at of 0: the tie, tombstone and zero-time cases need generated tables."""
    biggest = 0
    for data, index, sst, keys, val, cr, tb in fixtures(ora):
        assert all(a < b for a, b in zip(keys, keys[1:]))
        assert not tb.any() and (cr != 0).all()
        starts = sorted(sst.fields)
        assert sst.ioffs[0] == 0 and sst.ioffs == sorted(set(sst.ioffs)) and set(sst.ioffs) <= set(starts)
        ends = sst.ioffs[1:] + [len(data)]
        for b, (s, e) in enumerate(zip(sst.ioffs, ends)):
            biggest = max(biggest, e - s)
            last = max(p for p in starts[np.searchsorted(starts, s):np.searchsorted(starts, e)])
            klen = ref._u32(data, last)
            assert data[last + 4:last + 4 + klen] == sst.ikeys[b]
            assert last + klen + 17 == e
    assert biggest == 4092
