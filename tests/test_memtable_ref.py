"""The Python restatement of the memtable's semantics (tests/memtable_ref.py) against cases worked
out by hand.  CPU only."""
import numpy as np

import memtable_ref as ref


def test_prefix_pair_sorts_prefix_first():
    assert ref.sort_ids([b"ab", b"a"]).tolist() == [1, 0]
    assert ref.sort_ids([b"a\x00", b"a", b"a\x00\x00"]).tolist() == [1, 0, 2]


def test_bytes_are_unsigned():
    # 0x80 and 0xff sort after 0x7f (Rust u8, not i8)
    assert ref.sort_ids([b"\xff", b"\x80", b"\x7f", b"\x00"]).tolist() == [3, 2, 1, 0]
    assert ref.sort_ids([b"k\x80", b"k\x7f\xff"]).tolist() == [1, 0]


def test_empty_key_is_a_key_and_sorts_first():
    assert ref.sort_ids([b"b", b"", b"a"]).tolist() == [1, 2, 0]
    assert ref.sort_ids([b"", b"x", b""]).tolist() == [2, 1]


def test_threefold_duplicate_keeps_the_last_insert():
    keys = [b"k", b"a", b"k", b"z", b"k", b"a"]
    assert ref.sort_ids(keys).tolist() == [5, 4, 3]
    assert ref.sort_ids([]).size == 0 and ref.sort_ids([]).dtype == np.uint32


def test_insert_count_with_forced_collisions():
    """m = 64, k = 3, hashes chosen by hand: a key whose bits earlier keys cover is skipped and
    is not counted, though it was never set."""
    f = ref.FilterModel(64, 3)
    rows = [[1, 2, 3],            # new: bits 1 2 3
            [65, 130, 323],       # 1 2 3 again (mod 64): contained, skipped
            [1, 2, 4],            # bit 4 is clear: new
            [4, 3, 2],            # covered by two different keys: contained
            [5, 5, 5],            # one bit three times: new
            [1, 2, 3]]            # a repeat of the first key
    assert f.insert_many(rows) == 3
    assert f.bits == {1, 2, 3, 4, 5} and f.num_elements == 3
    assert f.words().tolist() == [0b111110, 0]
    # the same rows against a filter that already holds bits 1 2 4: only [5, 5, 5] and [1, 2, 3] are new
    g = ref.FilterModel.from_words(64, 3, np.array([0b10110, 0], np.uint32))
    assert g.bits == {1, 2, 4}
    assert g.insert_many(rows) == 2 and g.bits == {1, 2, 3, 4, 5}
    # k = 0: every key is contained
    assert ref.FilterModel(64, 0).insert_many([[], []]) == 0
