"""The memtable's two semantics restated in Python -- the reference the GPU tests compare with.

MemTable::insert (memtable/mem.rs:207-221) is `if !contains(key) { set(key) }` on the filter and
SkipMap::insert on the entries.  crossbeam-skiplist 0.1.3 removes an entry of the same key before
it inserts, so the last insert of a key wins; the map iterates in ascending `Ord for [u8]` order,
which is Python's bytes order.
"""
import numpy as np


def sort_ids(keys):
    """ids of the entries a SkipMap holds after insert(keys[j]) for j = 0..n-1, in key order."""
    last = {}
    for j, k in enumerate(keys):
        last[bytes(k)] = j
    return np.asarray([last[k] for k in sorted(last)], dtype=np.uint32)


class FilterModel:
    """A Bloom filter as a Python set of bit indices: bf.rs:84-105 with `hash % m`."""

    def __init__(self, m, k, bits=()):
        self.m, self.k = m, k
        self.bits = set(bits)
        self.num_elements = 0

    @classmethod
    def from_words(cls, m, k, words):
        w = np.asarray(words, dtype=np.uint32)
        idx = np.flatnonzero(np.unpackbits(w.view(np.uint8), bitorder="little")[:m])
        return cls(m, k, (int(i) for i in idx))

    def key_bits(self, hashes):
        return [int(h) % self.m for h in hashes]

    def insert_many(self, hash_rows):
        """mem.rs:209-211 over the batch in order; hash_rows[j] = the k hashes of key j
        (oracle.hashes).  Returns the number of sets that ran."""
        fresh = 0
        for row in hash_rows:
            b = self.key_bits(row[:self.k])
            if all(x in self.bits for x in b):  # k == 0: vacuously contained (bf.rs:104)
                continue
            self.bits.update(b)
            fresh += 1
        self.num_elements = (self.num_elements + fresh) & 0xFFFFFFFF
        return fresh

    def words(self):
        w = np.zeros((self.m + 31) // 32, dtype=np.uint32)
        for b in self.bits:
            w[b >> 5] |= np.uint32(1 << (b & 31))
        return w


def insert_model(ora, batch, m, k, words=None):
    """The model run over a HostBatch against prior `words` -> (FilterModel, n_new)."""
    f = FilterModel(m, k) if words is None else FilterModel.from_words(m, k, words)
    rows = ora.hashes(batch, k) if k else np.zeros((batch.n, 0), np.uint64)
    return f, f.insert_many(rows)
