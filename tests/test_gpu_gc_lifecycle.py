"""gc.collect_device inside the store's lifecycle (tests/store_model.py): for every scenario the GC's
chunk is collected in one device pass over the tables and the memtable filters the GPU produced, and
the result is held against the model's gc, against gc.collect on the same handles byte for byte, and
its puts, flushed, against the files of the model's apply_gc."""
import numpy as np
import pytest

import store_model as sm
from test_gpu_gc_collect import same_bytes
from test_gpu_store_lifecycle import Life, model
from test_gpu_vlog_recover_gc import same_gc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(sm.SCENARIOS))
def test_collect_device_in_the_lifecycle(vbf, ora, name):
    from velarixdb_amd import BloomFilter, Table, ValueLog, gc, memtable
    stores, _ = model(ora, name)
    s = stores[-1].clone()
    life = Life(vbf, name)
    tables = []
    try:
        gens = life.generations()
        log = life.log()
        tail, chunk = sm.gc_chunk([d["vo"] for d in gens], life.base)
        filters = [d["filter"] for d in gens]
        tables = [Table.open(d, i) for d, i in life.files()]
        with ValueLog.open(log, base=life.base) as vl:
            got = gc.collect_device(vl, tables, tail, chunk, life.base + len(log), sm.GC_NOW, filters=filters)
            host = gc.collect(vl, tables, tail, chunk, life.base + len(log), sm.GC_NOW, filters=filters)
            plain = gc.collect_device(vl, tables, tail, chunk, life.base + len(log), sm.GC_NOW)
        want = s.gc(tail, chunk)
        assert want is not None and want["invalid"] and len(want["append"]) > 1  # the chunk holds both kinds
        same_gc(got, want, s.log_size, sm.GC_NOW)
        same_bytes(got, host)
        same_bytes(plain, host)
        assert np.array_equal(plain.verdict, got.verdict)
        f = BloomFilter(sm.P, len(got.put_keys))
        res = memtable.flush(got.put_keys, got.put_val_offsets, got.put_created_ms, got.put_tombstones, filter=f)
        tab = s.apply_gc(want)
        assert res.data.tobytes() == tab.data and res.index.tobytes() == tab.index and np.array_equal(res.ids, tab.ids)
        assert np.array_equal(f.words(), tab.words)
    finally:
        for t in tables:
            t.close()
        life.close()
