"""CPU checks of stream_cases.py, whose cases test_gpu_dev_streams.py hands to the `_dev` entry points
with the inputs still pending on a side stream.

The GPU test proves something only if an input read too early gives another answer.  So, for every
case: each decoy has its input's byte length and type (asserted where the case is made), the
checkers accept the decoy without error (the expectations below exist), and the decoy's outputs and
at least one of its host-reported sizes differ from the real input's."""
import itertools

import numpy as np
import pytest

import host_call_cases as hc
import stream_cases as sc

# entry points that report a size to the host, by Case.call; the others report none
REPORT = {"decode": "n_out", "encode": "data_len", "rebuild": "n_out", "gather": "key_bytes", "merge": "n_out",
          "table_scan": "n_out", "vlog_get": "value_bytes", "vlog_encode": "out_len", "vlog_walk": "n_out",
          "sort": "n_out", "insert": "n_new"}
CALLS = {"stateless": {"build", "probe", "probe_count", "hashes", "or_words", "or_fold", "popcount", "multi_probe", "gen_var"},
         "sst": {"decode", "encode", "rebuild", "gather", "merge"}, "tables": {"open", "table_get", "table_scan"},
         "vlog": {"vlog_get", "vlog_encode", "vlog_walk"}, "memtable": {"sort", "insert"}}


@pytest.mark.parametrize("family", list(sc.FAMILIES))
def test_a_premature_read_gives_another_answer(ora, family):
    cases = sc.FAMILIES[family](ora)
    assert {c.call for c in cases} == CALLS[family]
    assert len({(c.call, c.ident) for c in cases}) == len(cases)
    for c in cases:
        where = "%s %s" % (c.call, c.ident)
        assert c.real and set(c.real) == set(c.decoy), where
        for name in c.real:
            assert c.real[name].nbytes == c.decoy[name].nbytes > 0, (where, name)
        changed = [name for name in c.real if hc.blob(c.real[name]) != hc.blob(c.decoy[name])]
        assert changed, where
        # the inputs without a decoy of their own (module docstring of stream_cases.py)
        same = set(c.real) - set(changed)
        assert same <= {"decode": {"blocks"}, "rebuild": {"blocks"}, "open": {"blocks"},
                        "merge": {"offsets", "map_off"}}.get(c.call, set()), where
        assert len(c.want) == len(c.decoy_want) > 0, where
        assert hc.blob(c.want) != hc.blob(c.decoy_want), where + ": the decoy has the real input's answer"
        assert set(c.sizes) == set(c.decoy_sizes), where
        assert (c.call in REPORT) == bool(c.sizes), where
        if c.sizes and not c.meta.get("sizes_fixed"):
            assert c.sizes[REPORT[c.call]] != c.decoy_sizes[REPORT[c.call]], where + ": no reported size differs"
        if c.meta.get("sizes_fixed"):
            assert c.meta["stride"] > 0 and c.sizes == c.decoy_sizes  # closed form: the keys' bytes cannot change them


def test_shapes(ora):
    """The sizes the issue of these tests names: more than one workgroup and one tile, slice or
    threshold edge of each kernel."""
    by = {}
    for family in sc.FAMILIES:
        for c in sc.FAMILIES[family](ora):
            by.setdefault(c.call, []).append(c)
    assert {c.meta["n"] for c in by["table_get"]} == set(hc.GET_SIZES) and len(by["table_get"]) == 8
    assert {(c.meta["nranges"], c.meta["flags"]) for c in by["table_scan"]} == set(hc.SCAN_SHAPES)
    assert {c.meta["n"] for c in by["open"]} == set(hc.FLUSH_SIZES)
    assert {c.meta["n"] for c in by["encode"]} == {1, 4, 300, 5_000}
    assert {c.meta["n"] for c in by["decode"]} == {4, 300, 5_000}
    builds = {(c.meta["strategy"], c.meta["k"]) for c in by["build"]}
    assert {(sc.PARTITIONED, 10), (sc.PARTITIONED, 7), (sc.ATOMIC, 10), (sc.PARTITIONED | sc.FRESH, 10),
            (sc.ATOMIC | sc.FRESH, 10)} <= builds
    assert all((c.meta["n"], c.meta["stride"], c.meta["m"]) == (60_000, 16, 2_000_003) for c in by["build"])
    assert {(c.meta["strategy"], c.call) for c in by["probe"] + by["probe_count"]} == {
        (1, "probe"), (2, "probe"), (1, "probe_count"), (2, "probe_count")}
    assert by["sort"][0].meta["n"] == by["insert"][0].meta["n"] == 2049
    lens = {len(v) for _, v, *_ in sc.vlog_entries()}
    assert {sc.SLICE - 1, sc.SLICE, sc.SLICE + 1} <= lens and max(lens) > 2 * sc.SLICE
    walk = by["vlog_walk"][0]
    assert 2 * (8 << 20) < walk.real["log"].size and walk.sizes["stop"] == walk.decoy_sizes["stop"] == 0
    assert walk.sizes["n_out"] == walk.decoy_sizes["n_out"] + 1


def test_real_answers_are_not_trivial(ora):
    get = sc.get_case(ora, 4_099, True)
    found = get.want[0]
    assert (found == 0).any() and (found == 1).any() and (found == 2).any() and not get.decoy_want[0].any()
    for with_keys in (False, True):
        st = sc.vlog_get_case(with_keys).want[0].tolist()
        assert {0, 1, 2, 3, 4} <= set(st) and (5 in st) == with_keys
        assert not sc.vlog_get_case(with_keys).decoy_want[0].any()  # found == 0: every item skipped
    p = sc.probe_case(ora, sc.PARTITIONED, 10, False)
    assert p.want[0][:30_000].all() and not p.want[0][30_000:].all() and not p.decoy_want[0].any()
    m = sc.merge_case(ora)
    assert 0 < m.want[0].size < m.meta["total"] and m.want[1] != m.meta["start"]
    assert sc.sort_case().want[0].size > 400 and sc.sort_case().decoy_want[0].tolist() == [2048]
    ins = sc.insert_case(ora)
    assert ins.sizes["n_new"] > 400 and ins.decoy_sizes["n_new"] == 1
    d = sc.decode_case(ora, 5_000)
    assert d.decoy_sizes["n_out"] < d.sizes["n_out"] and d.decoy["data"].size == d.real["data"].size


@pytest.mark.parametrize("family", sc.THREAD_FAMILIES)
def test_threads_hold_different_jobs_in_every_round(ora, family):
    per_thread = sc.thread_jobs(ora, family)
    assert len(per_thread) == sc.STREAM_THREADS and all(len(jobs) == sc.STREAM_ROUNDS for jobs in per_thread)
    for r in range(sc.STREAM_ROUNDS):
        row = [jobs[r] for jobs in per_thread]
        assert len({c.call for c in row}) == 1, (family, r)  # one entry point per round: the same workspace slots
        for a, b in itertools.combinations(row, 2):
            assert hc.fingerprint(a.real) != hc.fingerprint(b.real), (family, r, a.ident, b.ident)
            assert hc.fingerprint(a.want) != hc.fingerprint(b.want), (family, r, a.ident, b.ident)
    for jobs in per_thread:
        assert all(a is not b for a, b in zip(jobs, jobs[1:]))
    assert len({c.call for c in per_thread[0]}) == (1 if family == "memtable" else 2)
