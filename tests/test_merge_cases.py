"""CPU: the NumPy model of the merged hits (tests/merge_cases.py) against a dict-of-dicts brute force on seeded small inputs, and the
crafted inputs of tests/test_gpu_merge.py against what they claim: both paths, every row length, duplicates inside and across parts,
each path once per payload combination."""
import numpy as np
import pytest

from tests import merge_cases as MC
from tests import select_cases as SC
from tests import transpose_cases as TC

U64, U32 = np.uint64, np.uint32


def random_parts(rng, n_parts, payload_sets, ascending=True, repeats=False):
    nq, nt = int(rng.integers(1, 7)), int(rng.integers(1, 12))
    return [TC.random_record(rng, nq, nt, 6, payloads=payload_sets[p % len(payload_sets)], ascending=ascending, repeats=repeats) for p in range(n_parts)], nt


def test_model_equals_the_brute_force():
    rng = np.random.default_rng(61)
    paths, combined = set(), 0
    for trial in range(120):
        sets = [MC.PAYLOAD_SETS[int(rng.integers(0, 5))]] if trial % 3 else list(MC.PAYLOAD_SETS)
        parts, nt = random_parts(rng, int(rng.integers(1, 5)), sets, ascending=bool(trial % 2), repeats=trial % 5 == 0)
        bases = [int(b) for b in (np.arange(len(parts)) * nt if trial % 4 == 0 else rng.integers(0, 2 * nt, len(parts)))]
        got, fig = MC.merge_model(parts, bases, add=True)
        assert not SC.same(got, MC.merge_brute(parts, bases, add=True)), trial
        assert fig["hits"] == sum(len(r["t"]) for r in parts) and fig["hits"] - fig["combined"] == len(got["t"]) and fig["parts"] == len(parts)
        if fig["path"] == "concat":
            assert fig["combined"] == 0, trial  # duplicates cannot exist on the concat path
        if fig["combined"]:
            for f in (MC.merge_model, MC.merge_brute):
                with pytest.raises(MC.Duplicate):
                    f(parts, bases, add=False)
        else:
            assert not SC.same(MC.merge_model(parts, bases, add=False)[0], got)
        rows = [got["t"][int(a):int(b)].astype(np.int64) for a, b in zip(got["o"][:-1], got["o"][1:])]
        assert all(np.all(np.diff(r) > 0) for r in rows)  # strictly ascending
        paths.add(fig["path"])
        combined += fig["combined"]
    assert paths == {"concat", "sort"} and combined > 100


def test_the_result_carries_what_every_part_carries():
    rng = np.random.default_rng(67)
    for a in MC.PAYLOAD_SETS:
        for b in MC.PAYLOAD_SETS:
            parts = [TC.random_record(rng, 5, 9, 4, payloads=a), TC.random_record(rng, 5, 9, 4, payloads=b)]
            got, _ = MC.merge_model(parts, (0, 9))
            want = tuple(p for p in SC.PAYLOADS if parts[0][p] is not None and parts[1][p] is not None)
            assert tuple(p for p in SC.PAYLOADS if got[p] is not None) == want == MC.carried(parts)
            assert not SC.same(got, MC.merge_brute(parts, (0, 9)))


def test_each_path_once_per_payload_combination():
    """what tests/test_gpu_merge.py does with every object of its zoo, on records of the same payloads"""
    rng = np.random.default_rng(71)
    for payloads in MC.PAYLOAD_SETS:
        rec = TC.random_record(rng, 30, 50, 20, payloads=payloads)
        seen = set()
        for bases, add, path in MC.self_merge_plans(50):
            got, fig = MC.merge_model([rec, rec], bases, add)
            assert fig["path"] == path and fig["combined"] == (len(rec["t"]) if path == "sort" else 0), payloads
            assert MC.carried([rec, rec]) == tuple(p for p in SC.PAYLOADS if rec[p] is not None)
            seen.add(fig["path"])
        assert seen == {"concat", "sort"}


def test_the_crafted_inputs_reach_what_they_claim():
    for interleaved, path in ((False, "concat"), (True, "sort")):
        parts, bases = MC.row_length_parts(interleaved)
        got, fig = MC.merge_model(parts, bases)
        lens = np.diff(got["o"]).astype(int).tolist()
        assert lens[:16] == list(MC.MERGED_ROW_LENGTHS) and lens[16:] == [0, 7] and fig == dict(path=path, parts=3, hits=sum(lens), combined=0)
        per_part = np.stack([np.diff(r["o"]).astype(int) for r in parts])
        whole_from_last = (per_part[0] == 0) & (per_part[1] == 0) & (per_part[2] > 0)
        empty_in_the_middle = (per_part[0] > 0) & (per_part[1] == 0) & (per_part[2] > 0)
        assert whole_from_last.any() and empty_in_the_middle.any() and (per_part.sum(0) == 0).any() and (per_part.min(0) > 0).any()
        assert all(MC.ascending(r) for r in parts) and all(r["total"] is not None for r in parts)
        if interleaved:  # the rows really interleave: some row's neighbours in the result come from different parts
            assert any(len(set((got["t"][int(a):int(b)] % 3).tolist())) == 3 for a, b in zip(got["o"][:-1], got["o"][1:]))
    for n in (1, 2, 3, 8, MC.MAX_PARTS):
        parts, bases = MC.many_parts(n)
        got, fig = MC.merge_model(parts, bases)
        assert fig["path"] == "concat" and fig["parts"] == n and len(got["t"]) == fig["hits"] > 0
        assert n == 1 or any(len(r["t"]) and not np.diff(r["o"])[1::2].any() for r in parts[1::2])
    across, inside, saturating = MC.duplicate_parts()
    for parts, combined in ((across, 2), (inside, 1), (saturating, 4)):
        with pytest.raises(MC.Duplicate):
            MC.merge_model(parts)
        got, fig = MC.merge_model(parts, add=True)
        assert fig["path"] == "sort" and fig["combined"] == combined and not SC.same(got, MC.merge_brute(parts, add=True))
    assert MC.path_of(inside[1:], (0,)) == "sort" and not MC.ascending(inside[1])  # a duplicate inside one part
    got, _ = MC.merge_model(across, add=True)
    assert int(got["s"][0]) == MC.MAX32 == int(got["total"][0]) and int(got["s"][2]) == 19  # 2^32 - 1 plus 1 saturates; 8 + 11
    for interleaved, path in ((False, "concat"), (True, "sort")):
        parts, bases = MC.caps_parts(interleaved)
        got, fig = MC.merge_model(parts, bases)
        assert fig["path"] == path and fig["hits"] > 3 * 256 * 2 and len(got["o"]) == 601 and fig["combined"] == 0
    with pytest.raises(MC.Unsupported):
        MC.merge_model([SC.record([0, 1], [1], [1])], [MC.MAX32])
    assert int(MC.merge_model([SC.record([0, 1], [0], [1])], [MC.MAX32])[0]["t"][0]) == MC.MAX32


def test_the_shard_builders_split_and_cover():
    t, tc, q, qc = MC.search_sets()
    assert len(t[0]) == 38 and len(q[0]) == 41
    shards = MC.target_shards(t, tc, [0, 11, 12, 37])
    assert [len(c[0]) - 1 for c, _ in shards] == [11, 1, 25] and np.array_equal(np.concatenate([c[1] for c, _ in shards]), t[1])
    assert np.array_equal(np.concatenate([k for _, k in shards]), tc)
    halves = MC.value_shards(t, tc, 2)
    assert all(len(c[0]) == 38 for c, _ in halves) and sum(len(c[1]) for c, _ in halves) == len(t[1]) and all(len(c[1]) for c, _ in halves)
    assert all(np.all(c[1] % U64(2) == U64(k)) for k, (c, _) in enumerate(halves))
    assert all(int(c[0][-1]) == len(c[1]) == len(k) for c, k in halves)


def test_wrong_models_are_caught():
    parts, bases = MC.row_length_parts(True)
    shifted, sbases = MC.row_length_parts(False)
    want = MC.merge_model(shifted, sbases)[0]
    assert SC.same(MC.wrong_no_shift(shifted, sbases), want)
    assert SC.same(MC.wrong_part_order(parts, bases), MC.merge_model(parts, bases)[0])
    assert not SC.same(MC.wrong_part_order(shifted, sbases), want)  # (behind one another the part order IS the order: the concat path)
    across, _, _ = MC.duplicate_parts()
    assert SC.same(MC.wrong_wraps(across, None, True), MC.merge_model(across, None, True)[0])
    rng = np.random.default_rng(73)
    mixed = [TC.random_record(rng, 5, 9, 4, payloads=("total", "dot")), TC.random_record(rng, 5, 9, 4, payloads=("dot",))]
    assert SC.same(MC.wrong_keeps_all_payloads(mixed, (0, 9)), MC.merge_model(mixed, (0, 9))[0])
