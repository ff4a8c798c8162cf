"""GPU: the weighted formulas of a result are bound to the VALUES of the call's operand sets, not to the objects (bio_amd/sketches.py:
Index.search_counted, Sets.neighbors_counted, Sets.compare_counted fetch the operands' norms when a formula first asks).  Once a formula
was asked the norms are a snapshot: overwriting or closing the operand changes nothing.  Before that, a formula asked after the operand
was written through `into=` or closed raises ValueError -- it must not mix the call's dot and min_sum with other sets' norms, and a
closed operand's null handle must not reach the library."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
U64, U32 = np.uint64, np.uint32
FORMULAS = ("cosine", "angular_similarity", "weighted_jaccard", "bray_curtis")


def operands(engine):
    """a (3 sets) and b (2 sets) of three to five counted members, and `other`: sets of other sizes and counts to overwrite a with"""
    a = engine.sets_from_arrays_counted(np.array([0, 3, 7, 12], U64), np.array([1, 2, 3, 2, 3, 4, 5, 1, 3, 5, 7, 9], U64), np.arange(1, 13, dtype=U32))
    b = engine.sets_from_arrays_counted(np.array([0, 4, 9], U64), np.array([1, 2, 3, 4, 3, 5, 7, 9, 11], U64), np.array([2, 7, 1, 8, 2, 8, 1, 8, 2], U32))
    other = engine.sets_from_arrays_counted(np.array([0, 5, 9], U64), np.array([1, 2, 3, 4, 5, 2, 4, 6, 8], U64), np.full(9, 6, U32))
    return a, b, other


def overwrite(a, other):
    """a becomes other | other: two sets where there were three, uncounted"""
    assert other.union(other, into=a) is a and a.info()["n_sets"] == 2


def expected(res, a_norms, b_norms):
    """the four formulas from the result's own integers and the operands' norms as they were at the call, in the docstrings' operation order"""
    dot, ms = np.asarray(res.dot, U64).astype(np.float64), np.asarray(res.min_sum, U64).astype(np.float64)
    (qa, ta), (qb, tb) = a_norms, b_norms
    if dot.ndim == 2:
        qa, ta, qb, tb = qa[:, None], ta[:, None], qb[None, :], tb[None, :]
    else:
        i, j = res.query().astype(np.int64), res.target.astype(np.int64)
        qa, ta, qb, tb = qa[i], ta[i], qb[j], tb[j]
    cos = dot / (np.sqrt(qa.astype(np.float64)) * np.sqrt(qb.astype(np.float64)))
    den = ta.astype(np.float64) + tb.astype(np.float64)
    return dict(cosine=cos, angular_similarity=1.0 - 2.0 * np.arccos(np.minimum(cos, 1.0)) / np.pi, weighted_jaccard=ms / (den - ms), bray_curtis=1.0 - 2.0 * ms / den)


def make(binding, a, b):
    if binding == "search_counted":
        ix = b.index_counted()
        return ix.search_counted(a), ix
    return (a.neighbors_counted(b) if binding == "neighbors_counted" else a.compare_counted(b)), None


@pytest.mark.parametrize("binding", ["search_counted", "neighbors_counted", "compare_counted"])
def test_asked_before_the_operand_is_overwritten_the_formulas_stay(engine, binding):
    a, b, other = operands(engine)
    norms = (a.sumsq(), a.totals()), (b.sumsq(), b.totals())
    res, ix = make(binding, a, b)
    want = expected(res, *norms)
    assert np.asarray(res.dot).size >= 4 and np.array_equal(res.cosine(), want["cosine"])  # the first formula fetches the norms
    overwrite(a, other)
    for name in FORMULAS:
        assert np.array_equal(getattr(res, name)(), want[name]), name
    a.close()
    for name in FORMULAS:
        assert np.array_equal(getattr(res, name)(), want[name]), name
    for x in (res, ix, b, other):
        if x is not None:
            x.close()


@pytest.mark.parametrize("binding", ["search_counted", "neighbors_counted", "compare_counted"])
def test_asked_after_the_operand_was_written_or_closed_the_formulas_raise(engine, binding):
    a, b, other = operands(engine)
    res, ix = make(binding, a, b)
    shared = np.array(res.shared)
    overwrite(a, other)
    for name in FORMULAS:
        with pytest.raises(ValueError, match="the operand sets were written or closed since the call"):
            getattr(res, name)()
    assert np.array_equal(res.shared, shared) and res.dot is not None  # the result itself is what it was
    a2, b2, _ = operands(engine)
    res2, ix2 = make(binding, a2, b2)
    a2.close()  # a closed operand: no handle to ask
    for name in FORMULAS:
        with pytest.raises(ValueError, match="the operand sets were written or closed since the call"):
            getattr(res2, name)()
    if binding != "search_counted":  # the second operand counts as well (the index keeps its targets' norms itself)
        a3, b3, _ = operands(engine)
        res3, _ = make(binding, a3, b3)
        overwrite(b3, other)
        with pytest.raises(ValueError, match="written or closed"):
            res3.cosine()
        for x in (res3, a3, b3):
            x.close()
    else:  # the index's own norms outlive its source sets
        a4, b4, _ = operands(engine)
        norms = (a4.sumsq(), a4.totals()), (b4.sumsq(), b4.totals())
        res4, ix4 = make(binding, a4, b4)
        want = expected(res4, *norms)
        overwrite(b4, other)
        b4.close()
        for name in FORMULAS:
            assert np.array_equal(getattr(res4, name)(), want[name]), name
        ix4.close()  # its norms were fetched: a snapshot
        assert np.array_equal(res4.cosine(), want["cosine"])
        a5, b5, _ = operands(engine)
        res5, ix5 = make(binding, a5, b5)
        ix5.close()  # ... and a handle closed before any formula asked: nothing to fetch them through
        with pytest.raises(ValueError, match="the index was closed since the call"):
            res5.cosine()
        for x in (res4, a4, res5, a5, b5):
            x.close()
    for x in (res, ix, a, b, other, res2, ix2, b2):
        if x is not None:
            x.close()
