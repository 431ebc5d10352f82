"""Pair scores and candidate lists on SGD-trained models (include/ocffm.h
ocffm_sgd_score / _recommend_among / _label_ranks_among / _evaluate_among,
SgdTrainer.score and candidates= on recommend / label_ranks / evaluate).

The contract is bitwise: a (row, item) pair has the bits recommend and
label_ranks give it, a row's top-N among a list is its full ranking filtered
to the list, and a label's rank among a list is its place in the list's
distinct candidates united with the row's labels.  So the checks compare
exactly, on the cases of tests/test_sgd_rank.py (38 rows with a row and an
item without nodes, 70 items, KP 4 / 16 / 128, both norm settings); one check
goes against the numpy reference with test_sgd_rank's derived tolerance.
"""
import numpy as np
import pytest

import ocffm
import synth
from test_eval_among import host_among, same3
from test_rerank import LENGTHS, filtered, lists_of, ragged_lists, same
from test_sgd_rank import PRM, Case, case, integer_w

pytestmark = pytest.mark.gpu

NONE = ocffm.REC_NONE
N = 70
CASES = [(3, 1, 1, 0), (16, 2, 2, 1), (16, 3, 1, 1), (100, 1, 1, 1), (100, 1, 1, 0)]


@pytest.mark.parametrize("k,fu,fv,norm", CASES)
def test_score(k, fu, fv, norm):
    c = case(k, fu, fv, norm, extra=True)
    m = c.xrows.m
    items, scores = c.t.recommend(c.X, topn=N)
    assert (items != NONE).all()
    prow = np.repeat(np.arange(m), N)
    pitem, want = items.reshape(-1), scores.reshape(-1)
    got = c.t.score(c.X, prow, pitem)
    assert got.dtype == np.float64 and got.shape == (m * N,)
    assert (got == want).all()
    assert (m * N - 3) % 64
    for cnt in (1, 17, m * N - 3):
        assert (c.t.score(c.X, prow[:cnt], pitem[:cnt]) == want[:cnt]).all(), cnt
    # the labels: label_ranks' scores, -inf for the label >= n of row 3
    yptr = c.xrows.yptr.astype(np.int64)
    lrow = np.repeat(np.arange(m), np.diff(yptr))
    _, lsc, _ = c.t.label_ranks(c.X)
    ls = c.t.score(c.X, lrow, c.xrows.ycol)
    assert (ls == lsc).all() and (ls == -np.inf).sum() == 1
    assert (c.t.score(c.X, [0, 2, m - 1], [N, N + 1, 10 * N]) == -np.inf).all()
    assert c.t.score(c.X, [], []).shape == (0,)


def test_score_against_numpy_reference():
    c = case(16, 2, 2, 1, extra=True)
    ref, tol = c.ref()
    m = c.xrows.m
    rr, jj = np.divmod(np.arange(m * N), N)
    got = c.t.score(c.X, rr, jj).reshape(m, N)
    err = np.abs(got - ref)
    print("score vs numpy: worst err / tol", float((err / np.maximum(tol, 1e-300)).max()))
    assert (err <= tol).all(), float((err - tol).max())


@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("k,fu,fv,norm", CASES)
def test_recommend_among_ragged(k, fu, fv, norm, exclude):
    c = case(k, fu, fv, norm, extra=True)
    m = c.xrows.m
    per_row = ragged_lists(17, rows=m, n=N)
    assert {len(x) for x in per_row} == set(LENGTHS)
    assert any(len(set(x)) < len(x) for x in per_row) and any(j >= N for x in per_row for j in x)
    assert len(per_row[2]) > 1 and any(5 in x for x in per_row)  # the row and the item without nodes
    cand = lists_of(per_row)
    full = c.t.recommend(c.X, topn=N, exclude_labels=exclude)
    for topn in (1, 10, 70, 128):
        want = filtered(full[0], full[1], per_row, topn)
        got = c.t.recommend(c.X, topn=topn, exclude_labels=exclude, candidates=cand)
        assert got[0].dtype == np.uint32 and got[0].shape == (m, topn)
        assert same(got, want), topn
    # a sub-range of the rows with its own lists
    got = c.t.recommend(c.X, topn=10, row0=5, rows=18, exclude_labels=exclude, candidates=lists_of(per_row[5:23]))
    want = filtered(full[0], full[1], per_row, 10)
    assert same(got, (want[0][5:23], want[1][5:23]))


@pytest.mark.parametrize("k,fu,fv,norm", CASES)
def test_label_ranks_among(k, fu, fv, norm):
    c = case(k, fu, fv, norm, extra=True)
    m = c.xrows.m
    rng = np.random.default_rng(7)
    whole = [[int(j) for j in rng.permutation(np.r_[np.arange(N), rng.integers(0, 10 * N, size=11)])]
             for _ in range(m)]
    # seen: three fixed items per row and the row's first label
    xr = c.xrows
    seen_labs = [np.r_[c.labels[i][:1], [2, 33, 69]] for i in range(m)]
    sp = np.zeros(m + 1, dtype=np.uint64)
    sp[1:] = np.cumsum([len(x) for x in seen_labs])
    S = ocffm.ImpData.from_rows(synth.Rows(xr.xptr, xr.fid, xr.idx, xr.val, sp,
                                           np.concatenate(seen_labs).astype(np.uint64)))
    for seen in (None, S):
        want = c.t.label_ranks(c.X, seen=seen)
        got = c.t.label_ranks(c.X, seen=seen, candidates=lists_of(whole))
        assert same3(got, want), seen is not None
    per_row = ragged_lists(17, rows=m, n=N)
    assert len(per_row[2]) > 1 and any(5 in x for x in per_row)  # the row and the item without nodes
    assert any(int(j) not in per_row[i] for i in range(m) for j in c.labels[i])
    assert any(int(j) in per_row[i] for i in range(m) for j in c.labels[i])
    for seen in (None, S):
        want = host_among(c.t, c.X, per_row, seen)
        got = c.t.label_ranks(c.X, seen=seen, candidates=lists_of(per_row))
        assert same3(got, want), seen is not None
        assert (got[0] != NONE).any() and (got[0] == NONE).any()
    # the duplicate label of row 4 shares its rank; evaluate is eval_from_ranks of these
    yptr = xr.yptr.astype(np.int64)
    r, s, nc = c.t.label_ranks(c.X, candidates=lists_of(per_row))
    assert r[yptr[5] - 1] == r[yptr[4]] and s[yptr[5] - 1] == s[yptr[4]]
    ev = c.t.evaluate(c.X, cuts=(1, 5, 20), candidates=lists_of(per_row))
    want = ocffm.eval_from_ranks(xr.yptr, r, nc, scores=s, cuts=(1, 5, 20))
    assert ev.keys() == want.keys()
    for key in ev:
        np.testing.assert_array_equal(np.asarray(ev[key]), np.asarray(want[key]), err_msg=key)


def test_cutting(monkeypatch):
    """OCFFM_REC_SEG and OCFFM_REC_ROWS are read at create: the second trainer
    takes the first one's W through set_w."""
    key, kw = (16, 2, 2, 1), dict(extra=True)
    c = case(*key, **kw)
    m = c.xrows.m
    per_row = ragged_lists(17, rows=m, n=N)
    cand = lists_of(per_row)

    def run(t, X):
        return t.recommend(X, topn=10, candidates=cand) + t.label_ranks(X, candidates=cand)

    base = run(c.t, c.X)
    w = c.t.get("W")
    for seg, rows in (("16", None), ("32", "5")):
        monkeypatch.setenv("OCFFM_REC_SEG", seg)
        if rows is None:
            monkeypatch.delenv("OCFFM_REC_ROWS", raising=False)
        else:
            monkeypatch.setenv("OCFFM_REC_ROWS", rows)
        d = Case(*key, epochs=0, **kw)
        d.t.set_w(w)
        for a, b in zip(base, run(d.t, d.X)):
            np.testing.assert_array_equal(a, b)


def test_model_changes():
    c = Case(16, 2, 2, 1, extra=True)
    m = c.xrows.m
    per_row = ragged_lists(17, rows=m, n=N)
    cand = lists_of(per_row)
    assert c.t.counter("rank_item_builds") == 0
    rr, jj = np.divmod(np.arange(m * N), N)

    def check():
        full = c.t.recommend(c.X, topn=N)
        got = c.t.recommend(c.X, topn=10, candidates=cand)
        assert same(got, filtered(full[0], full[1], per_row, 10))
        S = c.t.score(c.X, rr, jj).reshape(m, N)
        assert (np.take_along_axis(S, full[0].astype(np.int64), axis=1) == full[1]).all()
        assert same3(c.t.label_ranks(c.X, candidates=cand), host_among(c.t, c.X, per_row))
        c.t.evaluate(c.X, candidates=cand)
        return S

    s0 = check()
    assert c.t.counter("rank_item_builds") == 1
    assert c.t.counter("rank_kernel_us") > 0 and c.t.counter("rank_setup_us") > 0
    c.t.epoch()
    s1 = check()
    assert c.t.counter("rank_item_builds") == 2 and (s1 != s0).any()
    integer_w(c, 4)
    s2 = check()
    assert c.t.counter("rank_item_builds") == 3 and (s2 != s1).any()
    c.t.score(c.X, [0], [0])
    assert c.t.counter("rank_item_builds") == 3


def test_errors():
    c = case(16, 2, 2, 1, extra=True)
    t, X = c.t, c.X
    m = c.xrows.m
    cptr, ccol = lists_of(ragged_lists(17, rows=m, n=N))
    L = ocffm.lib()
    vp = ocffm._ptr

    def code(fn):
        with pytest.raises(ocffm.OcffmError) as e:
            fn()
        return e.value.code

    items = np.zeros((m, 4), np.uint32)
    ranks = np.zeros(int(c.xrows.yptr[-1]), np.uint32)
    bad0 = cptr.copy()
    bad0[0] = 1
    dec = cptr.copy()
    dec[3] = dec[2] - 1
    among = lambda cp, cc, topn=4, it=items, rows=m, x=X.h: L.ocffm_sgd_recommend_among(  # noqa: E731
        t.h, x, 0, rows, None if cp is None else vp(cp), None if cc is None else vp(cc), topn, 0,
        None if it is None else vp(it), None)
    lranks = lambda cp, cc, rk=ranks: L.ocffm_sgd_label_ranks_among(  # noqa: E731
        t.h, X.h, None, None if cp is None else vp(cp), None if cc is None else vp(cc),
        None if rk is None else vp(rk), None, None)
    assert among(cptr, ccol) == ocffm.OK and lranks(cptr, ccol) == ocffm.OK  # NULL scores / ncand
    for fn in (among, lranks):
        assert fn(None, ccol) == ocffm.E_ARG
        assert fn(bad0, ccol) == ocffm.E_ARG
        assert fn(dec, ccol) == ocffm.E_ARG
        assert fn(cptr, None) == ocffm.E_ARG
    assert among(cptr, ccol, topn=0) == ocffm.E_ARG
    assert among(cptr, ccol, topn=129) == ocffm.E_ARG
    assert among(cptr, ccol, it=None) == ocffm.E_ARG
    assert among(cptr, ccol, x=None) == ocffm.E_ARG
    assert among(cptr, ccol, rows=m + 1) == ocffm.E_ARG
    assert among(np.zeros(1, np.uint64), ccol, rows=0) == ocffm.OK
    assert lranks(cptr, ccol, rk=None) == ocffm.E_ARG
    assert code(lambda: t.recommend(X, topn=4, candidates=(cptr[:-1], ccol))) == ocffm.E_ARG
    assert code(lambda: t.label_ranks(X, candidates=(cptr[:-1], ccol))) == ocffm.E_ARG
    assert code(lambda: t.label_ranks(c.V, candidates=(np.zeros(N + 1, np.uint64), ccol))) == ocffm.E_ARG  # no labels
    assert code(lambda: t.evaluate(X, cuts=(5, 5), candidates=(cptr, ccol))) == ocffm.E_ARG
    assert code(lambda: t.score(X, [m], [0])) == ocffm.E_ARG  # prow out of range
    out = np.zeros(1)
    one = np.zeros(1, np.uint32)
    assert L.ocffm_sgd_score(t.h, X.h, 1, None, vp(one), vp(out)) == ocffm.E_ARG
    assert L.ocffm_sgd_score(t.h, X.h, 1, vp(one), vp(one), None) == ocffm.E_ARG
    assert L.ocffm_sgd_score(t.h, None, 1, vp(one), vp(one), vp(out)) == ocffm.E_ARG
    assert L.ocffm_sgd_score(t.h, X.h, 0, None, None, None) == ocffm.OK
    rows = synth._build_rows([[(0, 1, 1.0)], [(2, 0, 1.0)]], [np.array([1]), np.array([2])])
    Xb = ocffm.ImpData.from_rows(rows)
    two = (np.array([0, 1, 2], np.uint64), np.array([3, 4], np.uint32))
    assert code(lambda: t.recommend(Xb, topn=3, candidates=two)) == ocffm.E_DATA
    assert code(lambda: t.label_ranks(Xb, candidates=two)) == ocffm.E_DATA
    assert code(lambda: t.score(Xb, [0], [0])) == ocffm.E_DATA
    empty = ocffm.ImpData.from_rows(synth._build_rows([], []))
    none = (np.zeros(1, np.uint64), np.zeros(0, np.uint32))
    assert t.recommend(empty, topn=3, candidates=none)[0].shape == (0, 3)
    assert t.label_ranks(empty, candidates=none)[0].size == 0
    V0 = ocffm.ImpData.from_rows(synth._build_rows([[] for _ in range(70)], None))
    t0 = ocffm.SgdTrainer(c.U, V0, k=4, **PRM)
    assert code(lambda: t0.recommend(X, topn=3, candidates=(cptr, ccol))) == ocffm.E_ARG
    assert code(lambda: t0.label_ranks(X, candidates=(cptr, ccol))) == ocffm.E_ARG
    assert code(lambda: t0.score(X, [0], [0])) == ocffm.E_ARG
