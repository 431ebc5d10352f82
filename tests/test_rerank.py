"""Top-N among per-row candidate lists and scores of (row, item) pairs
(ocffm_problem_recommend_among / ocffm_problem_score, ImpProblem.recommend
with candidates= / ImpProblem.score, train --rec-candidates).

The contract is bitwise: a (row, item) pair has the score recommend and
label_ranks return for it, and a row's result among a list is its full
ranking filtered to the list's distinct candidates.  So the checks compare
exactly, against recommend(topn=70) on the n = 70 shapes of
tests/test_recommend.py (every warm row's whole ranking) or against score()
sorted on the host by (-score, item).  One check per precision goes against
the numpy reference with test_recommend's tolerance, for independence from
the kernels.
"""
import os
import subprocess

import numpy as np
import pytest

import ocffm
import synth
from test_recommend import (NONE, TRAIN, _cli_files, cold_rows, dataset, popularity, real_problem, reference,
                            tie_problem, tol_for, with_labels)

gpu = pytest.mark.gpu
N, ROWS = 70, 37
LENGTHS = (0, 1, 15, 16, 17, 140)


# ---------------------------------------------------------------- helpers
_PROBLEMS = {}


def problem(kind, k, precision):
    """test_recommend's problems, built once per (kind, k, precision)."""
    key = (kind, k, precision)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = real_problem(k, precision) if kind == "real" else tie_problem(precision)
    return _PROBLEMS[key]


def lists_of(per_row):
    cptr = np.zeros(len(per_row) + 1, dtype=np.uint64)
    cptr[1:] = np.cumsum([len(x) for x in per_row])
    ccol = np.array([j for x in per_row for j in x], dtype=np.uint32)
    return cptr, ccol


def ragged_lists(seed, rows=ROWS, n=N):
    """Lengths 0, 1, 15, 16, 17, 140 in turn; entries drawn with repeats, about
    one in six from [n, 10 n]."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(rows):
        ln = LENGTHS[i % len(LENGTHS)]
        x = rng.integers(0, n, size=ln)
        junk = rng.random(ln) < 1 / 6
        x[junk] = rng.integers(n, 10 * n + 1, size=int(junk.sum()))
        out.append([int(j) for j in x])
    return out


def filtered(full_items, full_scores, per_row, topn):
    """Each row's full ranking filtered to the distinct members of its list."""
    rows = len(per_row)
    items = np.full((rows, topn), NONE, dtype=np.uint32)
    scores = np.full((rows, topn), -np.inf)
    for i, lst in enumerate(per_row):
        members = set(lst)
        keep = [t for t in range(full_items.shape[1]) if full_items[i, t] != NONE and int(full_items[i, t]) in members]
        keep = keep[:topn]
        items[i, :len(keep)] = full_items[i, keep]
        scores[i, :len(keep)] = full_scores[i, keep]
    return items, scores


def same(got, want):
    return (got[0] == want[0]).all() and (got[1] == want[1]).all()


# ------------------------------------------------ 1. score equals what exists
@gpu
@pytest.mark.parametrize("k", [5, 32])
@pytest.mark.parametrize("precision", [ocffm.FP64, ocffm.FP32])
def test_score_equals_recommend_and_label_ranks(k, precision):
    g = problem("real", k, precision)
    X = g._keep[1]
    cold = cold_rows(X)
    assert cold.any() and not cold.all()
    items, scores = g.recommend(X, topn=N)
    filled = items != NONE
    assert filled[~cold].all()  # every warm row's full ranking
    rr = np.repeat(np.arange(ROWS), N).reshape(ROWS, N)
    prow, pitem = rr[filled], items[filled]
    got = g.score(X, prow, pitem)
    assert got.dtype == np.float64 and got.shape == prow.shape
    assert (got == scores[filled]).all()
    # pair counts that are no multiple of 16 or 64
    for cnt in (1, 17, ROWS * N - 3):
        assert (g.score(X, prow[:cnt], pitem[:cnt]) == scores[filled][:cnt]).all(), cnt
    # the labels of X
    yptr, ycol = X.labels()
    lrow = np.repeat(np.arange(ROWS), np.diff(yptr.astype(np.int64)))
    _, lsc, _ = g.label_ranks(X)
    assert (g.score(X, lrow, ycol) == lsc).all()
    # cold rows: popular[j]
    pop = popularity(g._keep[0])
    ci = np.nonzero(cold)[0]
    cr = np.repeat(ci, len(pop))
    cj = np.tile(np.arange(len(pop)), len(ci))
    assert (g.score(X, cr, cj) == pop[cj]).all()
    # no candidates: item >= n
    assert (g.score(X, [0, int(ci[0]), ROWS - 1], [N, N, 10 * N]) == -np.inf).all()


@gpu
@pytest.mark.parametrize("precision", [ocffm.FP64, ocffm.FP32])
def test_score_against_numpy_reference(precision):
    g = problem("real", 32, precision)
    X = g._keep[1]
    ref, _ = reference(g, X, True)
    rr, jj = np.divmod(np.arange(ROWS * N), N)
    got = g.score(X, rr, jj).reshape(ROWS, N)
    fin = np.isfinite(ref)
    assert (np.isfinite(got) == fin).all()
    err = float(np.abs(got[fin] - ref[fin]).max())
    tol = tol_for(precision, ref)
    print("score vs numpy: max err", err, "tol", tol)
    assert err <= tol


@gpu
@pytest.mark.parametrize("precision", [ocffm.FP64, ocffm.FP32])
def test_score_beyond_npop_on_cold_rows(precision):
    """A train set whose labels stop at 59: npop = 60 < n = 70."""
    ds = dataset(5, "real")
    t = ds.train
    cut = {i: [int(j) for j in t.ycol[int(t.yptr[i]):int(t.yptr[i + 1])] if j < 60] or [0] for i in range(t.m)}
    cut[0] = sorted(set(cut[0]) | {59})
    ds2 = synth.Dataset("npop", with_labels(ds, t, cut), ds.item, ds.test, k=5, params=ds.params)
    g = ocffm.problem_from_dataset(ds2, precision=precision, self_side=True)
    ocffm.srand(1)
    g.init()
    U, X, _ = g._keep
    assert int(U.info["n"]) == 60
    pop = popularity(U)
    cold = cold_rows(X)
    ci, wi = int(np.nonzero(cold)[0][0]), int(np.nonzero(~cold)[0][0])
    got = g.score(X, [ci, ci, ci, wi, wi, wi], [59, 60, 69, 59, 60, 69])
    assert got[0] == pop[59] and (got[1:3] == -np.inf).all() and np.isfinite(got[3:]).all()
    # and the same rule in the lists: a cold row's candidates stop at npop
    cptr, ccol = lists_of([[69, 60, 59, 3]] * ROWS)
    items, scores = g.recommend(X, topn=4, candidates=(cptr, ccol))
    assert set(items[ci].tolist()) == {59, 3, NONE} and (items[ci][2:] == NONE).all()
    assert sorted(items[wi].tolist()) == [3, 59, 60, 69]
    assert (scores[wi] == np.sort(g.score(X, [wi] * 4, [69, 60, 59, 3]))[::-1]).all()
    g.close()


# ------------------------------------------- 2. full lists reproduce recommend
@gpu
@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("precision", [ocffm.FP64, ocffm.FP32])
def test_full_lists_reproduce_recommend(precision, exclude):
    g = problem("real", 5, precision)
    X = g._keep[1]
    rng = np.random.default_rng(3)
    cptr, ccol = lists_of([rng.permutation(N).tolist() for _ in range(ROWS)])
    for topn in (1, 10, 64, 65, 70, 128):
        want = g.recommend(X, topn=topn, exclude_labels=exclude)
        got = g.recommend(X, topn=topn, exclude_labels=exclude, candidates=(cptr, ccol))
        assert got[0].dtype == np.uint32 and got[0].shape == (ROWS, topn)
        assert same(got, want), topn


# --------------------------------------------- 3. subsets, duplicates, junk
@gpu
@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("precision", [ocffm.FP64, ocffm.FP32])
@pytest.mark.parametrize("kind,k", [("real", 5), ("real", 32), ("ties", 5)])
def test_subsets_duplicates_junk(kind, k, precision, exclude):
    g = problem(kind, k, precision)
    X = g._keep[1]
    cold = cold_rows(X)
    per_row = ragged_lists(17)
    assert {len(x) for x in per_row} == set(LENGTHS)
    assert any(len(set(x)) < len(x) for x in per_row) and any(j >= N for x in per_row for j in x)
    assert any(cold[i] and len(per_row[i]) > 1 for i in range(ROWS))
    cptr, ccol = lists_of(per_row)
    full = g.recommend(X, topn=N, exclude_labels=exclude)
    for topn in (1, 10, 70):
        want = filtered(full[0], full[1], per_row, topn)
        got = g.recommend(X, topn=topn, exclude_labels=exclude, candidates=(cptr, ccol))
        assert same(got, want), topn
    if kind == "ties":  # the item-index tie-break is exercised
        assert any((np.diff(full[1][i][:20]) == 0).any() for i in range(ROWS))


# ------------------------------------------------------- 4. every padded KP
@gpu
@pytest.mark.parametrize("k,n", [(3, 70), (16, 70), (64, 70), (100, 70), (8, 1500)])
@pytest.mark.parametrize("precision", [ocffm.FP64, ocffm.FP32])
def test_every_padded_k(k, n, precision):
    """KP = 4, 16, 64, 128 on the drawn tables (init, no epoch), the depths
    past the chunks k_rerank keeps in registers among them; and n = 1500 with
    lists of 3,000 entries, the 1,500 items twice over, so that copies straddle
    any split.  Expected: score() of all pairs sorted by (-score, item)."""
    ds = synth.general(seed=6, m=120, n=n, fu=2, fv=2, k=k, nnz_user=2, vals="real", test_rows=37)
    g = ocffm.problem_from_dataset(ds, precision=precision, self_side=True)
    ocffm.srand(1)
    g.init()
    X = g._keep[1]
    rng = np.random.default_rng(8)
    if n == 1500:
        per_row = [np.concatenate([rng.permutation(n), rng.permutation(n)]).tolist() for _ in range(ROWS)]
    else:
        per_row = ragged_lists(23, n=n)
    rr, jj = np.divmod(np.arange(ROWS * n), n)
    S = g.score(X, rr, jj).reshape(ROWS, n)
    cptr, ccol = lists_of(per_row)
    for topn in (10, 128):
        items = np.full((ROWS, topn), NONE, dtype=np.uint32)
        scores = np.full((ROWS, topn), -np.inf)
        for i in range(ROWS):
            mem = np.array(sorted({j for j in per_row[i] if j < n and np.isfinite(S[i, j])}), dtype=np.int64)
            order = mem[np.lexsort((mem, -S[i, mem]))][:topn] if len(mem) else mem
            items[i, :len(order)] = order
            scores[i, :len(order)] = S[i, order]
        got = g.recommend(X, topn=topn, candidates=(cptr, ccol))
        assert same(got, (items, scores)), topn
    g.close()


# ------------------------------------------------------------ 5. invariance
@gpu
@pytest.mark.parametrize("precision", [ocffm.FP64, ocffm.FP32])
def test_invariance(precision, monkeypatch, tmp_path):
    """OCFFM_REC_SEG and OCFFM_REC_ROWS are read when a problem is created, so
    each setting gets a fresh problem on the saved model."""
    snap = str(tmp_path / "model.bin")
    problem("real", 5, precision).save_binary(snap)
    per_row = ragged_lists(17)
    cptr, ccol = lists_of(per_row)
    rng = np.random.default_rng(4)
    shuffled = lists_of([rng.permutation(x).tolist() for x in per_row])
    part = lists_of(per_row[5:23])
    results = []
    for seg in (None, "16", "48"):
        for rows in (None, "5"):
            for name, val in (("OCFFM_REC_SEG", seg), ("OCFFM_REC_ROWS", rows)):
                if val is None:
                    monkeypatch.delenv(name, raising=False)
                else:
                    monkeypatch.setenv(name, val)
            g = ocffm.problem_from_dataset(dataset(5, "real"), precision=precision, self_side=True)
            g.load_binary(snap)
            X = g._keep[1]
            b12 = ocffm.block_index(0, 2, g.f)
            w0 = g.get("W", b12)
            full = g.recommend(X, topn=10, candidates=(cptr, ccol))
            assert same(g.recommend(X, topn=10, candidates=(cptr, ccol)), full)
            assert same(g.recommend(X, topn=10, candidates=shuffled), full)
            got = g.recommend(X, topn=10, row0=5, rows=18, candidates=part)
            assert same(got, (full[0][5:23], full[1][5:23]))
            assert (g.get("W", b12) == w0).all()
            assert same(full, filtered(*g.recommend(X, topn=N), per_row, 10))
            results.append(full)
            g.close()
    for r in results[1:]:
        assert same(r, results[0])


# ---------------------------------------------------------------- 6. errors
@gpu
def test_errors():
    ds = dataset(5, "real")
    g = ocffm.problem_from_dataset(ds, precision=ocffm.FP64, self_side=True)
    X = g._keep[1]
    cptr, ccol = lists_of(ragged_lists(17))

    def code(fn, *a, **kw):
        with pytest.raises(ocffm.OcffmError) as e:
            fn(*a, **kw)
        return e.value.code

    def raw(cp, cc, rows=ROWS, topn=10):
        """The C entry point, for list arrays ImpProblem.recommend would turn down itself."""
        cp = np.ascontiguousarray(cp, dtype=np.uint64)
        cc = np.ascontiguousarray(cc, dtype=np.uint32)
        items = np.zeros((rows, topn), dtype=np.uint32)
        return ocffm.lib().ocffm_problem_recommend_among(g.h, X.h, 0, rows, ocffm._ptr(cp), ocffm._ptr(cc), topn, 0,
                                                         ocffm._ptr(items), None)

    assert code(g.recommend, X, topn=10, candidates=(cptr, ccol)) == ocffm.E_STATE  # before init
    assert code(g.score, X, [0], [0]) == ocffm.E_STATE
    ocffm.srand(1)
    g.init()
    good = g.recommend(X, topn=10, candidates=(cptr, ccol))
    good_s = g.score(X, [0, 5, 36], [1, 2, 3])
    assert code(g.recommend, X, topn=0, candidates=(cptr, ccol)) == ocffm.E_ARG
    assert code(g.recommend, X, topn=129, candidates=(cptr, ccol)) == ocffm.E_ARG
    assert code(g.recommend, X, topn=10, row0=30, rows=8, candidates=(cptr[:9], ccol)) == ocffm.E_ARG
    bad0 = cptr.copy()
    bad0[0] = 1
    assert raw(bad0, ccol) == ocffm.E_ARG
    dec = cptr.copy()
    dec[3] = dec[2] - 1
    assert raw(dec, ccol) == ocffm.E_ARG
    assert ocffm.lib().ocffm_problem_recommend_among(g.h, X.h, 0, ROWS, None, ocffm._ptr(ccol), 10, 0,
                                                     ocffm._ptr(np.zeros((ROWS, 10), dtype=np.uint32)),
                                                     None) == ocffm.E_ARG
    assert code(g.score, X, [ROWS], [0]) == ocffm.E_ARG  # prow out of range
    # built without the train Ds: an out-of-range index is kept
    bad = synth.Rows(ds.test.xptr, ds.test.fid, ds.test.idx.copy(), ds.test.val, ds.test.yptr, ds.test.ycol)
    bad.idx[0] = int(g._keep[0].Ds[int(bad.fid[0])]) + 3
    Xbad = ocffm.ImpData.from_rows(bad)
    assert code(g.recommend, Xbad, topn=10, candidates=(cptr, ccol)) == ocffm.E_DATA
    assert code(g.score, Xbad, [0], [0]) == ocffm.E_DATA
    items, scores = g.recommend(X, topn=10, rows=0, candidates=(np.zeros(1, dtype=np.uint64), ccol[:0]))
    assert items.shape == (0, 10) and scores.shape == (0, 10)
    assert g.score(X, [], []).shape == (0,)
    # a valid call afterwards still gives the earlier bits
    assert same(g.recommend(X, topn=10, candidates=(cptr, ccol)), good)
    assert (g.score(X, [0, 5, 36], [1, 2, 3]) == good_s).all()
    g.close()


# ------------------------------------------------------------------- 7. CLI
@gpu
def test_cli_matches_python(tmp_path):
    tr, it, te = _cli_files(tmp_path)
    out, cand = str(tmp_path / "out.txt"), str(tmp_path / "cand.txt")
    per_row = ragged_lists(29, rows=100, n=50)
    with open(cand, "w") as f:
        for x in per_row:
            f.write(" ".join(str(j) for j in x) + "\n")
    r = subprocess.run([TRAIN, "-k", "4", "-t", "2", "--fp64", "--recommend", te, "--topn", "7", "--rec-unseen",
                        "--rec-candidates", cand, "--rec-out", out, it, tr], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    U = ocffm.ImpData.read(tr, True)
    V = ocffm.ImpData.read(it, False)
    V.trans_y(U)
    X = ocffm.ImpData.read(te, True, U.Ds)
    g = ocffm.ImpProblem(U, None, V, ocffm.Parameter(k=4, nr_pass=2, precision=ocffm.FP64))
    ocffm.srand(1)
    g.init()
    g.one_epoch()
    g.one_epoch()
    items, scores = g.recommend(X, topn=7, exclude_labels=True, candidates=lists_of(per_row))
    lines = open(out).read().split("\n")
    assert lines[-1] == "" and len(lines) - 1 == int(X.info["m"]) == 100
    want = [" ".join("%d:%.17g" % (items[i, t], scores[i, t]) for t in range(7) if items[i, t] != NONE)
            for i in range(100)]
    assert lines[:-1] == want
    assert any(w == "" for w in want) and any(len(w.split()) == 7 for w in want)
    g.close()


def test_cli_usage_errors(tmp_path):
    """--rec-candidates without --recommend fails before anything is read; a
    malformed list file fails before any device work (this test has no GPU)."""
    missing = str(tmp_path / "nothing")
    out = str(tmp_path / "out.txt")
    r = subprocess.run([TRAIN, "--rec-candidates", missing, "--rec-out", out, missing, missing],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "--recommend" in r.stderr, (r.returncode, r.stderr)
    assert "--rec-candidates" in subprocess.run([TRAIN], capture_output=True, text=True).stderr
    tr, it, te = _cli_files(tmp_path)
    ok = ["1 2 3"] * 100
    for name, lines in (("short", ok[:99]), ("long", ok + [""]), ("neg", ok[:50] + ["1 -2"] + ok[51:]),
                        ("word", ok[:99] + ["4 x7"]), ("frac", ["1.5"] + ok[1:])):
        cand = str(tmp_path / name)
        with open(cand, "w") as f:
            f.write("\n".join(lines) + "\n")
        r = subprocess.run([TRAIN, "--recommend", te, "--rec-candidates", cand, "--rec-out", out, it, tr],
                           capture_output=True, text=True)
        assert r.returncode == 1 and name in r.stderr, (name, r.returncode, r.stderr)
        assert not os.path.exists(out)
