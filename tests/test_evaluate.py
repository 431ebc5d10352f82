"""Ranking evaluation (ocffm_problem_label_ranks / ocffm_problem_evaluate /
ImpProblem.label_ranks / ImpProblem.evaluate / train --eval).

The reference is the numpy fp64 score matrix of tests/test_recommend.py
(reference()), ranked with np.lexsort on (score descending, item ascending).
For real-valued models a rank may move across candidates whose reference
score is within 2 tol of the label's (tol_for: 1e-12 fp64, 1e-3 fp32,
relative): the rank must lie in [#{ref > ref_p + 2 tol}, #{ref >= ref_p -
2 tol} - 1].  Integer tables give exact scores in both precisions, so those
tests compare ranks exactly.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import ocffm
import synth
from test_recommend import (NONE, TRAIN, _cli_files, cold_rows, dataset, real_problem, reference, tie_problem,
                            tol_for, with_labels)

gpu = pytest.mark.gpu
CUTS = (5, 10, 20, 40, 80)


def exact_ranks(ref, X, seen=None):
    """ranks / ncand by np.lexsort over each row's candidates (finite reference
    score, not in seen's row); NONE for a label that is no candidate."""
    yptr, ycol = X.labels()
    m, n = ref.shape
    ranks = np.full(len(ycol), NONE, dtype=np.uint32)
    ncand = np.zeros(m, dtype=np.uint32)
    if seen is not None:
        sptr, scol = seen.labels()
    for i in range(m):
        ok = np.isfinite(ref[i])
        if seen is not None:
            s = scol[int(sptr[i]):int(sptr[i + 1])].astype(np.int64)
            ok[s[s < n]] = False
        cand = np.nonzero(ok)[0]
        ncand[i] = len(cand)
        order = cand[np.lexsort((cand, -ref[i, cand]))]
        place = np.full(n, NONE, dtype=np.uint32)
        place[order] = np.arange(len(order), dtype=np.uint32)
        for p in range(int(yptr[i]), int(yptr[i + 1])):
            if ycol[p] < n:
                ranks[p] = place[int(ycol[p])]
    return ranks, ncand


def integer_tables(g, seed=11):
    """tie_problem's tables on any problem: integer W / H in [-3, 3]."""
    rng = np.random.default_rng(seed)
    fu = int(g._keep[0].info["f"])
    for f1 in range(fu):
        for f2 in range(fu, g.f):
            b12 = ocffm.block_index(f1, f2, g.f)
            for what in "WH":
                g.set(what, b12, rng.integers(-3, 4, size=g.get(what, b12).size).astype(np.float64))


# ------------------------------------------------------------ 1. rank parity
@gpu
@pytest.mark.parametrize("k", [5, 32])
@pytest.mark.parametrize("precision", [ocffm.FP64, ocffm.FP32])
def test_rank_parity(k, precision):
    g = real_problem(k, precision)
    X = g._keep[1]
    ref, cold = reference(g, X, True)
    assert cold.any() and not cold.all()
    tol = tol_for(precision, ref)
    ranks, scores, ncand = g.label_ranks(X)
    yptr, ycol = X.labels()
    assert ranks.dtype == np.uint32 and ranks.shape == scores.shape == ycol.shape and ncand.shape == (37,)
    want, want_nc = exact_ranks(ref, X)
    assert (ncand == want_nc).all()
    n = ref.shape[1]
    checked = 0
    for i in range(37):
        fin = np.isfinite(ref[i])
        for p in range(int(yptr[i]), int(yptr[i + 1])):
            j = int(ycol[p])
            if j >= n or not fin[j]:
                assert ranks[p] == NONE and scores[p] == -np.inf
                continue
            print(i, j, int(ranks[p]), int(want[p]), abs(scores[p] - ref[i, j]), tol)
            assert abs(scores[p] - ref[i, j]) <= tol, (i, j)
            if cold[i]:  # popularity order is exact
                assert ranks[p] == want[p] and scores[p] == ref[i, j], (i, j)
            else:
                lo = int((ref[i, fin] > ref[i, j] + 2 * tol).sum())
                hi = int((ref[i, fin] >= ref[i, j] - 2 * tol).sum()) - 1
                assert lo <= int(ranks[p]) <= hi, (i, j, lo, int(ranks[p]), hi)
            checked += 1
    assert checked > 37


# ------------------------------------------------------------ 2. exact order
@gpu
@pytest.mark.parametrize("precision", [ocffm.FP64, ocffm.FP32])
def test_exact_order_and_determinism(precision, monkeypatch, tmp_path):
    """Ranks equal the lexsort order under many ties, for every forced slicing
    and chunking, and when the rows are moved to other positions.  The two
    variables are read when a problem is created, so each setting gets a fresh
    problem on the saved model (as test_recommend's determinism test does)."""
    g0 = tie_problem(precision)
    snap = str(tmp_path / "model.bin")
    g0.save_binary(snap)
    X = g0._keep[1]
    ref, cold = reference(g0, X, False)
    assert max(len(np.unique(r)) for r in ref[~cold]) < ref.shape[1]  # tied
    want, want_nc = exact_ranks(ref, X)
    base = g0.label_ranks(X)
    assert (base[0] == want).all() and (base[2] == want_nc).all()
    yptr, ycol = X.labels()
    for i in range(37):
        for p in range(int(yptr[i]), int(yptr[i + 1])):
            assert base[1][p] == ref[i, int(ycol[p])]
    g0.close()
    ds = dataset(5, "ones")
    # the rows in reverse order: every row at another position (and in another tile half)
    perm = np.arange(36, -1, -1)
    t = ds.test
    cnt = np.diff(t.xptr.astype(np.int64))
    xp = np.zeros(38, dtype=np.uint64)
    xp[1:] = np.cumsum(cnt[perm])
    pick = np.concatenate([np.arange(int(t.xptr[i]), int(t.xptr[i + 1])) for i in perm]).astype(np.int64)
    moved = with_labels(ds, synth.Rows(xp, t.fid[pick], t.idx[pick], t.val[pick], np.zeros(38, dtype=np.uint64),
                                       np.zeros(0, dtype=np.uint64)),
                        {a: list(t.ycol[int(t.yptr[i]):int(t.yptr[i + 1])]) for a, i in enumerate(perm)})
    for slices in ("1", "2", "3"):
        for rows in ("1", "7", "33"):
            monkeypatch.setenv("OCFFM_REC_SLICES", slices)
            monkeypatch.setenv("OCFFM_REC_ROWS", rows)
            g = ocffm.problem_from_dataset(ds, precision=precision, self_side=False)
            g.load_binary(snap)
            got = g.label_ranks(X)
            again = g.label_ranks(X)
            for a, b, c in zip(got, again, base):
                assert (a == b).all() and (a == c).all(), (slices, rows)
            if (slices, rows) in (("1", "1"), ("3", "7"), ("2", "33")):
                Xm = ocffm.ImpData.from_rows(moved, ds=g._keep[0].Ds)
                mr, ms, mn = g.label_ranks(Xm)
                myptr, _ = Xm.labels()
                for a, i in enumerate(perm):
                    sl_m = slice(int(myptr[a]), int(myptr[a + 1]))
                    sl_o = slice(int(yptr[i]), int(yptr[i + 1]))
                    assert (mr[sl_m] == base[0][sl_o]).all() and (ms[sl_m] == base[1][sl_o]).all()
                    assert mn[a] == base[2][i]
            g.close()


# ------------------------------------------------- 3. agreement with recommend
@gpu
@pytest.mark.parametrize("precision", [ocffm.FP64, ocffm.FP32])
def test_agrees_with_recommend(precision):
    g = real_problem(5, precision)
    ds = dataset(5, "real")
    U, X = g._keep[0], g._keep[1]
    n = 70
    yptr, ycol = X.labels()
    ranks, scores, ncand = g.label_ranks(X)
    items, top = g.recommend(X, topn=128)
    assert (ncand == (items != NONE).sum(axis=1)).all()
    seen_ranked = 0
    for i in range(37):
        for p in range(int(yptr[i]), int(yptr[i + 1])):
            if ranks[p] != NONE and ranks[p] < 128:
                assert items[i, ranks[p]] == ycol[p], (i, p)
                assert scores[p] == top[i, ranks[p]], (i, p)  # bit-identical
                seen_ranked += 1
    assert seen_ranked > 37
    # seen rows: each row has seen its first label, three fixed items and one item >= n
    changes = {}
    for i in range(37):
        lab = [int(j) for j in ycol[int(yptr[i]):int(yptr[i + 1])]]
        changes[i] = lab[:1] + [2, 33, 69, n + 4]
    srows = with_labels(ds, ds.test, changes)
    S = ocffm.ImpData.from_rows(srows, ds=U.Ds)
    ranks, scores, ncand = g.label_ranks(X, seen=S)
    items, top = g.recommend(S, topn=128, exclude_labels=True)
    assert (ncand == (items != NONE).sum(axis=1)).all()
    none = ranked = 0
    for i in range(37):
        seen_i = set(changes[i])
        for p in range(int(yptr[i]), int(yptr[i + 1])):
            if int(ycol[p]) in seen_i:
                assert ranks[p] == NONE and scores[p] == -np.inf
                none += 1
            elif ranks[p] != NONE:
                assert items[i, ranks[p]] == ycol[p] and scores[p] == top[i, ranks[p]], (i, p)
                ranked += 1
    assert none >= 37 and ranked > 0


# ------------------------------------------------------- 4. label edge cases
@gpu
@pytest.mark.parametrize("precision", [ocffm.FP64, ocffm.FP32])
def test_label_edge_cases(precision):
    g = tie_problem(precision)
    ds = dataset(5, "ones")
    U = g._keep[0]
    n, npop = 70, int(U.info["n"])
    cold = cold_rows(g._keep[1])
    warm = np.nonzero(~cold)[0]
    c0 = int(np.nonzero(cold)[0][0])
    r_none, r_all, r_dup, r_big = (int(x) for x in warm[:4])
    changes = {r_none: [], r_all: list(range(n)), r_dup: [3, 40, 3, 3, 40, 7], r_big: [5, n, 10 * n, 6],
               c0: [0, npop - 1, npop, n + 1]}
    X = ocffm.ImpData.from_rows(with_labels(ds, ds.test, changes), ds=U.Ds)
    ref, _ = reference(g, X, False)
    want, want_nc = exact_ranks(ref, X)
    ranks, scores, ncand = g.label_ranks(X)
    assert (ranks == want).all() and (ncand == want_nc).all()
    yptr, ycol = X.labels()
    row = lambda i: ranks[int(yptr[i]):int(yptr[i + 1])]
    assert len(row(r_none)) == 0
    assert sorted(row(r_all).tolist()) == list(range(n))  # every place once
    d = row(r_dup)
    assert d[0] == d[2] == d[3] and d[1] == d[4] and len(set(d.tolist())) == 3
    assert row(r_big)[1] == NONE and row(r_big)[2] == NONE and row(r_big)[0] != NONE and row(r_big)[3] != NONE
    assert row(c0)[0] != NONE and row(c0)[1] != NONE and row(c0)[2] == NONE and row(c0)[3] == NONE
    assert ncand[c0] == npop and ncand[r_all] == n
    sc = scores[int(yptr[r_big]):int(yptr[r_big + 1])]
    assert sc[1] == -np.inf and sc[2] == -np.inf and sc[0] == ref[r_big, 5]
    e = g.evaluate(X, cuts=(1, 3, 10, 200))
    w = ocffm.eval_from_ranks(yptr, want, want_nc, scores, cuts=(1, 3, 10, 200))
    assert e["rows_used"] == w["rows_used"] <= 36 and e["labels"] == len(ycol)
    for key in ("prec", "recall", "ndcg", "map", "hit"):
        assert (e[key] == w[key]).all()
    assert e["mrr"] == w["mrr"] and e["auc"] == w["auc"] and e["loss"] == w["loss"]


@gpu
@pytest.mark.parametrize("precision", [ocffm.FP64, ocffm.FP32])
def test_label_count_paths(precision):
    """The count kernel searches a row's labels in LDS up to 16 of them and in
    global memory above, keeps its counters in LDS up to 128 labels and adds to
    the global ones directly above: rows with 0, 1, 16, 17, 100, 128, 129, 200
    and all 300 items as labels, with and without seen items."""
    ds = synth.general(seed=8, m=150, n=300, fu=2, fv=2, k=5, nnz_user=2, vals="ones", test_rows=37)
    g = ocffm.problem_from_dataset(ds, precision=precision, self_side=False)
    ocffm.srand(1)
    g.init()
    integer_tables(g)
    U = g._keep[0]
    n = 300
    warm = np.nonzero(~cold_rows(g._keep[1]))[0]
    rng = np.random.default_rng(3)
    counts = [0, 1, 16, 17, 100, 128, 129, 200, 300]
    assert len(warm) >= len(counts)
    changes = {int(warm[a]): [int(j) for j in rng.permutation(n)[:c]] for a, c in enumerate(counts)}
    X = ocffm.ImpData.from_rows(with_labels(ds, ds.test, changes), ds=U.Ds)
    ref, _ = reference(g, X, False)
    assert max(len(np.unique(r)) for r in ref[warm]) < n  # tied
    want, want_nc = exact_ranks(ref, X)
    ranks, _, ncand = g.label_ranks(X)
    assert (ranks == want).all() and (ncand == want_nc).all()
    S = ocffm.ImpData.from_rows(with_labels(ds, ds.test, {i: [int(j) for j in rng.permutation(n)[:40]]
                                                          for i in range(37)}), ds=U.Ds)
    want, want_nc = exact_ranks(ref, X, seen=S)
    ranks, _, ncand = g.label_ranks(X, seen=S)
    assert (ranks == want).all() and (ncand == want_nc).all()
    assert (ranks == NONE).any() and (ranks != NONE).any()


# ---------------------------------------------- 5. agreement with validate()
@gpu
@pytest.mark.parametrize("precision", [ocffm.FP64, ocffm.FP32])
def test_agrees_with_validate(precision):
    g = tie_problem(precision)
    U, X, V = g._keep
    n = int(V.info["m"])
    yptr, ycol = X.labels()
    ref, _ = reference(g, X, False)
    # the preconditions under which evaluate and validate() define the same numbers
    assert int(U.info["n"]) == n == 70
    assert (np.diff(yptr.astype(np.int64)) >= 1).all() and (ycol < n).all()
    for i in range(37):
        lab = ycol[int(yptr[i]):int(yptr[i + 1])]
        assert len(set(lab.tolist())) == len(lab)
    assert (ref > -1000).all()
    before = g.validate()
    e = g.evaluate(X, cuts=CUTS)
    after = g.validate()
    assert e["rows"] == e["rows_used"] == 37 and e["labels"] == e["labels_ranked"] == len(ycol)
    print(e, before)
    np.testing.assert_allclose(e["prec"], before["prec"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(e["ndcg"], before["ndcg"], rtol=0, atol=1e-12)
    assert abs(e["loss"] - before["loss"]) <= 1e-12
    assert after["loss"] == before["loss"]
    assert (after["prec"] == before["prec"]).all() and (after["ndcg"] == before["ndcg"]).all()


# ------------------------------------------------------ 6. errors and limits
@gpu
def test_errors_and_limits():
    ds = dataset(5, "real")
    g = ocffm.problem_from_dataset(ds, precision=ocffm.FP64, self_side=True)
    U, X = g._keep[0], g._keep[1]

    def code(fn, *a, **kw):
        with pytest.raises(ocffm.OcffmError) as e:
            fn(*a, **kw)
        return e.value.code

    assert code(g.evaluate, X) == ocffm.E_STATE  # before init
    assert code(g.label_ranks, X) == ocffm.E_STATE
    ocffm.srand(1)
    g.init()
    good = g.evaluate(X)
    assert good["cuts"] == list(CUTS) and good["rows_used"] == 37
    assert code(g.evaluate, X, cuts=()) == ocffm.E_ARG
    assert code(g.evaluate, X, cuts=tuple(range(1, 10))) == ocffm.E_ARG
    assert code(g.evaluate, X, cuts=(0, 5)) == ocffm.E_ARG
    assert code(g.evaluate, X, cuts=(5, 5)) == ocffm.E_ARG
    assert code(g.evaluate, X, cuts=(10, 5)) == ocffm.E_ARG
    t = ds.test
    short = ocffm.ImpData.from_rows(synth.Rows(t.xptr[:31], t.fid, t.idx, t.val, t.yptr[:31], t.ycol), ds=U.Ds)
    assert code(g.evaluate, X, seen=short) == ocffm.E_ARG  # seen.m != X.m
    assert code(g.label_ranks, X, seen=short) == ocffm.E_ARG
    nolab = ocffm.ImpData.from_rows(synth.Rows(t.xptr, t.fid, t.idx, t.val), ds=U.Ds)
    assert code(g.evaluate, nolab) == ocffm.E_ARG  # X without labels
    assert code(g.label_ranks, nolab) == ocffm.E_ARG
    lib = ocffm.lib()
    cuts = np.array(CUTS, dtype=np.uint32)
    assert lib.ocffm_problem_evaluate(g.h, X.h, None, cuts.ctypes.data_as(C.c_void_p), 5, None) == ocffm.E_ARG
    assert lib.ocffm_problem_label_ranks(g.h, X.h, None, None, None, None) == ocffm.E_ARG  # NULL ranks
    bad = synth.Rows(t.xptr, t.fid, t.idx.copy(), t.val, t.yptr, t.ycol)
    bad.idx[0] = int(U.Ds[int(bad.fid[0])]) + 3
    assert code(g.evaluate, ocffm.ImpData.from_rows(bad)) == ocffm.E_DATA
    z = np.zeros(0)
    empty = ocffm.ImpData.from_rows(synth.Rows(np.zeros(1, dtype=np.uint64), z.astype(np.uint32),
                                               z.astype(np.uint64), z, np.zeros(1, dtype=np.uint64),
                                               z.astype(np.uint64)), ds=U.Ds)
    e = g.evaluate(empty)
    assert e["rows"] == 0 and e["rows_used"] == 0 and e["mrr"] == 0 and (e["prec"] == 0).all()
    r, s, nc = g.label_ranks(empty)
    assert r.shape == s.shape == nc.shape == (0,)
    after = g.evaluate(X)  # a later valid call still works, and gives the same bits
    assert after["mrr"] == good["mrr"] and after["auc"] == good["auc"] and (after["ndcg"] == good["ndcg"]).all()


# -------------------------------------------------------------------- 7. CLI
@gpu
def test_cli_matches_python(tmp_path):
    tr, it, te = _cli_files(tmp_path)
    base = [TRAIN, "-k", "4", "-t", "2", "--fp64"]
    r = subprocess.run(base + ["--eval", te, "--eval-cuts", "1,5,20", it, tr], capture_output=True, text=True)
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
    e = g.evaluate(X, cuts=(1, 5, 20))
    lines = [ln.split() for ln in r.stdout.split("\n") if ln.startswith("eval ")]
    assert len(lines) == 3 + 3
    assert lines[0] == ["eval", "rows", str(e["rows"]), "rows_used", str(e["rows_used"]), "labels", str(e["labels"]),
                        "labels_ranked", str(e["labels_ranked"])]
    assert lines[1][1::2] == ["loss", "mrr", "auc"]
    for name, tok in zip(("loss", "mrr", "auc"), lines[1][2::2]):
        assert abs(float(tok) - e[name]) <= 1e-12, name
    assert lines[2] == ["eval", "cut", "prec", "recall", "ndcg", "map", "hit"]
    for s, ln in enumerate(lines[3:]):
        assert int(ln[1]) == (1, 5, 20)[s]
        for name, tok in zip(("prec", "recall", "ndcg", "map", "hit"), ln[2:]):
            assert abs(float(tok) - e[name][s]) <= 1e-12, (name, s)
    assert e["rows_used"] == 100 and e["mrr"] > 0
    # the seen file: the test rows themselves, so no label is left to rank
    r2 = subprocess.run(base + ["--eval", te, "--eval-seen", te, it, tr], capture_output=True, text=True)
    assert r2.returncode == 0, r2.stderr
    first = [ln.split() for ln in r2.stdout.split("\n") if ln.startswith("eval ")][0]
    assert first[4] == "0" and first[8] == "0"


def test_cli_usage(tmp_path):
    """Fails before anything is read: no device work, no files needed."""
    missing = str(tmp_path / "nothing")
    for args in (["--eval", missing, "--eval-cuts", "0,5"], ["--eval", missing, "--eval-cuts", "5,5"],
                 ["--eval", missing, "--eval-cuts", "1,2,3,4,5,6,7,8,9"], ["--eval", missing, "--eval-cuts", "5;6"],
                 ["--eval-seen", missing]):
        r = subprocess.run([TRAIN] + args + [missing, missing], capture_output=True, text=True)
        assert r.returncode == 1, (args, r.returncode, r.stderr)
    usage = subprocess.run([TRAIN], capture_output=True, text=True).stderr
    assert "--eval <path>" in usage and "--eval-cuts" in usage and "--eval-seen" in usage


# ------------------------------------------------------------- 8. statistics
@gpu
def test_statistics():
    g = real_problem(5, ocffm.FP32)
    X = g._keep[1]
    g.reset_stats()
    g.set_profiling(True)
    g.evaluate(X)
    g.set_profiling(False)
    st = g.kernel_stats()
    assert st["evaluate"]["launches"] >= 2 and st["evaluate"]["total_ms"] > 0
    assert st["evaluate"]["alg_flops"] > 0 and st["evaluate"]["alg_bytes"] > 0
    assert "recommend" not in st or st["recommend"]["launches"] == 0
    assert g.counter("eval_setup_us") > 0
