"""Label ranks among per-row candidate lists (ocffm_problem_label_ranks_among /
ocffm_problem_evaluate_among, ImpProblem.label_ranks / evaluate with
candidates=, train --eval-candidates).

The contract is bitwise and set-valued: row i's candidate set K_i is the
distinct candidates of its list united with its candidate labels, a label's
rank is its place in K_i under (score descending, item ascending), and every
score is score()'s.  So the expected values are built on the host from
score() over K_i with np.lexsort, or taken from label_ranks when the lists
hold the whole catalogue, and every comparison is exact.
"""
import subprocess

import numpy as np
import pytest

import ocffm
import synth
from test_evaluate import integer_tables
from test_recommend import NONE, TRAIN, _cli_files, cold_rows, dataset, with_labels
from test_rerank import LENGTHS, N, ROWS, lists_of, problem, ragged_lists

gpu = pytest.mark.gpu


# ---------------------------------------------------------------- helpers
def host_among(g, X, per_row, seen=None):
    """ranks, scores, ncand from score() over K_i: the distinct members of the
    list and the labels with a finite score that seen's row does not hold."""
    yptr, ycol = X.labels()
    m = int(X.info["m"])
    if seen is not None:
        sptr, scol = seen.labels()
    mem = []
    for i in range(m):
        s = set(per_row[i]) | {int(j) for j in ycol[int(yptr[i]):int(yptr[i + 1])]}
        if seen is not None:
            s -= {int(j) for j in scol[int(sptr[i]):int(sptr[i + 1])]}
        mem.append(np.array(sorted(j for j in s if j < 2 ** 32 - 1), dtype=np.int64))
    prow = np.concatenate([np.full(len(x), i) for i, x in enumerate(mem)]).astype(np.uint32)
    pitem = np.concatenate(mem).astype(np.uint32)
    sc = g.score(X, prow, pitem) if len(pitem) else np.zeros(0)
    ranks = np.full(len(ycol), NONE, dtype=np.uint32)
    scores = np.full(len(ycol), -np.inf)
    ncand = np.zeros(m, dtype=np.uint32)
    at = 0
    for i in range(m):
        v = sc[at:at + len(mem[i])]
        at += len(mem[i])
        fin = np.isfinite(v)
        items, v = mem[i][fin], v[fin]
        order = np.lexsort((items, -v))
        place = {int(items[o]): (t, v[o]) for t, o in enumerate(order)}
        ncand[i] = len(items)
        for p in range(int(yptr[i]), int(yptr[i + 1])):
            if int(ycol[p]) in place:
                ranks[p], scores[p] = place[int(ycol[p])]
    return ranks, scores, ncand


def same3(got, want):
    return all((a == b).all() for a, b in zip(got, want))


def seen_file(g, k=5):
    """Each row has seen its first label, three fixed items and one item >= n
    (test_evaluate.test_agrees_with_recommend's seen rows)."""
    ds = dataset(k, "real")
    yptr, ycol = g._keep[1].labels()
    changes = {i: [int(j) for j in ycol[int(yptr[i]):int(yptr[i + 1])]][:1] + [2, 33, 69, N + 4] for i in range(ROWS)}
    return ocffm.ImpData.from_rows(with_labels(ds, ds.test, changes), ds=g._keep[0].Ds)


def label_sets(X):
    yptr, ycol = X.labels()
    return [[int(j) for j in ycol[int(yptr[i]):int(yptr[i + 1])]] for i in range(int(X.info["m"]))]


# -------------------------------------------------------- 1. whole catalogue
@gpu
@pytest.mark.parametrize("k", [5, 32])
@pytest.mark.parametrize("precision", [ocffm.FP64, ocffm.FP32])
def test_whole_catalogue_equals_label_ranks(k, precision):
    g = problem("real", k, precision)
    X = g._keep[1]
    cold = cold_rows(X)
    assert cold.any() and not cold.all()
    rng = np.random.default_rng(5)
    per_row = []
    for i in range(ROWS):
        x = np.concatenate([rng.permutation(N), rng.integers(0, N, size=9), rng.integers(N, 10 * N + 1, size=7)])
        per_row.append([int(j) for j in rng.permutation(x)])
    cand = lists_of(per_row)
    for seen in (None, seen_file(g, k)):
        want = g.label_ranks(X, seen=seen)
        got = g.label_ranks(X, seen=seen, candidates=cand)
        assert got[0].dtype == np.uint32 and got[1].dtype == np.float64 and got[2].dtype == np.uint32
        assert same3(got, want), seen is not None
        assert (want[0] != NONE).any()


# ------------------------------------------------------------ 2. ragged lists
@gpu
@pytest.mark.parametrize("with_seen", [False, True])
@pytest.mark.parametrize("precision", [ocffm.FP64, ocffm.FP32])
@pytest.mark.parametrize("k", [5, 32])
def test_ragged_lists(k, precision, with_seen):
    g = problem("real", k, precision)
    X = g._keep[1]
    per_row = ragged_lists(17)
    labs = label_sets(X)
    assert {len(x) for x in per_row} == set(LENGTHS)
    assert any(len(set(x)) < len(x) for x in per_row) and any(j >= N for x in per_row for j in x)
    assert any(j not in per_row[i] for i in range(ROWS) for j in labs[i])
    assert any(j in per_row[i] for i in range(ROWS) for j in labs[i])
    seen = seen_file(g, k) if with_seen else None
    want = host_among(g, X, per_row, seen)
    got = g.label_ranks(X, seen=seen, candidates=lists_of(per_row))
    assert same3(got, want)
    yptr, ycol = X.labels()
    lrow = np.repeat(np.arange(ROWS), np.diff(yptr.astype(np.int64)))
    ranked = got[0] != NONE
    assert ranked.any() and (got[1][ranked] == g.score(X, lrow, ycol)[ranked]).all()
    if seen is not None:
        assert (~ranked).any()
    # an empty list: the row's candidate labels alone
    empties = [i for i in range(ROWS) if not per_row[i]]
    assert empties
    for i in empties:
        assert got[2][i] == len({int(ycol[p]) for p in range(int(yptr[i]), int(yptr[i + 1])) if ranked[p]})


# -------------------------------------------------------------------- 3. ties
@gpu
@pytest.mark.parametrize("precision", [ocffm.FP64, ocffm.FP32])
def test_ties(precision):
    g = problem("ties", 5, precision)
    X = g._keep[1]
    per_row = ragged_lists(19)
    labs = label_sets(X)
    want = host_among(g, X, per_row)
    got = g.label_ranks(X, candidates=lists_of(per_row))
    assert same3(got, want)
    # some candidate ties with a label in score: the item index decides
    tied = 0
    for i in range(ROWS):
        others = sorted({j for j in per_row[i] if j < N} - set(labs[i]))
        if not others or not labs[i]:
            continue
        so = g.score(X, [i] * len(others), others)
        sl = g.score(X, [i] * len(labs[i]), labs[i])
        tied += int(np.isin(sl[np.isfinite(sl)], so).sum())
    assert tied > 0


# ------------------------------------------------------------ 4. label counts
@gpu
@pytest.mark.parametrize("precision", [ocffm.FP64, ocffm.FP32])
def test_label_counts(precision):
    """test_evaluate.test_label_count_paths' n = 300 problem: rows with 0, 1,
    16, 17, 128, 129 and 300 labels, lists of 150 random entries."""
    ds = synth.general(seed=8, m=150, n=300, fu=2, fv=2, k=5, nnz_user=2, vals="ones", test_rows=37)
    g = ocffm.problem_from_dataset(ds, precision=precision, self_side=False)
    ocffm.srand(1)
    g.init()
    integer_tables(g)
    U = g._keep[0]
    n = 300
    warm = np.nonzero(~cold_rows(g._keep[1]))[0]
    rng = np.random.default_rng(3)
    counts = [0, 1, 16, 17, 128, 129, 300]
    assert len(warm) >= len(counts)
    changes = {int(warm[a]): [int(j) for j in rng.permutation(n)[:c]] for a, c in enumerate(counts)}
    X = ocffm.ImpData.from_rows(with_labels(ds, ds.test, changes), ds=U.Ds)
    per_row = [[int(j) for j in rng.integers(0, n + 30, size=150)] for _ in range(37)]
    want = host_among(g, X, per_row)
    got = g.label_ranks(X, candidates=lists_of(per_row))
    assert same3(got, want)
    assert got[2][int(warm[6])] == n and got[2][int(warm[0])] == len({j for j in per_row[int(warm[0])] if j < n})
    S = ocffm.ImpData.from_rows(with_labels(ds, ds.test, {i: [int(j) for j in rng.permutation(n)[:40]]
                                                          for i in range(37)}), ds=U.Ds)
    want = host_among(g, X, per_row, S)
    got = g.label_ranks(X, seen=S, candidates=lists_of(per_row))
    assert same3(got, want)
    assert (got[0] == NONE).any() and (got[0] != NONE).any()
    g.close()


# ----------------------------------------------------------------- 5. cutting
@gpu
@pytest.mark.parametrize("precision", [ocffm.FP64, ocffm.FP32])
def test_cutting(precision, monkeypatch, tmp_path):
    """OCFFM_REC_SEG and OCFFM_REC_ROWS are read when a problem is created, so
    each setting gets a fresh problem on the saved model."""
    snap = str(tmp_path / "model.bin")
    g0 = problem("real", 5, precision)
    g0.save_binary(snap)
    X0 = g0._keep[1]
    labs = label_sets(X0)
    warm = np.nonzero(~cold_rows(X0))[0]
    r, c = (int(i) for i in [i for i in warm if labs[i]][:2])
    per_row = ragged_lists(17)
    per_row[c] = [41] * 40 + per_row[c]  # a run of equal entries spans whole segments of 16 and 32
    per_row[r] = []
    other = [list(x) for x in per_row]
    other[r] = list(range(40))
    rng = np.random.default_rng(4)
    shuffled = [[int(j) for j in rng.permutation(x)] for x in per_row]
    def work_items(res, seg):
        yptr, _ = X0.labels()
        return sum(-(-int(res[2][i]) // seg) for i in range(ROWS)
                   if (res[0][int(yptr[i]):int(yptr[i + 1])] != NONE).any())

    results = []
    for seg in (None, "16", "32"):
        for rows in (None, "5"):
            for name, val in (("OCFFM_REC_SEG", seg), ("OCFFM_REC_ROWS", rows)):
                if val is None:
                    monkeypatch.delenv(name, raising=False)
                else:
                    monkeypatch.setenv(name, val)
            g = ocffm.problem_from_dataset(dataset(5, "real"), precision=precision, self_side=True)
            g.load_binary(snap)
            X = g._keep[1]
            got = [g.label_ranks(X, candidates=lists_of(x)) for x in (per_row, other, shuffled)]
            if not results:  # the defaults, against the host construction
                assert same3(got[0], host_among(g, X, per_row)) and same3(got[1], host_among(g, X, other))
                # the two calls' work items differ by 2: one count is no multiple of the 4 waves of a block
                assert work_items(got[1], 16) - work_items(got[0], 16) == 2
            assert same3(got[2], got[0]), (seg, rows)
            results.append(got)
            g.close()
    for got in results[1:]:
        assert same3(got[0], results[0][0]) and same3(got[1], results[0][1])


# ------------------------------------------------- 6. agreement with recommend
@gpu
@pytest.mark.parametrize("precision", [ocffm.FP64, ocffm.FP32])
def test_agrees_with_recommend(precision):
    g = problem("real", 5, precision)
    X = g._keep[1]
    per_row = ragged_lists(17)
    labs = label_sets(X)
    ranks, scores, ncand = g.label_ranks(X, candidates=lists_of(per_row))
    items, top = g.recommend(X, topn=128, candidates=lists_of([per_row[i] + labs[i] for i in range(ROWS)]))
    assert (ncand == (items != NONE).sum(axis=1)).all()
    yptr, ycol = X.labels()
    checked = 0
    for i in range(ROWS):
        for p in range(int(yptr[i]), int(yptr[i + 1])):
            if ranks[p] != NONE and ranks[p] < 128:
                assert items[i, ranks[p]] == ycol[p] and scores[p] == top[i, ranks[p]], (i, p)
                checked += 1
    assert checked > ROWS


# --------------------------------------------------------------- 7. evaluate
@gpu
@pytest.mark.parametrize("precision", [ocffm.FP64, ocffm.FP32])
def test_evaluate_among(precision):
    g = problem("real", 5, precision)
    X = g._keep[1]
    cand = lists_of(ragged_lists(17))
    cuts = (1, 5, 20)
    for seen in (None, seen_file(g)):
        r, s, nc = g.label_ranks(X, seen=seen, candidates=cand)
        e = g.evaluate(X, cuts=cuts, seen=seen, candidates=cand)
        w = ocffm.eval_from_ranks(X.labels()[0], r, nc, scores=s, cuts=cuts)
        assert e.keys() == w.keys()
        for key in e:
            assert (np.asarray(e[key]) == np.asarray(w[key])).all(), key
    assert e["rows"] == ROWS and 0 < e["rows_used"] <= ROWS


# ----------------------------------------------------------------- 8. errors
@gpu
def test_errors():
    ds = dataset(5, "real")
    g = ocffm.problem_from_dataset(ds, precision=ocffm.FP64, self_side=True)
    U, X = g._keep[0], g._keep[1]
    cptr, ccol = lists_of(ragged_lists(17))
    yptr, ycol = X.labels()
    L = ocffm.lib()

    def code(fn, *a, **kw):
        with pytest.raises(ocffm.OcffmError) as e:
            fn(*a, **kw)
        return e.value.code

    def raw(cp, cc, ranks=True):
        cp = None if cp is None else np.ascontiguousarray(cp, dtype=np.uint64)
        cc = None if cc is None else np.ascontiguousarray(cc, dtype=np.uint32)
        rk = np.zeros(len(ycol), dtype=np.uint32)
        return L.ocffm_problem_label_ranks_among(g.h, X.h, None, ocffm._ptr(cp), ocffm._ptr(cc),
                                                 ocffm._ptr(rk) if ranks else None, None, None)

    assert code(g.label_ranks, X, candidates=(cptr, ccol)) == ocffm.E_STATE  # before init
    assert code(g.evaluate, X, candidates=(cptr, ccol)) == ocffm.E_STATE
    ocffm.srand(1)
    g.init()
    good = g.label_ranks(X, candidates=(cptr, ccol))
    assert raw(cptr, ccol) == ocffm.OK  # NULL scores and ncand
    assert raw(None, ccol) == ocffm.E_ARG
    bad0 = cptr.copy()
    bad0[0] = 1
    assert raw(bad0, ccol) == ocffm.E_ARG
    dec = cptr.copy()
    dec[3] = dec[2] - 1
    assert raw(dec, ccol) == ocffm.E_ARG
    assert raw(cptr, None) == ocffm.E_ARG
    assert raw(np.zeros(ROWS + 1), None) == ocffm.OK  # empty lists need no ccol
    assert raw(cptr, ccol, ranks=False) == ocffm.E_ARG
    assert code(g.label_ranks, X, candidates=(cptr[:-1], ccol)) == ocffm.E_ARG  # not m + 1 offsets
    assert code(g.evaluate, X, cuts=(5, 5), candidates=(cptr, ccol)) == ocffm.E_ARG
    assert code(g.evaluate, X, cuts=(), candidates=(cptr, ccol)) == ocffm.E_ARG
    t = ds.test
    short = ocffm.ImpData.from_rows(synth.Rows(t.xptr[:31], t.fid, t.idx, t.val, t.yptr[:31], t.ycol), ds=U.Ds)
    assert code(g.label_ranks, X, seen=short, candidates=(cptr, ccol)) == ocffm.E_ARG
    nolab = ocffm.ImpData.from_rows(synth.Rows(t.xptr, t.fid, t.idx, t.val), ds=U.Ds)
    assert code(g.label_ranks, nolab, candidates=(cptr, ccol)) == ocffm.E_ARG
    bad = synth.Rows(t.xptr, t.fid, t.idx.copy(), t.val, t.yptr, t.ycol)
    bad.idx[0] = int(U.Ds[int(bad.fid[0])]) + 3
    assert code(g.label_ranks, ocffm.ImpData.from_rows(bad), candidates=(cptr, ccol)) == ocffm.E_DATA
    z = np.zeros(0)
    empty = ocffm.ImpData.from_rows(synth.Rows(np.zeros(1, dtype=np.uint64), z.astype(np.uint32),
                                               z.astype(np.uint64), z, np.zeros(1, dtype=np.uint64),
                                               z.astype(np.uint64)), ds=U.Ds)
    none = (np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    r, s, nc = g.label_ranks(empty, candidates=none)
    assert r.shape == s.shape == nc.shape == (0,)
    assert g.evaluate(empty, candidates=none)["rows"] == 0
    assert same3(g.label_ranks(X, candidates=(cptr, ccol)), good)  # a later valid call gives the same bits
    g.close()


# -------------------------------------------------------------------- 9. CLI
def _write_lists(path, per_row):
    with open(path, "w") as f:
        for x in per_row:
            f.write(" ".join(str(j) for j in x) + "\n")


@gpu
def test_cli_matches_python(tmp_path):
    tr, it, te = _cli_files(tmp_path)
    cand = str(tmp_path / "cand.txt")
    per_row = ragged_lists(29, rows=100, n=50)
    _write_lists(cand, per_row)
    r = subprocess.run([TRAIN, "-k", "4", "-t", "2", "--fp64", "--eval", te, "--eval-cuts", "1,5,20",
                        "--eval-candidates", cand, it, tr], capture_output=True, text=True)
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
    e = g.evaluate(X, cuts=(1, 5, 20), candidates=lists_of(per_row))
    full = g.evaluate(X, cuts=(1, 5, 20))
    assert e["mrr"] != full["mrr"]  # (the lists matter)
    lines = [ln.split() for ln in r.stdout.split("\n") if ln.startswith("eval ")]
    assert len(lines) == 3 + 3
    assert lines[0] == ["eval", "rows", str(e["rows"]), "rows_used", str(e["rows_used"]), "labels", str(e["labels"]),
                        "labels_ranked", str(e["labels_ranked"])]
    for name, tok in zip(("loss", "mrr", "auc"), lines[1][2::2]):
        assert abs(float(tok) - e[name]) <= 1e-12, name
    for s, ln in enumerate(lines[3:]):
        assert int(ln[1]) == (1, 5, 20)[s]
        for name, tok in zip(("prec", "recall", "ndcg", "map", "hit"), ln[2:]):
            assert abs(float(tok) - e[name][s]) <= 1e-12, (name, s)
    g.close()


def test_cli_usage_errors(tmp_path):
    """--eval-candidates without --eval fails before anything is read; a wrong
    line count fails before any device work (this test has no GPU)."""
    missing = str(tmp_path / "nothing")
    r = subprocess.run([TRAIN, "--eval-candidates", missing, missing, missing], capture_output=True, text=True)
    assert r.returncode == 1 and "--eval" in r.stderr, (r.returncode, r.stderr)
    assert "--eval-candidates" in subprocess.run([TRAIN], capture_output=True, text=True).stderr
    tr, it, te = _cli_files(tmp_path)
    cand = str(tmp_path / "short")
    _write_lists(cand, [[1, 2, 3]] * 99)
    r = subprocess.run([TRAIN, "--eval", te, "--eval-candidates", cand, it, tr], capture_output=True, text=True)
    assert r.returncode == 1 and "short" in r.stderr and "--eval file" in r.stderr, (r.returncode, r.stderr)
    assert "eval " not in r.stdout
