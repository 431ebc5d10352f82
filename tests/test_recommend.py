"""Top-N recommendation (ocffm_problem_recommend / ImpProblem.recommend / train --recommend).

The reference scores are numpy fp64 products of the problem's own tables
(W / H through get(), the per-field CSR of X through ImpData.field(), Q and b
through get()), independent of the fused score-and-select kernels.

Tolerances (assert_topn): 1e-12 * max(1, max|ref|) in fp64 (the project's
per-kernel fp64 bound; the depth is at most 4 blocks x 32 terms here) and
1e-3 * max(1, max|ref|) in fp32 (the stated fp32 contract).  The tie tests use
integer tables, whose scores are exact in both precisions whatever the
summation order, and compare exactly.
"""
import os
import subprocess

import numpy as np
import pytest

import ocffm
import synth

gpu = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(REPO, "one-class-ffm_amd", "train")
NONE = 0xFFFFFFFF


# ------------------------------------------------------------ reference
def field_matrix(X, fi, D):
    """Dense rows x D matrix of field fi of X (duplicates add, as utx does)."""
    m = int(X.info["m"])
    A = np.zeros((m, D))
    if fi < X.info["f"]:
        xptr, xidx, xval = X.field(fi)
        rows = np.repeat(np.arange(m), np.diff(xptr))
        np.add.at(A, (rows, xidx), xval)
    return A


def popularity(U):
    _, ycol = U.labels()
    cnt = np.bincount(ycol.astype(np.int64), minlength=int(U.info["n"])).astype(np.float64)
    return cnt / cnt.sum()


def cold_rows(X):
    m = int(X.info["m"])
    kept = np.zeros(m, dtype=np.int64)
    for fi in range(int(X.info["f"])):
        kept += np.diff(X.field(fi)[0])
    return kept == 0


def reference(g, X, self_side):
    """ref[i, j]: a_i + b_j + sum_c <P_c[i], Q_c[j]>; cold rows: popular[j]
    for j < npop and -inf (not a candidate) beyond."""
    U, _, V = g._keep
    fu, fv, f, k = int(U.info["f"]), int(V.info["f"]), g.f, g.k
    n, m = int(V.info["m"]), int(X.info["m"])
    Ds = [int(d) for d in U.Ds]
    ref = np.zeros((m, n)) + g.get("b")[None, :]
    for f1 in range(fu):
        A = field_matrix(X, f1, Ds[f1])
        for f2 in range(fu, f):
            b12 = ocffm.block_index(f1, f2, f)
            P = A @ g.get("W", b12).reshape(Ds[f1], k)
            ref += P @ g.get("Q", b12).reshape(n, k).T
    if self_side:
        a = np.zeros(m)
        for f1 in range(fu):
            for f2 in range(f1, fu):
                b12 = ocffm.block_index(f1, f2, f)
                a += ((field_matrix(X, f1, Ds[f1]) @ g.get("W", b12).reshape(Ds[f1], k)) *
                      (field_matrix(X, f2, Ds[f2]) @ g.get("H", b12).reshape(Ds[f2], k))).sum(axis=1)
        ref += a[:, None]
    cold = cold_rows(X)
    pop = popularity(U)
    for i in np.nonzero(cold)[0]:
        ref[i, :] = -np.inf
        ref[i, :len(pop)] = pop
    return ref, cold


def excluded_sets(X, n, on):
    yptr, ycol = X.labels()
    out = []
    for i in range(int(X.info["m"])):
        lab = ycol[int(yptr[i]):int(yptr[i + 1])] if on else []
        out.append({int(j) for j in lab if j < n})
    return out


def exact_topn(ref_row, topn, excluded):
    n = len(ref_row)
    order = np.lexsort((np.arange(n), -ref_row))
    keep = [j for j in order if np.isfinite(ref_row[j]) and int(j) not in excluded][:topn]
    items = np.full(topn, NONE, dtype=np.uint32)
    scores = np.full(topn, -np.inf)
    items[:len(keep)] = keep
    scores[:len(keep)] = ref_row[keep]
    return items, scores


def assert_topn(items, scores, ref, tol, excluded):
    """The rank check for real-valued models (per row)."""
    m, n = ref.shape
    topn = items.shape[1]
    assert scores.shape == items.shape and m == items.shape[0]
    for i in range(m):
        cand = [j for j in range(n) if np.isfinite(ref[i, j]) and j not in excluded[i]]
        filled = items[i] != NONE
        nf = int(filled.sum())
        assert filled[:nf].all() and nf == min(topn, len(cand)), (i, nf, len(cand))
        assert (scores[i, nf:] == -np.inf).all()
        it = items[i, :nf].astype(np.int64)
        sc = scores[i, :nf]
        assert len(set(it.tolist())) == nf and (it < n).all()
        assert not (set(it.tolist()) - set(cand)), i
        assert (np.diff(sc) <= 0).all(), i
        eq = np.diff(sc) == 0
        assert (np.diff(it)[eq] > 0).all(), i
        err = np.abs(sc - ref[i, it]).max() if nf else 0.0
        assert err <= tol, (i, err, tol)
        rest = sorted(set(cand) - set(it.tolist()))
        if rest:
            assert ref[i, rest].max() <= sc[-1] + 2 * tol, (i, ref[i, rest].max(), sc[-1])


def tol_for(precision, ref):
    big = max(1.0, float(np.abs(ref[np.isfinite(ref)]).max()))
    return (1e-12 if precision == ocffm.FP64 else 1e-3) * big


# ----------------------------------------------------------------- setups
_DS = {}


def dataset(k, vals):
    key = (k, vals)
    if key not in _DS:
        _DS[key] = synth.general(seed=5, m=300, n=70, fu=2, fv=2, k=k, nnz_user=2, vals=vals, test_rows=37)
    return _DS[key]


def real_problem(k, precision):
    """Test 1's setup: init and one epoch, self_side on."""
    g = ocffm.problem_from_dataset(dataset(k, "real"), precision=precision, self_side=True)
    ocffm.srand(1)
    g.init()
    g.one_epoch()
    return g


def tie_problem(precision):
    """Test 2's setup: unit values, no side blocks, integer W / H in [-3, 3]."""
    g = ocffm.problem_from_dataset(dataset(5, "ones"), precision=precision, self_side=False)
    ocffm.srand(1)
    g.init()
    rng = np.random.default_rng(11)
    fu = int(g._keep[0].info["f"])
    for f1 in range(fu):
        for f2 in range(fu, g.f):
            b12 = ocffm.block_index(f1, f2, g.f)
            for what in "WH":
                g.set(what, b12, rng.integers(-3, 4, size=g.get(what, b12).size).astype(np.float64))
    return g


def with_labels(ds, X_rows, changes):
    """A copy of X_rows with the label lists of some rows replaced."""
    labs = [list(X_rows.ycol[int(X_rows.yptr[i]):int(X_rows.yptr[i + 1])]) for i in range(X_rows.m)]
    for i, lab in changes.items():
        labs[i] = list(lab)
    yptr = np.zeros(X_rows.m + 1, dtype=np.uint64)
    yptr[1:] = np.cumsum([len(x) for x in labs])
    ycol = np.array([j for lab in labs for j in lab], dtype=np.uint64)
    return synth.Rows(X_rows.xptr, X_rows.fid, X_rows.idx, X_rows.val, yptr, ycol)


# ------------------------------------------------------------------ tests
@gpu
@pytest.mark.parametrize("k", [5, 32])
@pytest.mark.parametrize("precision", [ocffm.FP64, ocffm.FP32])
def test_parity_ragged_shapes(k, precision):
    g = real_problem(k, precision)
    X = g._keep[1]
    ref, cold = reference(g, X, True)
    assert cold.any() and not cold.all()
    n = ref.shape[1]
    pop = popularity(g._keep[0])
    tol = tol_for(precision, ref)
    none = excluded_sets(X, n, False)
    for topn in (1, 10, 64, 65, 128):
        items, scores = g.recommend(X, topn=topn)
        assert items.dtype == np.uint32 and items.shape == (37, topn)
        assert_topn(items, scores, ref, tol, none)
        for i in np.nonzero(cold)[0]:  # popularity ranking, exactly
            ei, es = exact_topn(ref[i], topn, set())
            assert (items[i] == ei).all() and (scores[i] == es).all()
            assert (scores[i][items[i] != NONE] == pop[items[i][items[i] != NONE]]).all()


@gpu
@pytest.mark.parametrize("k,n", [(3, 70), (16, 70), (64, 70), (100, 70), (8, 1500)])
@pytest.mark.parametrize("precision", [ocffm.FP64, ocffm.FP32])
def test_every_padded_k(k, n, precision):
    """KP = 4, 16, 64, 128 (8 and 32 run above), and an item count at which
    the default slicing splits the items (n = 1500: 6 slices), on the drawn
    tables (init, no epoch)."""
    ds = synth.general(seed=6, m=120, n=n, fu=2, fv=2, k=k, nnz_user=2, vals="real", test_rows=37)
    g = ocffm.problem_from_dataset(ds, precision=precision, self_side=True)
    ocffm.srand(1)
    g.init()
    X = g._keep[1]
    ref, _ = reference(g, X, True)
    items, scores = g.recommend(X, topn=10)
    assert_topn(items, scores, ref, tol_for(precision, ref), excluded_sets(X, n, False))


@gpu
@pytest.mark.parametrize("precision", [ocffm.FP64, ocffm.FP32])
def test_exact_order_under_ties(precision):
    g = tie_problem(precision)
    X = g._keep[1]
    ref, cold = reference(g, X, False)
    warm = ref[~cold]
    assert (warm == np.round(warm)).all()
    assert max(len(np.unique(r)) for r in warm) < ref.shape[1]  # tied
    for topn in (1, 7, 70):
        items, scores = g.recommend(X, topn=topn)
        for i in range(ref.shape[0]):
            ei, es = exact_topn(ref[i], topn, set())
            assert (items[i] == ei).all(), (i, topn)
            assert (scores[i] == es).all(), (i, topn)


@gpu
@pytest.mark.parametrize("case", ["real", "ties"])
def test_exclusion(case):
    g = real_problem(5, ocffm.FP64) if case == "real" else tie_problem(ocffm.FP64)
    ds = dataset(5, "real" if case == "real" else "ones")
    U = g._keep[0]
    n = 70
    warm = np.nonzero(~cold_rows(g._keep[1]))[0]
    r_big, r_most = int(warm[0]), int(warm[1])
    base = list(ds.test.ycol[int(ds.test.yptr[r_big]):int(ds.test.yptr[r_big + 1])])
    left = {3, 40, 69}
    rows = with_labels(ds, ds.test, {r_big: base + [n + 5, 10 * n], r_most: [j for j in range(n) if j not in left]})
    X = ocffm.ImpData.from_rows(rows, ds=U.Ds)
    ref, cold = reference(g, X, case == "real")
    excl = excluded_sets(X, n, True)
    assert excl[r_big] == set(int(j) for j in base) and len(excl[r_most]) == n - 3
    for topn in (7, 70):
        items, scores = g.recommend(X, topn=topn, exclude_labels=True)
        for i in range(ref.shape[0]):
            got = set(items[i][items[i] != NONE].tolist())
            assert not (got & excl[i]), i
        assert set(items[r_most][:3].tolist()) == left
        assert (items[r_most][3:] == NONE).all() and (scores[r_most][3:] == -np.inf).all()
        if case == "ties":
            for i in range(ref.shape[0]):
                ei, es = exact_topn(ref[i], topn, excl[i])
                assert (items[i] == ei).all() and (scores[i] == es).all(), (i, topn)
        else:
            assert_topn(items, scores, ref, tol_for(ocffm.FP64, ref), excl)


@gpu
def test_agrees_with_validate():
    ds = synth.tiny()
    g = ocffm.problem_from_dataset(ds, precision=ocffm.FP64)
    ocffm.srand(1)
    g.init()
    g.one_epoch()
    U, X, V = g._keep
    n = int(V.info["m"])
    assert int(U.info["n"]) == n == 50 and not cold_rows(X).any()
    ref, _ = reference(g, X, True)
    top = -np.sort(-ref, axis=1)[:, :51]
    assert (np.abs(np.diff(top, axis=1)) > 1e-9).all()  # a property of the input: no near-ties
    items, _ = g.recommend(X, topn=80)
    yptr, ycol = X.labels()
    cuts = [5, 10, 20, 40, 80]
    m = items.shape[0]
    prec, ndcg = np.zeros(5), np.zeros(5)
    for i in range(m):
        lab = set(int(j) for j in ycol[int(yptr[i]):int(yptr[i + 1])])
        hit = np.array([it != NONE and int(it) in lab for it in items[i]], dtype=np.float64)
        gain = 1.0 / np.log2(np.arange(80) + 2.0)
        for s, c in enumerate(cuts):
            prec[s] += hit[:c].sum()
            ndcg[s] += (hit[:c] * gain[:c]).sum() / gain[:min(len(lab), c)].sum()
    prec /= m * np.array(cuts, dtype=np.float64)
    ndcg /= m
    v = g.validate()
    np.testing.assert_allclose(prec, v["prec"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(ndcg, v["ndcg"], rtol=0, atol=1e-12)


@gpu
@pytest.mark.parametrize("precision", [ocffm.FP64, ocffm.FP32])
def test_slicing_chunking_determinism(precision, monkeypatch, tmp_path):
    snap = str(tmp_path / "model.bin")
    real_problem(5, precision).save_binary(snap)
    results = []
    for slices in (None, "1", "3"):
        for rows in (None, "5"):
            for name, val in (("OCFFM_REC_SLICES", slices), ("OCFFM_REC_ROWS", rows)):
                if val is None:
                    monkeypatch.delenv(name, raising=False)
                else:
                    monkeypatch.setenv(name, val)
            g = ocffm.problem_from_dataset(dataset(5, "real"), precision=precision, self_side=True)
            g.load_binary(snap)
            X = g._keep[1]
            b12 = ocffm.block_index(0, 2, g.f)
            w0 = g.get("W", b12)
            full = g.recommend(X, topn=10)
            again = g.recommend(X, topn=10)
            part = g.recommend(X, topn=10, row0=5, rows=18)
            assert (g.get("W", b12) == w0).all()
            assert (full[0] == again[0]).all() and (full[1] == again[1]).all()
            assert (part[0] == full[0][5:23]).all() and (part[1] == full[1][5:23]).all()
            results.append(full)
            g.close()
    for it, sc in results[1:]:
        assert (it == results[0][0]).all() and (sc == results[0][1]).all()
    assert (results[0][0] != NONE).all()


@gpu
def test_errors():
    ds = dataset(5, "real")
    g = ocffm.problem_from_dataset(ds, precision=ocffm.FP64, self_side=True)
    X = g._keep[1]

    def code(**kw):
        with pytest.raises(ocffm.OcffmError) as e:
            g.recommend(X, **kw)
        return e.value.code

    assert code(topn=10) == ocffm.E_STATE  # before init
    ocffm.srand(1)
    g.init()
    good = g.recommend(X, topn=10)
    assert code(topn=0) == ocffm.E_ARG
    assert code(topn=129) == ocffm.E_ARG
    assert code(topn=10, row0=30, rows=8) == ocffm.E_ARG
    # built without the train Ds: an out-of-range index is kept
    bad = synth.Rows(ds.test.xptr, ds.test.fid, ds.test.idx.copy(), ds.test.val, ds.test.yptr, ds.test.ycol)
    bad.idx[0] = int(g._keep[0].Ds[int(bad.fid[0])]) + 3
    Xbad = ocffm.ImpData.from_rows(bad)
    with pytest.raises(ocffm.OcffmError) as e:
        g.recommend(Xbad, topn=10)
    assert e.value.code == ocffm.E_DATA
    items, scores = g.recommend(X, topn=10, rows=0)
    assert items.shape == (0, 10) and scores.shape == (0, 10)
    after = g.recommend(X, topn=10)  # a later valid call still works
    assert (after[0] == good[0]).all() and (after[1] == good[1]).all()


def _cli_files(tmp_path):
    ds = synth.tiny()
    tr, it, te = (str(tmp_path / x) for x in ("tr", "item", "te"))
    ds.train.write(tr)
    ds.item.write(it)
    ds.test.write(te)
    return tr, it, te


@gpu
def test_cli_matches_python(tmp_path):
    tr, it, te = _cli_files(tmp_path)
    out = str(tmp_path / "out.txt")
    r = subprocess.run([TRAIN, "-k", "4", "-t", "2", "--fp64", "--recommend", te, "--topn", "7", "--rec-unseen",
                        "--rec-out", out, it, tr], capture_output=True, text=True)
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
    items, scores = g.recommend(X, topn=7, exclude_labels=True)
    lines = open(out).read().split("\n")
    assert lines[-1] == "" and len(lines) - 1 == int(X.info["m"]) == 100
    for i, line in enumerate(lines[:-1]):
        toks = line.split()
        assert len(toks) <= 7
        nf = int((items[i] != NONE).sum())
        assert len(toks) == nf
        assert [int(t.split(":")[0]) for t in toks] == items[i, :nf].tolist(), i
        assert [float(t.split(":")[1]) for t in toks] == [float("%.17g" % s) for s in scores[i, :nf]], i


def test_cli_usage_errors(tmp_path):
    """Fails before anything is read: no device work, no files needed."""
    missing = str(tmp_path / "nothing")
    out = str(tmp_path / "out.txt")
    for args in (["--recommend", missing],
                 ["--recommend", missing, "--rec-out", out, "--topn", "0"],
                 ["--recommend", missing, "--rec-out", out, "--topn", "129"]):
        r = subprocess.run([TRAIN] + args + [missing, missing], capture_output=True, text=True)
        assert r.returncode == 1, (args, r.returncode, r.stderr)
        assert not os.path.exists(out)
    assert "--recommend" in subprocess.run([TRAIN], capture_output=True, text=True).stderr
