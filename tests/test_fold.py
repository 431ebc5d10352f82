"""Folding new users in from their history (ocffm_model_fold_in and the _fold
serving entries / Model.fold_in, fold= / predict --fold-*).

The reference is tests/fold_ref.py: the normal equations in numpy fp64 on the
model's own tables (Model.get('Q'), Model.get('b'), and P, a formed from W / H
as test_model's model_reference forms them).

Tolerances of delta: 1e-9 * max(1, max|delta_ref|) in fp64, the project's fp64
parity contract; every case asserts cond(A_i) <= 1e4 on the reference side, so
the bound rests on the input (eps * cond ~ 1e-12) and not on the code under
test.  1e-3 * max(1, max|delta_ref|) in fp32, the project's fp32 contract: the
fold's own arithmetic is fp64, the slack covers the fp32 projection and Gram
tiles.  The serving checks compare with ref + <delta_i, q_j> under
test_recommend's tol_for, delta being fold_in's (whose parity is asserted
separately): they test the apply step and the serving chain.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import ocffm
import synth
from fold_ref import fold_gradient, fold_objective, fold_reference, normal_equations
from test_model import PREDICT, cross_blocks, model_reference
from test_recommend import (NONE, assert_topn, cold_rows, dataset, excluded_sets, field_matrix, popularity,
                            real_problem, tol_for, with_labels)

gpu = pytest.mark.gpu

PRECISIONS = [ocffm.FP64, ocffm.FP32]
N = 70
OMEGA, LAM, R = 0.1, 0.1, -1.0


# ---------------------------------------------------------------- helpers
def delta_tol(precision, ref):
    return (1e-9 if precision == ocffm.FP64 else 1e-3) * max(1.0, float(np.abs(ref).max()))


def tables(M, X):
    """Qs [C] (n x k), b, P [m, C, k], a [m] of the model on the rows X."""
    i = M.info
    f, fu, k = i["f"], i["fu"], i["k"]
    Ds = [int(d) for d in M.Ds]
    m = int(X.info["m"])
    A = [field_matrix(X, fi, Ds[fi]) for fi in range(fu)]
    Qs, P = [], np.zeros((m, fu * (f - fu), k))
    n = int(i["n"])
    for c, (f1, f2) in enumerate(cross_blocks(fu, f)):
        b12 = ocffm.block_index(f1, f2, f)
        Qs.append(M.get("Q", b12).reshape(n, k))
        P[:, c, :] = A[f1] @ M.get("W", b12).reshape(Ds[f1], k)
    a = np.zeros(m)
    for f1 in range(fu):
        for f2 in range(f1, fu):
            b12 = ocffm.block_index(f1, f2, f)
            if i["used"][b12]:
                a += ((A[f1] @ M.get("W", b12).reshape(Ds[f1], k)) * (A[f2] @ M.get("H", b12).reshape(Ds[f2], k))).sum(axis=1)
    return Qs, M.get("b"), P, a


def row_labels(rows):
    return [[int(j) for j in rows.ycol[int(rows.yptr[i]):int(rows.yptr[i + 1])]] for i in range(rows.m)]


def subset(rows, idx):
    """The rows idx of a synth.Rows, labels included."""
    feats = [[(int(rows.fid[p]), int(rows.idx[p]), float(rows.val[p]))
              for p in range(int(rows.xptr[i]), int(rows.xptr[i + 1]))] for i in idx]
    if rows.yptr is None:
        return synth._build_rows(feats, None)
    all_labs = row_labels(rows)
    return synth._build_rows(feats, [np.array(all_labs[i], dtype=np.uint64) for i in idx])


def history_rows(test, n, seed=3):
    """The test rows with the history lists of the issue: per warm row empty,
    one item, 17 (one tile and one), all n, a repeat, an item >= n, only items
    >= n (empty after the filter); a row without nodes with a history and one
    without; the other rows keep their own labels."""
    rng = np.random.default_rng(seed)
    Xd = ocffm.ImpData.from_rows(test)
    cold = np.nonzero(cold_rows(Xd))[0]
    warm = np.nonzero(~cold_rows(Xd))[0]
    assert len(cold) >= 2 and len(warm) >= 8
    ch = {int(warm[0]): [], int(warm[1]): [41 % n], int(warm[2]): sorted(rng.choice(n, size=17, replace=False).tolist()),
          int(warm[3]): list(range(n)), int(warm[4]): [5, 9, 5, 33, 9], int(warm[5]): [2, n, 10 * n, 17],
          int(warm[6]): [n + 5], int(cold[0]): [3, 8, 20], int(cold[1]): []}
    return with_labels(None, test, ch), ch


_SET = {}


def setup(k, precision):
    """(problem, model from it, X, hist, hist's label lists, the special rows) on test_recommend's dataset."""
    key = (k, precision)
    if key not in _SET:
        g = real_problem(k, precision)
        M = ocffm.Model.from_problem(g)
        ds = dataset(k, "real")
        U = g._keep[0]
        hrows, ch = history_rows(ds.test, N)
        X = ocffm.ImpData.from_rows(ds.test, ds=U.Ds)
        H = ocffm.ImpData.from_rows(hrows, ds=U.Ds)
        _SET[key] = (g, M, X, H, row_labels(hrows), ch)
    return _SET[key]


@pytest.fixture(scope="module", autouse=True)
def _cleanup():
    yield
    for g, M, *_ in _SET.values():
        M.close()
        g.close()
    _SET.clear()


def check_delta(M, X, hists, field, precision, delta, nhist, tag):
    """delta, nhist against fold_ref on the model's own tables; returns the reference."""
    i = M.info
    fv, k, n = i["fv"], i["k"], int(i["n"])
    Qs, b, P, a = tables(M, X)
    ref = np.zeros_like(delta)
    worst = 0.0
    for r in range(len(hists)):
        args = (Qs, b, P[r], a[r], hists[r], field, fv, k, OMEGA, LAM, R)
        A, _, H = normal_equations(*args)
        assert nhist[r] == len(H), (r, nhist[r], len(H))
        if len(H) == 0:
            assert (delta[r] == 0).all(), r
            continue
        assert np.linalg.cond(A) <= 1e4, (r, np.linalg.cond(A))
        ref[r] = fold_reference(*args)
        err = float(np.abs(delta[r] - ref[r]).max())
        worst = max(worst, err / delta_tol(precision, ref[r]))
        assert err <= delta_tol(precision, ref[r]), (tag, r, err, delta_tol(precision, ref[r]))
    print(f"{tag}: worst |delta - ref| / tol = {worst:.3e}")
    return ref


# ------------------------------------------------------------------ tests
@gpu
@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("k", [5, 8])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_delta_parity(k, precision, field):
    """Test 1: delta against the numpy normal equations, every history shape."""
    g, M, X, H, hists, ch = setup(k, precision)
    delta, nhist = M.fold_in(X, H, field, OMEGA, LAM, R)
    assert delta.shape == (37, 2 * k) and nhist.dtype == np.uint32
    for r, lab in ch.items():
        assert nhist[r] == len({j for j in lab if j < N}), r
    assert nhist[[r for r, lab in ch.items() if lab == list(range(N))][0]] == N
    check_delta(M, X, hists, field, precision, delta, nhist, f"k {k} fp{precision} field {field}")
    assert M.counter("fold_rows") == int((nhist > 0).sum())


def drawn_model(k, fv, n, precision):
    ds = synth.general(seed=6, m=120, n=n, fu=2, fv=fv, k=k, nnz_user=2, vals="real", test_rows=37)
    g = ocffm.problem_from_dataset(ds, precision=precision, self_side=True)
    ocffm.srand(1)
    g.init()
    return ds, g


@gpu
@pytest.mark.parametrize("k,fv,n", [(1, 2, 70), (3, 1, 70), (16, 2, 70), (33, 1, 70), (24, 2, 70), (64, 2, 70), (128, 1, 70),
                                    (16, 2, 1500)])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_padded_k_and_the_cap(k, fv, n, precision):
    """Test 2: KP 4 .. 128 on drawn tables (init only), d = 128 (the largest
    LDS request) both ways, and n = 1500: several row ranges of the aggregates."""
    ds, g = drawn_model(k, fv, n, precision)
    M = ocffm.Model.from_problem(g)
    U = g._keep[0]
    rng = np.random.default_rng(k)
    hrows = with_labels(None, ds.test, {0: [], 1: sorted(rng.choice(n, size=17, replace=False).tolist()),
                                        2: list(range(n)), 3: [n - 1, n, 0, n - 1]})
    X = ocffm.ImpData.from_rows(ds.test, ds=U.Ds)
    H = ocffm.ImpData.from_rows(hrows, ds=U.Ds)
    field = k % 2
    delta, nhist = M.fold_in(X, H, field, OMEGA, LAM, R)
    assert delta.shape == (37, fv * k)
    check_delta(M, X, row_labels(hrows), field, precision, delta, nhist, f"k {k} fv {fv} n {n} fp{precision}")
    M.close()
    g.close()


@gpu
def test_d_above_the_cap_is_an_argument_error():
    ds, g = drawn_model(65, 2, 70, ocffm.FP64)
    M = ocffm.Model.from_problem(g)
    X = ocffm.ImpData.from_rows(ds.test, ds=g._keep[0].Ds)
    with pytest.raises(ocffm.OcffmError) as e:
        M.fold_in(X, X, 0, OMEGA, LAM, R)
    assert e.value.code == ocffm.E_ARG and "OCFFM_FOLD_MAX_D" in str(e.value)
    M.close()
    g.close()


@gpu
@pytest.mark.parametrize("field", [0, 1])
def test_optimality(field):
    """Test 3 (fp64): the gradient of F_i at delta, summed over the items in
    numpy, is below 1e-9 |rhs_i|, and F_i(delta) < F_i(0)."""
    g, M, X, H, hists, _ = setup(8, ocffm.FP64)
    delta, nhist = M.fold_in(X, H, field, OMEGA, LAM, R)
    Qs, b, P, a = tables(M, X)
    worst = 0.0
    for r in np.nonzero(nhist)[0]:
        args = (Qs, b, P[r], a[r], hists[r], field, 2, 8, OMEGA, LAM, R)
        _, rhs, _ = normal_equations(*args)
        gn = float(np.linalg.norm(fold_gradient(delta[r], *args)))
        worst = max(worst, gn / float(np.linalg.norm(rhs)))
        assert gn <= 1e-9 * float(np.linalg.norm(rhs)), (r, gn)
        assert fold_objective(delta[r], *args) < fold_objective(np.zeros(16), *args), r
    print(f"field {field}: worst |grad| / |rhs| = {worst:.3e}")


def folded_reference(M, g, X, delta, nhist, field):
    """ref[i, j]: model_reference's for the rows that are not folded, z_ij +
    <delta_i, q_j> from the projected tables for the folded ones."""
    U, _, V = g._keep
    ref, cold, _, _ = model_reference(M, X, V, popularity(U))
    Qs, b, P, a = tables(M, X)
    fv = M.info["fv"]
    q = np.concatenate([Qs[field * fv + gg] for gg in range(fv)], axis=1)
    for r in np.nonzero(nhist)[0]:
        ref[r] = a[r] + b + sum(Qs[c] @ P[r, c] for c in range(len(Qs))) + q @ delta[r]
    return ref, cold


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_serving_on_folded_rows(precision, monkeypatch):
    """Test 4."""
    g, M, X, H, hists, ch = setup(5, precision)
    field = 0
    fold = (H, field, OMEGA, LAM, R)
    delta, nhist = M.fold_in(X, H, field, OMEGA, LAM, R)
    ref, cold = folded_reference(M, g, X, delta, nhist, field)
    tol = tol_for(precision, ref)
    items, scores = M.recommend(X, topn=20, fold=fold)
    assert_topn(items, scores, ref, tol, excluded_sets(X, N, False))
    # the labels' scores are recommend's, bit for bit
    full_i, full_s = M.recommend(X, topn=N, fold=fold)
    ranks, lsc, ncand = M.label_ranks(X, fold=fold)
    yptr, ycol = X.labels()
    hits = 0
    for i in range(37):
        for p in range(int(yptr[i]), int(yptr[i + 1])):
            at = np.nonzero(full_i[i] == ycol[p])[0]
            if len(at):
                assert lsc[p] == full_s[i, at[0]], (i, p)
                hits += 1
    assert hits > 50
    # a row range, and another chunking, give the same bits
    part_i, part_s = M.recommend(X, topn=20, row0=5, rows=9, fold=fold)
    assert np.array_equal(part_i, items[5:14]) and np.array_equal(part_s, scores[5:14])
    monkeypatch.setenv("OCFFM_REC_ROWS", "7")
    M7 = ocffm.Model.from_problem(g)
    monkeypatch.delenv("OCFFM_REC_ROWS")
    i7, s7 = M7.recommend(X, topn=20, fold=fold)
    assert np.array_equal(i7, items) and np.array_equal(s7, scores)
    r7 = M7.label_ranks(X, fold=fold)
    assert all(np.array_equal(u, v) for u, v in zip(r7, (ranks, lsc, ncand)))
    M7.close()
    # rows without a history: the plain calls' bits, the cold row's popularity included
    plain_i, plain_s = M.recommend(X, topn=20)
    pr, ps, pn = M.label_ranks(X)
    empty = np.nonzero(nhist == 0)[0]
    cold_empty = [r for r in empty if cold[r]]
    assert len(empty) >= 3 and cold_empty
    for r in empty:
        assert np.array_equal(items[r], plain_i[r]) and np.array_equal(scores[r], plain_s[r])
        sl = slice(int(yptr[r]), int(yptr[r + 1]))
        assert np.array_equal(ranks[sl], pr[sl]) and np.array_equal(lsc[sl], ps[sl]) and ncand[r] == pn[r]
    pop = popularity(g._keep[0])
    c = cold_empty[0]
    assert (scores[c][items[c] != NONE] == pop[items[c][items[c] != NONE]]).all()
    # a row without nodes but with a history is not cold: n candidates
    cf = [r for r, lab in ch.items() if cold[r] and lab][0]
    assert nhist[cf] == 3 and ncand[cf] == N and (full_i[cf] != NONE).all()
    # exclusion is of X's own labels
    xi, _ = M.recommend(X, topn=20, exclude_labels=True, fold=fold)
    excl = excluded_sets(X, N, True)
    for i in range(37):
        assert not (set(xi[i][xi[i] != NONE].tolist()) & excl[i]), i
    # evaluate_fold is label_ranks_fold followed by eval_from_ranks
    e = M.evaluate(X, cuts=(1, 5), seen=H, fold=fold)
    rk, sc, nc = M.label_ranks(X, seen=H, fold=fold)
    e2 = ocffm.eval_from_ranks(yptr, rk, nc, scores=sc, cuts=(1, 5))
    assert e["auc"] == e2["auc"] and np.array_equal(e["ndcg"], e2["ndcg"]) and e["labels_ranked"] == e2["labels_ranked"]


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_determinism_and_independence(precision):
    """Test 5."""
    g, M, X, H, hists, _ = setup(8, precision)
    d1, n1 = M.fold_in(X, H, 1, OMEGA, LAM, R)
    d2, n2 = M.fold_in(X, H, 1, OMEGA, LAM, R)
    assert np.array_equal(d1, d2) and np.array_equal(n1, n2) and np.abs(d1).max() > 0
    ds = dataset(8, "real")
    hrows, _ = history_rows(ds.test, N)
    pick = [3, 11, 30]
    U = g._keep[0]
    Xs = ocffm.ImpData.from_rows(subset(ds.test, pick), ds=U.Ds)
    Hs = ocffm.ImpData.from_rows(subset(hrows, pick), ds=U.Ds)
    d3, n3 = M.fold_in(Xs, Hs, 1, OMEGA, LAM, R)
    assert np.array_equal(d3, d1[pick]) and np.array_equal(n3, n1[pick])


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_catalogue_cache(precision):
    """Test 6."""
    g, _, X, H, hists, _ = setup(5, precision)
    M = ocffm.Model.from_problem(g)
    assert M.counter("fold_stats_builds") == 0
    d0, n0 = M.fold_in(X, H, 0, OMEGA, LAM, R)
    M.fold_in(X, H, 1, OMEGA, LAM, R)
    assert M.counter("fold_stats_builds") == 1 and M.counter("fold_stats_us") >= 0
    # the item rows in another order, the histories remapped
    ds = dataset(5, "real")
    perm = np.random.default_rng(17).permutation(N)  # new row t is old row perm[t]
    inv = np.argsort(perm)
    Vp = ocffm.ImpData.from_rows(subset(ds.item, perm.tolist()), ds=M.item_Ds)
    M.set_items(Vp)
    hrows, _ = history_rows(ds.test, N)
    remap = {i: [int(inv[j]) if j < N else j for j in lab] for i, lab in enumerate(row_labels(hrows))}
    Hp = ocffm.ImpData.from_rows(with_labels(None, ds.test, remap), ds=g._keep[0].Ds)
    d1, n1 = M.fold_in(X, Hp, 0, OMEGA, LAM, R)
    assert M.counter("fold_stats_builds") == 2
    assert np.array_equal(n0, n1)
    for r in range(37):
        assert np.abs(d1[r] - d0[r]).max() <= delta_tol(precision, d0[r]), r
    M.close()


@gpu
def test_errors(tmp_path):
    """Test 7."""
    g, M, X, H, hists, _ = setup(5, ocffm.FP64)
    L = ocffm.lib()
    fo = ocffm._Fold(0, OMEGA, LAM, R)
    delta = np.zeros((37, 10))
    ptr = delta.ctypes.data_as(C.c_void_p)
    assert L.ocffm_model_fold_in(M.h, X.h, H.h, None, ptr, None) == ocffm.E_ARG
    assert L.ocffm_model_fold_in(M.h, X.h, None, C.byref(fo), ptr, None) == ocffm.E_ARG
    assert L.ocffm_model_fold_in(M.h, X.h, H.h, C.byref(fo), None, None) == ocffm.E_ARG
    items = np.zeros((37, 5), dtype=np.uint32)
    iptr = items.ctypes.data_as(C.c_void_p)
    assert L.ocffm_model_recommend_fold(M.h, X.h, None, C.byref(fo), 0, 37, 5, 0, iptr, None) == ocffm.E_ARG
    assert L.ocffm_model_recommend_fold(M.h, X.h, H.h, None, 0, 37, 5, 0, iptr, None) == ocffm.E_ARG
    assert L.ocffm_model_fold_in(M.h, X.h, H.h, C.byref(fo), ptr, None) == ocffm.OK  # (the arguments above were the fault)
    nan, inf = float("nan"), float("inf")
    bad = [(2, OMEGA, LAM, R), (0, OMEGA, 0.0, R), (0, OMEGA, -1.0, R), (0, -0.1, LAM, R), (0, nan, LAM, R),
           (0, OMEGA, nan, R), (0, OMEGA, LAM, nan), (0, inf, LAM, R), (0, OMEGA, inf, R), (0, OMEGA, LAM, -inf)]
    for field, w, lam, r in bad:
        for call in (lambda: M.fold_in(X, H, field, w, lam, r), lambda: M.recommend(X, fold=(H, field, w, lam, r)),
                     lambda: M.label_ranks(X, fold=(H, field, w, lam, r)),
                     lambda: M.evaluate(X, fold=(H, field, w, lam, r))):
            with pytest.raises(ocffm.OcffmError) as e:
                call()
            assert e.value.code == ocffm.E_ARG, (field, w, lam, r)
    ds = dataset(5, "real")
    U = g._keep[0]
    t = ds.test
    nolab = ocffm.ImpData.from_rows(synth.Rows(t.xptr, t.fid, t.idx, t.val), ds=U.Ds)
    short = ocffm.ImpData.from_rows(subset(t, list(range(36))), ds=U.Ds)
    for hist in (nolab, short):
        with pytest.raises(ocffm.OcffmError) as e:
            M.fold_in(X, hist, 0, OMEGA, LAM, R)
        assert e.value.code == ocffm.E_ARG
        with pytest.raises(ocffm.OcffmError) as e:
            M.recommend(X, fold=(hist, 0, OMEGA, LAM, R))
        assert e.value.code == ocffm.E_ARG
    # the list forms do not fold
    cand = (np.zeros(38, dtype=np.uint64), np.zeros(1, dtype=np.uint32))
    for call in (M.recommend, M.label_ranks, M.evaluate):
        with pytest.raises(ValueError):
            call(X, candidates=cand, fold=(H, 0, OMEGA, LAM, R))
    # a model from a file has no catalogue yet
    path = str(tmp_path / "m.bin")
    g.save_binary(path)
    F = ocffm.Model.load_binary(path)
    with pytest.raises(ocffm.OcffmError) as e:
        F.fold_in(X, H, 0, OMEGA, LAM, R)
    assert e.value.code == ocffm.E_STATE
    with pytest.raises(ocffm.OcffmError) as e:
        F.recommend(X, fold=(H, 0, OMEGA, LAM, R))
    assert e.value.code == ocffm.E_STATE
    # an empty catalogue: delta = 0, no history, the plain entries' NONE results
    F.set_items(ocffm.ImpData.from_rows(synth._build_rows([], None), ds=F.item_Ds))
    d, nh = F.fold_in(X, H, 0, OMEGA, LAM, R)
    assert (d == 0).all() and (nh == 0).all()
    it, sc = F.recommend(X, topn=5, fold=(H, 0, OMEGA, LAM, R))
    assert (it == NONE).all() and (sc == -np.inf).all()
    rk, sc, nc = F.label_ranks(X, fold=(H, 0, OMEGA, LAM, R))
    assert (rk == NONE).all() and (nc == 0).all()
    # no rows
    it, sc = M.recommend(X, topn=5, rows=0, fold=(H, 0, OMEGA, LAM, R))
    assert it.shape == (0, 5)
    F.close()


def _rec_lines(path):
    return [[(int(t.split(":")[0]), float(t.split(":")[1])) for t in line.split()]
            for line in open(path).read().split("\n")[:-1]]


@gpu
def test_predict_fold(tmp_path):
    """Test 8: predict --fold-* prints Model.recommend(fold=...)'s lists and
    Model.evaluate(fold=...)'s table; without the flags nothing changes (the
    plain call's lists, as test_model's test_cli checks byte for byte)."""
    g, _, _, _, _, _ = setup(5, ocffm.FP64)
    ds = dataset(5, "real")
    mbin, it, te, hi, out, out0 = (str(tmp_path / x) for x in ("m.bin", "item", "te", "hist", "rec", "rec0"))
    g.save_binary(mbin)
    ds.item.write(it)
    ds.test.write(te)
    _, ch = history_rows(ds.test, N)
    # (in a file a row's label block cannot be empty: the rows with a changed, non-empty history)
    hrows = with_labels(None, ds.test, {r: lab for r, lab in ch.items() if lab})
    hrows.write(hi)
    r = subprocess.run([PREDICT, "--binary", "--recommend", te, "--topn", "7", "--rec-out", out, "--eval", te,
                        "--eval-seen", hi, "--eval-cuts", "1,5", "--fold-field", "0", "--fold-history", hi,
                        "--fold-omega", str(OMEGA), "--fold-lambda", str(LAM), "--fold-r", str(R), mbin, it],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    M = ocffm.Model.load_binary(mbin)
    M.set_items(ocffm.ImpData.read(it, False, M.item_Ds))
    X = ocffm.ImpData.read(te, True, M.Ds[:2])
    H = ocffm.ImpData.read(hi, True, M.Ds[:2])
    fold = (H, 0, OMEGA, LAM, R)
    items, scores = M.recommend(X, topn=7, fold=fold)
    got = _rec_lines(out)
    assert len(got) == 37
    for i in range(37):
        nf = int((items[i] != NONE).sum())
        assert [j for j, _ in got[i]] == items[i, :nf].tolist(), i
        assert [v for _, v in got[i]] == [float("%.17g" % s) for s in scores[i, :nf]], i
    e = M.evaluate(X, cuts=(1, 5), seen=H, fold=fold)
    line = [x for x in r.stdout.split("\n") if x.startswith("eval loss")][0]
    assert line == "eval loss %.17g mrr %.17g auc %.17g" % (e["loss"], e["mrr"], e["auc"])
    # without the flags: the plain lists
    r = subprocess.run([PREDICT, "--binary", "--recommend", te, "--topn", "7", "--rec-out", out0, mbin, it],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    items0, scores0 = M.recommend(X, topn=7)
    got0 = _rec_lines(out0)
    for i in range(37):
        nf = int((items0[i] != NONE).sum())
        assert [j for j, _ in got0[i]] == items0[i, :nf].tolist(), i
        assert [v for _, v in got0[i]] == [float("%.17g" % s) for s in scores0[i, :nf]], i
    assert got != got0
    M.close()
    # usage errors: exit 1 before any device work
    for args in (["--fold-field", "0"], ["--fold-history", hi],
                 ["--fold-field", "0", "--fold-history", hi],
                 ["--recommend", te, "--rec-out", out, "--rec-candidates", te, "--fold-field", "0", "--fold-history", hi]):
        r = subprocess.run([PREDICT, "--binary"] + args + [mbin, it], capture_output=True, text=True)
        assert r.returncode == 1 and r.stderr.strip(), args
