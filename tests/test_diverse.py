"""Diversified top-N (include/ocffm_diverse.h ocffm_model_recommend_diverse,
ocffm.Model.recommend_diverse, predict --diversify).

The expected values are built from public outputs alone: the row's pool is
``M.recommend(topn=pool)`` (or with ``candidates=``), the pair similarities
are ``M.item_similarity`` over all pairs of the pool, and the greedy itself is
tests/diverse_ref.py (numpy fp64, every operation rounded on its own).  The
contract pins every bit, so items, pos, scores and mmr are compared for
equality in both precisions; no tolerance is involved except where a property
of the input is stated (a twin pair's cosine is 1 within 1e-6 fp32 / 1e-12
fp64, the rounding of one product of a norm's inverse).

The knobs OCFFM_REC_ROWS / OCFFM_REC_SLICES / OCFFM_REC_SEG are read when a
model is created, so, as in the other determinism tests, each setting gets a
fresh model on the same snapshot."""
import os
import subprocess

import numpy as np
import pytest

import ocffm
import synth
from diverse_ref import mmr as mmr_ref
from test_model import PREDICT, TRAIN, _assert_rec_file, _cli_files, lists_for
from test_recommend import NONE, cold_rows, dataset, popularity, real_problem, tie_problem
from test_similar import item_feats

gpu = pytest.mark.gpu

PRECISIONS = [ocffm.FP64, ocffm.FP32]
N = 70      # items of test_recommend's dataset
ROWS = 37   # its test rows


# ------------------------------------------------------------ reference
def expected(M, X, topn, pool, theta, **kw):
    """(items, scores, mmr, pos) from recommend(topn=pool), item_similarity and diverse_ref."""
    pi, ps = M.recommend(X, topn=pool, **kw)
    cs = (pi != NONE).sum(axis=1)
    a = np.concatenate([np.repeat(pi[i, :c], c) for i, c in enumerate(cs)] + [np.zeros(0, dtype=np.uint32)])
    b = np.concatenate([np.tile(pi[i, :c], c) for i, c in enumerate(cs)] + [np.zeros(0, dtype=np.uint32)])
    flat = M.item_similarity(a, b)
    assert np.isfinite(flat).all()
    sims, o = [], 0
    for c in cs:
        sims.append(flat[o:o + c * c].reshape(c, c))
        o += c * c
    return mmr_ref(pi, ps, sims, theta, topn), (pi, ps)


def same(got, want):
    assert len(got) == len(want) == 4
    for name, g, w in zip(("items", "scores", "mmr", "pos"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        bad = np.nonzero(~((g == w) | ((g != g) & (w != w))))
        assert bad[0].size == 0, (name, bad[0][:5], bad[1][:5], g[bad][:5], w[bad][:5])


_TRAINED = {}


@pytest.fixture(scope="module")
def trained():
    """(trained problem, a model taken from it) per (k, precision): test_recommend's setup."""
    def make(k, precision):
        if (k, precision) not in _TRAINED:
            g = real_problem(k, precision)
            _TRAINED[(k, precision)] = (g, ocffm.Model.from_problem(g))
        return _TRAINED[(k, precision)]
    yield make
    for g, M in _TRAINED.values():
        M.close()
        g.close()
    _TRAINED.clear()


# ------------------------------------------------------------------ tests
THETA_MOVES = 0.3  # the not-vacuous condition of test_parity holds at the issue's first choice


@gpu
@pytest.mark.parametrize("k", [5, 32])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_parity(k, precision, trained):
    """Test 1: ragged and full 16-tiles of the pool, and a pool larger than
    the 70 candidates (the tail is NONE), at theta 0.3 and 1.  Not vacuous: at
    (10, 40) and theta = THETA_MOVES the reference's items differ from
    recommend(topn=10) in at least half of the rows (the fraction is printed
    for each of 0.3, 0.5, 0.7, 0.9)."""
    g, M = trained(k, precision)
    X = g._keep[1]
    assert cold_rows(X).any() and not cold_rows(X).all()
    plain = M.recommend(X, topn=10)[0]
    for theta in (0.3, 0.5, 0.7, 0.9):
        want, _ = expected(M, X, 10, 40, theta)
        moved = int((want[0] != plain).any(axis=1).sum())
        print("k", k, "precision", precision, "theta", theta, "rows moved", moved, "of", ROWS)
        if theta == THETA_MOVES:
            assert 2 * moved >= ROWS, (theta, moved)
    for topn, pool in ((1, 1), (10, 15), (10, 16), (10, 17), (16, 33), (10, 40), (69, 128)):
        for theta in (0.3, 1.0):
            want, (pi, _) = expected(M, X, topn, pool, theta)
            got = M.recommend_diverse(X, topn=topn, theta=theta, pool=pool)
            assert got[0].dtype == np.uint32 and got[3].dtype == np.uint32 and got[0].shape == (ROWS, topn)
            same(got, want)
            assert (got[0][:, 0] == pi[:, 0]).all() and (got[3][:, 0] == 0).all()
            filled = got[0] != NONE
            assert ((got[1] == -np.inf) == ~filled).all() and ((got[3] == NONE) == ~filled).all()
            if pool == 128:
                assert (pi[:, N:] == NONE).all() and filled.all()  # 70 candidates, 69 picks
    # the default pool is min(128, 4 topn)
    same(M.recommend_diverse(X, topn=10), M.recommend_diverse(X, topn=10, theta=0.3, pool=40))
    same(M.recommend_diverse(X, topn=40, theta=0.3), M.recommend_diverse(X, topn=40, theta=0.3, pool=128))


@gpu
@pytest.mark.parametrize("k,n", [(3, 70), (8, 70), (16, 70), (64, 70), (128, 70), (8, 1500)])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_padded_k(k, n, precision):
    """Test 2: KP = 4, 8, 16, 64, 128 (32 runs above) on the drawn tables; at
    n = 1500 the pool is full: 128 of 128, all 8 x 8 tiles, every position taken."""
    ds = synth.general(seed=6, m=120, n=n, fu=2, fv=2, k=k, nnz_user=2, vals="real", test_rows=37)
    g = ocffm.problem_from_dataset(ds, precision=precision, self_side=True)
    ocffm.srand(1)
    g.init()
    M = ocffm.Model.from_problem(g)
    X = g._keep[1]
    for topn, pool in (((128, 128),) if n == 1500 else ((10, 40), (70, 70))):
        want, (pi, _) = expected(M, X, topn, pool, 0.3)
        got = M.recommend_diverse(X, topn=topn, theta=0.3, pool=pool)
        same(got, want)
        warm = ~cold_rows(X)
        if n == 1500:
            assert (pi[warm] != NONE).all()
            assert (np.sort(got[3][warm], axis=1) == np.arange(128)).all()
    M.close()
    g.close()


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_theta_zero_is_recommend(precision, trained):
    """Test 3."""
    g, M = trained(5, precision)
    X = g._keep[1]
    cand = lists_for(ROWS, N, 8)
    for topn in (1, 10, 64):
        for kw in ({}, {"candidates": cand}, {"exclude_labels": True}):
            ri, rs = M.recommend(X, topn=topn, **kw)
            for pool in (topn, 128):
                items, scores, mv, pos = M.recommend_diverse(X, topn=topn, theta=0.0, pool=pool, **kw)
                assert np.array_equal(items, ri) and np.array_equal(scores, rs), (topn, pool, kw.keys())
                filled = ri != NONE
                assert (pos[filled] == np.broadcast_to(np.arange(topn), ri.shape)[filled]).all()
                assert (pos[~filled] == NONE).all() and (mv[~filled] == -np.inf).all()
                assert (mv[:, 1:] <= mv[:, :-1]).all()  # rel falls with the score (-inf past the picks)


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_ties_and_duplicates(precision):
    """Test 4: items j and j + 35 are the same feature rows on tie_problem's
    integer tables, and the H rows of item 3's (and so 38's) nodes are zero:
    zero embeddings."""
    g = tie_problem(precision)
    U, X, _ = g._keep
    fu, f = int(U.info["f"]), g.f
    feats = item_feats(dataset(5, "ones").item)
    feats = feats[:35] + feats[:35]
    zero = 3
    for f1 in range(fu):
        for f2 in range(fu, f):
            b12 = ocffm.block_index(f1, f2, f)
            H = g.get("H", b12).reshape(-1, g.k)
            for fid, idx, _ in feats[zero]:
                if fid == f2 - fu:
                    H[idx] = 0.0
            g.set("H", b12, H.reshape(-1))
    M = ocffm.Model.from_problem(g)
    M.set_items(ocffm.ImpData.from_rows(synth._build_rows(feats, None), ds=M.item_Ds))
    M.set_popularity(popularity(U))
    allj = np.arange(N)
    zs = np.nonzero((M.item_similarity(allj, allj) == 0.0))[0]  # the zero-norm items
    assert {zero, zero + 35} <= set(zs.tolist()) and len(zs) < N // 2
    for z in (zero, zero + 35):
        assert (M.item_similarity(np.full(N, z), allj) == 0.0).all()
    tol = 1e-12 if precision == ocffm.FP64 else 1e-6
    twin = M.item_similarity(allj[:35], allj[:35] + 35)
    live = np.array([j for j in range(35) if j not in set(zs.tolist())])
    assert (np.abs(twin[live] - 1.0) <= tol).all()
    theta = 0.5
    w = 1.0 - theta
    for topn, pool in ((70, 70), (70, 128), (10, 40)):
        want, (pi, ps) = expected(M, X, topn, pool, theta)
        got = M.recommend_diverse(X, topn=topn, theta=theta, pool=pool)
        same(got, want)
    items, scores, mv, pos = M.recommend_diverse(X, topn=70, theta=theta, pool=70)
    pi, ps = M.recommend(X, topn=70)
    pairs = 0
    for i in np.nonzero(~cold_rows(X))[0]:  # (a cold row ranks by popularity, which the copies do not share)
        c = int((pi[i] != NONE).sum())
        assert c == N
        rng = ps[i, 0] - ps[i, c - 1]
        where = {int(j): t for t, j in enumerate(items[i]) if j != NONE}
        place = {int(j): p for p, j in enumerate(pi[i, :c])}
        for j in live:
            if j in place and j + 35 in place:
                pairs += 1
                assert place[j] < place[j + 35] and ps[i, place[j]] == ps[i, place[j + 35]]  # same score: by item
                assert where[j] < where[j + 35], (i, j)  # the lower position first
                t = where[j + 35]
                rel = 0.0 if rng == 0 else (scores[i, t] - ps[i, c - 1]) / rng
                # the first copy is taken, so ms >= sim(twin) >= 1 - tol; no cosine exceeds 1 + tol
                assert w * rel - theta * (1 + tol) - 1e-15 <= mv[i, t] <= w * rel - theta * (1 - tol) + 1e-15, (i, j)
    assert pairs > ROWS
    M.close()
    g.close()


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_exclusion_cold_rows_and_lists(precision, trained):
    """Test 5: exclude_labels, rows without a kept node (the pool is by
    popularity, the selection still by catalogue similarity) and candidate lists with
    repeats, entries >= n and an empty list."""
    g, M = trained(5, precision)
    U, X, _ = g._keep
    cold = cold_rows(X)
    assert cold.any()
    pop = popularity(U)
    want, (pi, ps) = expected(M, X, 10, 40, 0.3, exclude_labels=True)
    got = M.recommend_diverse(X, topn=10, theta=0.3, pool=40, exclude_labels=True)
    same(got, want)
    yptr, ycol = X.labels()
    plain40, plain10 = M.recommend(X, topn=40)[0], M.recommend(X, topn=10)[0]
    hit = 0
    for i in range(ROWS):
        lab = set(int(j) for j in ycol[int(yptr[i]):int(yptr[i + 1])])
        hit += bool(lab & set(plain40[i].tolist()))
        assert not lab & set(got[0][i].tolist())
    assert hit > 0  # (the exclusion changed some pool)
    got = M.recommend_diverse(X, topn=10, theta=0.7, pool=40)
    same(got, expected(M, X, 10, 40, 0.7)[0])
    moved = 0
    for i in np.nonzero(cold)[0]:
        f = got[0][i] != NONE
        assert (got[1][i][f] == pop[got[0][i][f]]).all()  # the model score of a cold row is the popularity
        moved += not np.array_equal(got[0][i], plain10[i])
    assert moved > 0  # the selection is not the popularity order
    cptr, ccol = lists_for(ROWS, N, 8)
    lens = np.diff(cptr.astype(np.int64))
    assert (lens == 0).any() and (ccol >= N).any() and max(lens) > 16
    assert any(len(set(ccol[int(cptr[i]):int(cptr[i + 1])].tolist())) < lens[i] for i in range(ROWS))
    for topn, pool, kw in ((10, 40, {}), (5, 17, {"exclude_labels": True}), (40, 128, {})):
        want, _ = expected(M, X, topn, pool, 0.3, candidates=(cptr, ccol), **kw)
        got = M.recommend_diverse(X, topn=topn, theta=0.3, pool=pool, candidates=(cptr, ccol), **kw)
        same(got, want)
    empty = int(np.nonzero(lens == 0)[0][0])
    assert (got[0][empty] == NONE).all() and (got[2][empty] == -np.inf).all() and (got[3][empty] == NONE).all()


def reversed_rows(r):
    """The rows of a synth.Rows in reversed order."""
    feats = [[(int(r.fid[p]), int(r.idx[p]), float(r.val[p])) for p in range(int(r.xptr[i]), int(r.xptr[i + 1]))]
             for i in range(r.m)][::-1]
    labs = [np.asarray(r.ycol[int(r.yptr[i]):int(r.yptr[i + 1])]) for i in range(r.m)][::-1]
    return synth._build_rows(feats, labs)


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_determinism(precision, monkeypatch, tmp_path):
    """Test 6: row chunks, item slices and list segments change no bit; nor do
    the row's place in the call, the other rows, or a second call."""
    g = real_problem(5, precision)
    U, X, V = g._keep
    snap = str(tmp_path / "model.bin")
    g.save_binary(snap)
    pop = popularity(U)
    cand = lists_for(ROWS, N, 8)
    knobs = ("OCFFM_REC_ROWS", "OCFFM_REC_SLICES", "OCFFM_REC_SEG")

    def run(M):
        return (M.recommend_diverse(X, topn=10, theta=0.3, pool=40) +
                M.recommend_diverse(X, topn=33, theta=0.6, pool=128, exclude_labels=True) +
                M.recommend_diverse(X, topn=10, theta=0.3, pool=40, candidates=cand))

    results = []
    for setting in ({}, {"OCFFM_REC_ROWS": "1"}, {"OCFFM_REC_ROWS": "7"}, {"OCFFM_REC_SLICES": "1"},
                    {"OCFFM_REC_SLICES": "3"}, {"OCFFM_REC_SEG": "16"},
                    {"OCFFM_REC_ROWS": "7", "OCFFM_REC_SLICES": "3", "OCFFM_REC_SEG": "16"}):
        for name in knobs:
            monkeypatch.delenv(name, raising=False)
        for name, val in setting.items():
            monkeypatch.setenv(name, val)
        M = ocffm.Model.load_binary(snap, precision)
        for name in setting:
            monkeypatch.delenv(name)  # read at create: gone before the calls
        M.set_items(V)
        M.set_popularity(pop)
        results.append(run(M))
        if not setting:
            again = run(M)
            for x, y in zip(again, results[0]):
                assert np.array_equal(x, y)
            full = results[0][:4]
            part = M.recommend_diverse(X, topn=10, theta=0.3, pool=40, row0=5, rows=18)
            same(part, tuple(a[5:23] for a in full))
            Xr = ocffm.ImpData.from_rows(reversed_rows(dataset(5, "real").test), ds=U.Ds)
            same(M.recommend_diverse(Xr, topn=10, theta=0.3, pool=40), tuple(a[::-1] for a in full))
            want, _ = expected(M, X, 10, 40, 0.3)
            same(full, want)
        M.close()
    g.close()
    for r in results[1:]:
        assert len(r) == len(results[0]) == 12
        for x, y in zip(r, results[0]):
            assert x.dtype == y.dtype and np.array_equal(x, y)
    assert (results[0][0] != NONE).all()


@gpu
def test_errors_and_degenerate_inputs(trained, tmp_path):
    """Test 7, first half: the error codes of ocffm_diverse.h."""
    g, _ = trained(5, ocffm.FP64)
    U, X, V = g._keep
    snap = str(tmp_path / "m.bin")
    g.save_binary(snap)
    M = ocffm.Model.load_binary(snap, ocffm.FP64)
    L = ocffm.lib()
    P = ocffm._ptr
    items = np.zeros((ROWS, 10), dtype=np.uint32)
    scores = np.zeros((ROWS, 10), dtype=np.float64)
    mv = np.zeros((ROWS, 10), dtype=np.float64)
    pos = np.zeros((ROWS, 10), dtype=np.uint32)
    cptr, ccol = lists_for(ROWS, N, 8)

    def call(Xh=X.h, row0=0, rows=ROWS, cp=None, cc=None, topn=10, pool=40, theta=0.3, flags=0, ip=P(items),
             sp=P(scores), mp=P(mv), pp=P(pos)):
        return L.ocffm_model_recommend_diverse(M.h, Xh, row0, rows, cp, cc, topn, pool, theta, flags, ip, sp, mp, pp)

    assert call() == ocffm.E_STATE  # before set_items
    M.set_items(V)
    assert call() == ocffm.OK
    good = tuple(a.copy() for a in (items, scores, mv, pos))
    same(good, M.recommend_diverse(X, topn=10, theta=0.3, pool=40))
    # recommend's own: topn, the row window, null X and items
    assert call(topn=0, pool=40) == ocffm.E_ARG and call(topn=129, pool=129) == ocffm.E_ARG
    assert call(row0=ROWS - 3, rows=4) == ocffm.E_ARG and call(row0=ROWS + 1, rows=0) == ocffm.E_ARG
    assert call(Xh=None) == ocffm.E_ARG and call(ip=None) == ocffm.E_ARG
    assert L.ocffm_model_recommend_diverse(None, X.h, 0, ROWS, None, None, 10, 40, 0.3, 0, P(items), None, None,
                                           None) == ocffm.E_ARG
    # the pool, theta and the flags
    assert call(pool=9) == ocffm.E_ARG and call(pool=129) == ocffm.E_ARG and call(pool=0) == ocffm.E_ARG
    assert call(pool=10) == ocffm.OK and call(pool=128) == ocffm.OK
    for theta in (-1e-9, 1.0000001, float("nan"), float("inf"), -float("inf")):
        assert call(theta=theta) == ocffm.E_ARG, theta
    assert call(theta=0.0) == ocffm.OK and call(theta=1.0) == ocffm.OK
    assert call(flags=2) == ocffm.E_ARG and call(flags=3) == ocffm.E_ARG and call(flags=1) == ocffm.OK
    # the lists
    x0 = cptr.copy()
    x0[0] = 1
    xd = cptr.copy()
    xd[5] = xd[6] + 1
    assert call(cp=None, cc=P(ccol)) == ocffm.E_ARG           # ccol without cptr
    assert call(cp=P(cptr), cc=None) == ocffm.E_ARG           # entries without ccol
    assert call(cp=P(x0), cc=P(ccol)) == ocffm.E_ARG          # does not start at 0
    assert call(cp=P(xd), cc=P(ccol)) == ocffm.E_ARG          # decreases
    assert call(cp=P(cptr), cc=P(ccol)) == ocffm.OK
    assert call(cp=P(np.zeros(ROWS + 1, dtype=np.uint64)), cc=None) == ocffm.OK  # empty lists need no ccol
    assert (items == NONE).all() and (pos == NONE).all() and (scores == -np.inf).all() and (mv == -np.inf).all()
    # optional outputs, zero rows
    assert call(sp=None, mp=None, pp=None) == ocffm.OK
    assert np.array_equal(items, good[0])
    assert call(rows=0) == ocffm.OK and call(row0=ROWS, rows=0) == ocffm.OK
    e = M.recommend_diverse(X, topn=10, rows=0)
    assert all(a.shape == (0, 10) for a in e)
    with pytest.raises(ocffm.OcffmError) as err:
        M.recommend_diverse(X, topn=10, pool=5)
    assert err.value.code == ocffm.E_ARG
    # a later valid call still works
    assert call() == ocffm.OK
    same((items, scores, mv, pos), good)
    # an empty catalogue: rows of NONE
    M.set_items(ocffm.ImpData.from_rows(synth._build_rows([], None), ds=M.item_Ds))
    assert M.info["n"] == 0
    e = M.recommend_diverse(X, topn=6, theta=0.3, pool=20)
    assert (e[0] == NONE).all() and (e[1] == -np.inf).all() and (e[2] == -np.inf).all() and (e[3] == NONE).all()
    M.close()


@gpu
def test_cli(tmp_path):
    """Test 7, second half: predict --diversify writes what
    Model.recommend_diverse returns on the same files, in --rec-out's format
    (item:score with the model score, %.17g), compared as test_model's CLI
    test compares."""
    tr, it, te = _cli_files(tmp_path)
    mbin, out = str(tmp_path / "m.bin"), str(tmp_path / "rec.txt")
    r = subprocess.run([TRAIN, "-k", "4", "-t", "2", "--fp64", "--binary-out", mbin, it, tr], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    U = ocffm.ImpData.read(tr, True)
    M = ocffm.Model.load_binary(mbin)
    M.set_items(ocffm.ImpData.read(it, False, M.item_Ds))
    M.set_popularity(popularity(U))
    X = ocffm.ImpData.read(te, True, M.Ds[:M.info["fu"]])
    base = [PREDICT, "--binary", "--popularity", tr, "--recommend", te, "--rec-out", out]
    r = subprocess.run(base + ["--topn", "7", "--diversify", "0.6", mbin, it], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    items, scores, _, _ = M.recommend_diverse(X, topn=7, theta=0.6)  # (the default pool on both sides: 28)
    _assert_rec_file(out, items, scores, 7)
    assert not np.array_equal(items, M.recommend(X, topn=7)[0])
    cptr, ccol = lists_for(100, 50, 6)
    cand = str(tmp_path / "cand")
    with open(cand, "w") as fh:
        for i in range(100):
            fh.write(" ".join(str(int(j)) for j in ccol[int(cptr[i]):int(cptr[i + 1])]) + "\n")
    r = subprocess.run(base + ["--topn", "5", "--diversify", "0.4", "--pool", "50", "--rec-unseen", "--rec-candidates",
                               cand, mbin, it], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    items, scores, _, _ = M.recommend_diverse(X, topn=5, theta=0.4, pool=50, exclude_labels=True,
                                              candidates=(cptr, ccol))
    _assert_rec_file(out, items, scores, 5)
    r = subprocess.run(base + ["--topn", "5", "--diversify", "0", "--fp32", mbin, it], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    M32 = ocffm.Model.load_binary(mbin, ocffm.FP32)
    M32.set_items(ocffm.ImpData.read(it, False, M.item_Ds))
    M32.set_popularity(popularity(U))
    _assert_rec_file(out, *M32.recommend(X, topn=5), 5)
    M32.close()
    M.close()


@gpu
def test_counters(trained, tmp_path):
    """Test 8: the inverse norms are built once per catalogue, whichever entry
    asks first; the MMR launches are timed on their own."""
    g, _ = trained(5, ocffm.FP64)
    U, X, V = g._keep
    snap = str(tmp_path / "m.bin")
    g.save_binary(snap)
    M = ocffm.Model.load_binary(snap, ocffm.FP64)
    M.set_items(V)
    assert M.counter("sim_norm_builds") == 0 and M.counter("div_kernel_us") == 0
    M.recommend(X, topn=10)
    assert M.counter("sim_norm_builds") == 0
    first = M.recommend_diverse(X, topn=10)
    assert M.counter("sim_norm_builds") == 1
    assert M.counter("div_kernel_us") > 0 and M.counter("div_setup_us") >= 0
    assert M.counter("rank_kernel_us") >= M.counter("div_kernel_us")
    M.recommend_diverse(X, topn=5, theta=0.9, pool=128, candidates=lists_for(ROWS, N, 8))
    assert M.counter("div_kernel_us") > 0
    M.item_similarity([0, 1], [1, 2])
    same(M.recommend_diverse(X, topn=10), first)
    assert M.counter("sim_norm_builds") == 1
    assert M.counter("fold_stats_builds") == 0
    feats = item_feats(dataset(5, "real").item)
    feats = [[(fi, ix, 3.0 * v) for fi, ix, v in feats[(7 * j + 3) % N]] for j in range(N)] + feats[:13]
    M.set_items(ocffm.ImpData.from_rows(synth._build_rows(feats, None), ds=M.item_Ds))
    assert M.counter("sim_norm_builds") == 1
    got = M.recommend_diverse(X, topn=10, theta=0.5, pool=40)
    assert M.counter("sim_norm_builds") == 2
    same(got, expected(M, X, 10, 40, 0.5)[0])  # stale norms would show
    assert M.counter("sim_norm_builds") == 2
    M.close()
