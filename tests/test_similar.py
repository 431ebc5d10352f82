"""Similar items (include/ocffm_similar.h: ocffm_model_similar_items /
similar_to / item_similarity, ocffm.Model, predict --similar).

The reference is numpy fp64 on E = hstack(M.get("Q", b12) over the cross
blocks): (E E^T) / outer(norm, norm) with 0 where a norm is 0, E E^T for the
inner product; it shares nothing with the norm, gather and sweep kernels.
Tolerances are test_recommend's tol_for (1e-12 fp64, 1e-3 fp32, times
max(1, max|ref|)) and the rank check is its assert_topn.  Integer tables give
exact inner products in both precisions and compare exactly; the symmetry,
pair, chunking and ordering properties are compared bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import ocffm
import synth
from test_model import assert_same, cross_blocks, seen_for, serve_all
from test_recommend import NONE, assert_topn, dataset, exact_topn, field_matrix, real_problem, tie_problem, tol_for

gpu = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(REPO, "one-class-ffm_amd", "train")
PREDICT = os.path.join(REPO, "one-class-ffm_amd", "predict")
PRECISIONS = [ocffm.FP64, ocffm.FP32]
METRICS = ["cosine", "dot"]
N = 70  # items of test_recommend's dataset


# ------------------------------------------------------------ reference
def embedding(M):
    i = M.info
    n, k = int(i["n"]), int(i["k"])
    return np.hstack([M.get("Q", ocffm.block_index(f1, f2, i["f"])).reshape(n, k)
                      for f1, f2 in cross_blocks(i["fu"], i["f"])])


def sim_ref(E, metric, Eq=None):
    Eq = E if Eq is None else Eq
    dot = Eq @ E.T
    if metric == "dot":
        return dot
    den = np.outer(np.sqrt((Eq * Eq).sum(axis=1)), np.sqrt((E * E).sum(axis=1)))
    return np.where(den > 0, dot / np.where(den > 0, den, 1.0), 0.0)


def singles(q):
    return [{int(j)} for j in q]


def item_feats(rows):
    return [[(int(rows.fid[p]), int(rows.idx[p]), float(rows.val[p]))
             for p in range(int(rows.xptr[j]), int(rows.xptr[j + 1]))] for j in range(rows.m)]


_TRAINED = {}


@pytest.fixture(scope="module")
def trained():
    """(trained problem, a model taken from it, E) per (k, precision): test 1's setup."""
    def make(k, precision):
        if (k, precision) not in _TRAINED:
            g = real_problem(k, precision)
            M = ocffm.Model.from_problem(g)
            _TRAINED[(k, precision)] = (g, M, embedding(M))
        return _TRAINED[(k, precision)]
    yield make
    for g, M, _ in _TRAINED.values():
        M.close()
        g.close()
    _TRAINED.clear()


# ------------------------------------------------------------------ tests
@gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("k", [5, 32])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_parity(k, precision, metric, trained):
    """Test 1: all 70 items as queries (row tiles of 32, 32 and 6 against one
    full item tile and a ragged one)."""
    _, M, E = trained(k, precision)
    ref = sim_ref(E, metric)
    tol = tol_for(precision, ref)
    q = np.arange(N)
    norm = np.sqrt((E * E).sum(axis=1))
    for topn in (10, 128):
        items, scores = M.similar_items(q, topn=topn, metric=metric)
        assert items.dtype == np.uint32 and scores.dtype == np.float64 and items.shape == (N, topn)
        full = items != NONE
        print(metric, topn, "max err", float(np.abs(scores[full] - ref[np.nonzero(full)[0], items[full]]).max()), "tol", tol)
        assert_topn(items, scores, ref, tol, singles(q))
        assert not (items == q[:, None]).any()  # the query is absent from its own row
        if topn == 128:  # 69 candidates: the tail is empty
            assert (items[:, 69:] == NONE).all() and (scores[:, 69:] == -np.inf).all() and (items[:, :69] != NONE).all()
        ki, ks = M.similar_items(q, topn=topn, metric=metric, keep_self=True)
        assert_topn(ki, ks, ref, tol, [set()] * N)
        if metric == "cosine":
            # an item with a direction of its own ranks first in its own row, at 1
            own = [j for j in range(N) if norm[j] > 0 and (np.delete(ref[j], j) < 1 - 10 * tol).all()]
            assert len(own) > N // 2
            for j in own:
                assert ki[j, 0] == j and abs(ks[j, 0] - 1.0) <= tol, (j, ki[j, 0], ks[j, 0])


@gpu
@pytest.mark.parametrize("k,n", [(3, 70), (8, 70), (16, 70), (64, 70), (128, 70), (8, 1500)])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_padded_k(k, n, precision):
    """Test 2: KP = 4, 8, 16, 64, 128 (32 runs above) on the drawn tables, and
    an item count at which the default plan slices the items (n = 1500)."""
    ds = synth.general(seed=6, m=120, n=n, fu=2, fv=2, k=k, nnz_user=2, vals="real", test_rows=37)
    g = ocffm.problem_from_dataset(ds, precision=precision, self_side=True)
    ocffm.srand(1)
    g.init()
    M = ocffm.Model.from_problem(g)
    E = embedding(M)
    rng = np.random.default_rng(17)
    q = rng.choice(n, size=45, replace=False)
    q = rng.permutation(np.concatenate([q, q[[0, 7]]]))
    for metric in METRICS:
        ref = sim_ref(E, metric)
        items, scores = M.similar_items(q, topn=10, metric=metric)
        assert_topn(items, scores, ref[q], tol_for(precision, ref), singles(q))
        for a in range(len(q)):  # repeated queries give identical rows
            for b in range(a + 1, len(q)):
                if q[a] == q[b]:
                    assert np.array_equal(items[a], items[b]) and np.array_equal(scores[a], scores[b])
    assert sum(int((q == x).sum()) - 1 for x in set(q.tolist())) == 2
    M.close()
    g.close()


@gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_exact_properties(precision, metric, trained):
    """Test 3: symmetry, sweep == pair, order and repeat independence, bit for bit."""
    for k in (5, 32):
        _, M, _ = trained(k, precision)
        rng = np.random.default_rng(23)
        a, b = rng.integers(0, N, size=500), rng.integers(0, N, size=500)
        sab, sba = M.item_similarity(a, b, metric=metric), M.item_similarity(b, a, metric=metric)
        assert sab.dtype == np.float64 and np.array_equal(sab, sba)
        assert np.isfinite(sab).all() and len(np.unique(sab)) > 100
        q = np.arange(N)
        for keep in (False, True):
            items, scores = M.similar_items(q, topn=128, metric=metric, keep_self=keep)
            full = items != NONE
            rows = np.nonzero(full)[0]
            pair = M.item_similarity(q[rows], items[full], metric=metric)
            assert np.array_equal(pair, scores[full])
            again = M.similar_items(q, topn=128, metric=metric, keep_self=keep)
            assert np.array_equal(again[0], items) and np.array_equal(again[1], scores)
        items, scores = M.similar_items(q, topn=10, metric=metric)
        perm = rng.permutation(N)
        pi, ps = M.similar_items(q[perm], topn=10, metric=metric)
        assert np.array_equal(pi, items[perm]) and np.array_equal(ps, scores[perm])
        part = M.similar_items(q[5:23], topn=10, metric=metric)
        assert np.array_equal(part[0], items[5:23]) and np.array_equal(part[1], scores[5:23])


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_slicing_chunking_determinism(precision, monkeypatch, tmp_path):
    """Test 3, third property: OCFFM_REC_SLICES x OCFFM_REC_ROWS change no bit."""
    snap = str(tmp_path / "model.bin")
    g = real_problem(5, precision)
    g.save_binary(snap)
    V = g._keep[2]
    results = []
    for slices in (None, "1", "3"):
        for rows in (None, "5"):
            for name, val in (("OCFFM_REC_SLICES", slices), ("OCFFM_REC_ROWS", rows)):
                if val is None:
                    monkeypatch.delenv(name, raising=False)
                else:
                    monkeypatch.setenv(name, val)
            M = ocffm.Model.load_binary(snap, precision)
            M.set_items(V)
            out = []
            for metric in METRICS:
                out += list(M.similar_items(np.arange(N), topn=10, metric=metric))
                out += list(M.similar_to(V, topn=10, metric=metric))
            results.append(out)
            M.close()
    g.close()
    for out in results[1:]:
        for x, y in zip(out, results[0]):
            assert np.array_equal(x, y)
    assert (results[0][0] != NONE).all()


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_exact_order_under_ties(precision):
    """Test 4: a catalogue whose rows 2t and 2t + 1 are the same feature rows
    (66 items) plus 5 of their own, on integer tables: inner products are
    exact integers, so the whole result is numpy's lexsort top-N."""
    g = tie_problem(precision)
    M = ocffm.Model.from_problem(g)
    d0, d1 = (int(d) for d in M.item_Ds)
    rows = [[(0, t % d0, 1.0), (1, t % d1, 1.0)] for t in range(38)]
    feats = [rows[t // 2] for t in range(66)] + rows[33:]
    n = len(feats)
    assert n == 71
    M.set_items(ocffm.ImpData.from_rows(synth._build_rows(feats, None), ds=M.item_Ds))
    E = embedding(M)
    assert (E == np.round(E)).all() and ((E * E).sum(axis=1) > 0).all()
    ref = sim_ref(E, "dot")
    assert max(len(np.unique(r)) for r in ref) < n  # tied
    q = np.arange(n)
    for topn in (1, 7, 70, 128):
        for keep in (False, True):
            items, scores = M.similar_items(q, topn=topn, metric="dot", keep_self=keep)
            for i in range(n):
                ei, es = exact_topn(ref[i], topn, set() if keep else {i})
                assert (items[i] == ei).all(), (i, topn, keep)
                assert (scores[i] == es).all(), (i, topn, keep)
    cref = sim_ref(E, "cosine")
    tol = tol_for(precision, cref)
    for i in range(66):  # (a property of the input: no other item is parallel to a twin pair)
        assert (np.delete(cref[i], [i, i ^ 1]) < 1 - 10 * tol).all()
    items, scores = M.similar_items(q, topn=5)
    for i in range(66):
        assert items[i, 0] == (i ^ 1) and abs(scores[i, 0] - 1.0) <= tol, (i, items[i, 0], scores[i, 0])
    assert_topn(items, scores, cref, tol, singles(q))
    M.close()
    g.close()


@gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_exclusion_lists(precision, metric, trained):
    """Test 5: ragged per-query lists united with the query itself."""
    _, M, E = trained(5, precision)
    ref = sim_ref(E, metric)
    tol = tol_for(precision, ref)
    q = np.array([0, 5, 12, 69, 5])
    lists = [[], [3, 3, 8, 8, 3, 5], [N, N + 7, 10 * N, 4], [j for j in range(N) if j != 69], [69, 0]]
    xptr = np.zeros(len(q) + 1, dtype=np.uint64)
    xptr[1:] = np.cumsum([len(x) for x in lists])
    xcol = np.array([j for x in lists for j in x], dtype=np.uint32)
    listed = [{j for j in x if j < N} for x in lists]
    for topn in (7, 128):
        items, scores = M.similar_items(q, topn=topn, metric=metric, exclude=(xptr, xcol))
        for i in range(len(q)):
            got = set(items[i][items[i] != NONE].tolist())
            assert not (got & listed[i]) and int(q[i]) not in got, i
        assert (items[3] == NONE).all() and (scores[3] == -np.inf).all()
        assert_topn(items, scores, ref[q], tol, [listed[i] | {int(q[i])} for i in range(len(q))])
        # the query itself comes back only with keep_self
        ki, ks = M.similar_items(q, topn=topn, metric=metric, keep_self=True, exclude=(xptr, xcol))
        assert_topn(ki, ks, ref[q], tol, listed)
        assert ki[3, 0] == 69 and (ki[3, 1:] == NONE).all()
        assert not (ki[1] == 5).any()  # (listed by the caller)
        if topn == 128:
            assert (ki[0] == 0).any() and (ki[2] == 12).any() and (ki[4] == 5).any()


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_zero_vectors(precision, trained):
    """Test 6: items without a kept node (an empty row; a node with idx >= Ds,
    dropped at read) are zero vectors: cosine exactly 0, still candidates."""
    g, _, _ = trained(5, precision)
    M = ocffm.Model.from_problem(g)
    feats = item_feats(dataset(5, "real").item)
    feats[10] = []
    feats[50] = [(0, int(M.item_Ds[0]) + 5, 1.0)]
    M.set_items(ocffm.ImpData.from_rows(synth._build_rows(feats, None), ds=M.item_Ds))
    E = embedding(M)
    zero = np.nonzero((E * E).sum(axis=1) == 0)[0]
    assert {10, 50} <= set(zero.tolist()) and len(zero) < N // 2
    allj = np.arange(N)
    for z in (10, 50):
        s = M.item_similarity(np.full(N, z), allj)
        assert (s == 0.0).all()
        assert (M.item_similarity(allj, np.full(N, z)) == 0.0).all()
    items, scores = M.similar_items(zero, topn=10)
    for r, z in enumerate(zero):
        assert items[r].tolist() == [j for j in range(N) if j != z][:10] and (scores[r] == 0.0).all()
    for metric in METRICS:
        ref = sim_ref(E, metric)
        for keep in (False, True):
            items, scores = M.similar_items(allj, topn=128, metric=metric, keep_self=keep)
            assert not np.isnan(scores).any()
            assert ((scores == -np.inf) == (items == NONE)).all()
            assert_topn(items, scores, ref, tol_for(precision, ref), [set()] * N if keep else singles(allj))
        assert not np.isnan(M.item_similarity(np.repeat(allj, N), np.tile(allj, N), metric=metric)).any()
    M.close()


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_similar_to(precision, trained, tmp_path):
    """Test 7: queries by item rows; copies of catalogue rows give
    similar_items' bits, a new row the numpy reference through H.  The
    catalogue is set from V, so its rows are projections like the queries'."""
    g, _, _ = trained(5, precision)
    snap = str(tmp_path / "m.bin")
    g.save_binary(snap)
    M = ocffm.Model.load_binary(snap, precision)
    M.set_items(g._keep[2])
    E = embedding(M)
    i = M.info
    f, fu, k = i["f"], i["fu"], i["k"]
    Ds = [int(d) for d in M.Ds]
    feats = item_feats(dataset(5, "real").item)
    new = [(0, 1, 0.75), (1, 2, 1.5), (0, Ds[fu] - 1, -0.5), (1, 0, 2.0)]
    Vq = ocffm.ImpData.from_rows(synth._build_rows([feats[3], new, feats[40], feats[69], []], None), ds=M.item_Ds)
    Eq = np.hstack([field_matrix(Vq, f2 - fu, Ds[f2]) @ M.get("H", ocffm.block_index(f1, f2, f)).reshape(Ds[f2], k)
                    for f1, f2 in cross_blocks(fu, f)])
    for metric in METRICS:
        ref = sim_ref(E, metric, Eq)
        tol = tol_for(precision, ref)
        want = M.similar_items([3, 40, 69], topn=128, metric=metric, keep_self=True)
        items, scores = M.similar_to(Vq, topn=128, metric=metric)
        assert items.shape == (5, 128)
        assert np.array_equal(items[[0, 2, 3]], want[0]) and np.array_equal(scores[[0, 2, 3]], want[1])
        assert_topn(items, scores, ref, tol, [set()] * 5)
        assert (items[:, :N] != NONE).all() and (items[:, N:] == NONE).all()
        if metric == "cosine":
            assert (scores[4, :N] == 0.0).all() and items[4, :N].tolist() == list(range(N))  # the empty row
        # windows
        wi, ws = M.similar_to(Vq, topn=128, row0=1, rows=3, metric=metric)
        assert np.array_equal(wi, items[1:4]) and np.array_equal(ws, scores[1:4])
        wi, ws = M.similar_to(Vq, topn=128, row0=2, metric=metric)
        assert np.array_equal(wi, items[2:]) and np.array_equal(ws, scores[2:])
        # lists: the shape of similar_items'
        xptr = np.array([0, 2, 2, 3], dtype=np.uint64)
        xcol = np.array([3, N + 1, 40], dtype=np.uint32)
        wi, ws = M.similar_to(Vq, topn=10, row0=0, rows=3, metric=metric, exclude=(xptr, xcol))
        assert_topn(wi, ws, ref[:3], tol, [{3}, set(), {40}])
        assert not (wi[0] == 3).any() and not (wi[2] == 40).any()
    M.close()


@gpu
def test_norm_cache_and_counters(trained, tmp_path):
    """Test 8: the inverse norms are built once per catalogue; similarity
    calls leave the other serving entries and the fold aggregates alone."""
    g, _, _ = trained(5, ocffm.FP64)
    snap = str(tmp_path / "m.bin")
    g.save_binary(snap)
    U, X, V = g._keep
    seen = seen_for(dataset(5, "real").test, U, N, 9)
    M = ocffm.Model.load_binary(snap, ocffm.FP64)
    M.set_items(V)
    assert M.counter("sim_norm_builds") == 0
    before = serve_all(M, X, seen, N)
    q = np.arange(N)
    first = M.similar_items(q, topn=10)
    assert M.counter("sim_norm_builds") == 1 and M.counter("sim_norm_us") >= 0
    assert M.counter("sim_setup_us") >= 0 and M.counter("rank_kernel_us") > 0
    second = M.similar_items(q, topn=10)
    M.item_similarity(q, q[::-1])
    M.similar_to(V, topn=10)
    M.similar_items(q, topn=10, metric="dot")
    assert M.counter("sim_norm_builds") == 1
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
    assert_same(serve_all(M, X, seen, N), before)
    assert M.counter("fold_stats_builds") == 0
    E = embedding(M)
    ref = sim_ref(E, "cosine")
    assert_topn(first[0], first[1], ref, tol_for(ocffm.FP64, ref), singles(q))
    # another catalogue: the norms are its own
    feats = item_feats(dataset(5, "real").item)
    feats = [[(fi, ix, 3.0 * v) for fi, ix, v in feats[(7 * j + 3) % N]] for j in range(N)] + feats[:13]
    V2 = ocffm.ImpData.from_rows(synth._build_rows(feats, None), ds=M.item_Ds)
    M.set_items(V2)
    assert M.counter("sim_norm_builds") == 1
    q2 = np.arange(len(feats))
    items, scores = M.similar_items(q2, topn=10)
    assert M.counter("sim_norm_builds") == 2
    E2 = embedding(M)
    assert np.abs((E2 * E2).sum(axis=1)[:N] - (E * E).sum(axis=1)[:N]).max() > 1.0  # stale norms would show
    ref2 = sim_ref(E2, "cosine")
    assert_topn(items, scores, ref2, tol_for(ocffm.FP64, ref2), singles(q2))
    pair = M.item_similarity(q2, q2[::-1])
    assert np.abs(pair - ref2[q2, q2[::-1]]).max() <= tol_for(ocffm.FP64, ref2)
    M.similar_items(q2, topn=10)
    assert M.counter("sim_norm_builds") == 2
    M.close()


@gpu
def test_errors_and_degenerate_inputs(trained, tmp_path):
    """Test 9."""
    g, _, _ = trained(5, ocffm.FP64)
    snap = str(tmp_path / "m.bin")
    g.save_binary(snap)
    V = g._keep[2]
    M = ocffm.Model.load_binary(snap, ocffm.FP64)
    L = ocffm.lib()
    import ctypes as C
    q = np.arange(4, dtype=np.uint32)
    items = np.zeros((4, 10), dtype=np.uint32)
    scores = np.zeros((4, 10), dtype=np.float64)
    out = np.zeros(4, dtype=np.float64)
    P = ocffm._ptr

    def sim_items(nq=4, qp=P(q), xptr=None, xcol=None, topn=10, flags=0, ip=P(items), sp=P(scores)):
        return L.ocffm_model_similar_items(M.h, nq, qp, xptr, xcol, topn, flags, ip, sp)

    def sim_to(Vh, row0=0, rows=4, xptr=None, xcol=None, topn=10, flags=0, ip=P(items), sp=P(scores)):
        return L.ocffm_model_similar_to(M.h, Vh, row0, rows, xptr, xcol, topn, flags, ip, sp)

    def pairs(n=4, pa=P(q), pb=P(q), flags=0, op=P(out)):
        return L.ocffm_model_item_similarity(M.h, n, pa, pb, flags, op)

    # before set_items
    assert sim_items() == ocffm.E_STATE and sim_to(V.h) == ocffm.E_STATE and pairs() == ocffm.E_STATE
    M.set_items(V)
    assert sim_to(V.h) == ocffm.OK and pairs() == ocffm.OK and sim_items() == ocffm.OK
    good = (items.copy(), scores.copy())
    # topn, NULL arrays, flags
    for call in (sim_items, lambda **kw: sim_to(V.h, **kw)):
        assert call(topn=0) == ocffm.E_ARG
        assert call(topn=129) == ocffm.E_ARG
        assert call(ip=None) == ocffm.E_ARG
        assert call(flags=4) == ocffm.E_ARG
        assert call(sp=None) == ocffm.OK  # scores are optional
    assert sim_items(qp=None) == ocffm.E_ARG
    assert pairs(pa=None) == ocffm.E_ARG and pairs(pb=None) == ocffm.E_ARG and pairs(op=None) == ocffm.E_ARG
    assert pairs(flags=8) == ocffm.E_ARG
    # a query outside the catalogue
    bad = np.array([0, 1, N, 2], dtype=np.uint32)
    assert sim_items(qp=P(bad)) == ocffm.E_ARG
    # row windows of Vq
    assert sim_to(V.h, row0=N - 3, rows=4) == ocffm.E_ARG
    assert sim_to(V.h, row0=N + 1, rows=0) == ocffm.E_ARG
    assert sim_to(None) == ocffm.E_ARG
    # more fields than fv
    rows3 = synth._build_rows([[(0, 0, 1.0), (2, 0, 1.0)]] * 4, None)
    assert sim_to(ocffm.ImpData.from_rows(rows3).h) == ocffm.E_ARG
    # a node with idx >= Ds[fid] (built without the model's Ds: the index is kept)
    rowsd = synth._build_rows([[(0, int(M.item_Ds[0]) + 3, 1.0)]] * 4, None)
    Vbad = ocffm.ImpData.from_rows(rowsd)
    assert sim_to(Vbad.h) == ocffm.E_DATA
    # list pairs
    x0 = np.array([1, 1, 2, 2, 3], dtype=np.uint64)
    xd = np.array([0, 2, 1, 3, 3], dtype=np.uint64)
    xok = np.array([0, 1, 1, 2, 3], dtype=np.uint64)
    xc = np.array([5, 6, 7], dtype=np.uint32)
    for call in (sim_items, lambda **kw: sim_to(V.h, **kw)):
        assert call(xptr=P(x0), xcol=P(xc)) == ocffm.E_ARG    # does not start at 0
        assert call(xptr=P(xd), xcol=P(xc)) == ocffm.E_ARG    # decreases
        assert call(xptr=P(xok), xcol=None) == ocffm.E_ARG    # entries without xcol
        assert call(xptr=None, xcol=P(xc)) == ocffm.E_ARG     # xcol without xptr
        assert call(xptr=P(xok), xcol=P(xc)) == ocffm.OK
    # zero queries / pairs
    assert sim_items(nq=0) == ocffm.OK and sim_items(nq=0, qp=None) == ocffm.OK
    assert sim_to(V.h, rows=0) == ocffm.OK and pairs(n=0, pa=None, pb=None, op=None) == ocffm.OK
    e = M.similar_items([], topn=10)
    assert e[0].shape == (0, 10) and e[1].shape == (0, 10)
    assert M.item_similarity([], []).shape == (0,)
    # pairs outside the catalogue are -inf
    s = M.item_similarity([0, N, 3, 2 ** 32 - 1], [N, 0, 3, 1])
    assert (s[[0, 1, 3]] == -np.inf).all() and np.isfinite(s[2])
    # a later valid call still works
    assert sim_items() == ocffm.OK
    assert np.array_equal(items, good[0]) and np.array_equal(scores, good[1])
    # an empty catalogue
    M.set_items(ocffm.ImpData.from_rows(synth._build_rows([], None), ds=M.item_Ds))
    assert M.info["n"] == 0
    ei, es = M.similar_to(V, topn=6)
    assert ei.shape == (N, 6) and (ei == NONE).all() and (es == -np.inf).all()
    assert (M.item_similarity([0, 1], [1, 0]) == -np.inf).all()
    assert sim_items() == ocffm.E_ARG  # no catalogue index exists
    assert M.similar_items([], topn=3)[0].shape == (0, 3)
    M.close()


@gpu
def test_cli(tmp_path):
    """Test 10: predict --similar on a saved text model writes what
    Model.load_text(...).similar_items returns, in --rec-out's format."""
    ds = synth.tiny()
    tr, it = str(tmp_path / "tr"), str(tmp_path / "item")
    ds.train.write(tr)
    ds.item.write(it)
    mtxt, out = str(tmp_path / "m.txt"), str(tmp_path / "sim.txt")
    r = subprocess.run([TRAIN, "-k", "4", "-t", "2", "--fp64", "-o", mtxt, it, tr], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    M = ocffm.Model.load_text(mtxt)
    M.set_items(ocffm.ImpData.read(it, False, M.item_Ds))
    n = int(M.info["n"])
    assert n == 50

    def same(path, items, scores, topn):
        lines = open(path).read().split("\n")
        assert lines[-1] == "" and len(lines) - 1 == items.shape[0]
        for i, line in enumerate(lines[:-1]):
            toks = line.split()
            nf = int((items[i] != NONE).sum())
            assert len(toks) == nf <= topn
            assert [int(t.split(":")[0]) for t in toks] == items[i, :nf].tolist(), i
            assert [float(t.split(":")[1]) for t in toks] == [float("%.17g" % s) for s in scores[i, :nf]], i

    r = subprocess.run([PREDICT, "--similar", "all", "--topn", "7", "--sim-out", out, mtxt, it],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    items, scores = M.similar_items(range(n), 7)
    assert (items != NONE).all()
    same(out, items, scores, 7)
    qf = str(tmp_path / "q")
    with open(qf, "w") as fh:
        fh.write("49\n3\n\n 17 \n3\n")
    r = subprocess.run([PREDICT, "--similar", qf, "--topn", "60", "--sim-out", out, "--sim-metric", "dot", mtxt, it],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    items, scores = M.similar_items([49, 3, 17, 3], 60, metric="dot")
    same(out, items, scores, 60)
    M.close()
    os.remove(out)
    for args in (["--similar", "all", mtxt, it], ["--sim-out", out, mtxt, it],
                 ["--similar", "all", "--sim-out", out, "--sim-metric", "l2", mtxt, it],
                 ["--similar", str(tmp_path / "nothing"), "--sim-out", out, mtxt, it]):
        r = subprocess.run([PREDICT] + args, capture_output=True, text=True)
        assert r.returncode == 1 and r.stderr.strip() and not os.path.exists(out), args
    with open(qf, "w") as fh:
        fh.write("50\n")
    r = subprocess.run([PREDICT, "--similar", qf, "--sim-out", out, mtxt, it], capture_output=True, text=True)
    assert r.returncode == 1 and "error:" in r.stderr and not os.path.exists(out)  # OCFFM_E_ARG from the call
