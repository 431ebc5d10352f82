"""Serving from a saved model (ocffm_model / ocffm.Model / predict).

Bit comparisons are against the problem's own path (load_binary's block-by-
block projection, then the same serving driver).  Numeric references are numpy
fp64 products of the model's own W / H (Model.get) with the per-field CSR of
the rows (ImpData.field), independent of the projection kernel and the sweeps.
Tolerances are test_recommend's tol_for (1e-12 fp64, 1e-3 fp32, relative to
max(1, max|ref|)); label ranks take test_evaluate's window (the rank lies in
[#{ref > ref_p + 2 tol}, #{ref >= ref_p - 2 tol} - 1]).  Integer tables give
exact scores in both precisions and compare exactly."""
import os
import subprocess

import numpy as np
import pytest

import ocffm
import synth
from test_recommend import (NONE, assert_topn, cold_rows, dataset, exact_topn, excluded_sets, field_matrix,
                            popularity, real_problem, tie_problem, tol_for)

gpu = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(REPO, "one-class-ffm_amd", "train")
PREDICT = os.path.join(REPO, "one-class-ffm_amd", "predict")
PRECISIONS = [ocffm.FP64, ocffm.FP32]
N = 70  # items of test_recommend's dataset


# ---------------------------------------------------------------- helpers
def cross_blocks(fu, f):
    return [(f1, f2) for f1 in range(fu) for f2 in range(fu, f)]


def model_reference(M, X, V, pop=None):
    """ref[i, j] = a_i + b_j + sum_c <P_c[i], Q_c[j]> from the model's W / H
    alone; cold rows: pop[j] for j < len(pop), -inf (no candidate) beyond."""
    i = M.info
    f, fu, k = i["f"], i["fu"], i["k"]
    Ds = [int(d) for d in M.Ds]
    used = i["used"]
    m, n = int(X.info["m"]), int(V.info["m"])
    A = [field_matrix(X, fi, Ds[fi]) for fi in range(fu)] + [field_matrix(V, fi - fu, Ds[fi]) for fi in range(fu, f)]
    ref = np.zeros((m, n))
    Q, b = {}, np.zeros(n)
    for f1, f2 in cross_blocks(fu, f):
        b12 = ocffm.block_index(f1, f2, f)
        P = A[f1] @ M.get("W", b12).reshape(Ds[f1], k)
        Q[b12] = A[f2] @ M.get("H", b12).reshape(Ds[f2], k)
        ref += P @ Q[b12].T
    a = np.zeros(m)
    for lo, hi, acc in ((0, fu, a), (fu, f, b)):
        for f1 in range(lo, hi):
            for f2 in range(f1, hi):
                b12 = ocffm.block_index(f1, f2, f)
                if used[b12]:
                    acc += ((A[f1] @ M.get("W", b12).reshape(Ds[f1], k)) *
                            (A[f2] @ M.get("H", b12).reshape(Ds[f2], k))).sum(axis=1)
    ref += a[:, None] + b[None, :]
    cold = cold_rows(X)
    for r in np.nonzero(cold)[0]:
        ref[r, :] = -np.inf
        if pop is not None:
            ref[r, :len(pop)] = pop
    return ref, cold, Q, b


def lists_for(rows, n, seed):
    """Per-row candidate lists: ragged, with repeats and entries >= n, one empty."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 50, size=rows)
    lens[1 % rows] = 0
    cptr = np.zeros(rows + 1, dtype=np.uint64)
    cptr[1:] = np.cumsum(lens)
    ccol = rng.integers(0, n + 4, size=int(cptr[-1])).astype(np.uint32)
    return cptr, ccol


def seen_for(rows, U, n, seed):
    """A labelled copy of the rows whose labels play the seen items."""
    rng = np.random.default_rng(seed)
    labs = [np.sort(rng.choice(n + 3, size=int(rng.integers(0, 6)), replace=False)) for _ in range(rows.m)]
    yptr = np.zeros(rows.m + 1, dtype=np.uint64)
    yptr[1:] = np.cumsum([len(x) for x in labs])
    ycol = np.concatenate(labs).astype(np.uint64)
    return ocffm.ImpData.from_rows(synth.Rows(rows.xptr, rows.fid, rows.idx, rows.val, yptr, ycol), ds=U.Ds)


def serve_all(h, X, seen, n, seed=3):
    """Every serving entry of a problem or a model on X, plain and among lists."""
    m = int(X.info["m"])
    rng = np.random.default_rng(seed)
    prow = rng.integers(0, m, size=200)
    pitem = rng.integers(0, n + 3, size=200)
    cand = lists_for(m, n, seed + 1)
    out = dict(rec=h.recommend(X, topn=20), rec_x=h.recommend(X, topn=20, exclude_labels=True),
               score=(h.score(X, prow, pitem),), lr=h.label_ranks(X, seen=seen), ev=h.evaluate(X),
               ev_s=h.evaluate(X, seen=seen, cuts=(1, 3, 10)),
               rec_c=h.recommend(X, topn=20, candidates=cand),
               rec_cx=h.recommend(X, topn=20, exclude_labels=True, candidates=cand),
               lr_c=h.label_ranks(X, seen=seen, candidates=cand), ev_c=h.evaluate(X, candidates=cand))
    return out


def assert_same(a, b):
    assert a.keys() == b.keys()
    for key in a:
        x, y = a[key], b[key]
        if isinstance(x, dict):
            assert x.keys() == y.keys(), key
            for kk in x:
                assert np.array_equal(np.asarray(x[kk]), np.asarray(y[kk])), (key, kk)
        else:
            assert len(x) == len(y)
            for u, v in zip(x, y):
                assert u.dtype == v.dtype and np.array_equal(u, v), key


def assert_same_catalogue(M, g):
    fu, f = M.info["fu"], M.info["f"]
    for f1, f2 in cross_blocks(fu, f):
        b12 = ocffm.block_index(f1, f2, f)
        assert np.array_equal(M.get("Q", b12), g.get("Q", b12)), (f1, f2)
        for what in "WH":
            assert np.array_equal(M.get(what, b12), g.get(what, b12))
    assert np.array_equal(M.get("b"), g.get("b"))


_SNAP = {}


@pytest.fixture(scope="module")
def snapshot(tmp_path_factory):
    """(trained problem, its snapshot's path) per (k, precision): init and one epoch."""
    def make(k, precision):
        if (k, precision) not in _SNAP:
            g = real_problem(k, precision)
            path = str(tmp_path_factory.mktemp("snap") / f"m{k}_{precision}.bin")
            g.save_binary(path)
            _SNAP[(k, precision)] = (g, path)
        return _SNAP[(k, precision)]
    yield make
    for g, _ in _SNAP.values():
        g.close()
    _SNAP.clear()


def loaded_problem(k, precision, path, self_side=True, vals="real"):
    g2 = ocffm.problem_from_dataset(dataset(k, vals), precision=precision, self_side=self_side)
    g2.load_binary(path)
    return g2


# ------------------------------------------------------------------ tests
@gpu
@pytest.mark.parametrize("k", [5, 32, 100])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_bits_same_catalogue(k, precision, snapshot):
    """Test 1: a model that loaded the snapshot and projected V itself equals
    a problem that loaded it, on the catalogue's tables and every serving
    entry; a model taken from the trained problem equals that problem."""
    g, path = snapshot(k, precision)
    g2 = loaded_problem(k, precision, path)
    U, X, V = g2._keep
    seen = seen_for(dataset(k, "real").test, U, N, 9)
    M = ocffm.Model.load_binary(path, precision)
    i = M.info
    assert (i["f"], i["fu"], i["fv"], i["k"], i["precision"]) == (4, 2, 2, k, precision)
    assert np.array_equal(M.Ds, np.concatenate([U.Ds, V.Ds])) and np.array_equal(M.item_Ds, V.Ds)
    assert not i["has_items"]
    M.set_items(V)
    M.set_popularity(popularity(U))
    assert M.info["has_items"] and M.info["n"] == N and M.counter("project_us") >= 0
    assert_same_catalogue(M, g2)
    want = serve_all(g2, X, seen, N)
    assert cold_rows(X).any()
    assert_same(serve_all(M, X, seen, N), want)
    # the trained state: b was updated incrementally, not recomputed
    T = ocffm.Model.from_problem(g)
    assert T.info["has_items"] and T.info["npop"] == int(U.info["n"])
    assert_same_catalogue(T, g)
    assert_same(serve_all(T, X, seen, N), serve_all(g, X, seen, N))
    for h in (M, T, g2):
        h.close()


def edge_rows(rng, count, dims, labels_n=None):
    """Hand-made rows of two fields: the projection's edge cases first, then
    random rows of 0..3 real-valued nodes per field."""
    d0, d1 = dims
    feats = [
        [],                                                            # no node in any field
        [(0, d0 - 1, 1.0)],                                            # no node in field 1
        [(1, d1 - 1, 0.375)],                                          # no node in field 0
        [(0, q % d0, 0.25 + 0.125 * (q % 5)) for q in range(70)] + [(1, 0, 2.0)],  # wider than a wave
        [(0, 2, 0.5), (0, 2, 1.5), (1, 1, 2.0), (1, 1, -0.75)],        # repeated indices
        [(1, 1, 3.0), (0, 0, -1.25), (1, 0, 0.5)],                     # fields interleaved in the file
    ]
    while len(feats) < count:
        row = []
        for f in range(2):
            for _ in range(int(rng.integers(0, 4))):
                row.append((f, int(rng.integers(0, dims[f])), float(np.round(rng.random() * 2 - 0.5, 3))))
        feats.append(row)
    labels = None
    if labels_n is not None:
        labels = [np.sort(rng.choice(labels_n, size=int(rng.integers(1, 5)), replace=False)) for _ in range(count)]
    return synth._build_rows(feats, labels)


@gpu
@pytest.mark.parametrize("k", [3, 16, 64])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_projection_edges(k, precision, tmp_path, monkeypatch):
    """Test 2: k_project_side on hand-made rows (KP 4, 16, 64; test 1 runs 8,
    32, 128): 130 items (two full item tiles and a ragged one) and 40 query
    rows, against numpy, against the block-by-block path, and on a capped
    grid."""
    rng = np.random.default_rng(21)
    du, dv, n = (12, 7), (9, 6), 130
    item = edge_rows(rng, n, dv)
    train = edge_rows(rng, 60, du, labels_n=n)
    test = edge_rows(rng, 40, du, labels_n=n)
    ds = synth.Dataset("edges", train, item, test, k=k, params=dict(k=k, t=1, l=0.5, w=0.05, r=-1.0))
    g = ocffm.problem_from_dataset(ds, precision=precision, self_side=True)
    ocffm.srand(1)
    g.init()
    path = str(tmp_path / "m.bin")
    g.save_binary(path)
    g2 = ocffm.problem_from_dataset(ds, precision=precision, self_side=True)
    g2.load_binary(path)
    U, X, V = g2._keep
    assert [int(d) for d in U.Ds] == list(du) and [int(d) for d in V.Ds] == list(dv)

    def model():
        M = ocffm.Model.load_binary(path, precision)
        M.set_items(ocffm.ImpData.from_rows(item, ds=M.item_Ds))
        return M

    M = model()
    ref, cold, Q, b = model_reference(M, X, V)
    tol = tol_for(precision, ref)
    assert cold[0] and not cold[1:6].any()
    for b12, q in Q.items():
        got = M.get("Q", b12).reshape(n, k)
        err = float(np.abs(got - q).max())
        print("Q", b12, err, tol)
        assert err <= tol
        assert (got[0] == 0).all()  # the item without nodes
    print("b", float(np.abs(M.get("b") - b).max()), tol)
    assert np.abs(M.get("b") - b).max() <= tol and M.get("b")[0] == 0
    assert_same_catalogue(M, g2)
    # the query rows' projection: every pair's score, against numpy and the problem
    prow, pitem = np.divmod(np.arange(40 * n), n)
    sc = M.score(X, prow, pitem).reshape(40, n)
    assert (sc[cold] == -np.inf).all()  # the cold rows: no popularity, no candidate
    print("score", float(np.abs(sc[~cold] - ref[~cold]).max()), tol)
    assert np.abs(sc[~cold] - ref[~cold]).max() <= tol
    sp = g2.score(X, prow, pitem).reshape(40, n)
    assert np.array_equal(sc[~cold], sp[~cold])
    rec = M.recommend(X, topn=20)
    assert_topn(rec[0], rec[1], ref, tol, excluded_sets(X, n, False))
    # a grid of one block, whose subgroups stride over the (row, job) pairs
    monkeypatch.setenv("OCFFM_PROJECT_BLOCKS", "1")
    M1 = model()
    assert_same_catalogue(M1, g2)
    assert np.array_equal(M1.score(X, prow, pitem).reshape(40, n), sc)
    r1 = M1.recommend(X, topn=20)
    assert np.array_equal(r1[0], rec[0]) and np.array_equal(r1[1], rec[1])
    for h in (M, M1, g, g2):
        h.close()


def rank_window(ranks, scores, ncand, ref, X, tol):
    yptr, ycol = X.labels()
    for i in range(ref.shape[0]):
        fin = np.isfinite(ref[i])
        assert int(ncand[i]) == int(fin.sum())
        for p in range(int(yptr[i]), int(yptr[i + 1])):
            j = int(ycol[p])
            if j >= ref.shape[1] or not fin[j]:
                assert ranks[p] == NONE and scores[p] == -np.inf
                continue
            assert abs(scores[p] - ref[i, j]) <= tol, (i, j)
            lo = int((ref[i, fin] > ref[i, j] + 2 * tol).sum())
            hi = int((ref[i, fin] >= ref[i, j] - 2 * tol).sum()) - 1
            assert lo <= int(ranks[p]) <= hi, (i, j, int(ranks[p]), lo, hi)


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_new_catalogue(precision, snapshot):
    """Test 3: a catalogue the model was not trained on (V's rows in another
    order plus unseen feature combinations, 130 items), the popularity rules,
    and back to V."""
    g, path = snapshot(5, precision)
    g2 = loaded_problem(5, precision, path)
    U, X, V = g2._keep
    M = ocffm.Model.load_binary(path, precision)
    dv = [int(d) for d in M.item_Ds]
    item = dataset(5, "real").item
    rng = np.random.default_rng(31)
    feats = []
    for j in rng.permutation(N):
        feats.append([(int(item.fid[p]), int(item.idx[p]), float(item.val[p]))
                      for p in range(int(item.xptr[j]), int(item.xptr[j + 1]))])
    while len(feats) < 130:
        feats.append([(f, int(rng.integers(0, dv[f])), float(np.round(rng.random() * 2, 3) + 0.25))
                      for f in (0, 1, 0, 1)[:int(rng.integers(1, 5))]])
    Vn = ocffm.ImpData.from_rows(synth._build_rows(feats, None), ds=M.item_Ds)
    M.set_items(V)
    M.set_popularity(popularity(U))
    M.set_items(Vn)
    assert M.info["n"] == 130 and M.info["npop"] == 0  # set_items clears the popularity
    ref, cold, _, _ = model_reference(M, X, Vn)
    tol = tol_for(precision, ref)
    rec = M.recommend(X, topn=20)
    assert_topn(rec[0], rec[1], ref, tol, excluded_sets(X, 130, False))
    c = int(np.nonzero(cold)[0][0])
    assert (rec[0][c] == NONE).all() and (rec[1][c] == -np.inf).all()
    ranks, scores, ncand = M.label_ranks(X)
    rank_window(ranks, scores, ncand, ref, X, tol)
    # popularity over the first ten catalogue items, with ties: by value, then by index
    pop = np.array([0.5, 0.25, 0.5, 0.25, 0.125, 0.5, 0.0, 0.25, 1.0, 0.125])
    M.set_popularity(pop)
    assert M.info["npop"] == 10
    ref, _, _, _ = model_reference(M, X, Vn, pop)
    rec = M.recommend(X, topn=20)
    ei, es = exact_topn(ref[c], 20, set())
    assert ei[:10].tolist() == [8, 0, 2, 5, 1, 3, 7, 4, 9, 6] and (ei[10:] == NONE).all()
    assert np.array_equal(rec[0][c], ei) and np.array_equal(rec[1][c], es)
    assert_topn(rec[0], rec[1], ref, tol, excluded_sets(X, 130, False))
    ranks, scores, ncand = M.label_ranks(X)
    rank_window(ranks, scores, ncand, ref, X, tol)
    # an empty catalogue: no row has a candidate
    M.set_items(ocffm.ImpData.from_rows(synth._build_rows([], None), ds=M.item_Ds))
    rec = M.recommend(X, topn=5)
    assert M.info["n"] == 0 and (rec[0] == NONE).all() and (rec[1] == -np.inf).all()
    assert (M.score(X, [0, 1], [0, 5]) == -np.inf).all()
    ranks, scores, ncand = M.label_ranks(X)
    assert (ranks == NONE).all() and (scores == -np.inf).all() and (ncand == 0).all()
    # back to V: test 1's results
    M.set_items(V)
    M.set_popularity(popularity(U))
    seen = seen_for(dataset(5, "real").test, U, N, 9)
    assert_same_catalogue(M, g2)
    assert_same(serve_all(M, X, seen, N), serve_all(g2, X, seen, N))
    M.close()
    g2.close()


def parse_text_model(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    f, fu, fv, k = (int(x) for x in lines[:4])
    Ds = [int(x) for x in lines[4:4 + f]]
    tabs = {}
    for line in lines[4 + f:-1]:
        head, *vals = line.split(" ")
        what, f1, f2, row = head.split(",")
        t = tabs.setdefault((what, int(f1), int(f2)), [])
        assert int(row) == len(t) and len(vals) == k
        t.append([float(v) for v in vals])
    return f, fu, fv, k, Ds, {key: np.array(v) for key, v in tabs.items()}


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_text_model(precision, snapshot, tmp_path):
    """Test 4: the text model round trip, and a --ns model's file."""
    g, _ = snapshot(5, precision)
    U, X, V = g._keep
    path = str(tmp_path / "model.txt")
    g.save_model(path)
    f, fu, fv, k, Ds, tabs = parse_text_model(path)
    M = ocffm.Model.load_text(path, precision)
    i = M.info
    assert (i["f"], i["fu"], i["fv"], i["k"]) == (f, fu, fv, k) == (4, 2, 2, 5) and M.Ds.tolist() == Ds
    assert i["self_side"] and i["nused"] == 10 and len(tabs) == 20
    for (what, f1, f2), t in tabs.items():
        want = t if precision == ocffm.FP64 else t.astype(np.float32).astype(np.float64)
        assert np.array_equal(M.get(what, ocffm.block_index(f1, f2, f)).reshape(t.shape), want), (what, f1, f2)
    M.set_items(V)
    ref, _, _, _ = model_reference(M, X, V)
    rec = M.recommend(X, topn=20)
    assert_topn(rec[0], rec[1], ref, tol_for(precision, ref), excluded_sets(X, N, False))
    M.close()
    # --ns: the side blocks are unused, a and b are zero
    gn = ocffm.problem_from_dataset(dataset(5, "real"), precision=precision, self_side=False)
    ocffm.srand(1)
    gn.init()
    gn.save_model(path)
    Mn = ocffm.Model.load_text(path, precision)
    i = Mn.info
    assert not i["self_side"] and i["nused"] == 4
    assert [b for b in range(10) if i["used"][b]] == [ocffm.block_index(f1, f2, 4) for f1, f2 in cross_blocks(2, 4)]
    with pytest.raises(ocffm.OcffmError) as e:
        Mn.get("W", ocffm.block_index(0, 1, 4))
    assert e.value.code == ocffm.E_ARG
    Mn.set_items(V)
    assert (Mn.get("b") == 0).all()
    ref, cold, _, _ = model_reference(Mn, X, V)
    cross = np.zeros_like(ref)
    for f1, f2 in cross_blocks(2, 4):
        b12 = ocffm.block_index(f1, f2, 4)
        cross += (field_matrix(X, f1, Ds[f1]) @ Mn.get("W", b12).reshape(Ds[f1], 5)) @ Mn.get("Q", b12).reshape(N, 5).T
    tol = tol_for(precision, ref)
    assert np.abs(cross[~cold] - ref[~cold]).max() <= tol  # nothing but the cross blocks: a = b = 0
    prow, pitem = np.divmod(np.arange(37 * N), N)
    sc = Mn.score(X, prow, pitem).reshape(37, N)
    assert np.abs(sc[~cold] - ref[~cold]).max() <= tol
    Mn.close()
    gn.close()


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_integer_table_ties(precision, tmp_path):
    """Test 5: tie_problem's integer tables through a snapshot: exact scores,
    exact order (score descending, then item index)."""
    g = tie_problem(precision)
    U, X, V = g._keep
    path = str(tmp_path / "ties.bin")
    g.save_binary(path)
    M = ocffm.Model.load_binary(path, precision)
    assert not M.info["self_side"]
    M.set_items(V)
    pop = popularity(U)
    M.set_popularity(pop)
    ref, cold, _, _ = model_reference(M, X, V, pop)
    warm = ref[~cold]
    assert (warm == np.round(warm)).all() and max(len(np.unique(r)) for r in warm) < N  # exact and tied
    excl = excluded_sets(X, N, True)
    for topn in (1, 7, 70):
        items, scores = M.recommend(X, topn=topn)
        ix, sx = M.recommend(X, topn=topn, exclude_labels=True)
        for i in range(ref.shape[0]):
            ei, es = exact_topn(ref[i], topn, set())
            assert np.array_equal(items[i], ei) and np.array_equal(scores[i], es), (i, topn)
            ei, es = exact_topn(ref[i], topn, excl[i])
            assert np.array_equal(ix[i], ei) and np.array_equal(sx[i], es), (i, topn)
    gi, gs = g.recommend(X, topn=70)
    assert np.array_equal(gi, items) and np.array_equal(gs, scores)
    M.close()
    g.close()


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_chunking_and_slicing(precision, snapshot, monkeypatch):
    """Test 6: the knobs are read when the model is created; results do not
    depend on them."""
    g, path = snapshot(5, precision)
    U, X, V = g._keep
    seen = seen_for(dataset(5, "real").test, U, N, 9)
    results = []
    for knobs in ({}, {"OCFFM_REC_ROWS": "7", "OCFFM_REC_SLICES": "3", "OCFFM_REC_SEG": "16"},
                  {"OCFFM_REC_ROWS": "7"}, {"OCFFM_REC_SLICES": "3", "OCFFM_PROJECT_BLOCKS": "2"}):
        for name in ("OCFFM_REC_ROWS", "OCFFM_REC_SLICES", "OCFFM_REC_SEG", "OCFFM_PROJECT_BLOCKS"):
            monkeypatch.delenv(name, raising=False)
        for name, val in knobs.items():
            monkeypatch.setenv(name, val)
        M = ocffm.Model.load_binary(path, precision)
        for name in knobs:
            monkeypatch.delenv(name)  # read at create: gone before the calls
        M.set_items(V)
        M.set_popularity(popularity(U))
        results.append(serve_all(M, X, seen, N))
        part = M.recommend(X, topn=20, row0=5, rows=18)
        assert np.array_equal(part[0], results[-1]["rec"][0][5:23]) and np.array_equal(part[1], results[-1]["rec"][1][5:23])
        M.close()
    for r in results[1:]:
        assert_same(r, results[0])


@gpu
def test_errors(snapshot):
    """Test 7: the error codes of ocffm.h."""
    g, path = snapshot(5, ocffm.FP64)
    U, X, V = g._keep
    ds = dataset(5, "real")

    def code(fn, *a, **kw):
        with pytest.raises(ocffm.OcffmError) as e:
            fn(*a, **kw)
        return e.value.code

    M = ocffm.Model.load_binary(path)
    cand = lists_for(37, N, 4)
    # serving before set_items
    assert code(M.recommend, X, topn=5) == ocffm.E_STATE
    assert code(M.recommend, X, topn=5, candidates=cand) == ocffm.E_STATE
    assert code(M.score, X, [0], [0]) == ocffm.E_STATE
    assert code(M.label_ranks, X) == ocffm.E_STATE
    assert code(M.label_ranks, X, candidates=cand) == ocffm.E_STATE
    assert code(M.evaluate, X) == ocffm.E_STATE
    assert code(M.evaluate, X, candidates=cand) == ocffm.E_STATE
    assert code(M.set_popularity, [1.0]) == ocffm.E_STATE
    assert code(M.get, "b") == ocffm.E_STATE
    # a catalogue with too many fields, or an index beyond Ds
    wide = synth._build_rows([[(0, 0, 1.0), (2, 0, 1.0)]], None)
    assert code(M.set_items, ocffm.ImpData.from_rows(wide)) == ocffm.E_ARG
    far = synth._build_rows([[(0, int(M.item_Ds[0]), 1.0)]], None)
    assert code(M.set_items, ocffm.ImpData.from_rows(far)) == ocffm.E_DATA
    assert not M.info["has_items"]  # a refused catalogue leaves the model as it was
    M.set_items(V)
    good = M.recommend(X, topn=10)
    assert code(M.set_items, ocffm.ImpData.from_rows(far)) == ocffm.E_DATA
    assert M.info["n"] == N
    # the serving calls' arguments
    assert code(M.recommend, X, topn=0) == ocffm.E_ARG
    assert code(M.recommend, X, topn=129) == ocffm.E_ARG
    assert code(M.recommend, X, topn=129, candidates=cand) == ocffm.E_ARG
    assert code(M.recommend, X, topn=10, row0=30, rows=8) == ocffm.E_ARG
    t = ds.test
    wide = synth.Rows(t.xptr, np.where(np.arange(len(t.fid)) == 0, 2, t.fid).astype(np.uint32), t.idx, t.val, t.yptr, t.ycol)
    Xwide = ocffm.ImpData.from_rows(wide)
    bad = synth.Rows(t.xptr, t.fid, t.idx.copy(), t.val, t.yptr, t.ycol)
    bad.idx[0] = int(M.Ds[int(bad.fid[0])]) + 3
    Xbad = ocffm.ImpData.from_rows(bad)
    for fn, kw in ((M.recommend, dict(topn=5)), (M.label_ranks, {}), (M.evaluate, {}),
                   (M.recommend, dict(topn=5, candidates=cand)), (M.label_ranks, dict(candidates=cand))):
        assert code(fn, Xwide, **kw) == ocffm.E_ARG
        assert code(fn, Xbad, **kw) == ocffm.E_DATA
    assert code(M.score, Xwide, [0], [0]) == ocffm.E_ARG and code(M.score, Xbad, [0], [0]) == ocffm.E_DATA
    assert code(M.score, X, [37], [0]) == ocffm.E_ARG
    assert code(M.label_ranks, V) == ocffm.E_ARG  # no labels
    assert code(M.evaluate, X, cuts=(5, 5)) == ocffm.E_ARG
    assert code(M.evaluate, X, cuts=()) == ocffm.E_ARG
    assert code(M.get, "Q", ocffm.block_index(0, 1, 4)) == ocffm.E_ARG  # a side block
    assert code(M.get, "x") == ocffm.E_ARG and code(M.get, "W", 99) == ocffm.E_ARG
    # null outputs and a bad cptr, at the C entries
    L = ocffm.lib()
    import ctypes as C
    items = np.zeros(37 * 5, dtype=np.uint32)
    ranks = np.zeros(int(X.info["nnz_y"]), dtype=np.uint32)
    assert L.ocffm_model_recommend(M.h, X.h, 0, 37, 5, 0, None, None) == ocffm.E_ARG
    assert L.ocffm_model_recommend(M.h, None, 0, 37, 5, 0, ocffm._ptr(items), None) == ocffm.E_ARG
    assert L.ocffm_model_recommend(None, X.h, 0, 37, 5, 0, ocffm._ptr(items), None) == ocffm.E_ARG
    assert L.ocffm_model_label_ranks(M.h, X.h, None, None, None, None) == ocffm.E_ARG
    assert L.ocffm_model_evaluate(M.h, X.h, None, ocffm._ptr(np.array([5], dtype=np.uint32)), 1, None) == ocffm.E_ARG
    assert L.ocffm_model_score(M.h, X.h, 1, None, None, None) == ocffm.E_ARG
    assert L.ocffm_model_get_info(M.h, None) == ocffm.E_ARG
    assert L.ocffm_model_counter(M.h, None, None) == ocffm.E_ARG
    cptr = np.zeros(38, dtype=np.uint64)
    ccol = np.zeros(4, dtype=np.uint32)
    assert L.ocffm_model_recommend_among(M.h, X.h, 0, 37, None, ocffm._ptr(ccol), 5, 0, ocffm._ptr(items), None) == ocffm.E_ARG
    cptr[0] = 1
    assert L.ocffm_model_recommend_among(M.h, X.h, 0, 37, ocffm._ptr(cptr), ocffm._ptr(ccol), 5, 0, ocffm._ptr(items), None) == ocffm.E_ARG
    cptr[:] = 0
    cptr[3], cptr[4:] = 4, 2  # decreasing
    assert L.ocffm_model_label_ranks_among(M.h, X.h, None, ocffm._ptr(cptr), ocffm._ptr(ccol), ocffm._ptr(ranks), None, None) == ocffm.E_ARG
    cptr[4:] = 4
    assert L.ocffm_model_label_ranks_among(M.h, X.h, None, ocffm._ptr(cptr), None, ocffm._ptr(ranks), None, None) == ocffm.E_ARG
    h = C.c_void_p()
    assert L.ocffm_model_load_binary(b"/nonexistent/model.bin", ocffm.FP64, 0, C.byref(h)) == ocffm.E_IO and not h.value
    assert L.ocffm_model_load_binary(path.encode(), 16, 0, C.byref(h)) == ocffm.E_ARG and not h.value
    assert L.ocffm_model_load_text(path.encode(), ocffm.FP64, 0, C.byref(h)) == ocffm.E_DATA and not h.value
    # from_problem before init
    fresh = ocffm.problem_from_dataset(ds, precision=ocffm.FP64, self_side=True)
    assert code(ocffm.Model.from_problem, fresh) == ocffm.E_STATE
    fresh.close()
    # rows == 0, and a valid call after all of the above
    it0, sc0 = M.recommend(X, topn=10, rows=0)
    assert it0.shape == (0, 10) and sc0.shape == (0, 10)
    after = M.recommend(X, topn=10)
    assert np.array_equal(after[0], good[0]) and np.array_equal(after[1], good[1])
    assert M.counter("rec_setup_us") > 0 and M.counter("rank_kernel_us") > 0 and M.counter("nothing") == 0
    M.close()


def _cli_files(tmp_path):
    ds = synth.tiny()
    tr, it, te = (str(tmp_path / x) for x in ("tr", "item", "te"))
    ds.train.write(tr)
    ds.item.write(it)
    ds.test.write(te)
    return tr, it, te


def _assert_rec_file(path, items, scores, topn):
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and len(lines) - 1 == items.shape[0]
    for i, line in enumerate(lines[:-1]):
        toks = line.split()
        nf = int((items[i] != NONE).sum())
        assert len(toks) == nf <= topn
        assert [int(t.split(":")[0]) for t in toks] == items[i, :nf].tolist(), i
        assert [float(t.split(":")[1]) for t in toks] == [float("%.17g" % s) for s in scores[i, :nf]], i


def _eval_table(e):
    out = ["eval rows %d rows_used %d labels %d labels_ranked %d" % (e["rows"], e["rows_used"], e["labels"],
                                                                    e["labels_ranked"]),
           "eval loss %.17g mrr %.17g auc %.17g" % (e["loss"], e["mrr"], e["auc"]), "eval cut prec recall ndcg map hit"]
    for s, c in enumerate(e["cuts"]):
        out.append("eval %d %.17g %.17g %.17g %.17g %.17g" % (c, e["prec"][s], e["recall"][s], e["ndcg"][s],
                                                              e["map"][s], e["hit"][s]))
    return out


@gpu
def test_cli(tmp_path):
    """Test 8: train --binary-out, then predict on that snapshot.  train's own
    serving state after a solve is not the snapshot's (its b was updated
    incrementally), and the CLI has no way to make train load a snapshot, so
    predict's files are compared with ocffm.Model's results on the same
    snapshot, byte for byte after formatting, as test_cli_matches_python does."""
    tr, it, te = _cli_files(tmp_path)
    mbin, mtxt, a, b = (str(tmp_path / x) for x in ("m.bin", "m.txt", "a.txt", "b.txt"))
    r = subprocess.run([TRAIN, "-k", "4", "-t", "2", "--fp64", "-o", mtxt, "--binary-out", mbin, "--recommend", te,
                        "--topn", "7", "--rec-out", a, "--eval", te, it, tr], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    train_eval = [x for x in r.stdout.split("\n") if x.startswith("eval")]
    fi = ocffm.model_file_info(mbin, binary=True)
    assert fi["k"] == 4 and fi["self_side"] and ocffm.model_file_info(mtxt)["Ds"].tolist() == fi["Ds"].tolist()
    r = subprocess.run([PREDICT, "--fp64", "--binary", "--popularity", tr, "--recommend", te, "--topn", "7",
                        "--rec-out", b, "--eval", te, mbin, it], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    U = ocffm.ImpData.read(tr, True)
    M = ocffm.Model.load_binary(mbin)
    V = ocffm.ImpData.read(it, False, M.item_Ds)
    M.set_items(V)
    M.set_popularity(popularity(U))
    X = ocffm.ImpData.read(te, True, M.Ds[:fi["fu"]])
    items, scores = M.recommend(X, topn=7)
    _assert_rec_file(b, items, scores, 7)
    got = [x for x in r.stdout.split("\n") if x.startswith("eval")]
    assert got == _eval_table(M.evaluate(X))
    # train's own files: the same rows and table shape (its b differs in the last bits)
    assert len(open(a).read().split("\n")) == len(open(b).read().split("\n")) == 101
    assert [x.split()[:2] for x in train_eval] == [x.split()[:2] for x in got]
    # the other serving options: unseen, cuts, seen, candidate lists
    cptr, ccol = lists_for(100, 50, 6)
    cand = str(tmp_path / "cand")
    with open(cand, "w") as fh:
        for i in range(100):
            fh.write(" ".join(str(int(j)) for j in ccol[int(cptr[i]):int(cptr[i + 1])]) + "\n")
    r = subprocess.run([PREDICT, "--binary", "--popularity", tr, "--recommend", te, "--topn", "5", "--rec-unseen",
                        "--rec-candidates", cand, "--rec-out", b, "--eval", te, "--eval-cuts", "1,5", "--eval-seen", te,
                        "--eval-candidates", cand, mbin, it], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    items, scores = M.recommend(X, topn=5, exclude_labels=True, candidates=(cptr, ccol))
    _assert_rec_file(b, items, scores, 5)
    got = [x for x in r.stdout.split("\n") if x.startswith("eval")]
    assert got == _eval_table(M.evaluate(X, cuts=(1, 5), seen=X, candidates=(cptr, ccol)))
    # the text model: six digits per value, the right shape
    r = subprocess.run([PREDICT, "--fp32", "--recommend", te, "--topn", "7", "--rec-out", b, mtxt, it],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = open(b).read().split("\n")
    assert len(lines) == 101 and all(len(x.split()) == 7 for x in lines[:-1])
    M.close()
    # a malformed model file fails before any output is written
    os.remove(b)
    r = subprocess.run([PREDICT, "--binary", "--recommend", te, "--rec-out", b, mtxt, it], capture_output=True, text=True)
    assert r.returncode == 2 and "error:" in r.stderr and not os.path.exists(b)


def test_cli_usage_errors(tmp_path):
    """Fails before anything is read: no device work, no files needed."""
    missing = str(tmp_path / "nothing")
    out = str(tmp_path / "out.txt")
    r = subprocess.run([PREDICT], capture_output=True, text=True)
    assert r.returncode == 1 and "usage: predict" in r.stderr and "--popularity" in r.stderr
    for args in (["--recommend", missing, missing, missing],
                 ["--recommend", missing, "--rec-out", out, "--topn", "0", missing, missing],
                 ["--recommend", missing, "--rec-out", out, "--topn", "129", missing, missing],
                 ["--topn", "abc", missing, missing],
                 ["--eval-seen", missing, missing, missing],
                 ["--eval", missing, "--eval-cuts", "5,5", missing, missing],
                 ["--recommend", missing, "--rec-out", out, missing],
                 ["--recommend", missing, "--rec-out", out, missing, missing, "extra"],
                 ["--popularity"]):
        r = subprocess.run([PREDICT] + args, capture_output=True, text=True)
        assert r.returncode == 1 and r.stderr.strip(), (args, r.returncode, r.stderr)
        assert not os.path.exists(out)
    r = subprocess.run([PREDICT, "--recommend", missing, "--rec-out", out, missing, missing], capture_output=True, text=True)
    assert r.returncode == 2 and "error:" in r.stderr and not os.path.exists(out)  # unreadable model: OCFFM_E_IO
    assert "--binary-out" in subprocess.run([TRAIN], capture_output=True, text=True).stderr
