"""Top-N recommendation and ranking evaluation of SGD-trained models
(include/ocffm.h ocffm_sgd_recommend / _label_ranks / _evaluate / _counter).

The reference is numpy in fp64 from the W read back, decomposition-free: phi's
double loop over the node pairs of (user row, item row), divided by sum x^2
when the trainer normalises (vectorised over the rows x items pairs, the pair
loop itself is the one of tests/test_sgd.py::test_phi_matches_numpy).

Score tolerance (derived, not tuned): with T(i, j) the same pair sum over the
absolute values of every product (elementwise inside the dot products, times
rn), a score may differ from the reference by at most
    2 (C KP + |U_i| + |V_j| + 8) 2^-24 T(i, j):
the bound of an fp32 sum of that many terms, times 2.

Shapes: 37 or 38 rows and 70 items (no multiples of the 32-row / 64-item
tiles), 1,500 items at k = 8 with the slices forced to 1 and to 5, k of 3, 16,
64 and 100 (KP 4, 16, 64, 128), (fu, fv) of (1, 1), (2, 2) and (3, 1) (depths
C KP below 16 and no multiples of 64), both norm settings, real values, two
nodes in one field on either side, one feature twice in a row, a user row and
an item row without nodes, a query row wider than any train row, a label
>= n.
"""
import numpy as np
import pytest

import ocffm
import synth

pytestmark = pytest.mark.gpu

NONE = ocffm.REC_NONE
PRM = {"eta": 0.2, "lambda": 2e-5, "nneg": 1, "neg_power": 0.75, "adagrad": 1, "seed": 5}
D = 11  # features per field


# ------------------------------------------------------------------ data
def make_rows(rng, m, nf, n_labels, empty_row, integer=False):
    """m rows over nf fields of D features: one node per field with a real
    value, except row 0 (two nodes in field 0), row 1 (one feature twice) and
    empty_row (no node).  n_labels > 0: 1..4 labels below it per row."""
    feats, labels = [], []
    for i in range(m):
        row = [(f, int(rng.integers(0, D)), 1.0 if integer else float(rng.uniform(0.25, 2.0))) for f in range(nf)]
        if i == 0:
            row.insert(1, (0, (row[0][1] + 1) % D, 1.0 if integer else 0.75))
        if i == 1:
            row.append(row[-1])
        if i == empty_row:
            row = []
        feats.append(row)
        labels.append(rng.choice(n_labels, size=int(rng.integers(1, 5)), replace=False) if n_labels else None)
    return synth._build_rows(feats, labels if n_labels else None)


class Case:
    """A trainer on hand-built rows, its query file X (the train rows; extra:
    one label >= n on row 3, a duplicate label on row 4, and a last row of 9
    nodes, wider than any train row) and the node lists for the reference."""

    def __init__(self, k, fu, fv, norm, m=37, n=70, extra=False, integer=False, seed=3, epochs=1):
        rng = np.random.default_rng(seed)
        self.k, self.fu, self.fv, self.norm, self.n = k, fu, fv, norm, n
        self.train = make_rows(rng, m, fu, n, empty_row=2, integer=integer)
        self.item = make_rows(rng, n, fv, 0, empty_row=5, integer=integer)
        # every field's last feature appears, so Ds = D for all fields
        for rows, nf in ((self.train, fu), (self.item, fv)):
            for f in range(nf):
                sel = np.flatnonzero(rows.fid == f)
                rows.idx[sel[-1]] = D - 1
        self.U = ocffm.ImpData.from_rows(self.train)
        self.V = ocffm.ImpData.from_rows(self.item)
        self.t = ocffm.SgdTrainer(self.U, self.V, k=k, norm=norm, **PRM)
        for _ in range(epochs):
            self.t.epoch()
        xr = self.train
        if extra:
            feats = [[(int(xr.fid[p]), int(xr.idx[p]), float(xr.val[p])) for p in range(int(xr.xptr[i]), int(xr.xptr[i + 1]))]
                     for i in range(m)]
            labels = [xr.ycol[int(xr.yptr[i]):int(xr.yptr[i + 1])].astype(np.int64) for i in range(m)]
            labels[3] = np.r_[labels[3], n + 7]
            labels[4] = np.r_[labels[4], labels[4][0]]
            feats.append([(f % fu, int(rng.integers(0, D)), float(rng.uniform(0.25, 2.0))) for f in range(9)])
            labels.append(np.array([1, 2]))
            xr = synth._build_rows(feats, labels)
        self.xrows = xr
        self.X = ocffm.ImpData.from_rows(xr)
        off = np.arange(fu + fv + 1) * D
        self.un = padded(xr, 0, off)
        self.vn = padded(self.item, fu, off)
        self.labels = [xr.ycol[int(xr.yptr[i]):int(xr.yptr[i + 1])].astype(np.int64) for i in range(xr.m)]

    def W(self):
        i = self.t.info
        return self.t.get("W").astype(np.float64).reshape(-1, i["n_fields"], i["kp"])

    def ref(self):
        """(scores, tolerances), rows x n, from the current W."""
        i = self.t.info
        S, T = ref_scores(self.W(), self.un, self.vn, self.norm)
        terms = self.fu * self.fv * i["kp"] + self.un[3][:, None] + self.vn[3][None, :] + 8
        return S, 2.0 * terms * 2.0 ** -24 * T


def padded(rows, fbase, off):
    """Node lists (field-major within a row, file order within a field) padded
    to the widest row with x = 0: j, f, x [m, w] and the rows' widths.  x is
    rounded to fp32, as the trainer holds it."""
    m = rows.m
    lists = []
    for i in range(m):
        b, e = int(rows.xptr[i]), int(rows.xptr[i + 1])
        order = sorted(range(b, e), key=lambda t: int(rows.fid[t]))  # (stable)
        lists.append([(int(off[fbase + rows.fid[t]] + rows.idx[t]), fbase + int(rows.fid[t]),
                       float(np.float32(rows.val[t]))) for t in order])
    w = max(1, max(len(l) for l in lists))
    j = np.zeros((m, w), np.int64)
    f = np.full((m, w), fbase, np.int64)
    x = np.zeros((m, w))
    for i, l in enumerate(lists):
        for a, (jj, ff, xx) in enumerate(l):
            j[i, a], f[i, a], x[i, a] = jj, ff, xx
    return j, f, x, np.array([len(l) for l in lists])


def ref_scores(W, un, vn, norm):
    """phi of every (row, item): the double loop over the node pairs of the
    instance (user nodes, then item nodes), each pair for all instances at
    once; and the same sum over absolute values."""
    ju, fu, xu, _ = un
    jv, fv, xv, _ = vn
    m, n = ju.shape[0], jv.shape[0]
    S = np.zeros((m, n))
    T = np.zeros((m, n))
    # instance node a: (j, f, x) broadcast to [m, n]
    inst = [(ju[:, a][:, None], fu[:, a][:, None], xu[:, a][:, None]) for a in range(ju.shape[1])] + \
           [(jv[:, b][None, :], fv[:, b][None, :], xv[:, b][None, :]) for b in range(jv.shape[1])]
    for a in range(len(inst)):
        for b in range(a + 1, len(inst)):
            (ja, fa, xa), (jb, fb, xb) = inst[a], inst[b]
            prod = W[ja, fb] * W[jb, fa]  # [.., .., kp]
            xx = xa * xb
            S += prod.sum(-1) * xx
            T += np.abs(prod).sum(-1) * np.abs(xx)
    if norm:
        s2 = (xu * xu).sum(1)[:, None] + (xv * xv).sum(1)[None, :]
        rn = np.where(s2 > 0, 1.0 / np.where(s2 > 0, s2, 1.0), 1.0)
        S, T = S * rn, T * rn
    return S, T


def check_topn(items, scores, ref, tol, excluded):
    """tests/test_recommend.py assert_topn with a per-pair tolerance."""
    m, n = ref.shape
    topn = items.shape[1]
    assert scores.shape == items.shape and m == items.shape[0]
    for i in range(m):
        cand = [j for j in range(n) if j not in excluded[i]]
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
        err = np.abs(sc - ref[i, it])
        assert (err <= tol[i, it]).all(), (i, float((err - tol[i, it]).max()), float(err.max()))
        rest = sorted(set(cand) - set(it.tolist()))
        if rest and nf:
            over = ref[i, rest] - 2 * tol[i, rest]
            assert over.max() <= sc[-1], (i, float(over.max()), float(sc[-1]))


def ranks_from_all(items, scores, labels, n, excluded=None):
    """Label ranks and scores from recommend(topn = n)'s returned bits under
    (score descending, item ascending)."""
    rk, sc = [], []
    for i, labs in enumerate(labels):
        pos = {int(j): p for p, j in enumerate(items[i]) if j != NONE}
        for j in labs:
            if int(j) in pos:
                rk.append(pos[int(j)])
                sc.append(scores[i, pos[int(j)]])
            else:
                rk.append(ocffm.RANK_NONE)
                sc.append(-np.inf)
    return np.array(rk, np.uint32), np.array(sc)


_CASES = {}


def case(*key, **kw):
    full = key + tuple(sorted(kw.items()))
    if full not in _CASES:
        _CASES[full] = Case(*key, **kw)
    return _CASES[full]


# ----------------------------------------------------------------- tests
def test_all_scores_against_reference_and_phi():
    """n = 70, topn = 70, X = the train rows: every score of every row."""
    c = case(16, 2, 2, 1)
    ref, tol = c.ref()
    items, scores = c.t.recommend(c.X, topn=70)
    assert items.shape == (37, 70) and items.dtype == np.uint32 and scores.dtype == np.float64
    assert (np.sort(items, axis=1) == np.arange(70)).all()
    got = np.empty_like(ref)
    np.put_along_axis(got, items.astype(np.int64), scores, axis=1)
    err = np.abs(got - ref)
    print("all scores: worst err / tol", float((err / np.maximum(tol, 1e-300)).max()), "max tol", float(tol.max()))
    assert (err <= tol).all(), float((err - tol).max())
    uu, jj = np.divmod(np.arange(37 * 70), 70)
    phi = c.t.phi(uu.astype(np.uint32), jj.astype(np.uint32)).astype(np.float64).reshape(37, 70)
    bound = tol + 1e-5 * np.maximum(1.0, np.abs(phi))
    assert (np.abs(got - phi) <= bound).all(), float((np.abs(got - phi) - bound).max())
    check_topn(items, scores, ref, tol, [set()] * 37)


@pytest.mark.parametrize("k,fu,fv,norm", [(3, 1, 1, 0), (3, 3, 1, 1), (16, 2, 2, 0), (16, 3, 1, 1), (64, 2, 2, 1),
                                          (100, 1, 1, 1), (100, 1, 1, 0)])
def test_ragged_parity(k, fu, fv, norm):
    """After one HOGWILD epoch: top-10 and label ranks against the reference,
    and label_ranks against recommend(topn = n) without a tolerance."""
    c = case(k, fu, fv, norm, extra=True)
    ref, tol = c.ref()
    m = c.xrows.m
    assert m == 38
    items, scores = c.t.recommend(c.X, topn=10)
    check_topn(items, scores, ref, tol, [set()] * m)
    allj, alls = c.t.recommend(c.X, topn=70)
    check_topn(allj, alls, ref, tol, [set()] * m)
    assert (allj[:, :10] == items).all() and (alls[:, :10] == scores).all()
    ranks, lsc, ncand = c.t.label_ranks(c.X)
    erk, esc = ranks_from_all(allj, alls, c.labels, c.n)
    assert (ncand == c.n).all()
    np.testing.assert_array_equal(ranks, erk)
    np.testing.assert_array_equal(lsc, esc)
    # the label >= n of row 3 is ignored; the duplicate of row 4 shares its rank
    yptr = c.xrows.yptr.astype(np.int64)
    assert ranks[yptr[4] - 1] == ocffm.RANK_NONE and lsc[yptr[4] - 1] == -np.inf
    assert ranks[yptr[5] - 1] == ranks[yptr[4]] and lsc[yptr[5] - 1] == lsc[yptr[4]]
    # the rows without nodes: B_j rn / A_i rn, which the reference states as well
    assert np.isfinite(alls).all()


def integer_w(c, seed):
    i = c.t.info
    rng = np.random.default_rng(seed)
    w = np.zeros((i["n_features"], i["n_fields"], i["kp"]), np.float32)
    w[:, :, :c.k] = rng.integers(-2, 3, (i["n_features"], i["n_fields"], c.k))
    c.t.set_w(w.reshape(-1))


@pytest.mark.parametrize("norm", [0, 1])
def test_exact_order_under_ties(norm):
    """Small integer W and unit values: every sum is exact, ties are many.
    norm = 1: rows of exactly 2 user and 2 item nodes, rn = 0.25 exactly."""
    if norm == 0:
        c = Case(3, 2, 2, 0, integer=True, epochs=0, seed=11)
        rows = list(range(37))
        cols = np.arange(70)
    else:
        c = Case(3, 2, 2, 1, integer=True, epochs=0, seed=12)
        rows = [i for i in range(37) if c.un[3][i] == 2]
        cols = np.flatnonzero(c.vn[3] == 2)
        assert len(rows) > 20 and cols.size > 40
    integer_w(c, 21)
    ref, _ = c.ref()
    items, scores = c.t.recommend(c.X, topn=70)
    assert len(np.unique(ref)) < ref.size / 4  # (ties)
    for i in rows:
        keep = np.isin(items[i], cols)
        it, sc = items[i][keep].astype(np.int64), scores[i][keep]
        order = cols[np.lexsort((cols, -ref[i, cols]))]
        np.testing.assert_array_equal(it, order)
        np.testing.assert_array_equal(sc, ref[i, order])
    if norm == 0:  # a short list under ties as well
        it5, sc5 = c.t.recommend(c.X, topn=5)
        assert (it5 == items[:, :5]).all() and (sc5 == scores[:, :5]).all()


def test_exclusion():
    c = case(16, 2, 2, 1, extra=True)
    ref, tol = c.ref()
    m = c.xrows.m
    excl = [set(int(j) for j in l if j < c.n) for l in c.labels]
    items, scores = c.t.recommend(c.X, topn=70, exclude_labels=True)
    check_topn(items, scores, ref, tol, excl)
    allj, alls = c.t.recommend(c.X, topn=70)
    for i in range(m):  # the others keep their bits
        keep = ~np.isin(allj[i], list(excl[i]))
        nf = int(keep.sum())
        assert (items[i, :nf] == allj[i][keep]).all() and (scores[i, :nf] == alls[i][keep]).all()
    # seen: X's own labels are all seen; a second file's labels are ranked among the rest
    rng = np.random.default_rng(8)
    labs2 = [rng.choice(c.n, size=3, replace=False) for _ in range(m)]
    xr = c.xrows
    Y = synth.Rows(xr.xptr, xr.fid, xr.idx, xr.val, np.arange(m + 1, dtype=np.uint64) * 3,
                   np.concatenate(labs2).astype(np.uint64))
    Yd = ocffm.ImpData.from_rows(Y)
    ranks, lsc, ncand = c.t.label_ranks(Yd, seen=c.X)
    assert (ncand == np.array([c.n - len(e) for e in excl])).all()
    erk, esc = ranks_from_all(items, scores, labs2, c.n)
    np.testing.assert_array_equal(ranks, erk)
    np.testing.assert_array_equal(lsc, esc)
    assert (ranks == ocffm.RANK_NONE).sum() == sum(int(j) in excl[i] for i in range(m) for j in labs2[i])


def test_label_ranks_and_evaluate():
    """n = 70: see test_ragged_parity (no tolerance).  n = 1500: each rank
    lies between the reference counts at score -/+ tolerance; evaluate equals
    eval_from_ranks of label_ranks."""
    c = case(8, 2, 2, 1, n=1500, extra=True)
    ref, tol = c.ref()
    ranks, lsc, ncand = c.t.label_ranks(c.X)
    p = 0
    for i, labs in enumerate(c.labels):
        for j in labs:
            if j >= c.n:
                assert ranks[p] == ocffm.RANK_NONE
            else:
                assert abs(lsc[p] - ref[i, j]) <= tol[i, j]
                others = np.arange(c.n) != j
                lo = int(((ref[i] - tol[i] > ref[i, j] + tol[i, j]) & others).sum())
                hi = int(((ref[i] + tol[i] >= ref[i, j] - tol[i, j]) & others).sum())
                assert lo <= ranks[p] <= hi, (i, j, lo, int(ranks[p]), hi)
            p += 1
    assert p == ranks.size
    for cur in (c, case(16, 2, 2, 1, extra=True)):
        r, s, nc = cur.t.label_ranks(cur.X)
        ev = cur.t.evaluate(cur.X, cuts=(1, 5, 20))
        want = ocffm.eval_from_ranks(cur.xrows.yptr, r, nc, scores=s, cuts=(1, 5, 20))
        assert ev.keys() == want.keys()
        for key in ev:
            np.testing.assert_array_equal(np.asarray(ev[key]), np.asarray(want[key]), err_msg=key)


def test_determinism(monkeypatch):
    """Chunking, slicing, a sub-range and a second call give identical bits.
    (The knobs are read at create: the second trainer takes the first one's W
    through set_w.)"""
    def run(c):
        return c.t.recommend(c.X, topn=20) + c.t.label_ranks(c.X)

    for key, kw in (((16, 2, 2, 1), dict(extra=True)), ((8, 2, 2, 1), dict(n=1500, extra=True))):
        monkeypatch.delenv("OCFFM_REC_ROWS", raising=False)
        monkeypatch.delenv("OCFFM_REC_SLICES", raising=False)
        c = case(*key, **kw)
        base = run(c)
        for a, b in zip(base, run(c)):
            np.testing.assert_array_equal(a, b)
        it2, sc2 = c.t.recommend(c.X, topn=20, row0=5, rows=30)
        np.testing.assert_array_equal(it2, base[0][5:35])
        np.testing.assert_array_equal(sc2, base[1][5:35])
        w = c.t.get("W")
        for slices in ("1", "5"):
            monkeypatch.setenv("OCFFM_REC_ROWS", "32")
            monkeypatch.setenv("OCFFM_REC_SLICES", slices)
            d = Case(*key, epochs=0, **kw)
            d.t.set_w(w)
            for a, b in zip(base, run(d)):
                np.testing.assert_array_equal(a, b)


def test_model_changes_rebuild_the_item_side():
    c = Case(16, 2, 2, 1, extra=True)
    assert c.t.counter("rank_item_builds") == 0 and c.t.counter("no_such_counter") == 0
    c.t.recommend(c.X, topn=5)
    c.t.label_ranks(c.X)
    assert c.t.counter("rank_item_builds") == 1
    assert c.t.counter("rank_kernel_us") > 0 and c.t.counter("rank_setup_us") > 0
    c.t.epoch()
    items, scores = c.t.recommend(c.X, topn=10)
    c.t.evaluate(c.X)
    assert c.t.counter("rank_item_builds") == 2
    ref, tol = c.ref()
    check_topn(items, scores, ref, tol, [set()] * c.xrows.m)
    integer_w(c, 4)
    items, scores = c.t.recommend(c.X, topn=10)
    assert c.t.counter("rank_item_builds") == 3
    ref, tol = c.ref()
    check_topn(items, scores, ref, tol, [set()] * c.xrows.m)
    c.t.recommend(c.X, topn=10)
    assert c.t.counter("rank_item_builds") == 3


def test_errors():
    c = case(16, 2, 2, 1, extra=True)
    t, X = c.t, c.X

    def code(fn):
        with pytest.raises(ocffm.OcffmError) as e:
            fn()
        return e.value.code

    L = ocffm.lib()
    m = c.xrows.m
    items = np.zeros((m, 4), np.uint32)
    ranks = np.zeros(int(c.xrows.yptr[-1]), np.uint32)
    vp = lambda a: a.ctypes.data_as(ocffm.C.c_void_p)  # noqa: E731
    assert L.ocffm_sgd_recommend(t.h, X.h, 0, m, 0, 0, vp(items), None) == ocffm.E_ARG           # topn == 0
    assert L.ocffm_sgd_recommend(t.h, X.h, 0, m, 129, 0, vp(items), None) == ocffm.E_ARG         # topn > MAX
    assert L.ocffm_sgd_recommend(t.h, X.h, 1, m, 4, 0, vp(items), None) == ocffm.E_ARG           # range
    assert L.ocffm_sgd_recommend(t.h, X.h, 0, m, 4, 0, None, None) == ocffm.E_ARG                # NULL items
    assert L.ocffm_sgd_recommend(t.h, None, 0, m, 4, 0, vp(items), None) == ocffm.E_ARG          # NULL X
    assert L.ocffm_sgd_recommend(t.h, X.h, 0, 0, 4, 0, vp(items), None) == ocffm.OK              # rows == 0
    assert L.ocffm_sgd_recommend(t.h, X.h, 0, m, 4, 0, vp(items), None) == ocffm.OK              # NULL scores
    assert L.ocffm_sgd_label_ranks(t.h, X.h, None, None, None, None) == ocffm.E_ARG              # NULL ranks
    assert L.ocffm_sgd_label_ranks(t.h, X.h, None, vp(ranks), None, None) == ocffm.OK
    assert code(lambda: t.label_ranks(c.V)) == ocffm.E_ARG                                       # no labels
    short = ocffm.ImpData.from_rows(make_rows(np.random.default_rng(1), 5, 2, 70, empty_row=-1))
    assert code(lambda: t.label_ranks(X, seen=short)) == ocffm.E_ARG                             # seen.m != X.m
    assert code(lambda: t.evaluate(X, cuts=())) == ocffm.E_ARG
    assert code(lambda: t.evaluate(X, cuts=(5, 5))) == ocffm.E_ARG
    assert L.ocffm_sgd_evaluate(t.h, X.h, None, None, 1, None) == ocffm.E_ARG
    cnt = ocffm.C.c_int64(0)
    assert L.ocffm_sgd_counter(t.h, None, ocffm.C.byref(cnt)) == ocffm.E_ARG
    # data errors: a field past the user side, an index past the train Ds
    for bad in ((2, 0, 1.0), (0, D, 1.0)):
        rows = synth._build_rows([[(0, 1, 1.0)], [bad]], [np.array([1]), np.array([2])])
        Xb = ocffm.ImpData.from_rows(rows)
        assert code(lambda: t.recommend(Xb, topn=3)) == ocffm.E_DATA
        assert code(lambda: t.label_ranks(Xb)) == ocffm.E_DATA
        assert code(lambda: t.evaluate(Xb)) == ocffm.E_DATA
        assert t.recommend(Xb, topn=3, rows=1)[0].shape == (1, 3)  # (the rows of the call are checked)
    # an empty file
    empty = ocffm.ImpData.from_rows(synth._build_rows([], []))
    assert t.recommend(empty, topn=3)[0].shape == (0, 3)
    assert t.label_ranks(empty)[0].size == 0
    # no cross block: a trainer without item fields
    V0 = ocffm.ImpData.from_rows(synth._build_rows([[] for _ in range(70)], None))
    t0 = ocffm.SgdTrainer(c.U, V0, k=4, **PRM)
    assert code(lambda: t0.recommend(X, topn=3)) == ocffm.E_ARG
    assert code(lambda: t0.label_ranks(X)) == ocffm.E_ARG
    assert code(lambda: t0.evaluate(X)) == ocffm.E_ARG
