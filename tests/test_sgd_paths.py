"""k_sgd (one-class-ffm_amd/csrc/sgd.hip) on wide multi-hot rows, in the
multi-wave launch, in the permuted instance order and at a saturated logistic;
the SGD trainer's constructor refusals.

References: oracle/sgd_oracle.cpp (serial CPU statement, fp32 storage) at the
project's tolerances (max|dW| <= 2e-4 max|W|, loss 1e-4 relative, G rtol 1e-3
atol 1e-6), and for the saturated case an fp64 numpy restatement of the epoch
(`epoch64` below: the oracle's header formulas, instance by instance, with the
stable softplus), which the CPU test pins against the oracle.  Before the first
epoch every trainer gets a centred copy of its initial W (half the init range
off the k real columns), so that phi and kappa take both signs.

No feature appears twice within one row of any input here.  Two slots of one
instance would then store to the same row of W, and the kernel does not define
which store lands last; that is not tested.

Shapes.  Serial mode against the oracle, synth.multi_hot rows (24 or 40 users,
20 items, real values in [0.25, 2], one user row with one node, one without
nodes that has positives, one item row without nodes; k / fields fu + fv /
widest instance / slots):
  k 4   1 + 1   40 + 24 = 64 nodes   128 slots (2 per subgroup), 2016 pairs,
                                     same-field slots, 40 nodes in one field
  k 4   5 + 3   40 + 24 = 64         512 (8 per subgroup: every register full),
                                     also with OCFFM_SGD_OCC=0
  k 3   61 + 3  5 + 3 = 8            512, field index 63, sparse fields
  k 100 1 + 1   5 + 3 = 8            16 (8 per subgroup of 32 lanes)
  k 100 2 + 2   2 + 2 = 4            16, one node per field
  k 32  2 + 2   10 + 6 = 16          64 (8 per subgroup)
  k 16  2 + 1   9 + 4 = 13           39 (4 per subgroup, last round part filled)
with adagrad and norm spread over them, nneg 1 or 2; the padding columns of
k = 3 and k = 100 stay W = 0, G = 1.
Multi-wave launch: synth.conflict_free(777, rich) (F = 4, six nodes, nneg = 0),
k 5 and 32: one wave, the default 780 waves, 20 waves and 4 waves give
bit-identical W and G, and the one-wave run matches the oracle; also with the
users' two-node field first (ends=True), where the first and the last slot of
every instance, the rims of a wave's LDS region, are both in use.
Permuted order: conflict_free(1,050,000, plain), k 4, default launch, A != 1.
Saturated logistic: conflict_free(40, rich) with one negative per positive and
|phi| of about 100.
Draws in the multi-block launch: synth.tiny(seed 3, 300 x 40), eta = 0.
Refusals: k 0 and 129, 65 fields, 65 nodes, 17 slots at k 100, a label >= n.
"""
import functools

import numpy as np
import pytest

import ocffm
import synth
from test_sgd import OracleSgd, P, sgo  # noqa: F401

BASE = {"eta": 0.2, "lambda": 2e-5, "nneg": 1, "neg_power": 0.75, "adagrad": 1, "norm": 1, "seed": 5}
M64 = (1 << 64) - 1


# ------------------------------------------------------------- fp64 reference
def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def instance(o, prm, epoch, T, qq):
    """(user row, item row, label) of instance qq (the oracle header's draw)."""
    p, r = divmod(qq, 1 + prm["nneg"])
    u = int(o.pu[p])
    if r == 0:
        return u, int(o.pv[p]), 1.0
    h = mix64((prm["seed"] + 0x9E3779B97F4A7C15 * (epoch * T + qq)) & M64)
    idx = (h >> 32) % o.n_items
    coin = (h & 0xFFFFFF) / 16777216.0
    return u, (idx if coin < float(o.prob[idx]) else int(o.alias[idx])), -1.0


def row_nodes(o, u, it):
    (up, un, uf, ux), (vp, vn, vf, vx) = o.u, o.v
    a, b, c, d = int(up[u]), int(up[u + 1]), int(vp[it]), int(vp[it + 1])
    return (np.r_[un[a:b], vn[c:d]].astype(np.int64), np.r_[uf[a:b], vf[c:d]].astype(np.int64),
            np.r_[ux[a:b], vx[c:d]].astype(np.float64))


def phi64(W3, j, f, x, norm):
    """phi in fp64 from W3 [features, fields, kp]."""
    if j.size < 2:
        return 0.0
    Wab = W3[j[:, None], f[None, :]]  # [a, b] = W[j_a][f_b]
    phi = np.triu(np.einsum("abk,bak->ab", Wab, Wab) * np.outer(x, x), 1).sum()
    s = (x * x).sum()
    return phi / s if norm and s > 0 else phi


def epoch64(o, W3, G3, prm, epoch, A, B):
    """One serial epoch in fp64 with the saturating logistic; W3, G3 in place.
    Returns (summed loss, [(label, phi)] in instance order)."""
    T = o.pu.size * (1 + prm["nneg"])
    F = W3.shape[1]
    loss, seen = 0.0, []
    for q in range(T):
        qq = (A * q + B) % T
        u, it, y = instance(o, prm, epoch, T, qq)
        j, f, x = row_nodes(o, u, it)
        s = (x * x).sum()
        rn = 1.0 / s if prm["norm"] and s > 0 else 1.0
        phi = phi64(W3, j, f, x, prm["norm"])
        seen.append((y, phi))
        z = -y * phi
        e = np.exp(-abs(z))
        kappa = -y * (1.0 / (1.0 + e) if z > 0 else e / (1.0 + e))
        loss += max(z, 0.0) + np.log1p(e)
        steps = []
        for a in range(j.size):
            for fl in range(F):
                b = np.flatnonzero((f == fl) & (np.arange(j.size) != a))
                if b.size == 0:
                    continue
                acc = (x[b, None] * W3[j[b], f[a]]).sum(axis=0)
                w = W3[j[a], fl]
                g = prm["lambda"] * w + kappa * rn * x[a] * acc
                if prm["adagrad"]:
                    gv = G3[j[a], fl] + g * g
                    steps.append((j[a], fl, w - prm["eta"] * g / np.sqrt(gv), gv))
                else:
                    steps.append((j[a], fl, w - prm["eta"] * g, G3[j[a], fl].copy()))
        for (ja, fl, w, gv) in steps:
            W3[ja, fl], G3[ja, fl] = w, gv
    return loss, seen


def max_abs_phi(o, W, F, kp, norm):
    """max |phi| over every (user with a positive, item) pair: a superset of
    the instances an epoch can draw."""
    W3 = W.astype(np.float64).reshape(-1, F, kp)
    return max(abs(phi64(W3, *row_nodes(o, u, it), norm)) for u in np.unique(o.pu) for it in range(o.n_items))


# ------------------------------------------------------------------- helpers
def make(ds, **kw):
    U = ocffm.ImpData.from_rows(ds.train)
    V = ocffm.ImpData.from_rows(ds.item)
    return ocffm.SgdTrainer(U, V, **kw)


def centre(t, k, scale=1.0):
    """set_w a centred (and scaled) copy of the initial W; padding stays 0."""
    kp = t.info["kp"]
    W = t.get("W").copy().reshape(-1, kp)
    W[:, :k] -= np.float32(0.5) / np.sqrt(np.float32(k))
    W *= np.float32(scale)
    W = W.reshape(-1)
    t.set_w(W)
    return W


def check_epoch(tag, lg, lo, Wg, W, Gg, G, adagrad):
    """The project's tolerances (tests/test_sgd.py), figures printed first."""
    scale = np.abs(W).max()
    dw = np.abs(Wg - W).max() / scale
    dl = abs(lg - lo) / abs(lo)
    dg = (np.abs(Gg - G) / np.maximum(np.abs(G), 1e-30)).max()
    print(f"DEV {tag}: max|dW|/max|W| {dw:.2e}  loss rel {dl:.2e}  G rel {dg:.2e}  (loss {lg:.6f})")
    assert np.isfinite(lg) and np.isfinite(Wg).all() and np.isfinite(Gg).all(), tag
    assert dw <= 2e-4, (tag, dw)
    assert dl <= 1e-4, (tag, lg, lo)
    if adagrad:
        np.testing.assert_allclose(Gg, G, rtol=1e-3, atol=1e-6)
    else:
        np.testing.assert_array_equal(Gg, G)  # plain SGD leaves the AdaGrad sums alone


def run_against_oracle(tag, t, o, W, prm, epochs=2, before=None):
    """`epochs` epochs on the GPU and in the oracle, both continued from the GPU
    state after each one (no drift accumulation)."""
    G = t.get("G").copy()
    assert np.all(G == 1.0)
    for e in range(epochs):
        if before:
            before(W)
        lg = t.epoch()
        A, B, T = (int(x) for x in t.get("o"))
        assert T == t.info["instances"] == o.pu.size * (1 + prm["nneg"])
        lo = o.epoch(W, G, e, A, B) / T
        Wg, Gg = t.get("W").copy(), t.get("G").copy()
        check_epoch(f"{tag} epoch {e}", lg, lo, Wg, W, Gg, G, prm["adagrad"])
        W, G = Wg, Gg.copy()
    return W, G


# ------------------------------------------------ 1. serial mode, wide rows
# id: k, fu, fv, nu, nv, users, adagrad, norm, nneg, eta, scale of the centred W, OCFFM_SGD_OCC
WIDE = {
    "full_wave": (4, 1, 1, 40, 24, 24, 1, 0, 1, 0.02, 0.5, None),
    "slot_cap_k4": (4, 5, 3, 40, 24, 24, 0, 1, 2, 0.2, 1.0, None),
    "slot_cap_k4_occ0": (4, 5, 3, 40, 24, 24, 0, 1, 2, 0.2, 1.0, "0"),
    "fields64": (3, 61, 3, 5, 3, 40, 1, 1, 1, 0.2, 1.0, None),
    "slot_cap_k100": (100, 1, 1, 5, 3, 24, 0, 0, 2, 0.05, 1.0, None),
    "one_hot_k100": (100, 2, 2, 2, 2, 24, 1, 1, 1, 0.2, 1.0, None),
    "mid_k32": (32, 2, 2, 10, 6, 24, 1, 0, 1, 0.05, 1.0, None),
    "mid_k16": (16, 2, 1, 9, 4, 24, 0, 1, 1, 0.2, 1.0, None),
}


@functools.lru_cache(maxsize=None)
def wide_ds(fu, fv, nu, nv, m):
    return synth.multi_hot(17, fu, fv, nu, nv, m=m)


def test_wide_cases_spread_the_settings():
    """Each adagrad and norm value meets a multi-hot case and a case at 8 slots
    per subgroup (slots of the widest instance over the subgroups of a wave)."""
    for col in (6, 7):
        for val in (0, 1):
            rows = [c for c in WIDE.values() if c[col] == val]
            assert any(c[3] > c[1] or c[4] > c[2] for c in rows), (col, val)
            kp = [max(4, 1 << (c[0] - 1).bit_length()) for c in rows]
            assert any((c[3] + c[4]) * (c[1] + c[2]) > 4 * (64 // (p // 4)) for c, p in zip(rows, kp)), (col, val)


def test_epoch64_matches_oracle():
    """The fp64 restatement used for the saturated case agrees with the oracle
    where the logistic is not saturated (no GPU): multi-hot rows, both steps."""
    ds = wide_ds(2, 2, 10, 6, 24)
    for adagrad, norm in ((1, 0), (0, 1)):
        prm = dict(BASE, adagrad=adagrad, norm=norm, eta=0.05)
        F, kp, k = 4, 8, 5
        o = OracleSgd(ds, F, kp, prm)
        rng = np.random.default_rng(1)
        nf = int(max(o.u[1].max(), o.v[1].max())) + 1
        W = np.zeros((nf * F, kp), np.float32)
        W[:, :k] = rng.uniform(-0.2, 0.2, (nf * F, k))
        W = W.reshape(-1)
        G = np.ones_like(W)
        W3, G3 = W.astype(np.float64).reshape(nf, F, kp), G.astype(np.float64).reshape(nf, F, kp)
        T = o.pu.size * 2
        l64, seen = epoch64(o, W3, G3, prm, 0, 1, 7 % T)
        lo = o.epoch(W, G, 0, 1, 7 % T)
        assert {y for y, _ in seen} == {1.0, -1.0} and min(p for _, p in seen) < 0 < max(p for _, p in seen)
        assert abs(l64 - lo) <= 1e-5 * lo
        assert np.abs(W3.reshape(-1) - W).max() <= 2e-5 * np.abs(W).max()
        np.testing.assert_allclose(G3.reshape(-1), G, rtol=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(WIDE))
def test_serial_wide_rows_match_oracle(case, monkeypatch):
    k, fu, fv, nu, nv, m, adagrad, norm, nneg, eta, scale, occ = WIDE[case]
    if occ is not None:
        monkeypatch.setenv("OCFFM_SGD_OCC", occ)  # read when the trainer is made
    ds = wide_ds(fu, fv, nu, nv, m)
    prm = dict(BASE, adagrad=adagrad, norm=norm, nneg=nneg, eta=eta)
    t = make(ds, k=k, serial=1, **prm)
    info = t.info
    F, kp = info["n_fields"], info["kp"]
    assert F == fu + fv
    o = OracleSgd(ds, F, kp, prm)
    np.testing.assert_array_equal(t.get("p"), o.prob)
    np.testing.assert_array_equal(t.get("a"), o.alias)
    widths = np.diff(o.u[0])[o.pu] + np.diff(o.v[0])[o.pv]
    assert widths.max() == nu + nv and widths.min() == 0  # the widest instance and the empty one are trained
    W = centre(t, k, scale)
    assert (W < 0).any() and (W > 0).any()

    def before(Wc):  # overflow is the saturated test's subject
        if not norm:
            big = max_abs_phi(o, Wc, F, kp, norm)
            print(f"DEV {case}: max|phi| {big:.2f}")
            assert big < 30, big

    W, G = run_against_oracle(case, t, o, W, prm, before=before)
    if k in (3, 100):  # k_project and the serving sweeps read all KP columns
        assert np.all(W.reshape(-1, kp)[:, k:] == 0)
        assert np.all(G.reshape(-1, kp)[:, k:] == 1)


# -------------------------------------------- 2. multi-wave launch, exactly
@functools.lru_cache(maxsize=None)
def free_ds(m, rich, ends=False):
    return synth.conflict_free(m, rich, ends=ends)


def test_conflict_free_is_order_independent():
    """The argument the multi-wave tests rest on, in the oracle (no GPU): on
    conflict_free rows another instance order gives bit-identical W and G."""
    for ends in (False, True):
        _order_independent(free_ds(777, True, ends))


def _order_independent(ds):
    m = ds.train.m
    prm = dict(BASE, nneg=0)
    F, kp = 4, 8
    o = OracleSgd(ds, F, kp, prm)
    rows = [np.r_[o.u[1][o.u[0][u]:o.u[0][u + 1]], o.v[1][o.v[0][it]:o.v[0][it + 1]]] for u, it in zip(o.pu, o.pv)]
    assert all(r.size == 6 for r in rows) and np.unique(np.concatenate(rows)).size == 6 * m
    rng = np.random.default_rng(2)
    W0 = np.zeros((6 * m * F, kp), np.float32)
    W0[:, :5] = rng.uniform(-0.2, 0.2, (6 * m * F, 5))
    res = []
    for A, B in ((1, 0), (389, 12345 % m)):
        W, G = W0.reshape(-1).copy(), np.ones(W0.size, np.float32)
        loss = [o.epoch(W, G, e, A, B) for e in range(2)]
        res.append((W, G, loss))
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])
    np.testing.assert_allclose(res[0][2], res[1][2], rtol=1e-12)
    assert not np.array_equal(res[0][0], W0.reshape(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("k,adagrad,norm,ends", [(5, 1, 1, False), (32, 1, 0, False), (32, 0, 1, False),
                                                 (5, 0, 0, True), (32, 1, 1, True)])
def test_multi_wave_launches_equal_one_wave(k, adagrad, norm, ends, monkeypatch):
    """780 waves for 777 instances (some idle), 20 waves and 4 waves (many
    grid-stride rounds, T no multiple of the wave count) against one wave:
    W and G bit for bit, the mean loss to 1e-12 (the atomic sum order differs);
    the one-wave run against the oracle.  ends: the rows whose first and last
    slot are both in use, the two rows of a wave's LDS region that a wrong
    region stride shares with the neighbouring waves first."""
    m = 777
    ds = free_ds(m, True, ends)
    prm = dict(BASE, adagrad=adagrad, norm=norm, nneg=0)
    ser = make(ds, k=k, serial=1, **prm)
    W0 = centre(ser, k)
    runs = {}
    for grid in (None, "5", "1"):
        if grid is None:
            monkeypatch.delenv("OCFFM_SGD_GRID", raising=False)
        else:
            monkeypatch.setenv("OCFFM_SGD_GRID", grid)
        runs[grid] = make(ds, k=k, **prm)
        runs[grid].set_w(W0)
    monkeypatch.delenv("OCFFM_SGD_GRID", raising=False)
    info = ser.info
    assert info["instances"] == m
    o = OracleSgd(ds, info["n_fields"], info["kp"], prm)
    W, G = W0.copy(), ser.get("G").copy()
    for e in range(2):
        ls = ser.epoch()
        A, B, T = (int(x) for x in ser.get("o"))
        Ws, Gs = ser.get("W").copy(), ser.get("G").copy()
        assert not np.array_equal(Ws, W)
        for grid, t in runs.items():
            lt = t.epoch()
            np.testing.assert_array_equal(t.get("o"), ser.get("o"))
            np.testing.assert_array_equal(t.get("W"), Ws, err_msg=f"grid {grid} epoch {e}")
            np.testing.assert_array_equal(t.get("G"), Gs, err_msg=f"grid {grid} epoch {e}")
            assert abs(lt - ls) <= 1e-12 * abs(ls), (grid, e, lt, ls)
        lo = o.epoch(W, G, e, A, B) / T
        check_epoch(f"multi-wave k{k} epoch {e}", ls, lo, Ws, W, Gs, G, adagrad)
        W, G = Ws, Gs.copy()


# ------------------------------------------------- 3. permuted order, A != 1
class DirectOracle(OracleSgd):
    """OracleSgd on conflict_free(m, rich=False) with the node arrays written
    down (they are aranges) instead of walked row by row."""

    def __init__(self, ds, prm):
        m = ds.train.m
        ptr = np.arange(m + 1, dtype=np.uint64)
        ids = np.arange(m, dtype=np.uint32)
        self.u = (ptr, ids, np.zeros(m, np.uint32), ds.train.val.astype(np.float32))
        self.v = (ptr, ids + np.uint32(m), np.ones(m, np.uint32), ds.item.val.astype(np.float32))
        self.pu = ids
        self.pv = ds.train.ycol.astype(np.uint32)
        self.n_items = m
        self.prob = np.ones(m, np.float32)  # no negatives: never read
        self.alias = np.zeros(m, np.uint32)
        self.F, self.kp, self.prm = 2, 4, prm


@pytest.mark.gpu
@pytest.mark.parametrize("adagrad", [0, 1])
def test_permuted_order_visits_every_instance_once(adagrad):
    """T > 10^6, so epoch() finds a prime A: qq = (A q + B) mod T, stepped per
    wave by A (nwaves mod T) mod T.  On conflict-free rows an instance that is
    skipped or applied twice leaves its rows a whole step (about 1e-2) off."""
    m = 1_050_000
    ds = free_ds(m, False)
    assert np.array_equal(ds.train.idx, np.arange(m)) and np.array_equal(ds.item.idx, np.arange(m))
    prm = dict(BASE, adagrad=adagrad, nneg=0)
    t = make(ds, k=4, **prm)
    o = DirectOracle(ds, prm)
    W = centre(t, 4)
    G = t.get("G").copy()
    lg = t.epoch()
    A, B, T = (int(x) for x in t.get("o"))
    assert T == m and A in (1000003, 999983, 1000033, 999979, 1000037, 999961) and A != 1
    lo = o.epoch(W, G, 0, A, B) / T
    check_epoch(f"permuted adagrad {adagrad}", lg, lo, t.get("W"), W, t.get("G"), G, adagrad)


# ----------------------------------------------------- 4. saturated logistic
@pytest.mark.gpu
@pytest.mark.parametrize("adagrad", [0, 1])
def test_saturated_logistic_steps_with_unit_kappa(adagrad):
    """phi of about +-100 with the wrong sign for the label: z = -y phi is
    past expf's range (88.7).  kappa is then -y (1 - tiny), the loss z, and
    the slot rows move by that step; nothing is NaN or inf.  Reference:
    epoch64 (fp64) over the whole epoch.  W: rows towards the other side's
    fields hold c (item j's: s_j c, s_j = +-1 by j's parity), rows towards
    the own side's fields 0.1 c, so phi is about s_j k c^2 sum(x_u) sum(x_v)."""
    m, k, kp, F = 40, 4, 4, 4
    ds = free_ds(m, True)
    prm = dict(BASE, adagrad=adagrad, norm=0, nneg=1, eta=0.02)
    t = make(ds, k=k, serial=1, **prm)
    assert t.info["kp"] == kp and t.info["n_fields"] == F
    o = OracleSgd(ds, F, kp, prm)
    su = np.add.reduceat(o.u[3].astype(np.float64), o.u[0][:-1].astype(np.int64))
    sv = np.add.reduceat(o.v[3].astype(np.float64), o.v[0][:-1].astype(np.int64))
    c = np.sqrt(100.0 / (k * np.median(su) * np.median(sv)))
    W3 = np.zeros((6 * m, F, kp))
    W3[:3 * m, :2], W3[:3 * m, 2:] = 0.1 * c, c  # user features: ids below 3 m
    W3[3 * m:, 2:] = 0.1 * c
    for jrow in range(m):
        feats = o.v[1][o.v[0][jrow]:o.v[0][jrow + 1]].astype(np.int64)
        W3[feats, :2] = c if jrow % 2 == 0 else -c
    W = W3.astype(np.float32).reshape(-1)
    t.set_w(W)
    W3 = W.astype(np.float64).reshape(6 * m, F, kp)
    G3 = np.ones_like(W3)
    lg = t.epoch()
    A, B, T = (int(x) for x in t.get("o"))
    l64, seen = epoch64(o, W3, G3, prm, 0, A, B)
    assert any(y < 0 and p > 89 for y, p in seen) and any(y > 0 and p < -89 for y, p in seen)
    assert any(y * p > 89 for y, p in seen)  # and the harmless side: e^-z underflows
    Wg, Gg = t.get("W"), t.get("G")
    check_epoch(f"saturated adagrad {adagrad}", lg, l64 / T, Wg, W3.reshape(-1), Gg, G3.reshape(-1), adagrad)
    assert np.abs(Wg - W).max() > 50 * 2e-4 * np.abs(W).max()  # the steps are far above the tolerance


# ---------------------------------------------------- 5. constructor refusals
def _refused(ds, code, word=None, **kw):
    with pytest.raises(ocffm.OcffmError) as ei:
        make(ds, **dict(BASE, **kw))
    assert ei.value.code == code, ei.value
    msg = str(ei.value).split("]", 1)[1].strip()
    assert msg and (word is None or word in msg), ei.value


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 129])
def test_refuses_k_outside_range(k):
    _refused(wide_ds(2, 2, 2, 2, 24), ocffm.E_ARG, k=k)


@pytest.mark.gpu
def test_refuses_65_fields():
    _refused(synth.multi_hot(17, 62, 3, 5, 3, m=40), ocffm.E_ARG, "64 fields", k=3)


@pytest.mark.gpu
def test_refuses_65_nodes():
    _refused(synth.multi_hot(17, 1, 1, 41, 24), ocffm.E_ARG, "too wide", k=4)


@pytest.mark.gpu
def test_refuses_17_slots_at_k100():
    """One node per user row over 16 user fields, and an item field whose
    nodes all lie past the Ds the rows are read with, so that its rows are
    empty: 1 node x 17 fields, one slot more than 8 x (64 / 32)."""
    feats = [[(i % 16, i // 16, 1.0)] for i in range(32)]
    train = synth._build_rows(feats, [np.array([i % 5]) for i in range(32)])
    item = synth._build_rows([[(0, 7, 1.0)] for _ in range(5)], None)
    U = ocffm.ImpData.from_rows(train)
    V = ocffm.ImpData.from_rows(item, ds=np.array([3]))
    assert U.info["f"] == 16 and V.info["f"] == 1 and V.info["nnz_x"] == 0
    with pytest.raises(ocffm.OcffmError) as ei:
        ocffm.SgdTrainer(U, V, k=100, **BASE)
    assert ei.value.code == ocffm.E_ARG, ei.value
    assert "too wide" in str(ei.value) and "x fields 17 > 16 slots" in str(ei.value), ei.value


@pytest.mark.gpu
def test_refuses_label_beyond_item_rows():
    ds = synth.multi_hot(17, 2, 2, 2, 2)
    ds.train.ycol[5] = ds.item.m + 2
    _refused(ds, ocffm.E_DATA, "label", k=4)


# ------------------------------------------- 6. draws in the multi-block launch
@pytest.mark.gpu
@pytest.mark.parametrize("grid", [None, "3"])
def test_draws_in_the_default_launch_match_oracle(grid, monkeypatch):
    """eta = 0: W stays bit for bit, so every epoch's loss is a function of the
    drawn instances alone and must equal the oracle's under the same draws."""
    if grid is None:
        monkeypatch.delenv("OCFFM_SGD_GRID", raising=False)
    else:
        monkeypatch.setenv("OCFFM_SGD_GRID", grid)
    ds = synth.tiny(seed=3, m=300, n=40)
    prm = dict(BASE, eta=0.0, adagrad=0, nneg=2)
    t = make(ds, k=4, **prm)
    info = t.info
    o = OracleSgd(ds, info["n_fields"], info["kp"], prm)
    W0 = centre(t, 4)
    for e in range(2):
        lg = t.epoch()
        A, B, T = (int(x) for x in t.get("o"))
        assert T == info["positives"] * 3 == int(ds.train.yptr[-1]) * 3
        W, G = W0.copy(), np.ones_like(W0)
        lo = o.epoch(W, G, e, A, B) / T
        np.testing.assert_array_equal(W, W0)
        np.testing.assert_array_equal(t.get("W"), W0)
        assert abs(lg - lo) <= 1e-4 * abs(lo), (e, lg, lo)
