"""Partner columns: the cross row passes gather a one-hot, unit-valued
partner field's own D x k table through per-position columns instead of its
R x k projection (knob OCFFM_PCOL).

The path rests on one invariant: for a field with one node per row, every
value exactly 1 and not id-like, P[i] == W[xidx[i]] element for element after
every kernel that writes either (the sign of a zero apart).  Replacing the
gathered address then changes no gathered value and no order of any sum, so
every result is bit-identical with the knob on and off.  The tests check the
invariant itself on the GPU, the bit-identity, the per-half gradient and
Hessian-vector product against the oracle, and that fields which must not be
taken (real values, id-like, 2 D > rows) are not.

synth.kkbox_perm: 1,500 x 2,500 rows, artist D = 125 and genre D = 50 (both
eligible), real-valued id fields, a two-node context field.  Its six cross
blocks give the entering gradient pass every combination: (0,2) neither
table small, with the bias gather; (0,3) q small, dxs large; (0,4) both
small; (1,2) q large, dxs small.  The context field's rows run the MFMA tau
variant of the Hessian-vector pass.

Bounds: the invariant and the on / off comparison are exact (array_equal on
values, so +0 == -0); the per-half checks keep the suite's bounds (fp64 1e-12
of the largest entry at init, test_idfield_paths.half_refs' bound at the
trained state; fp32 1e-4).
"""
import struct

import numpy as np
import pytest

import ocffm
import oracle_lib as O
import synth
from test_gpu_parity import rel
from test_idfield_paths import CAPS, env_id, half_refs, perm_ds, set_env

pytestmark = pytest.mark.gpu

PCOL_COUNTERS = ("pcol_gd", "pcol_hs", "pcol_bytes")


# ------------------------------------------------------------------ fields
class Field:
    """What the solver derives of one field of one side, restated on the rows."""

    def __init__(self, rows, f):
        m = rows.m
        row_of = np.repeat(np.arange(m), np.diff(rows.xptr.astype(np.int64)))
        sel = rows.fid == f
        self.cols = rows.idx[sel].astype(np.int64)  # (row order: one entry per row where `one`)
        self.one = m > 0 and bool((np.bincount(row_of[sel], minlength=m) == 1).all())
        self.unit = bool(sel.any()) and bool((rows.val[sel] == 1.0).all())
        self.D = int(self.cols.max()) + 1 if sel.any() else 0
        self.idlike = self.one and self.D == m and np.unique(self.cols).size == m
        self.eligible = self.one and self.unit and not self.idlike and 2 * self.D <= m


def fields_of(ds):
    """(fu, [Field per global field index])."""
    fu, fv = int(ds.train.fid.max()) + 1, int(ds.item.fid.max()) + 1
    return fu, [Field(ds.train, f) for f in range(fu)] + [Field(ds.item, f) for f in range(fv)]


def blocks_of(ds, self_side=True):
    fu, F = fields_of(ds)
    f = len(F)
    return [(f1, f2, O.block_index(f1, f2, f)) for f1 in range(f) for f2 in range(f1, f)
            if self_side or f1 < fu <= f2]


def expected_pcol_bytes(ds):
    """4 B per positive for every eligible field that is some cross half's partner."""
    fu, F = fields_of(ds)
    return 4 * ds.n_positives * sum(1 for fl in F if fl.eligible)


def assert_invariant(g, ds, self_side, where):
    """P == W[col] (Q == H[col]) for every block and eligible field."""
    _, F = fields_of(ds)
    seen = 0
    for f1, f2, b12 in blocks_of(ds, self_side):
        for fl, tab, proj in ((f1, "W", "P"), (f2, "H", "Q")):
            if not F[fl].eligible:
                continue
            R = g.get(proj, b12).reshape(F[fl].cols.size, -1)
            T = g.get(tab, b12).reshape(-1, R.shape[1])
            assert T.shape[0] == F[fl].D
            assert np.array_equal(R, T[F[fl].cols]), (where, f1, f2, proj)
            seen += 1
    assert seen > 0
    return seen


def state(g, ds, self_side=True):
    out = {(w, b12): g.get(w, b12) for _, _, b12 in blocks_of(ds, self_side) for w in "WHPQ"}
    out.update({(w, 0): g.get(w) for w in "abuv"})
    return out


def run(monkeypatch, ds, env, precision, epochs, **kw):
    """Epochs from the seeded init under `env`: (state, CG log, counters)."""
    set_env(monkeypatch, env)
    g = ocffm.problem_from_dataset(ds, precision=precision, **kw)
    ocffm.srand(1)
    g.init()
    for _ in range(epochs):
        g.one_epoch()
    out = (state(g, ds, kw.get("self_side", True)), g.cg_log().copy(), {n: g.counter(n) for n in PCOL_COUNTERS})
    g.close()
    for k in env:
        monkeypatch.delenv("OCFFM_" + k)
    return out


def assert_same(on, off):
    assert on[0].keys() == off[0].keys()
    for key in on[0]:
        assert np.array_equal(on[0][key], off[0][key]), key
    np.testing.assert_array_equal(on[1], off[1])


# --------------------------------------------------------------- invariant
INVARIANT_ENVS = [{}, {"NO_FOLD": "1"}, {"CCG": "2"}, {"CGP": "0"}]


@pytest.mark.parametrize("precision", [ocffm.FP32, ocffm.FP64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("env", INVARIANT_ENVS, ids=env_id)
def test_invariant_kkbox_perm(monkeypatch, env, precision):
    """After init() and after each of 3 epochs the projection of every
    eligible field equals the gathered rows of its table, in every block, with
    the path on (the default); only artist and genre got columns."""
    ds = perm_ds()
    set_env(monkeypatch, env)
    g = ocffm.problem_from_dataset(ds, precision=precision)
    ocffm.srand(1)
    g.init()
    assert_invariant(g, ds, True, "init")
    for e in range(1, 4):
        g.one_epoch()
        assert_invariant(g, ds, True, f"epoch {e}")
    c = {n: g.counter(n) for n in PCOL_COUNTERS}
    print(env_id(env), c)
    assert c["pcol_gd"] > 0 and c["pcol_hs"] > 0
    assert c["pcol_bytes"] == expected_pcol_bytes(ds) == 8 * ds.n_positives
    g.close()


def cfg5_small():
    return synth.cfg5(m=300, n=60, d_user=50, k=64, name="cfg5_pcol")


@pytest.mark.parametrize("precision", [ocffm.FP32, ocffm.FP64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("env", [{}, {"XFUSE": "0"}], ids=env_id)
def test_invariant_cfg5(monkeypatch, env, precision):
    """Config 5's structure at test size: 39 eligible user fields (the item
    halves' partners), the id-like item field never taken.  The item halves'
    CG steps are k_hv_cross_id's by default (the item field is id-like), which
    stays on the projection: only their gradient passes take the path, and
    with OCFFM_XFUSE=0 their k_hs_cross_seg steps too."""
    ds = cfg5_small()
    set_env(monkeypatch, env)
    g = ocffm.problem_from_dataset(ds, precision=precision, self_side=False, k=64)
    ocffm.srand(1)
    g.init()
    assert assert_invariant(g, ds, False, "init") == 39
    for e in range(1, 4):
        g.one_epoch()
        assert_invariant(g, ds, False, f"epoch {e}")
    assert g.counter("pcol_gd") > 0
    assert (g.counter("pcol_hs") > 0) == (env.get("XFUSE") == "0")
    assert g.counter("pcol_bytes") == expected_pcol_bytes(ds) == 39 * 4 * ds.n_positives
    g.close()


# ------------------------------------------------------------ bit-identity
# (LAZY_BASE=0: every cross gradient pass reads the full base and gathers the
# partner bias, so it keeps the projection; the Hessian-vector passes take the path)
SEGS = {"LAZY_BASE": "0", "YTVIA": "0", "HOT": "2", "SEG_LEN": "2"}
ONOFF_CASES = [(k, {}) for k in (5, 32, 64, 128)] + [(32, dict(CAPS)), (32, {"YTVIA": "0", "HOT": "2", "SEG_LEN": "2"}),
                                                       (32, SEGS)]


@pytest.mark.parametrize("precision", [ocffm.FP32, ocffm.FP64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("k,env", ONOFF_CASES, ids=[f"k={k}-{env_id(e)}" for k, e in ONOFF_CASES])
def test_on_off_bit_identical(monkeypatch, k, env, precision):
    """OCFFM_PCOL=1 against 0 after 3 epochs (4 in fp32, where the column-Gram
    and hot-row paths engage from the previous epoch's CG counts): every W, H,
    P and Q, both biases, both y~ orientations and the CG log are equal."""
    ds = perm_ds()
    epochs = 4 if precision == ocffm.FP32 else 3
    on = run(monkeypatch, ds, dict(env, PCOL="1"), precision, epochs, k=k)
    off = run(monkeypatch, ds, dict(env, PCOL="0"), precision, epochs, k=k)
    print(k, env_id(env), on[2], off[2])
    assert_same(on, off)
    assert off[2] == {n: 0 for n in PCOL_COUNTERS}
    assert on[2]["pcol_hs"] > 0
    if env.get("LAZY_BASE") != "0":
        assert on[2]["pcol_gd"] > 0
    assert on[2]["pcol_bytes"] == 8 * ds.n_positives


# ---------------------------------------------------------------- per half
@pytest.fixture(scope="module")
def snap_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("pcol")


@pytest.mark.parametrize("precision", [ocffm.FP32, ocffm.FP64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("state_name", ["init", "trained"])
def test_cross_halves_against_oracle(state_name, precision, snap_dir):
    """Every cross half's gradient and Hessian-vector product against the
    fp64 oracle with the path on."""
    ds = perm_ds()
    fu, _ = fields_of(ds)
    path, refs = half_refs(state_name, snap_dir)
    g = ocffm.problem_from_dataset(ds, precision=precision, with_test=False)
    if state_name == "trained":
        g.load_binary(path)
    else:
        ocffm.srand(1)
        g.init()
    assert_invariant(g, ds, True, state_name)
    worst = {"grad": 0.0, "hv": 0.0}
    for f1, f2, half, G0, v, H0, tol64 in refs:
        if not f1 < fu <= f2:
            continue
        tol = 1e-4 if precision == ocffm.FP32 else tol64
        dg, dh = rel(g.grad(f1, f2, half), G0), rel(g.hv(f1, f2, half, v), H0)
        worst = {"grad": max(worst["grad"], dg), "hv": max(worst["hv"], dh)}
        assert dg <= tol, ("grad", f1, f2, half, dg, tol)
        assert dh <= tol, ("hv", f1, f2, half, dh, tol)
    print(state_name, worst)
    assert g.counter("pcol_hs") > 0
    g.close()


# ------------------------------------------------------ where it must not be
def real_valued():
    return synth.general(seed=5, m=200, n=120, fu=2, fv=2, k=8, vals="real", name="pcol_real")


def edge_fields():
    """Users with real-valued fields; items with a real-valued one-node field
    (never taken), a D = 1 field (every gather hits the same row), a field of
    D = 30 whose columns 10..28 are empty, and a unit field of D = 90 > n / 2
    (not taken).  Users 3 and 7 and items 0 and n - 1 have no positives."""
    n = 120
    ds = synth.general(seed=6, m=200, n=n, fu=2, fv=1, k=8, vals="real", name="pcol_edge")
    rng = np.random.default_rng(9)
    tr = ds.train
    row_of = np.repeat(np.arange(tr.m), np.diff(tr.yptr.astype(np.int64)))
    keep = ~np.isin(row_of, (3, 7)) & ~np.isin(tr.ycol, (0, n - 1))
    yptr = np.zeros(tr.m + 1, dtype=np.uint64)
    np.cumsum(np.bincount(row_of[keep], minlength=tr.m), out=yptr[1:])
    train = synth.Rows(tr.xptr, tr.fid, tr.idx, tr.val, yptr, tr.ycol[keep])
    col = lambda a: np.asarray(a, dtype=np.uint64)[:, None]
    ones = np.ones((n, 1))
    sparse = rng.integers(0, 10, size=n)
    sparse[-1] = 29
    wide = rng.integers(0, 90, size=n)
    wide[0] = 89
    item = synth._fast_rows(n, [(0, col(rng.integers(0, 40, size=n)), np.round(0.5 + rng.random((n, 1)), 3)),
                                (1, col(np.zeros(n)), ones), (2, col(sparse), ones), (3, col(wide), ones)])
    return synth.Dataset(ds.name, train, item, None, ds.k, dict(ds.params))


@pytest.mark.parametrize("precision", [ocffm.FP32, ocffm.FP64], ids=["fp32", "fp64"])
def test_real_values_not_taken(monkeypatch, precision):
    ds = real_valued()
    _, F = fields_of(ds)
    assert all(f.one and not f.unit and not f.idlike for f in F)
    on = run(monkeypatch, ds, {"PCOL": "1"}, precision, 3, with_test=False)
    off = run(monkeypatch, ds, {"PCOL": "0"}, precision, 3, with_test=False)
    assert on[2] == off[2] == {n: 0 for n in PCOL_COUNTERS}
    assert_same(on, off)


@pytest.mark.parametrize("precision", [ocffm.FP32, ocffm.FP64], ids=["fp32", "fp64"])
def test_edge_fields(monkeypatch, precision):
    ds = edge_fields()
    fu, F = fields_of(ds)
    assert [f.eligible for f in F] == [False, False, False, True, True, False]
    assert F[fu + 1].D == 1 and F[fu + 2].D == 30 and F[fu + 3].D == 90 and F[fu + 3].unit and F[fu + 3].one
    assert np.diff(ds.train.yptr.astype(np.int64)).min() == 0
    on = run(monkeypatch, ds, {"PCOL": "1"}, precision, 3)
    off = run(monkeypatch, ds, {"PCOL": "0"}, precision, 3)
    print(on[2])
    assert off[2] == {n: 0 for n in PCOL_COUNTERS}
    assert on[2]["pcol_gd"] > 0 and on[2]["pcol_hs"] > 0
    assert on[2]["pcol_bytes"] == expected_pcol_bytes(ds) == 2 * 4 * ds.n_positives
    assert_same(on, off)
    g = ocffm.problem_from_dataset(ds, precision=precision)
    ocffm.srand(1)
    g.init()
    g.one_epoch()
    assert_invariant(g, ds, True, "epoch 1")
    g.close()


# ------------------------------------------------------------------- flag
def fnv_u64(v):
    h = 0xcbf29ce484222325
    for b in struct.pack("<Q", v):
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.parametrize("host", [False, True], ids=["device-build", "host-build"])
def test_unit_flag_in_both_builds(monkeypatch, host):
    """The layout digest's flags word (one 1, id-like 2, owned 4, unit 8) of
    kkbox_perm's fields from the device build and from the host build."""
    monkeypatch.setenv("OCFFM_HOST_BUILD", "1" if host else "0")
    g = ocffm.problem_from_dataset(perm_ds(), precision=ocffm.FP32)
    d = g.layout_digest()
    g.close()
    want = {"U.F0.flags": 1 | 2, "U.F1.flags": 8, "V.F0.flags": 1 | 2, "V.F1.flags": 1 | 8, "V.F2.flags": 1 | 8}
    for name, flags in want.items():
        assert d[name] == fnv_u64(flags), (name, flags)
