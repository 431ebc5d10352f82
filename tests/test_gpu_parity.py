"""GPU parity: the HIP path (through the C ABI) against the CPU oracle.

Tolerances (written here):
  fp64 mode  : state (W, H, P, Q, a, b, y~) and objective within 1e-9 relative
               of the oracle; CG iteration counts identical; p@k / nDCG@k
               identical up to 1e-12.  Where the reference's own arithmetic
               drifts further on a set (ill-conditioned capped CG solves:
               k = 64 / 100 from epoch 2, heavy real-valued columns, the
               kkbox shape at full size), the bound is 3x that measured
               drift: the oracle at 2..16 threads (and, for kkbox_full, with
               the cblas_ddot orders of optimised BLAS builds) against itself
               at 1 thread, serial (tests/golden/fp64_envelope.json, made by
               tools/fp64_drift.py --envelope; fp64_tol below).  kdd12 at full
               size does not reproduce itself (its CG counts differ between
               reference runs): validation metrics within 3x their spread.
  fp32 mode  : objective and ploss within 1e-3 relative, p@k and nDCG@k
               within 2e-2 absolute (SURVEY §8c measured fp32 drift).
  per kernel : a half's gradient and Hessian-vector product at init within
               1e-4 (fp32) / 1e-12 (fp64) of its largest entry.
  trained state (test_fp32_trained.py, halves_ref.py; both precisions, every
  padded k but 32):
               a half at a trained state is held per feature row d to
               tol x max_c G_abs[d, c] (Hv_abs likewise), tol = 1e-4 / 1e-12,
               where G_abs is the half's sum with every elementary product
               replaced by its absolute value: the forward bound
               n u sum|terms| (n < 1,600 terms on those shapes, u = 2^-24).
               The scale is the terms', not the result's, because at a trained
               state the terms cancel (abs-sum 20 to 900 times the largest
               entry), and per row because a table-wide maximum hides the
               light rows.  Measured: fp32 <= 0.004, fp64 <= 0.0011 of it.
               Cached tables (P, Q, a, b, s, t, y~) after an epoch within
               1e-4 / 1e-11 of the larger of their definition's largest entry
               before and after the epoch (in-place updates round relative to
               what they started from).  Measured: fp32 <= 0.005, fp64
               <= 1.4e-4 of it.
  one-step regime (the same files): from W, H = float32(2^-7 N(0, 1)) at the
               smallest lambda of {8, .., 128} at which every half's CG stops
               after one step on the oracle, a half's update is -alpha G with
               G the in-epoch gradient, so one epoch compares the in-epoch
               passes with no CG iteration to amplify fp32 noise: tables
               within 1e-4 / 1e-9 of their largest reference entry, one CG
               step per half on both sides.  Measured: fp32 <= 0.015, fp64
               <= 5.7e-5 of it.  Per case: DESIGN.md §4.
Init is bit-exact in both modes' source tables: W/H come from the same host
rand() stream as the reference (ffm.cpp:71-78).
"""
import json
import os
import subprocess

import numpy as np
import pytest

import ocffm
import oracle_lib as O
import synth

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(REPO, "one-class-ffm_amd", "train")
ORACLE_TRAIN = os.path.join(REPO, "oracle", "oracle_train")


_ENV = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fp64_envelope.json")))


def fp64_tol(name, epochs):
    """max(1e-9, 3 x the reference arithmetic's own drift on this set after
    `epochs` epochs) — the oracle's reassociated sums (per-thread partials
    under schedule(guided), ffm.cpp:557,759) against its 1-thread run."""
    env = _ENV["sets"].get(name)
    return 1e-9 if env is None else max(1e-9, 3.0 * env[epochs - 1])


def pair(ds, precision=ocffm.FP64, self_side=True, freq=False, with_test=True, **kw):
    o = O.Oracle(ds, self_side=self_side, freq=freq, with_test=with_test, **kw)
    g = ocffm.problem_from_dataset(ds, precision=precision, self_side=self_side, freq=freq, with_test=with_test,
                                   **kw)
    ocffm.srand(1)
    o.init()
    ocffm.srand(1)
    g.init()
    return o, g


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max())) if b.size else 0.0


def state_names(o):
    out = []
    for f1 in range(o.f):
        for f2 in range(f1, o.f):
            if not o.self_side and not (f1 < o.fu <= f2):
                continue
            out.append(O.block_index(f1, f2, o.f))
    return out


def assert_state(o, g, tol, check_yt=True):
    for b12 in state_names(o):
        for what in "WHPQ":
            d = rel(g.get(what, b12), o.get(what, b12))
            assert d <= tol, (what, b12, d, tol)
    for what in "ab" + ("uv" if check_yt else ""):
        d = rel(g.get(what), o.get(what))
        assert d <= tol, (what, d, tol)


def gpu_objective(o, g):
    """Objective of the GPU state: load its W/H into the oracle and evaluate
    the reference's func() (ffm.cpp:1321-1351)."""
    for b12 in state_names(o):
        o.set("W", b12, g.get("W", b12))
        o.set("H", b12, g.get("H", b12))
    o.refresh()
    return o.func()


def test_init_state(tiny):
    o, g = pair(tiny)
    for b12 in state_names(o):
        np.testing.assert_array_equal(g.get("W", b12), o.get("W", b12))  # same host stream
        np.testing.assert_array_equal(g.get("H", b12), o.get("H", b12))
    assert_state(o, g, 1e-13)
    assert rel(g.get("s"), o.get("s")) <= 1e-12
    assert rel(g.get("t"), o.get("t")) <= 1e-12


@pytest.mark.parametrize("hot", ["", "2"])
@pytest.mark.parametrize("self_side", [True, False])
def test_gradient_and_hv_kernels(self_side, hot, monkeypatch):
    """Every half's gradient and Hessian-vector product (fp64) against the
    oracle.  OCFFM_HOT=2: every cross-half row with >= 2 positives reads a
    per-row Gram of its partner rows (k_gram_build) instead of gathering them."""
    if hot:
        monkeypatch.setenv("OCFFM_HOT", hot)
    ds = synth.general(seed=5, m=60, n=40, fu=2, fv=2, k=5, nnz_user=2, mean_pos=3.0, vals="real")
    o, g = pair(ds, self_side=self_side, with_test=False)
    rng = np.random.default_rng(0)
    for f1 in range(o.f):
        for f2 in range(f1, o.f):
            if not self_side and not (f1 < o.fu <= f2):
                continue
            for half in (0, 1):
                G0, G1 = o.grad(f1, f2, half), g.grad(f1, f2, half)
                assert rel(G1, G0) <= 1e-12, ("grad", f1, f2, half)
                v = rng.standard_normal(G0.size)
                H0, H1 = o.hv(f1, f2, half, v), g.hv(f1, f2, half, v)
                assert rel(H1, H0) <= 1e-12, ("hv", f1, f2, half)


def test_gradient_order_independent():
    """Gradients of side halves in any order (user side, item side, user side
    again, then a user-side block solve): the per-segment sums the side
    gradient passes share (k_seg_ysum, one buffer for both sides) must be
    recomputed whenever the other side's sums replaced them."""
    ds = synth.general(seed=5, m=60, n=40, fu=2, fv=2, k=5, nnz_user=2, mean_pos=3.0, vals="real")
    o, g = pair(ds, with_test=False)
    for f1, f2 in ((0, 0), (2, 2), (0, 1), (3, 3), (1, 1)):
        for half in (0, 1):
            assert rel(g.grad(f1, f2, half), o.grad(f1, f2, half)) <= 1e-12, (f1, f2, half)
    o.solve_block(2, 3)
    g.solve_block(2, 3)
    o.solve_block(0, 0)
    g.solve_block(0, 0)
    assert_state(o, g, 1e-9)
    np.testing.assert_array_equal(g.cg_log(), o.cg_log())


KK_RC = dict(seed=3, m=1500, n=4000, mean=20.0, name="kk_rc")  # ~24 % heavy positives on both sides


GRAM_EDGE_COLS = (1, 31, 32, 0, 33, 63, 64, 65, 129)  # rows of the user field's columns
GRAM_EDGE_POS = (1, 2, 31, 32, 33, 64, 65, 257)  # the user rows' positive counts, cycled


def gram_edges():
    """A hand-built set (k = 32, real-valued x) on the chunk boundaries of the
    Gram builds from gathered rows (kernels.hpp k_gram_build*).  418 users
    with ONE one-node field of 9 columns of 1, 31, 32, 0, 33, 63, 64, 65 and
    129 rows (OCFFM_CGRAM=2, side column Grams: an empty column that must
    store a zero Gram, one full 64-row wave chunk, a 64 + 1 two-chunk column,
    a three-chunk column); positive counts cycling through 1, 2, 31, 32, 33,
    64, 65 and 257 (OCFFM_HOT=2: the 32-row batch edge, two full batches, a
    row over HOT_CHUNK_MAX = 256 in two balanced chunks; OCFFM_CCG=2: the
    columns' position counts cross the 256-position cut several times); 300
    items (an id field and a one-node field of 5 uneven columns), item 0
    positive for nine users in ten (the item half's hot row of two chunks)."""
    rng = np.random.default_rng(17)
    n = 300

    def x():
        return float(np.round(0.25 + 1.5 * rng.random(), 3))

    feats, labels = [], []
    for c, rows in enumerate(GRAM_EDGE_COLS):
        for _ in range(rows):
            i = len(feats)
            feats.append([(0, c, x())])
            cnt = GRAM_EDGE_POS[i % len(GRAM_EDGE_POS)]
            if i % 10 == 0:
                pos = 1 + rng.choice(n - 1, size=cnt, replace=False)
            else:
                pos = np.append(0, 1 + rng.choice(n - 1, size=cnt - 1, replace=False))
            labels.append(np.sort(pos))
    train = synth._build_rows(feats, labels)
    cat = np.repeat(np.arange(5), (1, 64, 65, 40, 130))
    item = synth._build_rows([[(0, j, 1.0), (1, int(cat[j]), x())] for j in range(n)], None)
    return synth.Dataset("gram_edges", train, item, None, k=32,
                         params=dict(k=32, t=20, l=4.0, w=0.0078125, r=-1.0))


_HALF_REFS = {}


def half_refs(name):
    """(data set, [(f1, f2, half, gradient, v, Hessian-vector product)]) of
    every half from the fp64 oracle, computed once per data set."""
    if name not in _HALF_REFS:
        ds = gram_edges() if name == "gram_edges" else synth.kkbox(**KK_RC)
        o = O.Oracle(ds, with_test=False)
        ocffm.srand(1)
        o.init()
        rng = np.random.default_rng(3)
        refs = []
        for f1 in range(o.f):
            for f2 in range(f1, o.f):
                for half in (0, 1):
                    G0 = o.grad(f1, f2, half)
                    v = rng.standard_normal(G0.size)
                    refs.append((f1, f2, half, G0, v, o.hv(f1, f2, half, v)))
        _HALF_REFS[name] = (ds, refs)
    return _HALF_REFS[name]


def check_halves(env, monkeypatch, precision, tol):
    env = dict(env)
    ds, refs = half_refs(env.pop("ds", "kk_rc"))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g = ocffm.problem_from_dataset(ds, precision=precision, with_test=False)
    ocffm.srand(1)
    g.init()
    for f1, f2, half, G0, v, H0 in refs:
        G1 = g.grad(f1, f2, half)
        assert rel(G1, G0) <= tol, ("grad", f1, f2, half, rel(G1, G0))
        H1 = g.hv(f1, f2, half, v)
        assert rel(H1, H0) <= tol, ("hv", f1, f2, half, rel(H1, H0))


def edge_envs(envs):
    """The envs on gram_edges; ids like edges-CGRAM=2-NO_MFMA=1 (edges: no env)."""
    return [pytest.param(dict(e, ds="gram_edges"), id="-".join(["edges"] + [f"{k[6:]}={v}" for k, v in e.items()]))
            for e in envs]


ENVS_FP32 = [{}, {"OCFFM_NO_MFMA": "1"}, {"OCFFM_CGRAM": "2"}, {"OCFFM_CGRAM": "2", "OCFFM_NO_MFMA": "1"},
             {"OCFFM_TPRE": "1"}, {"OCFFM_HOT": "0"}, {"OCFFM_HOT": "2"}, {"OCFFM_HOT": "2", "OCFFM_NO_MFMA": "1"},
             {"OCFFM_CCG": "2"}, {"OCFFM_CCG": "2", "OCFFM_NO_MFMA": "1"}]
ENVS_FP64 = [{}, {"OCFFM_CGRAM": "2"}, {"OCFFM_CCG": "2"}, {"OCFFM_NO_MFMA": "1"}]


@pytest.mark.parametrize("env", ENVS_FP32 + edge_envs(ENVS_FP32))
def test_gradient_and_hv_fp32_k32(monkeypatch, env):
    """fp32 at k = 32 (the perf build: the cross halves' k x k Grams on MFMA,
    kernels.hpp k_gram_mfma32; OCFFM_CGRAM=2: every side half of a
    one-node field on per-column Grams, built on MFMA by k_gram_build_mfma
    with multi-chunk columns summed by k_gram_slot_sum, or by k_col_gram
    under OCFFM_NO_MFMA) against the fp64 oracle: every half's gradient and
    Hessian-vector product within 1e-4 of its largest entry.  On the kkbox
    shape KK_RC, and (edges*) on gram_edges, the chunk boundaries of the Gram
    builds."""
    check_halves(env, monkeypatch, ocffm.FP32, 1e-4)


@pytest.mark.parametrize("env", ENVS_FP64 + edge_envs(
    ENVS_FP64 + [{"OCFFM_HOT": "2"}, {"OCFFM_CGRAM": "2", "OCFFM_NO_MFMA": "1"}]))
def test_gradient_and_hv_fp64_k32(monkeypatch, env):
    """fp64 at k = 32, where the k x k work runs on the f64 matrix cores
    (v_mfma_f64_16x16x4f64: the cross-half aggregates k_gram_mfma_f64, the
    side-half column Grams under OCFFM_CGRAM=2 and the cross column Grams
    under OCFFM_CCG=2 on k_gram_build_mfma; OCFFM_NO_MFMA=1: the VALU
    kernels): every half's gradient and Hessian-vector product within 1e-12
    of the oracle's.  On the kkbox shape KK_RC, and (edges*) on gram_edges,
    the chunk boundaries of the Gram builds."""
    check_halves(env, monkeypatch, ocffm.FP64, 1e-12)


def test_epochs_fp32_k32():
    """Two fp32 epochs at k = 32: objective of the fp32 state (evaluated in
    fp64) within 1e-3 of the oracle's; CG counts within 1 per half."""
    ds = synth.kkbox(**KK_RC)
    o, g = pair(ds, precision=ocffm.FP32, with_test=False)
    for _ in range(2):
        o.one_epoch()
        g.one_epoch()
    f_ref = o.func()
    o2 = O.Oracle(ds, with_test=False)
    ocffm.srand(1)
    o2.init()
    assert abs(gpu_objective(o2, g) - f_ref) <= 1e-3 * abs(f_ref)
    assert np.abs(g.cg_log().astype(int) - o.cg_log().astype(int)).max() <= 1


def test_block_by_block_fp64(tiny):
    o, g = pair(tiny)
    for f1 in range(o.f):
        for f2 in range(f1, o.f):
            o.solve_block(f1, f2)
            g.solve_block(f1, f2)
            assert_state(o, g, 1e-9)
    np.testing.assert_array_equal(g.cg_log(), o.cg_log())


def test_epochs_fp64_tiny(tiny):
    o, g = pair(tiny)
    for e in range(3):
        o.one_epoch()
        g.one_epoch()
        assert_state(o, g, 1e-9)
        assert rel(g.get("s"), o.get("s")) <= 1e-9
        vo, vg = o.validate(), g.validate()
        assert abs(vg["loss"] - vo["loss"]) <= 1e-9 * abs(vo["loss"])
        np.testing.assert_allclose(vg["prec"], vo["prec"], atol=1e-12)
        np.testing.assert_allclose(vg["ndcg"], vo["ndcg"], atol=1e-12)
    np.testing.assert_array_equal(g.cg_log(), o.cg_log())


@pytest.mark.parametrize("k", [None, 128])
def test_epochs_fp32_tiny(tiny, k):
    """fp32 within 1e-3 of the fp64 oracle (north_star's tolerance); k = 128,
    the largest k, runs the VALU kernels at 32 lanes of 4 values per row."""
    kw = {} if k is None else {"k": k}
    ds = tiny if k is None else synth.tiny(seed=4, m=300)
    o, g = pair(ds, precision=ocffm.FP32, **kw)
    for e in range(3):
        o.one_epoch()
        g.one_epoch()
    vo, vg = o.validate(), g.validate()
    assert abs(vg["loss"] - vo["loss"]) <= 1e-3 * abs(vo["loss"])
    np.testing.assert_allclose(vg["prec"], vo["prec"], atol=2e-2)
    np.testing.assert_allclose(vg["ndcg"], vo["ndcg"], atol=2e-2)
    # objective of the fp32 state, evaluated in fp64 by a second oracle
    f_ref = o.func()
    o2 = O.Oracle(ds, **kw)
    ocffm.srand(1)
    o2.init()
    f32obj = gpu_objective(o2, g)
    assert abs(f32obj - f_ref) <= 1e-3 * abs(f_ref)


@pytest.mark.parametrize("variant", ["ns", "freq", "k5", "k16", "multi_nnz", "k1", "k64", "k100", "k128", "sparse",
                                     "kdd12", "outbrain", "wide_ns", "multi_nnz_pg", "freq_pg", "k64_pg"])
def test_variants_fp64(variant, monkeypatch):
    """Flags and shapes: --ns, --freq, k = 1 / 5 / 16 / 64 / 100 / 128 (padded
    rows of 4 .. 128: one to 64 lanes per row; 128 is the largest k the
    library takes), several nodes per field, a sparse
    set (users and items without positives, empty feature columns), and the
    field structures of BASELINE configs 2, 4 and 5 at test size:
    kdd12-shape (fu=2, fv=4, k=16), outbrain-shape (fu=2, fv=2, k=64, ~1
    positive per row) and the wide --ns set (fu=39, fv=1: 39 cross blocks)."""
    kw = {}
    pg = variant.endswith("_pg")
    if pg:
        # pair Grams (k_pg_step) forced on every multi-node field's side
        # halves: real-valued nodes, repeated features in a row, --freq, k = 64
        monkeypatch.setenv("OCFFM_PGRAM", "2")
        variant = variant[:-3]
    if variant == "kdd12":
        ds = synth.general(seed=31, m=400, n=120, fu=2, fv=4, k=16, mean_pos=3.0, test_rows=40, name="kdd12")
    elif variant == "outbrain":
        ds = synth.general(seed=32, m=400, n=60, fu=2, fv=2, k=64, mean_pos=1.0, test_rows=40, name="outbrain")
        kw["k"] = 64
    elif variant == "wide_ns":
        ds = synth.general(seed=33, m=200, n=40, fu=39, fv=1, k=8, d_user=[20] * 39, d_item=[40], mean_pos=3.0,
                           test_rows=20, name="wide_ns")
    elif variant == "multi_nnz":
        ds = synth.general(seed=9, m=150, n=70, fu=3, fv=2, k=8, nnz_user=3, mean_pos=4.0, vals="real", test_rows=30)
    elif variant == "sparse":
        ds = synth.general(seed=13, m=120, n=90, fu=2, fv=2, k=4, d_user=[300, 7], d_item=[200, 5], mean_pos=0.7,
                           test_rows=20)
    else:
        ds = synth.tiny(seed=4, m=300 if variant in ("k64", "k100", "k128") else 1000)
    if pg and variant != "multi_nnz":
        ds = synth.general(seed=19, m=300, n=80, fu=2, fv=2, k=8, nnz_user=3, mean_pos=4.0, vals="real", test_rows=30)
    for name, k in (("k1", 1), ("k5", 5), ("k16", 16), ("k64", 64), ("k100", 100), ("k128", 128)):
        if variant == name:
            kw["k"] = k
    o, g = pair(ds, self_side=variant not in ("ns", "wide_ns"), freq=variant == "freq", **kw)
    # three epochs.  At k = 64 / 100 / 128 block (1,1)'s W half runs into the
    # 20-iteration CG cap (ffm.cpp:761) from epoch 2 on this set, and that
    # ill-conditioned solve amplifies any reassociation: the reference's own
    # arithmetic drifts ~1e-6 (k = 64) / ~8e-9 (k = 100) between thread
    # counts there (fp64_envelope.json), so those epochs are held to 3x it
    epochs = 3
    for e in range(1, epochs + 1):
        o.one_epoch()
        g.one_epoch()
        assert_state(o, g, fp64_tol(variant, e))
    np.testing.assert_array_equal(g.cg_log(), o.cg_log())
    vo, vg = o.validate(), g.validate()
    assert abs(vg["loss"] - vo["loss"]) <= fp64_tol(variant, epochs) * abs(vo["loss"])
    np.testing.assert_allclose(vg["ndcg"], vo["ndcg"], atol=1e-12)


# BASELINE configs[4] (SURVEY §8d restated): --ns, 39 user fields + 1 item
# field, k = 64.  39 cross blocks: the C = 39 Grams of 64 x 64 (624 KB) do not
# fit the gradient pass's LDS.
def _cfg5_small(m=300, n=60, k=64, fu=39, seed=41, test_rows=30):
    return synth.general(seed=seed, m=m, n=n, fu=fu, fv=1, k=k, d_user=[max(4, m // 6)] * fu, d_item=[n],
                         mean_pos=4.0, test_rows=test_rows, name="cfg5_small")


def test_cfg5_shape_fp64():
    """Config-5 structure at test size in the parity mode: two epochs of all
    78 halves against the oracle within 1e-9 after each, identical CG
    counts, and the validation metrics (ffm.cpp:852-870, 630-703 with C = 39)."""
    ds = _cfg5_small()
    o, g = pair(ds, self_side=False, k=64)
    for e in (1, 2):
        o.one_epoch()
        g.one_epoch()
        assert_state(o, g, fp64_tol("cfg5_shape", e))
    np.testing.assert_array_equal(g.cg_log(), o.cg_log())
    vo, vg = o.validate(), g.validate()
    assert abs(vg["loss"] - vo["loss"]) <= 1e-9 * abs(vo["loss"])
    np.testing.assert_allclose(vg["ndcg"], vo["ndcg"], atol=1e-12)


@pytest.mark.parametrize("hot", ["", "2"])
@pytest.mark.parametrize("k,fu", [(64, 39), (32, 20)])
def test_cfg5_shape_fp32_mfma(k, fu, hot, monkeypatch):
    """The fp32 perf path at config-5 structure: the cross halves' T_i on MFMA
    ahead of the gradient pass (k_rows_T<KP>: the C Grams exceed 64 KB of
    LDS) and, at k = 64, the C cross Grams on MFMA (k_gram_mfma64), checked
    per half against the fp64 oracle (gradient and Hessian-vector within
    1e-4 of their largest entry) on 2,000 rows (several row chunks per
    block of both kernels, ragged tails).  OCFFM_HOT=2: the item halves'
    popular items (and every row with >= 2 positives) on per-row Grams built
    on MFMA (k_gram_build_mfma, KP = 32 / 64; multi-chunk items summed in slot
    order)."""
    if hot:
        monkeypatch.setenv("OCFFM_HOT", hot)
    ds = _cfg5_small(m=2003, n=301, k=k, fu=fu, seed=43, test_rows=0)
    o, g = pair(ds, precision=ocffm.FP32, self_side=False, k=k, with_test=False)
    rng = np.random.default_rng(5)
    for f1 in (0, fu // 2, fu - 1):
        for half in (0, 1):
            G0, G1 = o.grad(f1, fu, half), g.grad(f1, fu, half)
            assert rel(G1, G0) <= 1e-4, ("grad", f1, half, rel(G1, G0))
            v = rng.standard_normal(G0.size)
            H0, H1 = o.hv(f1, fu, half, v), g.hv(f1, fu, half, v)
            assert rel(H1, H0) <= 1e-4, ("hv", f1, half, rel(H1, H0))


def test_cfg5_shape_fp32_epochs():
    """Two fp32 epochs at config-5 structure (k = 64): objective of the fp32
    state (evaluated in fp64 by the oracle) within 1e-3 of the oracle's."""
    ds = _cfg5_small(m=800, n=120, seed=47, test_rows=0)
    o, g = pair(ds, precision=ocffm.FP32, self_side=False, k=64, with_test=False)
    for _ in range(2):
        o.one_epoch()
        g.one_epoch()
    f_ref = o.func()
    o2 = O.Oracle(ds, self_side=False, k=64, with_test=False)
    ocffm.srand(1)
    o2.init()
    assert abs(gpu_objective(o2, g) - f_ref) <= 1e-3 * abs(f_ref)
    assert np.abs(g.cg_log().astype(int) - o.cg_log().astype(int)).max() <= 1


def test_kkbox_small_fp64(kk_small):
    o, g = pair(kk_small)
    o.one_epoch()
    g.one_epoch()
    assert_state(o, g, 1e-9)
    np.testing.assert_array_equal(g.cg_log(), o.cg_log())
    vo, vg = o.validate(), g.validate()
    np.testing.assert_allclose(vg["prec"], vo["prec"], atol=1e-12)


HEAVY = dict(seed=13, m=1500, n=300, fu=2, fv=2, k=8, d_user=[1500, 3], d_item=[300, 2], nnz_user=1,
             mean_pos=12.0, vals="real")


@pytest.mark.parametrize("cgram", ["2", "0", "ccg"])
@pytest.mark.parametrize("precision", [ocffm.FP64, ocffm.FP32])
def test_heavy_columns(precision, cgram, monkeypatch):
    """Low-cardinality fields: columns with hundreds of rows go through the
    feature pass as several wave-chunks summed by the last to arrive
    (kernels.hpp: Job), in both the row and the segment CSC.  With
    OCFFM_CGRAM=2 the side halves of the one-node fields run on per-column
    Grams built from several chunks each (k_col_gram: ordered partial slots).
    "ccg": the cross halves over the one-node item fields on per-column cross
    Grams (OCFFM_CCG=2; real-valued x: weights x^2, multi-chunk columns)."""
    if cgram == "ccg":
        monkeypatch.setenv("OCFFM_CCG", "2")
    else:
        monkeypatch.setenv("OCFFM_CGRAM", cgram)
    ds = synth.general(**HEAVY)
    o, g = pair(ds, precision=precision, with_test=False)
    for e in (1, 2):
        o.one_epoch()
        g.one_epoch()
        if precision == ocffm.FP64:
            # 500-row real-valued columns make these halves worse conditioned:
            # the reference's own sums drift 1.5-3.3e-9 between thread counts
            # here (fp64_envelope.json "heavy"), the bound is 3x that
            assert_state(o, g, fp64_tol("heavy", e))
    if precision == ocffm.FP64:
        np.testing.assert_array_equal(g.cg_log(), o.cg_log())
    else:
        f_ref = o.func()
        o2 = O.Oracle(ds, with_test=False)
        ocffm.srand(1)
        o2.init()
        assert abs(gpu_objective(o2, g) - f_ref) <= 1e-3 * abs(f_ref)


@pytest.mark.parametrize("ds_name", ["heavy", "kkbox_s", "kkbox_s_cgram2", "kkbox_s_pgram2", "cfg5", "cfg5_k32",
                                     "cfg5_nomfma"])
def test_fp32_runs_bit_identical(ds_name, monkeypatch):
    """The default fp32 path has no order-dependent float sums (feature
    passes, Gram builds and grid reductions combine in a fixed order): two
    runs of the same epochs give bit-identical tables and CG logs.  "heavy"
    forces the Gram path onto multi-chunk columns (k_col_gram's partial slots)."""
    kw = {}
    if ds_name == "heavy":
        monkeypatch.setenv("OCFFM_CGRAM", "2")
        ds = synth.general(**HEAVY)
    elif ds_name.startswith("cfg5"):  # MFMA T pre-pass and KP = 64 Grams, heavy columns
        ds = synth.cfg5(m=20000, n=3000, d_user=2000, seed=3)
        kw = dict(k=32 if ds_name.endswith("k32") else 64, self_side=False)
        if ds_name.endswith("nomfma"):
            monkeypatch.setenv("OCFFM_NO_MFMA", "1")
    else:
        if ds_name.endswith("cgram2"):  # MFMA per-column Grams (k = 32), multi-chunk slot sums
            monkeypatch.setenv("OCFFM_CGRAM", "2")
        if ds_name.endswith("pgram2"):  # pair Grams on the context field's side halves
            monkeypatch.setenv("OCFFM_PGRAM", "2")
        ds = synth.kkbox(m=3000, n=4000, mean=20.0, seed=11, name="kk_det")
    runs = []
    for _ in range(2):
        g = ocffm.problem_from_dataset(ds, precision=ocffm.FP32, with_test=False, **kw)
        ocffm.srand(1)
        g.init()
        for _ in range(2):
            g.one_epoch()
        o = O.Oracle(ds, with_test=False, **kw)  # only for the block list
        runs.append(([g.get(w, b) for b in state_names(o) for w in "WH"], g.cg_log().copy()))
        g.close()
    for a, b in zip(runs[0][0], runs[1][0]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(runs[0][1], runs[1][1])


def test_speculative_update_bit_identical(monkeypatch):
    """The speculative end-of-half update (solver.hip half(): queued at the
    predicted CG count, guarded on the device by the next verdict) changes
    which kernels return at entry, never the result: predictions from the
    previous epoch, none, and fixed ones that hit, stop early and run past
    give bit-identical fp32 tables and CG logs over three epochs."""
    ds = synth.kkbox(m=3000, n=4000, mean=20.0, seed=11, name="kk_det")
    monkeypatch.setenv("OCFFM_PGRAM", "2")  # the pair-Gram halves take the speculative update too
    runs = {}
    for cfg in ({"OCFFM_SPEC": "0"}, {}, {"OCFFM_SPEC_FIXED": "1"}, {"OCFFM_SPEC_FIXED": "2"},
                {"OCFFM_SPEC_FIXED": "4"}):
        monkeypatch.delenv("OCFFM_SPEC", raising=False)
        monkeypatch.delenv("OCFFM_SPEC_FIXED", raising=False)
        for k, v in cfg.items():
            monkeypatch.setenv(k, v)
        g = ocffm.problem_from_dataset(ds, precision=ocffm.FP32, with_test=False)
        ocffm.srand(1)
        g.init()
        for _ in range(3):
            g.one_epoch()
        o = O.Oracle(ds, with_test=False)  # only for the block list
        runs[str(cfg)] = ([g.get(w, b) for b in state_names(o) for w in "WH"], g.cg_log().copy())
        g.close()
    ref = runs[str({"OCFFM_SPEC": "0"})]
    assert len(set(ref[1].tolist())) > 1  # the fixed predictions hit and miss
    for name, (tabs, cg) in runs.items():
        np.testing.assert_array_equal(cg, ref[1], err_msg=name)
        for a, b in zip(tabs, ref[0]):
            np.testing.assert_array_equal(a, b, err_msg=name)


@pytest.mark.parametrize("env", [{"OCFFM_FUSE": "0"}, {"OCFFM_SEG_LEN": "3"}, {"OCFFM_LOOKAHEAD": "3"},
                                 {"OCFFM_SEG_LEN": "2"}, {"OCFFM_CGRAM": "0"},
                                 {"OCFFM_NO_FOLD": "1"}, {"OCFFM_LAZY_BASE": "0"},
                                 {"OCFFM_SPEC_FIXED": "1"}, {"OCFFM_SPEC_FIXED": "2"}, {"OCFFM_SPEC": "0"},
                                 {"OCFFM_YSUM": "0"}, {"OCFFM_YTVIA": "0"}, {"OCFFM_HOT": "0"},
                                 {"OCFFM_HOT": "3"}, {"OCFFM_EXACT_R2": "1"}, {"OCFFM_CCG": "0"}, {"OCFFM_CCG": "2"},
                                 {"OCFFM_CGP": "0"}, {"OCFFM_PGRAM": "2"}, {"OCFFM_PGRAM": "0"},
                                 {"OCFFM_SIDE_REFRESH": "1"}, {"OCFFM_SIDE_REFRESH": "0"}, {"OCFFM_TAU_MFMA": "0"},
                                 {"OCFFM_SIDEP": "0"}, {"OCFFM_GFOLD": "0"}, {"OCFFM_SIDE_FULL": "0"},
                                 {"OCFFM_XFUSE": "0"}, {"OCFFM_XF_HOT": "8"}, {"OCFFM_XF_HOT": "100000"},
                                 {"OCFFM_XF_GB": "16"}, {"OCFFM_XF_GB": "8"}, {"OCFFM_NO_MFMA": "1", "OCFFM_XF_HOT": "8"},
                                 {"OCFFM_PGRAM": "2", "OCFFM_CGRAM": "2", "OCFFM_CCG": "2"}])
def test_execution_variants_fp64(kk_small, monkeypatch, env):
    """Schedule knobs (id-field row fusion, segment length, CG look-ahead)
    change the kernels that run, never the result."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    o, g = pair(kk_small, with_test=False)
    o.one_epoch()
    g.one_epoch()
    assert_state(o, g, 1e-9)
    np.testing.assert_array_equal(g.cg_log(), o.cg_log())


@pytest.mark.parametrize("coop", ["1", "0"])
@pytest.mark.parametrize("stall", ["0", "1", "2", "3"])
def test_persistent_cg_gives_up_and_recovers(kk_small, monkeypatch, stall, coop):
    """The persistent column-Gram CG (k_cg_cgram) forced to give up on its
    grid barrier: one block sleeps before step `stall` while the others'
    spin limit is tiny, as when other processes hold CUs.  The grid stops at
    that step with the state consistent, the update queued behind it returns
    at entry, and the host finishes the solve per step (solver.hip
    cgp_recover).  The fused id-like side halves (k_cg_side_id FULL) give up
    the same way; stall 0 is their gradient's barrier (the host then runs
    the whole CG and the update).  Two epochs (the second starts from recovered state:
    tickets, generation word, abort words) within 1e-9 of the oracle with
    identical CG counts (ffm.cpp:761-812)."""
    monkeypatch.setenv("OCFFM_CGP_SPIN", "2000")
    monkeypatch.setenv("OCFFM_CGP_STALL", stall)
    monkeypatch.setenv("OCFFM_CGP_COOP", coop)
    o, g = pair(kk_small, with_test=False)
    for _ in range(2):
        o.one_epoch()
        g.one_epoch()
        assert_state(o, g, 1e-9)
    np.testing.assert_array_equal(g.cg_log(), o.cg_log())
    launches, recovered = g.counter("cgp_launches"), g.counter("cgp_recovered")
    assert launches > 0 and g.counter("cgp_side_launches") > 0  # column-Gram and id-like side halves
    assert g.counter("cgp_side_full") > 0
    # every launch whose solve reached step `stall` gave up there
    assert recovered > 0
    assert g.counter("cgp_refused") == 0


def test_unsorted_labels():
    """Label lists in file order, not sorted (ffm.cpp:92-100 keeps them as
    written): positives, their segments and both orientations of y~ follow
    the file order (transY, ffm.cpp:259-294, sorts only by item)."""
    ds = synth.tiny(seed=9)
    rng = np.random.default_rng(1)
    t = ds.train
    for i in range(t.m):
        b, e = int(t.yptr[i]), int(t.yptr[i + 1])
        t.ycol[b:e] = rng.permutation(t.ycol[b:e])
    o, g = pair(ds)
    for _ in range(2):
        o.one_epoch()
        g.one_epoch()
    assert_state(o, g, 1e-9)
    np.testing.assert_array_equal(g.cg_log(), o.cg_log())


def test_cold_rows_and_duplicate_labels():
    ds = synth.tiny(seed=6)
    # a test row whose features are all dropped -> popularity scores
    t = ds.test
    t.idx[0] = 10_000
    t.idx[1] = 10_000
    o, g = pair(ds)
    o.one_epoch()
    g.one_epoch()
    vo, vg = o.validate(), g.validate()
    assert abs(vg["loss"] - vo["loss"]) <= 1e-9 * abs(vo["loss"])
    np.testing.assert_allclose(vg["prec"], vo["prec"], atol=1e-12)


def test_cli_matches_oracle_cli(tiny, tmp_path):
    paths = tiny.write(str(tmp_path))
    args = ["-k", "4", "-t", "10", "-p", paths["test"], "-o"]
    r1 = subprocess.run([TRAIN] + args + [str(tmp_path / "gpu.model"), paths["item"], paths["train"]],
                        capture_output=True, text=True, timeout=300)
    r2 = subprocess.run([ORACLE_TRAIN] + args + [str(tmp_path / "cpu.model"), paths["item"], paths["train"]],
                        capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stderr
    assert r2.returncode == 0, r2.stderr
    assert r1.stdout == r2.stdout
    a = open(tmp_path / "gpu.model").read().split("\n")
    b = open(tmp_path / "cpu.model").read().split("\n")
    assert len(a) == len(b)
    # The writer itself is byte-exact on identical tables
    # (test_boundary_gpu.py::test_text_model_byte_exact).  Here the tables are
    # two fp64 trainings (~1e-13 apart), so a value may round to the other
    # side of a 6th-significant-digit boundary: every token of a differing
    # line must still be the same label or a value within one unit of the
    # 6th significant digit.
    ndiff = 0
    for x, y in zip(a, b):
        if x == y:
            continue
        ndiff += 1
        tx, ty = x.split(" "), y.split(" ")
        assert len(tx) == len(ty) and tx[0] == ty[0], (x, y)
        for u, v in zip(tx[1:], ty[1:]):
            fu_, fv_ = float(u), float(v)
            assert abs(fu_ - fv_) <= 1.01e-5 * max(abs(fu_), abs(fv_)), (x, y)
    assert ndiff <= len(a) // 100


ORACLE_THREADS = 16  # the CPU share the GPU box allots one GPU


@pytest.fixture(scope="module")
def kk_full():
    # the headline set with a 1,537-row test split
    return synth.kkbox(test_frac=0.05)


def _full_pair(ds, precision):
    o = O.Oracle(ds, threads=ORACLE_THREADS)
    g = ocffm.problem_from_dataset(ds, precision=precision)
    ocffm.srand(1)
    o.init()
    ocffm.srand(1)
    g.init()
    return o, g


def test_kkbox_full_size_parity_fp64(kk_full):
    """Config 3 at its own size (30,755 users x 100,000 items, k = 32,
    2.1 M positives, l = 4, w = 2^-7): the paths that only appear there —
    the 30 k-user Pareto-head items cut into many segments and multi-chunk
    feature jobs, 8-17-step song-id halves, the gather offsets of 12.8 MB
    tables — against the oracle (ffm.cpp:852-870) on 16 threads, two fp64
    epochs from the same srand(1) init.  Every table of every block, both
    biases and both y~ orientations within max(1e-9, 3x the reference
    arithmetic's own drift at this size: the oracle at 2..16 threads against
    1 thread serial, and at 8 threads with the cblas_ddot orders of optimised
    BLAS builds, fp64_envelope.json "kkbox_full": 3.7e-9 / 8.5e-7 after
    epochs 1 / 2; the CG scalars' ddot order, which no thread count changes,
    is what the song-id and artist halves' 7-13-step solves amplify); CG
    logs identical; validate() (ffm.cpp:925-1016) on the test split after
    each epoch: loss within the same bound, p@k / nDCG@k within 1e-9 after
    epoch 1 and, after epoch 2, within two test rows' worth (2 / m_te: a
    near-tie in a top-k list may order the other way at 1e-6)."""
    o, g = _full_pair(kk_full, ocffm.FP64)
    mt = kk_full.test.m
    for e in (1, 2):
        o.one_epoch()
        g.one_epoch()
        tol = fp64_tol("kkbox_full", e)
        assert_state(o, g, tol)
        np.testing.assert_array_equal(g.cg_log(), o.cg_log())
        vo, vg = o.validate(), g.validate()
        assert abs(vg["loss"] - vo["loss"]) <= tol * abs(vo["loss"]), (e, vg["loss"], vo["loss"])
        atol = 1e-9 if e == 1 else 2.0 / mt
        np.testing.assert_allclose(vg["prec"], vo["prec"], atol=atol, err_msg=f"epoch {e}")
        np.testing.assert_allclose(vg["ndcg"], vo["ndcg"], atol=atol, err_msg=f"epoch {e}")


def test_kkbox_full_size_parity_fp32(kk_full):
    """The fp32 mode (the headline number's arithmetic) at the same size,
    two epochs, against the fp64 oracle: validation loss within 1e-3
    relative, p@k / nDCG@k within 2e-2 absolute (SURVEY §8c fp32 contract);
    CG counts within one step of the oracle's per half."""
    o, g = _full_pair(kk_full, ocffm.FP32)
    for _ in range(2):
        o.one_epoch()
        g.one_epoch()
    vo, vg = o.validate(), g.validate()
    assert abs(vg["loss"] - vo["loss"]) <= 1e-3 * abs(vo["loss"])
    np.testing.assert_allclose(vg["prec"], vo["prec"], atol=2e-2)
    np.testing.assert_allclose(vg["ndcg"], vo["ndcg"], atol=2e-2)
    assert np.abs(g.cg_log().astype(int) - o.cg_log().astype(int)).max() <= 1


@pytest.mark.parametrize("shape", ["kdd12", "outbrain"])
def test_full_size_metric_parity_fp64(shape):
    """Configs 2 and 4 at their own sizes (kdd12 500 k users x
    50 k ads, k = 16; outbrain one GPU's 250 k-row shard, 10 k ads, k = 64):
    one fp64 epoch against the oracle on 16 threads, then validate() on a
    500-row test split.  Here the reference arithmetic does not reproduce
    itself: across thread counts and cblas_ddot orders its CG counts differ
    (kdd12: in up to 6 of the 42 halves, its tables 0.4 apart,
    fp64_envelope.json "kdd12_full"; outbrain's k = 64 halves run into the
    20-step cap), so no state parity exists at these sizes.  The bound is 3x
    the spread of its own validation metrics over those runs
    (tests/golden/<shape>_full_spread.json, tools/fullsize_spread.py) plus
    one hit of one test row at each k, and the CG logs may differ in at most
    twice as many halves as two reference runs do (ffm.cpp:852-870,
    925-1016)."""
    spread = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                         f"{shape}_full_spread.json")))
    ds = getattr(synth, shape)(test_rows=500)
    o = O.Oracle(ds, threads=ORACLE_THREADS)
    g = ocffm.problem_from_dataset(ds, precision=ocffm.FP64)
    ocffm.srand(1)
    o.init()
    ocffm.srand(1)
    g.init()
    o.one_epoch()
    g.one_epoch()
    vo, vg = o.validate(), g.validate()
    assert abs(vg["loss"] - vo["loss"]) <= 3 * spread["loss_range"], (vg["loss"], vo["loss"])
    # plus one hit of one test row at each k (a range of 0 at large k over six runs)
    one = 1.0 / (ds.test.m * np.array([5, 10, 20, 40, 80]))
    np.testing.assert_array_less(np.abs(vg["prec"] - vo["prec"]), 3 * np.array(spread["prec_range"]) + one + 1e-12)
    np.testing.assert_array_less(np.abs(vg["ndcg"] - vo["ndcg"]), 3 * np.array(spread["ndcg_range"]) + 1e-12)
    cgo, cgg = o.cg_log(), g.cg_log()
    assert cgo.shape == cgg.shape and int(np.sum(cgo != cgg)) <= 2 * max(1, spread["cg_halves_differ"])


def test_kkbox_full_size_properties():
    """Config-3 size: size-independent properties after one fp32 epoch."""
    ds = synth.kkbox()
    g = ocffm.problem_from_dataset(ds, precision=ocffm.FP32, with_test=False)
    ocffm.srand(1)
    g.init()
    g.one_epoch()
    cg = g.cg_log()
    assert cg.size == 30 and cg.min() >= 1 and cg.max() <= 20
    yu, yv = g.get("u"), g.get("v")
    assert np.isfinite(yu).all()
    # both orientations of y~ hold identical values (ffm.cpp:455,462)
    assert np.array_equal(np.sort(yu), np.sort(yv))
