"""The id-field kernels on permuted ids, capped resident grids and the paths
chosen from the previous epoch's CG counts.

An id-like field has one node per row and every feature in exactly one row.
Every other input of the suite builds such a field as (fid, row, 1.0): column
== row and x == x^2 == 1, so a kernel that indexes a table by the row where
it needs the column, drops x, or takes x for x^2 passes there.  synth.kkbox_perm
shuffles both id fields and gives their nodes real values; its sizes (1,500
users, 2,500 items) are no multiple of a block's rows.

The knobs (read at create; DESIGN.md's knob list):
  OCFFM_NCU=n        plan as on a device of n CUs: every resident() cap and
                     k_cg_cgram's grid bound shrink, so blocks loop over rows,
                     segments and feature jobs, and tickets see fewer blocks
                     than jobs, at 1,500 rows;
  OCFFM_SIDEP_SM=2|4 k_cg_side_id with 2 / 4 rows per subgroup (ragged last
                     block, empty blocks of the XCD-rounded grid, multi-slot
                     write-back after a give-up);
  OCFFM_*_BLOCKS     the fixed grid caps.
Every case asserts through ocffm_problem_counter that it reached its path.

Bounds: fp64 state within fp64_tol (1e-9: the oracle's own drift on this set
is <= 4e-10 over three epochs at k = 5 / 32 / 64 / 128, fp64_envelope.json
"kkbox_perm*"), CG logs identical; fp32 per-half gradients and Hessian-vector
products within 1e-4 of their largest entry, fp32 epochs within the suite's
1e-3 objective contract.
"""
import numpy as np
import pytest

import ocffm
import oracle_lib as O
import synth
from test_gpu_parity import assert_state, fp64_tol, gpu_objective, rel, state_names

pytestmark = pytest.mark.gpu

CAPS = {"NCU": "1", "HS_BLOCKS": "2", "FEAT_BLOCKS": "3", "GD_BLOCKS": "2", "GRAM_BLOCKS": "2"}

_DS = []


def perm_ds():
    if not _DS:
        _DS.append(synth.kkbox_perm())
    return _DS[0]


def env_id(env):
    return "-".join(f"{k}={v}" for k, v in env.items()) or "default"


def set_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv("OCFFM_" + k, v)


class Snap:
    """An oracle's state (what assert_state reads), frozen after an epoch."""

    def __init__(self, o, objective):
        self.f, self.fu, self.self_side = o.f, o.fu, o.self_side
        self.tabs = {(w, b): o.get(w, b) for b in state_names(o) for w in "WHPQ"}
        self.tabs.update({(w, 0): o.get(w) for w in "abuv"})
        self.cg = o.cg_log().copy()
        self.val = o.validate()
        self.func = o.func() if objective else None  # (seconds at k = 128: only where a test reads it)

    def get(self, what, b12=0):
        return self.tabs[(what, b12)]


_EPOCH_REFS = {}


def epoch_refs(k, epochs):
    """The 1-thread oracle's state after each of `epochs` epochs on kkbox_perm
    at rank k, computed once per k."""
    if k not in _EPOCH_REFS or len(_EPOCH_REFS[k]) < epochs:
        o = O.Oracle(perm_ds(), k=k)
        ocffm.srand(1)
        o.init()
        snaps = []
        for _ in range(epochs):
            o.one_epoch()
            snaps.append(Snap(o, objective=k == 32 and len(snaps) == 1))  # test_perm_epochs_fp32: epoch 2
        _EPOCH_REFS[k] = snaps
    return _EPOCH_REFS[k]


def gpu_problem(precision, k=32):
    g = ocffm.problem_from_dataset(perm_ds(), precision=precision, k=k)
    ocffm.srand(1)
    g.init()
    return g


def check_epochs_fp64(monkeypatch, env, k, epochs, name, covered):
    set_env(monkeypatch, env)
    refs = epoch_refs(k, epochs)
    g = gpu_problem(ocffm.FP64, k)
    for e in range(1, epochs + 1):
        g.one_epoch()
        assert_state(refs[e - 1], g, fp64_tol(name, e))
    last = refs[epochs - 1]
    np.testing.assert_array_equal(g.cg_log(), last.cg)
    vg = g.validate()
    assert abs(vg["loss"] - last.val["loss"]) <= fp64_tol(name, epochs) * abs(last.val["loss"])
    np.testing.assert_allclose(vg["ndcg"], last.val["ndcg"], atol=1e-12)
    c = g.counter
    print(env_id(env), {n: c(n) for n in COUNTERS})
    for what, ok in covered(c).items():
        assert ok, (what, {n: c(n) for n in COUNTERS})
    g.close()


COUNTERS = ("cgp_launches", "cgp_side_launches", "cgp_side_full", "cgp_side_sm1", "cgp_side_sm2", "cgp_side_sm4",
            "cgp_side_res_sm1", "cgp_side_res_sm2", "cgp_side_res_sm4", "cgp_recovered", "cgp_refused", "xfuse_steps",
            "xfuse_strided", "ccg_halves", "hot_halves", "capped_launches")


def nothing(c):
    return {}


def sm(n, full=True):
    def covered(c):
        out = {f"sm{n}": c(f"cgp_side_sm{n}") > 0}
        if not full:
            out["not full"] = c("cgp_side_full") == 0
        return out
    return covered


def gave_up(n):
    def covered(c):
        return {f"sm{n}": c(f"cgp_side_sm{n}") > 0, "recovered": c("cgp_recovered") > 0,
                "refused": c("cgp_refused") == 0}
    return covered


EPOCH_CASES = [
    # the default selection: a column-Gram cross half (epoch 4), hot rows'
    # Grams read by the fused id-field cross steps, the id-like side halves
    # whole in one launch
    ({}, lambda c: {n: c(n) > 0 for n in ("ccg_halves", "hot_halves", "xfuse_steps", "cgp_side_full")}),
    ({"SIDEP_SM": "2"}, sm(2)),
    ({"SIDEP_SM": "4"}, sm(4)),
    ({"SIDEP_SM": "4", "SIDE_FULL": "0"}, sm(4, full=False)),
    ({"NCU": "1"}, lambda c: {n: c(n) > 0 for n in ("xfuse_strided", "capped_launches")}),
    # k_cg_cgram on genre (D = 50) and artist (D = 125) at a grid that is no whole round of the XCDs
    ({"NCU": "4"}, lambda c: {"column-Gram persistent CG": c("cgp_launches") - c("cgp_side_launches") > 0}),
    (CAPS, lambda c: {"capped": c("capped_launches") > 0}),
    # k_hs_cross_seg and the feature pass, capped
    ({"NCU": "1", "XFUSE": "0"}, lambda c: {"capped": c("capped_launches") > 0, "no xfuse": c("xfuse_steps") == 0}),
    # k_hs_side_row FZ, capped
    ({"NCU": "1", "SIDEP": "0"}, lambda c: {"capped": c("capped_launches") > 0,
                                            "no persistent side": c("cgp_side_launches") == 0}),
    ({"FUSE": "0"}, nothing),
    ({"NO_FOLD": "1"}, nothing),
    ({"GFOLD": "0"}, nothing),
    ({"XF_HOT": "8"}, nothing),
    ({"XF_GB": "8"}, lambda c: {"xfuse": c("xfuse_steps") > 0}),
    ({"HOT": "2"}, lambda c: {"hot": c("hot_halves") > 0}),
    ({"CCG": "2", "CGRAM": "2"}, lambda c: {"ccg": c("ccg_halves") > 0}),
    # the give-up of test_persistent_cg_gives_up_and_recovers with several
    # slots per subgroup: the write-back and the host continuation cover them
    ({"SIDEP_SM": "2", "CGP_SPIN": "2000", "CGP_STALL": "1"}, gave_up(2)),
    ({"SIDEP_SM": "4", "CGP_SPIN": "2000", "CGP_STALL": "0"}, gave_up(4)),
]


@pytest.mark.parametrize("env,covered", EPOCH_CASES, ids=[env_id(e) for e, _ in EPOCH_CASES])
def test_perm_epochs_fp64(monkeypatch, env, covered):
    """Three fp64 epochs on kkbox_perm under each knob: every table, both
    biases and both y~ orientations within fp64_tol after each epoch, CG logs
    identical, validate() loss within the same bound and nDCG within 1e-12;
    and the counters show that the knob's path ran.

    The default case runs a fourth epoch: half() puts a cross half on
    per-column Grams where the same half took >= 3 CG steps in the epoch
    before, and the first artist / genre cross half to do so on this set is
    block (1, 3)'s H half in epoch 3 (8 steps; 2 before), so the default
    selection reaches that path in epoch 4."""
    check_epochs_fp64(monkeypatch, env, 32, 3 if env else 4, "kkbox_perm", covered)


K_CASES = [
    (5, {"SIDEP_SM": "4"}, sm(4)),  # padded rows, KP = 8
    (64, {"SIDEP_SM": "2"}, sm(2)),
    # 16 lanes per row, k_hv_cross_id at its KP limit
    (64, {"NCU": "1"}, lambda c: {n: c(n) > 0 for n in ("xfuse_strided", "capped_launches")}),
    # kp > 64: no fused cross steps, the per-step path on permuted ids
    (128, {}, lambda c: {"no xfuse": c("xfuse_steps") == 0}),
]


@pytest.mark.parametrize("k,env,covered", K_CASES, ids=[f"k={k}-{env_id(e)}" for k, e, _ in K_CASES])
def test_perm_k_variants_fp64(monkeypatch, k, env, covered):
    """Two fp64 epochs on kkbox_perm at other ranks, same assertions."""
    check_epochs_fp64(monkeypatch, env, k, 2, f"kkbox_perm_k{k}", covered)


# ---------------------------------------------------------------- per half
_HALF_REFS = {}


def half_refs(state, tmp_dir):
    """Per half of kkbox_perm, from the 1-thread fp64 oracle: (f1, f2, half,
    gradient, v, Hessian-vector product, fp64 bound), at the init state or
    after two epochs ("trained": the state is also written with save_binary,
    for the GPU problem to load).  The fp64 bound at the trained state is
    max(1e-12, 3 x the difference of that half's gradient between the oracle
    trained on 16 threads and on 1): what the reference's own arithmetic
    leaves undetermined there."""
    if state not in _HALF_REFS:
        ds = perm_ds()

        def oracle(threads):
            o = O.Oracle(ds, threads=threads, with_test=False)
            ocffm.srand(1)
            o.init()
            if state == "trained":
                o.one_epoch()
                o.one_epoch()
            return o

        def halves(o):
            return [(f1, f2, half) for f1 in range(o.f) for f2 in range(f1, o.f) for half in (0, 1)]

        # The oracle's thread count is the process's (omp_set_num_threads at
        # create) while its per-thread buffers are sized by its own: two
        # oracles of different counts must not be alive together.  So the
        # 16-thread one first, and gone before the 1-thread checker exists.
        G16 = {}
        if state == "trained":
            o = oracle(16)
            G16 = {hh: o.grad(*hh) for hh in halves(o)}
            del o
        o = oracle(1)
        path = None
        if state == "trained":
            path = str(tmp_dir / "kkbox_perm_trained.bin")
            o.save_binary(path)
        rng = np.random.default_rng(3)
        refs = []
        for f1, f2, half in halves(o):
            G0 = o.grad(f1, f2, half)
            v = rng.standard_normal(G0.size)
            tol64 = 1e-12
            if state == "trained":
                tol64 = max(1e-12, 3.0 * rel(G16[(f1, f2, half)], G0))
            refs.append((f1, f2, half, G0, v, o.hv(f1, f2, half, v), tol64))
        _HALF_REFS[state] = (path, refs)
    return _HALF_REFS[state]


@pytest.fixture(scope="module")
def snap_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("idfield")


def check_halves(monkeypatch, env, state, precision, snap_dir):
    path, refs = half_refs(state, snap_dir)
    set_env(monkeypatch, env)
    g = ocffm.problem_from_dataset(perm_ds(), precision=precision, with_test=False)
    if state == "trained":
        g.load_binary(path)  # re-derives P, Q, the biases, sa / sb and y~ from W and H
    else:
        ocffm.srand(1)
        g.init()
    worst = {"grad": 0.0, "hv": 0.0}
    for f1, f2, half, G0, v, H0, tol64 in refs:
        tol = 1e-4 if precision == ocffm.FP32 else tol64
        dg = rel(g.grad(f1, f2, half), G0)
        dh = rel(g.hv(f1, f2, half, v), H0)
        worst = {"grad": max(worst["grad"], dg), "hv": max(worst["hv"], dh)}
        assert dg <= tol, ("grad", f1, f2, half, dg, tol)
        assert dh <= tol, ("hv", f1, f2, half, dh, tol)
    print(state, env_id(env), worst, "capped", g.counter("capped_launches"))
    if "NCU" in env:
        assert g.counter("capped_launches") > 0
    g.close()


HALF_ENVS_FP32 = [{}, {"NO_MFMA": "1"}, {"TPRE": "1"}, {"HOT": "2"}, {"CCG": "2"}, {"XFUSE": "0"}, {"TAU_MFMA": "0"},
                  {"NCU": "1"}, CAPS]
HALF_ENVS_FP64 = [{}, {"NCU": "1"}, {"XF_GB": "8"}]


def half_cases(envs):
    return [pytest.param(s, e, id=f"{s}-{env_id(e)}") for s in ("init", "trained") for e in envs]


@pytest.mark.parametrize("state,env", half_cases(HALF_ENVS_FP32))
def test_perm_halves_fp32(monkeypatch, state, env, snap_dir):
    """Every half's gradient and Hessian-vector product in fp32 against the
    fp64 oracle within 1e-4 of the largest entry, at the init state (a = b =
    0) and at a trained one (two oracle epochs, loaded from its snapshot;
    rounding W and H to fp32 alone moves the oracle's own gradients there by
    <= 1.2e-6 and its Hessian-vector products by <= 7e-8 of their largest
    entry, so 1e-4 keeps its meaning)."""
    check_halves(monkeypatch, env, state, ocffm.FP32, snap_dir)


@pytest.mark.parametrize("state,env", half_cases(HALF_ENVS_FP64))
def test_perm_halves_fp64(monkeypatch, state, env, snap_dir):
    """The fp64 twin: within 1e-12 at init; at the trained state within
    max(1e-12, 3 x the oracle's own 16-thread against 1-thread difference of
    that half's gradient)."""
    check_halves(monkeypatch, env, state, ocffm.FP64, snap_dir)


# ---------------------------------------------------------------- fp32 epochs
FP32_CASES = [({}, nothing), ({"SIDEP_SM": "2"}, sm(2)), ({"SIDEP_SM": "4"}, sm(4)),
              (CAPS, lambda c: {"capped": c("capped_launches") > 0})]


@pytest.mark.parametrize("env,covered", FP32_CASES, ids=[env_id(e) for e, _ in FP32_CASES])
def test_perm_epochs_fp32(monkeypatch, env, covered):
    """Two fp32 epochs: the objective of the fp32 state (evaluated in fp64)
    within 1e-3 of the oracle's and CG counts within 1 per half; and the
    cached state against the model's own tables: P and Q of every block
    within 1e-5 of the largest entry of the tables an oracle derives from the
    GPU's W and H, both y~ orientations holding the same values."""
    set_env(monkeypatch, env)
    ref = epoch_refs(32, 2)[1]
    g = gpu_problem(ocffm.FP32)
    g.one_epoch()
    g.one_epoch()
    o2 = O.Oracle(perm_ds())
    ocffm.srand(1)
    o2.init()
    f32obj = gpu_objective(o2, g)  # leaves o2 on the GPU's W / H, refreshed
    print(env_id(env), "objective", f32obj, ref.func, {n: g.counter(n) for n in COUNTERS})
    assert abs(f32obj - ref.func) <= 1e-3 * abs(ref.func)
    assert np.abs(g.cg_log().astype(int) - ref.cg.astype(int)).max() <= 1
    for b12 in state_names(o2):
        for what in "PQ":
            d = rel(g.get(what, b12), o2.get(what, b12))
            assert d <= 1e-5, (what, b12, d)
    assert np.array_equal(np.sort(g.get("u")), np.sort(g.get("v")))
    c = g.counter
    for what, ok in covered(c).items():
        assert ok, (what, {n: c(n) for n in COUNTERS})
    g.close()


@pytest.mark.parametrize("env", [CAPS, {"SIDEP_SM": "4"}], ids=env_id)
def test_perm_fp32_bit_identical(monkeypatch, env):
    """No order-dependent float sums where blocks loop and tickets see fewer
    blocks than jobs: two runs of two fp32 epochs give bit-identical tables
    and CG logs.  (Different caps need not agree with each other: their
    partial counts differ.)"""
    set_env(monkeypatch, env)
    names = state_names(epoch_refs(32, 2)[0])
    runs = []
    for _ in range(2):
        g = gpu_problem(ocffm.FP32)
        g.one_epoch()
        g.one_epoch()
        runs.append(([g.get(w, b) for b in names for w in "WH"], g.cg_log().copy()))
        g.close()
    for a, b in zip(runs[0][0], runs[1][0]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
