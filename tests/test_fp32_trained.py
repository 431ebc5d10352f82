"""Halves and cached tables at trained states, at every padded k but 32, and
the in-epoch passes step by step -- both precisions.

A. Two epochs from init on the small shapes of halves_ref.CASES.  After each,
   the GPU's W / H go into a fresh oracle (set + refresh): that oracle then
   holds the fp64 definition of every cached quantity at the GPU's own W / H.
   * cache coherence: P, Q of every used block, a, b, s, t and both y~
     orientations against it, within 1e-4 (fp32: the per-kernel contract) or
     1e-11 (fp64) of the larger of the reference's largest entry before and
     after the epoch (the tables are updated in place, an update rounds
     relative to the value it started from; at most 2 x 42 updates per epoch
     at 2^-24 each, 5e-6, leave a factor of 20).
   * every half's gradient and Hessian-vector product after the second epoch,
     per feature row d within tol x max_c G_abs[d, c] (Hv_abs likewise), the
     abs-sums of halves_ref at that state; tol = 1e-4 (fp32) / 1e-12 (fp64).
     This is the forward bound n u sum|terms|: the longest sum here is a heavy
     column's positives plus the C k products of y~, under 1,600 terms, and
     1,600 x 2^-24 < 1e-4, while one dropped or doubled term is at least
     1 / 1,600 of its row's scale.  At a trained state the terms cancel (the
     abs-sum is 20 to 900 times the gradient's largest entry), so "1e-4 of the
     largest entry" cannot hold there, and the scale is taken per row: a
     table-wide maximum would hide the light rows.
   * the same halves check at init and at a trained state (two oracle epochs,
     loaded from its binary snapshot) under the kernel-selection knobs that
     otherwise run at KP = 32 only.

B. One epoch from a small state (W, H = float32(2^-7 N(0, 1))) at a lambda at
   which every half's CG stops after one step, on the oracle (asserted, here
   and in test_halves_cpu.py) and on the GPU.  A half's update is then
   -alpha G with G the in-epoch gradient (BM_ENTER / BM_IN forms, block-
   excluded base, dxs, perm) and alpha = g^2 / g'Hg: no CG iteration amplifies
   fp32 noise, so the tables after the epoch are held to 1e-4 (fp32) / 1e-9
   (fp64) of their largest reference entry, then the cache coherence of A.

Measured worst ratios to the bounds: DESIGN.md §4.
"""
import tempfile

import numpy as np
import pytest

import halves_ref as R
import ocffm

pytestmark = pytest.mark.gpu

PREC = [pytest.param(ocffm.FP32, id="fp32"), pytest.param(ocffm.FP64, id="fp64")]
#                 caches  halves (row-wise)  halves at init (largest entry)  tables after the one-step epoch
TOL = {ocffm.FP32: dict(cache=1e-4, rows=1e-4, init=1e-4, state=1e-4),
       ocffm.FP64: dict(cache=1e-11, rows=1e-12, init=1e-12, state=1e-9)}


def blocks_of(o):
    return R.used_blocks(o.fu, o.f, o.self_side)


def cached(src, o):
    """{name: array} of every cached quantity (s, t only with side halves:
    under --ns neither side refreshes them after init)."""
    out = {}
    for _, _, b12 in blocks_of(o):
        for what in "PQ":
            out[f"{what}{b12}"] = src.get(what, b12)
    for what in "ab" + ("st" if o.self_side else "") + "uv":
        out[what] = src.get(what)
    return out


def scales(tabs):
    return {name: float(np.abs(x).max()) if x.size else 0.0 for name, x in tabs.items()}


def mirror(o2, g):
    """The fp64 definition of every cached quantity at the GPU's own W / H."""
    for _, _, b12 in blocks_of(o2):
        o2.set("W", b12, g.get("W", b12))
        o2.set("H", b12, g.get("H", b12))
    o2.refresh()


def check_caches(g, o2, before, tol, label):
    """g's cached tables against o2's; returns o2's scales (the next `before`)."""
    ref = cached(o2, o2)
    after = scales(ref)
    got = cached(g, o2)
    worst = (0.0, "")
    for name, x0 in ref.items():
        x = got[name]
        assert x.shape == x0.shape, (label, name)
        bound = tol * max(before[name], after[name])
        d = float(np.abs(x - x0).max()) if x0.size else 0.0
        if d > 0 and (bound == 0 or d / bound > worst[0]):
            worst = (d / bound if bound > 0 else np.inf, name)
        assert d <= bound, (label, name, d, bound)
    np.testing.assert_array_equal(np.sort(got["u"]), np.sort(got["v"]))
    print(f"[{label}] caches: worst ratio to the bound {worst[0]:.3g} ({worst[1]})")
    return after


def check_halves(g, o2, ds, tol_rows, tol_max, label, seed=21):
    """Every half's g.grad / g.hv against o2's: per feature row within
    tol_rows x the row's largest abs-sum; with tol_max also within tol_max of
    the reference's largest entry."""
    k = o2.k
    rng = np.random.default_rng(seed)
    vs = {(b12, half): rng.standard_normal((o2.get("W" if half == 0 else "H", b12).size // k, k))
          for _, _, b12 in blocks_of(o2) for half in (0, 1)}
    absol = R.halves(ds, R.state_of(o2, o2.fu, o2.f, k, o2.self_side), dict(k=k, omega=o2.omega, lam=o2.lam, r=o2.r),
                     vs=vs, absolute=True, self_side=o2.self_side)
    worst = {"grad": (0.0, None), "hv": (0.0, None)}
    fails = []
    for f1, f2, b12 in blocks_of(o2):
        for half in (0, 1):
            v = vs[(b12, half)]
            pairs = (("grad", g.grad(f1, f2, half), o2.grad(f1, f2, half), absol[(b12, half)][0]),
                     ("hv", g.hv(f1, f2, half, v.ravel()), o2.hv(f1, f2, half, v.ravel()), absol[(b12, half)][1]))
            for what, x, x0, xa in pairs:
                d = np.abs(x.reshape(-1, k) - x0.reshape(-1, k)).max(1)
                bound = tol_rows * xa.max(1)
                # a row whose terms are all zero (bound 0) must come out exactly
                ratio = float(np.where(bound > 0, d / np.maximum(bound, 1e-300), np.where(d > 0, np.inf, 0.0)).max())
                if ratio > worst[what][0]:
                    worst[what] = (ratio, (f1, f2, half))
                if ratio > 1:
                    fails.append((what, f1, f2, half, ratio))
                if tol_max is not None:
                    dm = float(d.max() / np.abs(x0).max())
                    if dm > tol_max:
                        fails.append((what + " (largest entry)", f1, f2, half, dm / tol_max))
    print(f"[{label}] halves: worst ratio to the row-wise bound: grad {worst['grad'][0]:.3g} {worst['grad'][1]}, "
          f"hv {worst['hv'][0]:.3g} {worst['hv'][1]}")
    assert not fails, (label, fails)


def gpu_at_init(ds, kw, precision, **over):
    g = ocffm.problem_from_dataset(ds, precision=precision, **dict(kw, **over))
    ocffm.srand(1)
    g.init()
    return g


# --------------------------------------------------------------------- A ---
@pytest.mark.parametrize("precision", PREC)
@pytest.mark.parametrize("name", list(R.CASES))
def test_trained_state(name, precision):
    """Two epochs from init: cache coherence after each, every half's
    gradient and Hessian-vector product after the second."""
    tol = TOL[precision]
    ds, kw = R.make_case(name)
    g = gpu_at_init(ds, kw, precision)
    _, o2 = R.fresh_oracle(name)  # the same init draw: the reference before epoch 1
    before = scales(cached(o2, o2))
    for e in (1, 2):
        g.one_epoch()
        mirror(o2, g)
        before = check_caches(g, o2, before, tol["cache"], f"{name} epoch {e}")
    check_halves(g, o2, ds, tol["rows"], None, f"{name} trained")
    g.close()


_TRAINED = {}


def trained_snapshot(name):
    """Binary snapshot (the reference's layout) of two oracle epochs, once per case."""
    if name not in _TRAINED:
        _, o = R.fresh_oracle(name)
        o.one_epoch()
        o.one_epoch()
        with tempfile.NamedTemporaryFile(suffix=".bin") as fh:
            o.save_binary(fh.name)
            _TRAINED[name] = open(fh.name, "rb").read()
    return _TRAINED[name]


ENV_CASES = [("outbrain_k64", {"OCFFM_NO_MFMA": "1"}), ("kdd12_k16", {"OCFFM_CGRAM": "2"}),
             ("outbrain_k64", {"OCFFM_CGRAM": "2"}), ("kdd12_k16", {"OCFFM_CCG": "2"}),
             ("outbrain_k64", {"OCFFM_CCG": "2"})]


@pytest.mark.parametrize("precision", PREC)
@pytest.mark.parametrize("name,env", ENV_CASES, ids=[f"{n}-{k[6:]}={v}" for n, e in ENV_CASES for k, v in e.items()])
def test_halves_kernel_selection(name, env, precision, monkeypatch, tmp_path):
    """The VALU builds (OCFFM_NO_MFMA=1) and the column-Gram builds of the
    side halves (OCFFM_CGRAM=2) and cross halves (OCFFM_CCG=2) at KP = 16 and
    64: every half at init (the largest-entry contract and the row-wise
    bound) and at a trained state (two oracle epochs, loaded from its binary
    snapshot; the reference at the GPU's own rounding of it)."""
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    tol = TOL[precision]
    ds, kw = R.make_case(name)
    label = f"{name} {env}"
    g = gpu_at_init(ds, kw, precision)
    g.set_profiling(True)
    _, o2 = R.fresh_oracle(name)
    mirror(o2, g)  # fp32 holds the init draw rounded
    check_halves(g, o2, ds, tol["rows"], tol["init"], label + " init")
    path = tmp_path / "trained.bin"
    path.write_bytes(trained_snapshot(name))
    g.load_binary(str(path))
    mirror(o2, g)
    check_halves(g, o2, ds, tol["rows"], None, label + " trained")
    # the knob reached these halves: the column-Gram builds and steps ran
    # (objective() collects the launches the debug entries queued)
    g.objective()
    ran = {kn for kn, st in g.kernel_stats().items() if st["launches"] > 0}
    print(f"[{label}] kernels: {sorted(ran)}")
    for key, need in (("OCFFM_CGRAM", {"col_gram", "hv_cgram"}), ("OCFFM_CCG", {"ccg_build", "hv_cgram"})):
        if key in env:
            assert need <= ran, (label, sorted(ran))
    g.close()


# --------------------------------------------------------------------- B ---
@pytest.mark.parametrize("precision", PREC)
@pytest.mark.parametrize("name", list(R.CASES))
def test_one_step_epoch(name, precision, tmp_path):
    """One epoch from the small state at halves_ref.ONE_STEP_LAMBDA: one CG
    step per half on both sides, every table within 1e-4 / 1e-9 of the
    oracle's largest entry, then the caches against their definition."""
    tol = TOL[precision]
    lam = R.ONE_STEP_LAMBDA[name]
    ds, kw = R.make_case(name)
    _, o = R.fresh_oracle(name, lam=lam)
    tabs0 = R.load_small_state(o)
    path = str(tmp_path / "small.bin")
    o.save_binary(path)
    g = gpu_at_init(ds, kw, precision, lam=lam)
    g.load_binary(path)  # W / H and everything derived from them, as init() derives it
    for (what, b12), x in tabs0.items():
        np.testing.assert_array_equal(g.get(what, b12), x)
    before = scales(cached(o, o))
    nhalves = 2 * len(blocks_of(o))
    o.cg_log_clear()
    o.one_epoch()
    cg_ref = o.cg_log()
    assert cg_ref.size == nhalves and (cg_ref == 1).all(), cg_ref
    g.one_epoch()
    cg = g.cg_log()[-nhalves:]
    assert cg.size == nhalves and (cg == 1).all(), cg
    worst = (0.0, "")
    moved = []
    for (what, b12), x0 in tabs0.items():
        ref, got = o.get(what, b12), g.get(what, b12)
        top = np.abs(ref).max()
        moved.append(top / np.abs(x0).max())
        d = float(np.abs(got - ref).max() / top)
        if d / tol["state"] > worst[0]:
            worst = (d / tol["state"], f"{what}{b12}")
        assert d <= tol["state"], (name, what, b12, d)
    print(f"[{name} lambda {lam}] tables after one epoch: worst ratio to the bound {worst[0]:.3g} ({worst[1]}); "
          f"max|W_new| / max|W0| per table {min(moved):.3g} .. {max(moved):.3g}")
    _, o2 = R.fresh_oracle(name, lam=lam)
    mirror(o2, g)
    check_caches(g, o2, before, tol["cache"], f"{name} one-step epoch")
    g.close()
