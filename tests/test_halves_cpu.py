"""The dense restatement of the halves (halves_ref.py) against the oracle, and
the reference-side conditions of the one-step regime (test_fp32_trained.py
4.B): CPU only.

The GPU tests bound a kernel's error by the restatement's abs-sums at a
trained state, and compare one epoch from a small state in which every half's
CG stops after one step.  Both premises are facts about the reference, so they
are checked here on every CPU run.
"""
import numpy as np
import pytest

import halves_ref as R
from halves_ref import LAMBDAS, ONE_STEP_LAMBDA, fresh_oracle, load_small_state

def oracle_halves(o, vs):
    out = {}
    for f1, f2, b12 in R.used_blocks(o.fu, o.f, o.self_side):
        for half in (0, 1):
            out[(b12, half)] = (o.grad(f1, f2, half).reshape(-1, o.k),
                                o.hv(f1, f2, half, vs[(b12, half)].ravel()).reshape(-1, o.k))
    return out


def directions(o, seed):
    rng = np.random.default_rng(seed)
    return {(b12, half): rng.standard_normal((o.get("W" if half == 0 else "H", b12).size // o.k, o.k))
            for _, _, b12 in R.used_blocks(o.fu, o.f, o.self_side) for half in (0, 1)}


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_matches_oracle(name):
    """At init and after two oracle epochs: the plain restatement equals
    o.grad / o.hv within 1e-12 of the largest entry, and the abs-sums dominate
    the values entrywise."""
    ds, o = fresh_oracle(name)
    prm = dict(k=o.k, omega=o.omega, lam=o.lam, r=o.r)
    for epochs in (0, 2):
        for _ in range(epochs):
            o.one_epoch()
        vs = directions(o, 11 + epochs)
        st = R.state_of(o, o.fu, o.f, o.k, o.self_side)
        plain = R.halves(ds, st, prm, vs=vs, self_side=o.self_side)
        absol = R.halves(ds, st, prm, vs=vs, self_side=o.self_side, absolute=True)
        ref = oracle_halves(o, vs)
        assert set(plain) == set(ref) and len(ref) == 2 * len(R.used_blocks(o.fu, o.f, o.self_side))
        for key in ref:
            for q, what in ((0, "grad"), (1, "hv")):
                x, x0, xa = plain[key][q], ref[key][q], absol[key][q]
                assert np.abs(x - x0).max() <= 1e-12 * np.abs(x0).max(), (what, key, epochs)
                # (1 + 1e-12): a row of one term has xa == |x| up to the sums' own rounding
                assert (xa * (1 + 1e-12) >= np.abs(x0)).all(), (what, key, epochs)
                assert (xa * (1 + 1e-12) >= np.abs(x)).all(), (what, key, epochs)


@pytest.mark.parametrize("name", list(R.CASES))
def test_one_step_regime_on_the_oracle(name):
    """From the small state, with the lambda the GPU test uses, every half's
    CG of one oracle epoch stops after exactly one step; with the next
    smaller lambda of the list at least one half takes more."""
    lam = ONE_STEP_LAMBDA[name]
    _, o = fresh_oracle(name, lam=lam)
    load_small_state(o)
    o.cg_log_clear()
    o.one_epoch()
    cg = o.cg_log()
    assert cg.size == 2 * len(R.used_blocks(o.fu, o.f, o.self_side))
    assert (cg == 1).all(), cg
    smaller = [x for x in LAMBDAS if x < lam]
    if smaller:
        _, o = fresh_oracle(name, lam=smaller[-1])
        load_small_state(o)
        o.cg_log_clear()
        o.one_epoch()
        assert (o.cg_log() != 1).any()
