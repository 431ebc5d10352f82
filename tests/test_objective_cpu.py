"""The objective's ABI surface and its closed form, without a GPU.

The closed-form combination of DESIGN §12 (Gram form and augmented form) is
pinned against the oracle's func() (ffm.cpp:1321-1351) independently of any
kernel; tests/test_objective.py then holds the kernels to the same numbers.
"""
import ctypes as C

import numpy as np
import pytest

import objective_ref as R
import ocffm
import oracle_lib as O
import synth


def test_library_exports_the_entry_points():
    L = ocffm.lib()
    for sym in ("ocffm_problem_objective", "ocffm_problem_solve_ex"):
        assert sym in ocffm.EXPORTS
        getattr(L, sym)


def test_null_arguments():
    L = ocffm.lib()
    ob = ocffm._Objective()
    assert L.ocffm_problem_objective(None, C.byref(ob)) == ocffm.E_ARG
    assert L.ocffm_problem_objective(None, None) == ocffm.E_ARG
    assert L.ocffm_problem_solve_ex(None, None, None) == ocffm.E_ARG
    opts = ocffm._SolveOpts(1, 0.0, 0)
    assert L.ocffm_problem_solve_ex(None, C.byref(opts), None) == ocffm.E_ARG


def test_struct_layouts():
    assert C.sizeof(ocffm._Objective) == 8 * 8
    assert C.sizeof(ocffm._SolveOpts) == 24 and ocffm._SolveOpts.tol.offset == 8
    assert C.sizeof(ocffm._SolveReport) == 24 and ocffm._SolveReport.objective0.offset == 8


@pytest.mark.parametrize("epochs", [0, 2])
@pytest.mark.parametrize("self_side", [True, False])
def test_closed_form_is_func(self_side, epochs):
    ds = synth.general(seed=5, m=60, n=40, fu=2, fv=2, k=5, nnz_user=2, mean_pos=3.0, vals="real")
    o = O.Oracle(ds, self_side=self_side, with_test=False)
    O.lib().orc_srand(1)
    o.init()
    for _ in range(epochs):
        o.one_epoch()
    want = o.func()
    args = (o.get, ds, o.f, o.fu, o.k, o.omega, o.r, o.lam, self_side)
    brute = R.terms(*args)["value"]
    gram = R.closed_form(*args)
    aug = R.closed_form(*args, augmented=True)
    for got in (brute, gram, aug):
        assert abs(got - want) <= 1e-12 * abs(want), (got, want)


def test_closed_form_without_cross_blocks():
    """C = 0: only n sum alpha^2 + m sum b^2 + 2 sum alpha sum b remains."""
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal(13), rng.standard_normal(9)
    P, Q = np.zeros((13, 0)), np.zeros((9, 0))
    brute = float(((a[:, None] + b[None, :] + 0.7) ** 2).sum())
    assert abs(R.all_gram(P, Q, a, b, -0.7) - brute) <= 1e-12 * brute
    assert abs(R.all_augmented(P, Q, a, b, -0.7) - brute) <= 1e-12 * brute
