"""The fold-in's closed form against a brute-force weighted least squares
(tests/fold_ref.py): numpy only, no GPU."""
import numpy as np
import pytest

from fold_ref import fold_brute, fold_objective, fold_reference, normal_equations

N, K, FU = 70, 8, 2
OMEGA, LAM, R = 0.1, 0.1, -1.0


def tables(fv, seed):
    rng = np.random.default_rng(seed)
    C = FU * fv
    Qs = [rng.normal(0, 0.3, size=(N, K)) for _ in range(C)]
    b = rng.normal(0, 0.2, size=N)
    P = rng.normal(0, 0.3, size=(C, K))
    a = float(rng.normal(0, 0.2))
    return Qs, b, P, a


def histories():
    rng = np.random.default_rng(3)
    return {
        "empty": [],
        "one": [41],
        "seventeen": list(rng.choice(N, size=17, replace=False)),
        "all": list(range(N)),
        "repeat": [5, 9, 5, 33, 9],
        "beyond": [2, N, 10 * N, 17],
        "only_beyond": [N + 1],
    }


@pytest.mark.parametrize("fv", [1, 2])
@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("name", list(histories()))
def test_closed_form_is_the_least_squares(fv, field, name):
    Qs, b, P, a = tables(fv, 10 * fv + field)
    hist = histories()[name]
    args = (Qs, b, P, a, hist, field, fv, K, OMEGA, LAM, R)
    ref, brute = fold_reference(*args), fold_brute(*args)
    assert ref.shape == (fv * K,)
    err = np.abs(ref - brute).max()
    print(f"fv {fv} field {field} {name}: |ref - brute| {err:.2e}")
    assert err <= 1e-12
    A, _, H = normal_equations(*args)
    assert len(H) == len({j for j in hist if j < N})
    assert np.linalg.cond(A) <= 1e4
    if len(H) == 0:
        assert (ref == 0).all()
    else:
        assert fold_objective(ref, *args) < fold_objective(np.zeros(fv * K), *args)


def test_fold_entries_are_declared_and_exported():
    """The fold entries live in include/ocffm_fold.h, which ocffm.h includes;
    the library exports every one and ocffm.FOLD_EXPORTS lists them."""
    import ctypes
    import os
    import re

    import ocffm

    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    syms = sorted(set(re.findall(r"\b(ocffm_[a-z_0-9]+)\s*\(", open(os.path.join(inc, "ocffm_fold.h")).read())))
    assert syms == sorted(ocffm.FOLD_EXPORTS) and len(syms) == 4
    assert '#include "ocffm_fold.h"' in open(os.path.join(inc, "ocffm.h")).read()
    lib = ctypes.CDLL(ocffm.LIB_PATH)
    assert all(hasattr(lib, s) for s in syms)
    assert not set(syms) & set(ocffm.EXPORTS)
