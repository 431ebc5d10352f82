"""The SGD trainer's serving entries without a GPU: the symbols are exported
and declared, and a NULL trainer is an argument error before any HIP call."""
import ctypes as C
import os

import numpy as np

import ocffm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ocffm_sgd_recommend", "ocffm_sgd_label_ranks", "ocffm_sgd_evaluate", "ocffm_sgd_counter")


def test_symbols_exported_and_declared():
    lib = ocffm.lib()
    header = open(os.path.join(REPO, "include", "ocffm.h")).read()
    for name in NAMES:
        assert name in ocffm.EXPORTS
        assert getattr(lib, name) is not None
        assert f"int {name}(ocffm_sgd *s," in header
    for meth in ("recommend", "label_ranks", "evaluate", "counter"):
        assert callable(getattr(ocffm.SgdTrainer, meth))


def test_null_trainer_is_an_argument_error():
    lib = ocffm.lib()
    items = np.zeros(4, np.uint32)
    cuts = np.array([5], np.uint32)
    ev = ocffm._Eval()
    val = C.c_int64(7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.ocffm_sgd_recommend(None, None, 0, 1, 4, 0, p(items), None) == ocffm.E_ARG
    assert b"null SGD trainer" in lib.ocffm_last_error()
    assert lib.ocffm_sgd_label_ranks(None, None, None, p(items), None, None) == ocffm.E_ARG
    assert lib.ocffm_sgd_evaluate(None, None, None, p(cuts), 1, C.byref(ev)) == ocffm.E_ARG
    assert lib.ocffm_sgd_counter(None, b"rank_item_builds", C.byref(val)) == ocffm.E_ARG
    assert val.value == 7
