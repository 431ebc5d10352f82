"""CPU tests of the similar-items boundary (include/ocffm_similar.h): the
entries are declared, exported and listed, and the Python wrappers reject a
malformed ``exclude`` pair or an unknown ``metric`` before they touch the
library.  No GPU compute here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ocffm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_declared_exported_and_listed():
    inc = os.path.join(REPO, "include")
    text = open(os.path.join(inc, "ocffm_similar.h")).read()
    syms = sorted(set(re.findall(r"\b(ocffm_[a-z_0-9]+)\s*\(", text)))
    assert syms == sorted(ocffm.SIMILAR_EXPORTS) and len(syms) == 3
    assert '#include "ocffm_similar.h"' in open(os.path.join(inc, "ocffm.h")).read()
    lib = C.CDLL(ocffm.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), s
    assert not set(syms) & set(ocffm.EXPORTS) and not set(syms) & set(ocffm.FOLD_EXPORTS)
    for name, bit in (("OCFFM_SIM_DOT", ocffm.SIM_DOT), ("OCFFM_SIM_KEEP_SELF", ocffm.SIM_KEEP_SELF)):
        assert re.search(r"#define %s %du\b" % (name, bit), text), name


class _Never:
    """A handle no library call may see."""

    @property
    def h(self):
        raise AssertionError("the wrapper touched the library")

    @property
    def info(self):
        raise AssertionError("the wrapper touched the library")


def _model():
    M = ocffm.Model.__new__(ocffm.Model)
    M.h = None  # (close() on a handle that was never made is a no-op)
    return M


def test_wrappers_reject_bad_arguments_before_the_library(monkeypatch):
    def no_lib():
        raise AssertionError("the wrapper touched the library")

    monkeypatch.setattr(ocffm, "lib", no_lib)
    M = _model()
    V = _Never()
    for metric in ("l2", "", "COSINE", None):
        with pytest.raises(ValueError):
            M.similar_items([0, 1], metric=metric)
        with pytest.raises(ValueError):
            M.similar_to(V, metric=metric)
        with pytest.raises(ValueError):
            M.item_similarity([0], [1], metric=metric)
    ccol = np.array([1, 2, 3], dtype=np.uint32)
    for cptr in ([0, 1], [0, 1, 2, 3], [0, 1, 9]):  # too short, too long, past ccol
        with pytest.raises(ocffm.OcffmError) as e:
            M.similar_items([0, 1], exclude=(cptr, ccol))
        assert e.value.code == ocffm.E_ARG
        with pytest.raises(ocffm.OcffmError) as e:
            M.similar_to(V, rows=2, exclude=(cptr, ccol))
        assert e.value.code == ocffm.E_ARG
    with pytest.raises(ocffm.OcffmError) as e:
        M.item_similarity([0, 1], [1])
    assert e.value.code == ocffm.E_ARG
