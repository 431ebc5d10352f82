"""CPU tests of the diversified top-N (include/ocffm_diverse.h): the numpy
reference (tests/diverse_ref.py) on hand-worked pools and against a brute-force
property, the boundary (the entry is declared, exported and listed) and the
usage errors of predict --diversify / --pool.  No GPU compute here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import ocffm
from diverse_ref import NONE, mmr, mmr_row

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREDICT = os.path.join(REPO, "one-class-ffm_amd", "predict")
INF = np.inf


# ------------------------------------------------------- hand-worked pools
def test_twins_tie_in_score():
    """Items 7 and 9 are the same vector (sim 1) and tie in score at the head;
    item 4 is unrelated and scores half the range lower."""
    items, scores = [7, 9, 4], [2.0, 2.0, 1.0]
    sim = [[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    it, sc, mv, ps = mmr_row(items, scores, sim, 0.5, 3)
    # step 0: position 0.  step 1: v(9) = 0.5 * 1 - 0.5 * 1 = 0, v(4) = 0.5 * 0 - 0.5 * 0 = 0: the tie goes to
    # the lower position, the twin.  step 2: item 4, v = 0 - 0 = 0.
    assert it.tolist() == [7, 9, 4] and ps.tolist() == [0, 1, 2]
    assert sc.tolist() == [2.0, 2.0, 1.0] and mv.tolist() == [0.5, 0.0, 0.0]
    # a little more weight on the similarity and the unrelated item overtakes the twin
    it, sc, mv, ps = mmr_row(items, scores, sim, 0.75, 3)
    assert it.tolist() == [7, 4, 9] and ps.tolist() == [0, 2, 1]
    assert mv.tolist() == [0.25, 0.0, 0.25 * 1.0 - 0.75 * 1.0]
    assert sc.tolist() == [2.0, 1.0, 2.0]


def test_all_equal_scores_rel_zero():
    sim = np.array([[1.0, 0.9, 0.1, 0.5], [0.9, 1.0, 0.2, 0.3], [0.1, 0.2, 1.0, 0.8], [0.5, 0.3, 0.8, 1.0]])
    it, sc, mv, ps = mmr_row([3, 5, 8, 9], [4.0] * 4, sim, 0.5, 4)
    # rel = 0: step 1 takes the least similar to 0 (position 2, -0.05); then ms = {1: 0.9, 3: 0.8}: position 3
    assert ps.tolist() == [0, 2, 3, 1] and it.tolist() == [3, 8, 9, 5]
    assert mv.tolist() == [0.0, 0.0 - 0.5 * 0.1, 0.0 - 0.5 * 0.8, 0.0 - 0.5 * 0.9]
    assert (sc == 4.0).all()


def test_theta_zero_is_the_identity_and_theta_one_ignores_scores():
    rng = np.random.default_rng(3)
    s = np.sort(rng.normal(size=9))[::-1]
    E = rng.normal(size=(9, 4))
    sim = E @ E.T
    it, sc, mv, ps = mmr_row(np.arange(20, 29), s, sim, 0.0, 6)
    assert ps.tolist() == list(range(6)) and it.tolist() == list(range(20, 26)) and (sc == s[:6]).all()
    assert (mv == (s[:6] - s[8]) / (s[0] - s[8])).all()
    it, sc, mv, ps = mmr_row(np.arange(20, 29), s, sim, 1.0, 4)
    assert ps[0] == 0 and mv[0] == 0.0
    assert ps[1] == int(np.argmin(np.where(np.arange(9) == 0, INF, sim[:, 0])))  # the least similar to position 0
    assert mv[1] == -sim[ps[1], 0]
    rest = [p for p in range(9) if p not in (0, int(ps[1]))]
    assert ps[2] == min(rest, key=lambda p: (max(sim[p, 0], sim[p, ps[1]]), p))


def test_short_pools():
    sim = np.eye(3)
    it, sc, mv, ps = mmr_row([5, 6, 2, NONE, NONE], [3.0, 2.0, 1.0, -INF, -INF], sim, 0.3, 5)  # c < topn
    assert it.tolist() == [5, 6, 2, NONE, NONE] and ps.tolist() == [0, 1, 2, NONE, NONE]
    assert sc.tolist() == [3.0, 2.0, 1.0, -INF, -INF] and (mv[3:] == -INF).all() and np.isfinite(mv[:3]).all()
    it, sc, mv, ps = mmr_row([11, NONE], [0.25, -INF], [[1.0]], 0.3, 2)  # c = 1: range = 0, rel = 0
    assert it.tolist() == [11, NONE] and sc.tolist() == [0.25, -INF] and mv.tolist() == [0.0, -INF]
    assert ps.tolist() == [0, NONE]
    it, sc, mv, ps = mmr_row([NONE, NONE], [-INF, -INF], np.zeros((0, 0)), 0.3, 2)  # c = 0
    assert (it == NONE).all() and (ps == NONE).all() and (sc == -INF).all() and (mv == -INF).all()
    out = mmr([[5, 6, 2], [1, NONE, NONE]], [[3.0, 2.0, 1.0], [1.0, -INF, -INF]], [sim, [[1.0]]], 0.3, 2)
    assert out[0].tolist() == [[5, 6], [1, NONE]] and out[3].tolist() == [[0, 1], [0, NONE]]


def test_negative_similarities_are_a_true_maximum():
    """ms is the largest similarity to a taken item even when all are negative:
    a negative ms raises v."""
    sim = np.array([[1.0, -0.5, -0.25], [-0.5, 1.0, -0.75], [-0.25, -0.75, 1.0]])
    it, sc, mv, ps = mmr_row([0, 1, 2], [1.0, 0.5, 0.0], sim, 0.5, 3)
    # step 1: v(1) = 0.25 + 0.25 = 0.5, v(2) = 0 + 0.125; step 2: ms(2) = max(-0.25, -0.75) = -0.25
    assert ps.tolist() == [0, 1, 2] and mv.tolist() == [0.5, 0.5, 0.125]


def test_every_pick_maximises_v():
    """Brute force on random 12-item pools: at every step the pick's v is the
    largest over the positions not yet taken, computed from scratch, and among
    equal v the lowest position wins.  Similarities on a coarse grid and
    repeated scores make ties common."""
    rng = np.random.default_rng(12)
    ties = 0
    for trial in range(60):
        c, topn = 12, int(rng.integers(1, 13))
        theta = np.float64(rng.choice([0.0, 0.25, 0.3, 0.5, 0.9, 1.0]))
        s = np.sort(rng.integers(0, 6, size=c).astype(np.float64))[::-1]
        A = rng.integers(-4, 5, size=(c, c)) / 4.0
        sim = np.triu(A, 1) + np.triu(A, 1).T + np.eye(c)
        it, sc, mv, ps = mmr_row(np.arange(100, 100 + c), s, lambda p, t: sim[p, t], theta, topn)
        w = np.float64(1.0) - theta
        rng_s = s[0] - s[-1]
        rel = np.zeros(c) if rng_s == 0 else (s - s[-1]) / rng_s
        assert ps[0] == 0 and mv[0] == w * rel[0]
        for step in range(1, topn):
            taken = [int(p) for p in ps[:step]]
            v = {p: w * rel[p] - theta * max(sim[p, u] for u in taken) for p in range(c) if p not in taken}
            top = max(v.values())
            winners = sorted(p for p in v if v[p] == top)
            ties += len(winners) > 1
            assert ps[step] == winners[0] and mv[step] == top, (trial, step)
        assert (it == 100 + ps).all() and (sc == s[ps]).all() and len(set(ps.tolist())) == topn
    assert ties > 20


# ---------------------------------------------------------------- boundary
def test_entry_declared_exported_and_listed():
    inc = os.path.join(REPO, "include")
    text = open(os.path.join(inc, "ocffm_diverse.h")).read()
    syms = sorted(set(re.findall(r"\b(ocffm_[a-z_0-9]+)\s*\(", text)))
    declared = sorted(set(re.findall(r"^int (ocffm_[a-z_0-9]+)\(", text, flags=re.M)))
    assert declared == sorted(ocffm.DIVERSE_EXPORTS) == ["ocffm_model_recommend_diverse"]
    assert set(declared) <= set(syms)
    main = open(os.path.join(inc, "ocffm.h")).read()
    assert '#include "ocffm_diverse.h"' in main
    assert main.index('#include "ocffm_similar.h"') < main.index('#include "ocffm_diverse.h"')
    lib = C.CDLL(ocffm.LIB_PATH)
    for s in declared:
        assert hasattr(lib, s), s
    others = set(ocffm.EXPORTS) | set(ocffm.FOLD_EXPORTS) | set(ocffm.SIMILAR_EXPORTS)
    assert not set(declared) & others
    assert re.search(r"#define OCFFM_DIV_MAX_POOL OCFFM_REC_MAX_TOPN\b", text)
    assert ocffm.DIV_MAX_POOL == ocffm.REC_MAX_TOPN == 128


# --------------------------------------------------------------------- CLI
def test_predict_usage_errors(tmp_path):
    """Every misuse of --diversify / --pool ends with status 1 and a message,
    before any file is read or written."""
    out = str(tmp_path / "rec.txt")
    missing = str(tmp_path / "nothing")
    rec = ["--recommend", missing, "--rec-out", out]
    cases = {
        "pool without diversify": rec + ["--pool", "40"],
        "theta above 1": rec + ["--diversify", "1.5"],
        "theta below 0": rec + ["--diversify", "-0.1"],
        "theta not a number": rec + ["--diversify", "lots"],
        "pool below topn": rec + ["--topn", "20", "--diversify", "0.3", "--pool", "19"],
        "pool above 128": rec + ["--diversify", "0.3", "--pool", "129"],
        "default pool is fine, explicit 0 is not": rec + ["--diversify", "0.3", "--pool", "0"],
        "with fold": rec + ["--diversify", "0.3", "--fold-field", "0", "--fold-history", missing],
        "without recommend": ["--diversify", "0.3"],
    }
    for name, args in cases.items():
        r = subprocess.run([PREDICT] + args + [missing, missing], capture_output=True, text=True)
        assert r.returncode == 1 and r.stderr.strip() and not os.path.exists(out), (name, r.returncode, r.stderr)
        assert "error:" not in r.stderr, name  # a usage error, not a failed call
    r = subprocess.run([PREDICT] + cases["with fold"] + [missing, missing], capture_output=True, text=True)
    assert "fold" in r.stderr and "not diversified" in r.stderr
    # a well-formed command line gets as far as the model file
    r = subprocess.run([PREDICT] + rec + ["--diversify", "0.3", "--pool", "40", missing, missing],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "error:" in r.stderr
    assert "--diversify" in subprocess.run([PREDICT], capture_output=True, text=True).stderr
