"""ocffm_eval_from_ranks (host code, no GPU) against a numpy restatement of
the definitions in include/ocffm.h, on hand-made ranks.  Compared to 1e-14:
both sides sum a handful of fp64 terms of size <= 1."""
import numpy as np
import pytest

import ocffm

NONE = ocffm.RANK_NONE


def restate(rows, ncand, cuts):
    """rows: per row a list of (rank, score) label entries (copies included)."""
    out = dict(rows=len(rows), rows_used=0, labels=sum(len(r) for r in rows), labels_ranked=0)
    acc = {key: np.zeros(len(cuts)) for key in ("prec", "recall", "ndcg", "map", "hit")}
    ploss = mrr = auc = 0.0
    auc_rows = 0
    for i, row in enumerate(rows):
        lab = sorted({r: s for r, s in row if r != NONE}.items())
        P = len(lab)
        if P == 0:
            continue
        out["rows_used"] += 1
        out["labels_ranked"] += P
        r = np.array([x[0] for x in lab], dtype=np.float64)
        ploss += sum((1 - x[1]) ** 2 for x in lab)
        mrr += 1 / (r[0] + 1)
        if ncand[i] > P:
            auc += 1 - (r - np.arange(P)).sum() / (P * (ncand[i] - P))
            auc_rows += 1
        for s, c in enumerate(cuts):
            hit = r < c
            t = np.arange(1, P + 1)
            acc["prec"][s] += hit.sum() / c
            acc["recall"][s] += hit.sum() / P
            acc["ndcg"][s] += (1 / np.log2(r[hit] + 2)).sum() / (1 / np.log2(np.arange(min(c, P)) + 2.0)).sum()
            acc["map"][s] += (t[hit] / (r[hit] + 1)).sum() / min(c, P)
            acc["hit"][s] += float(hit.any())
    u = out["rows_used"]
    out["loss"] = np.sqrt(ploss / u) if u else 0.0
    out["mrr"] = mrr / u if u else 0.0
    out["auc"] = auc / auc_rows if auc_rows else 0.0
    for key, v in acc.items():
        out[key] = v / u if u else v
    return out


def call(rows, ncand, cuts, with_scores=True):
    yptr = np.zeros(len(rows) + 1, dtype=np.uint64)
    yptr[1:] = np.cumsum([len(r) for r in rows])
    ranks = np.array([x[0] for r in rows for x in r], dtype=np.uint32)
    scores = np.array([x[1] for r in rows for x in r], dtype=np.float64)
    return ocffm.eval_from_ranks(yptr, ranks, np.array(ncand, dtype=np.uint32), scores if with_scores else None, cuts)


def compare(got, want, cuts):
    for key in ("rows", "rows_used", "labels", "labels_ranked"):
        assert got[key] == want[key], key
    assert got["cuts"] == list(cuts)
    for key in ("loss", "mrr", "auc"):
        assert abs(got[key] - want[key]) <= 1e-14, (key, got[key], want[key])
    for key in ("prec", "recall", "ndcg", "map", "hit"):
        assert got[key].shape == (len(cuts),)
        assert np.abs(got[key] - want[key]).max() <= 1e-14, (key, got[key], want[key])


ROWS = [
    [],                                                         # a row without labels
    [(NONE, -np.inf), (NONE, -np.inf)],                         # every label unranked
    [(4, 0.25), (0, 0.9), (4, 0.25), (NONE, -np.inf)],          # duplicate labels (one rank)
    [(r, 1.0 - 0.1 * r) for r in (0, 1, 2, 5, 7, 9, 30, 150)],  # P > c for c = 1, 3
    [(2, 0.5), (11, -0.5)],                                     # c = 200 > ncand = 12
    [(1, 0.3), (0, 0.4), (2, 0.1)],                             # ncand == P: no AUC term
    [(199, -2.0)],                                              # the last place inside c = 200
    [(200, -2.0), (7, 0.0)],
]
NCAND = [50, 0, 40, 300, 12, 3, 1000, 201]


@pytest.mark.parametrize("cuts", [(1, 3, 10, 200), (5, 10, 20, 40, 80), (2,), (1, 2, 3, 4, 5, 6, 7, 8)])
def test_against_restatement(cuts):
    compare(call(ROWS, NCAND, cuts), restate(ROWS, NCAND, cuts), cuts)


def test_known_values():
    """One row by hand: labels at ranks 0 and 2 of 5 candidates, cut 2."""
    e = call([[(0, 1.0), (2, 0.0)]], [5], (2,))
    assert e["rows_used"] == 1 and e["labels_ranked"] == 2
    assert e["prec"][0] == 0.5 and e["recall"][0] == 0.5 and e["hit"][0] == 1.0
    assert abs(e["ndcg"][0] - 1.0 / (1.0 + 1.0 / np.log2(3.0))) <= 1e-14
    assert e["map"][0] == 0.5 and e["mrr"] == 1.0
    assert abs(e["auc"] - (1 - 1.0 / 6.0)) <= 1e-14  # one of the 6 (label, other) pairs is inverted
    assert abs(e["loss"] - 1.0) <= 1e-14


def test_subsets_and_empty():
    cuts = (1, 3, 10, 200)
    for sel in ([0], [1], [0, 1], [5], [2, 4]):
        rows, nc = [ROWS[i] for i in sel], [NCAND[i] for i in sel]
        compare(call(rows, nc, cuts), restate(rows, nc, cuts), cuts)
    e = call([], [], cuts)
    assert e["rows"] == 0 and e["rows_used"] == 0 and e["mrr"] == 0 and (e["prec"] == 0).all()
    e = call(ROWS[:2], NCAND[:2], cuts)  # no ranked label anywhere: every metric 0
    assert e["rows_used"] == 0 and e["labels"] == 2 and e["loss"] == 0 and e["auc"] == 0 and (e["ndcg"] == 0).all()


def test_without_scores_loss_is_zero():
    cuts = (1, 3, 10, 200)
    got, want = call(ROWS, NCAND, cuts, with_scores=False), restate(ROWS, NCAND, cuts)
    want["loss"] = 0.0
    compare(got, want, cuts)


@pytest.mark.parametrize("cuts", [(), (0, 5), (5, 5), (10, 5), (1, 2, 3, 4, 5, 6, 7, 8, 9)])
def test_bad_cuts(cuts):
    with pytest.raises(ocffm.OcffmError) as e:
        call(ROWS, NCAND, cuts)
    assert e.value.code == ocffm.E_ARG
