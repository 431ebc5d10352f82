"""numpy fp64 reference of the diversified top-N (include/ocffm_diverse.h
ocffm_model_recommend_diverse): greedy MMR over one row's pool.

Every operation is a plain ``*``, ``-`` or ``/`` on numpy float64 scalars, so
each is rounded to fp64 on its own, which is what the contract prescribes
(nothing is fused)."""
import numpy as np

NONE = 0xFFFFFFFF


def mmr_row(pool_items, pool_scores, sim, theta, topn):
    """One row.  ``pool_items`` / ``pool_scores``: the row's pool in pool order
    (score descending), unfilled slots (``NONE`` / ``-inf``) last; ``sim``: a
    c x c matrix of the filled slots' pair similarities, or a callable
    ``sim(p, t)`` on pool positions.  Returns ``(items, scores, mmr, pos)`` of
    length ``topn``."""
    pool_items = np.asarray(pool_items, dtype=np.uint32)
    pool_scores = np.asarray(pool_scores, dtype=np.float64)
    c = int((pool_items != NONE).sum())
    assert (pool_items[:c] != NONE).all()
    theta = np.float64(theta)
    w = np.float64(1.0) - theta
    items = np.full(topn, NONE, dtype=np.uint32)
    scores = np.full(topn, -np.inf)
    mmr = np.full(topn, -np.inf)
    pos = np.full(topn, NONE, dtype=np.uint32)
    if c == 0:
        return items, scores, mmr, pos
    s = pool_scores[:c]
    rng = s[0] - s[c - 1]
    rel = np.zeros(c) if rng == 0 else (s - s[c - 1]) / rng
    if callable(sim):
        S = np.array([[sim(p, t) for t in range(c)] for p in range(c)], dtype=np.float64).reshape(c, c)
    else:
        S = np.asarray(sim, dtype=np.float64).reshape(c, c)
    items[0], scores[0], mmr[0], pos[0] = pool_items[0], s[0], w * rel[0], 0
    free = np.ones(c, dtype=bool)
    free[0] = False
    ms = np.full(c, -np.inf)
    u = 0
    for step in range(1, min(topn, c)):
        ms = np.where(S[:, u] > ms, S[:, u], ms)  # the largest similarity to a taken position so far
        v = w * rel - theta * ms                  # (elementwise: two rounded products, one rounded difference)
        best = -1
        for p in np.nonzero(free)[0]:             # (ascending p: an equal v stays with the lower position)
            if best < 0 or v[p] > v[best]:
                best = int(p)
        free[best] = False
        u = best
        items[step], scores[step], mmr[step], pos[step] = pool_items[best], s[best], v[best], best
    return items, scores, mmr, pos


def mmr(pool_items, pool_scores, sims, theta, topn):
    """Every row of a call: ``sims[i]`` is row i's matrix or callable."""
    out = [mmr_row(pool_items[i], pool_scores[i], sims[i], theta, topn) for i in range(len(pool_items))]
    if not out:
        z = np.zeros((0, topn))
        return z.astype(np.uint32), z, z.copy(), z.astype(np.uint32)
    return tuple(np.stack([o[t] for o in out]) for t in range(4))
