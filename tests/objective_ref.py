"""Brute-force and closed-form references of the training objective.

    F = 1/2 [ pos + omega (all - on_pos) + reg ]

from a state read through ``get(what, b12)`` (an ocffm.ImpProblem or an
oracle_lib.Oracle: 'P' / 'Q' of the cross blocks, 'a', 'b', 'W', 'H') and the
label lists of the training rows.  Everything is numpy fp64; ``terms`` builds
the dense m x n prediction matrix, so it is for test-sized problems only.
"""
import numpy as np

import oracle_lib as O


def cross_blocks(f, fu):
    return [O.block_index(f1, f2, f) for f1 in range(fu) for f2 in range(fu, f)]


def used_blocks(f, fu, self_side):
    return [(f1, f2, O.block_index(f1, f2, f)) for f1 in range(f) for f2 in range(f1, f)
            if self_side or (f1 < fu <= f2)]


def tables(get, f, fu, k, m, n):
    """(P, Q): the m x D and n x D concatenations of the cross projections (D = C k)."""
    cb = cross_blocks(f, fu)
    P = np.concatenate([get("P", c).reshape(m, k) for c in cb], axis=1) if cb else np.zeros((m, 0))
    Q = np.concatenate([get("Q", c).reshape(n, k) for c in cb], axis=1) if cb else np.zeros((n, 0))
    return P, Q


def labels(rows):
    """(i, j) index arrays of the label entries, repeats kept."""
    cnt = np.diff(rows.yptr.astype(np.int64))
    return np.repeat(np.arange(rows.m), cnt), rows.ycol.astype(np.int64)


def field_counts(ds, fu, fl, D):
    """Rows-of-nodes count of every feature of field fl (the --freq weights)."""
    rows, fi = (ds.train, fl) if fl < fu else (ds.item, fl - fu)
    return np.bincount(rows.idx[rows.fid == fi].astype(np.int64), minlength=D).astype(np.float64)


def reg_term(get, ds, f, fu, k, lam, self_side, freq):
    reg = 0.0
    for f1, f2, b12 in used_blocks(f, fu, self_side):
        for what, fl in (("W", f1), ("H", f2)):
            T = get(what, b12).reshape(-1, k)
            w = field_counts(ds, fu, fl, T.shape[0]) if freq else np.ones(T.shape[0])
            reg += lam * float(w @ (T * T).sum(1))
    return reg


def terms(get, ds, f, fu, k, omega, r, lam, self_side=True, freq=False):
    """The five terms by brute force over the dense m x n predictions."""
    m, n = ds.train.m, ds.item.m
    P, Q = tables(get, f, fu, k, m, n)
    a, b = get("a", 0), get("b", 0)
    Y = a[:, None] + b[None, :] + P @ Q.T
    li, lj = labels(ds.train)
    yl = Y[li, lj]
    out = dict(pos=float(((1.0 - yl) ** 2).sum()), on_pos=float(((r - yl) ** 2).sum()),
               all=float(((r - Y) ** 2).sum()), reg=reg_term(get, ds, f, fu, k, lam, self_side, freq))
    out["value"] = 0.5 * (out["pos"] + omega * (out["all"] - out["on_pos"]) + out["reg"])
    return out


def all_gram(P, Q, a, b, r):
    """`all` from the Grams and the O(D) aggregates."""
    m, n = P.shape[0], Q.shape[0]
    al = a - r
    GU, GV = P.T @ P, Q.T @ Q
    return float((GU * GV).sum() + 2 * (al @ P) @ Q.sum(0) + 2 * P.sum(0) @ (b @ Q) + n * (al @ al) + m * (b @ b)
                 + 2 * al.sum() * b.sum())


def all_augmented(P, Q, a, b, r):
    """`all` = <U~^T U~, V~^T V~>_F with U~_i = [p_i | alpha_i | 1], V~_j = [q_j | 1 | b_j]."""
    m, n = P.shape[0], Q.shape[0]
    Ua = np.concatenate([P, (a - r)[:, None], np.ones((m, 1))], axis=1)
    Va = np.concatenate([Q, np.ones((n, 1)), b[:, None]], axis=1)
    return float(((Ua.T @ Ua) * (Va.T @ Va)).sum())


def closed_form(get, ds, f, fu, k, omega, r, lam, self_side=True, freq=False, augmented=False):
    """value with `all` in closed form and pos / on_pos over the label entries only."""
    m, n = ds.train.m, ds.item.m
    P, Q = tables(get, f, fu, k, m, n)
    a, b = get("a", 0), get("b", 0)
    li, lj = labels(ds.train)
    yl = a[li] + b[lj] + (P[li] * Q[lj]).sum(1)
    pos, on_pos = float(((1.0 - yl) ** 2).sum()), float(((r - yl) ** 2).sum())
    al = (all_augmented if augmented else all_gram)(P, Q, a, b, r)
    return 0.5 * (pos + omega * (al - on_pos) + reg_term(get, ds, f, fu, k, lam, self_side, freq))
