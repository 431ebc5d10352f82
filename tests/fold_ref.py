"""numpy fp64 reference of the fold-in (include/ocffm_fold.h ocffm_model_fold_in).

One query row at a time.  ``Qs``: the C = fu * fv item-side cross tables, each
n x k (cross block c = f * fv + g); ``b``: b_j [n]; ``P``: the row's C projected
rows, C x k; ``a``: its side term; ``hist``: the row's history labels (any
order, repeats and labels >= n allowed).  The correction delta is d = fv * k
long, item field major.
"""
import numpy as np


def history(hist, n):
    """H_i: the sorted distinct labels < n."""
    return np.array(sorted({int(j) for j in hist if int(j) < n}), dtype=np.int64)


def pieces(Qs, b, P, a, field, fv):
    """z_j, q_j (n x d) and qfull_j (n x C k) of one row."""
    C = len(Qs)
    qfull = np.concatenate([np.asarray(Qs[c], dtype=np.float64) for c in range(C)], axis=1)
    p = np.concatenate([np.asarray(P[c], dtype=np.float64) for c in range(C)])
    z = a + np.asarray(b, dtype=np.float64) + qfull @ p
    q = np.concatenate([np.asarray(Qs[field * fv + g], dtype=np.float64) for g in range(fv)], axis=1)
    return z, q, qfull, p


def normal_equations(Qs, b, P, a, hist, field, fv, k, omega, lam, r):
    """(A, rhs, H) of the closed form."""
    n = len(b)
    H = history(hist, n)
    z, q, qfull, p = pieces(Qs, b, P, a, field, fv)
    d = fv * k
    lo = field * fv * k  # field f*'s entries of the C k long vectors (k, not kp, per table here)
    G = qfull.T @ qfull
    s = qfull.sum(axis=0)
    t = qfull.T @ np.asarray(b, dtype=np.float64)
    qh = q[H]
    A = omega * G[lo:lo + d, lo:lo + d] + lam * np.eye(d) + (1.0 - omega) * (qh.T @ qh)
    coef = (1.0 - z[H]) - omega * (r - z[H])
    rhs = qh.T @ coef + omega * ((r - a) * s[lo:lo + d] - t[lo:lo + d] - G[lo:lo + d, :] @ p)
    return A, rhs, H


def fold_reference(Qs, b, P, a, hist, field, fv, k, omega, lam, r):
    """delta by the normal equations; zero for an empty history (not folded)."""
    A, rhs, H = normal_equations(Qs, b, P, a, hist, field, fv, k, omega, lam, r)
    if len(H) == 0:
        return np.zeros(fv * k)
    return np.linalg.solve(A, rhs)


def fold_brute(Qs, b, P, a, hist, field, fv, k, omega, lam, r):
    """The same minimiser by a weighted least squares over all n items."""
    n = len(b)
    H = history(hist, n)
    d = fv * k
    if len(H) == 0:
        return np.zeros(d)
    z, q, _, _ = pieces(Qs, b, P, a, field, fv)
    w = np.full(n, omega, dtype=np.float64)
    y = r - z
    w[H] = 1.0
    y[H] = 1.0 - z[H]
    M = np.concatenate([np.sqrt(w)[:, None] * q, np.sqrt(lam) * np.eye(d)])
    v = np.concatenate([np.sqrt(w) * y, np.zeros(d)])
    return np.linalg.lstsq(M, v, rcond=None)[0]


def fold_objective(delta, Qs, b, P, a, hist, field, fv, k, omega, lam, r):
    """F_i(delta)."""
    n = len(b)
    H = history(hist, n)
    z, q, _, _ = pieces(Qs, b, P, a, field, fv)
    e = q @ delta
    inH = np.zeros(n, dtype=bool)
    inH[H] = True
    return float(((1.0 - z[inH] - e[inH]) ** 2).sum() + omega * ((r - z[~inH] - e[~inH]) ** 2).sum() +
                 lam * float(delta @ delta))


def fold_gradient(delta, Qs, b, P, a, hist, field, fv, k, omega, lam, r):
    """Half the gradient of F_i at delta, from the items (not from A): the
    residual of the normal equations."""
    n = len(b)
    H = history(hist, n)
    z, q, _, _ = pieces(Qs, b, P, a, field, fv)
    e = q @ delta
    w = np.full(n, omega, dtype=np.float64)
    y = r - z
    w[H] = 1.0
    y[H] = 1.0 - z[H]
    return q.T @ (w * (e - y)) + lam * delta
