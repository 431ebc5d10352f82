"""Dense numpy fp64 restatement of every half's gradient and Hessian-vector
product (gd_side / gd_cross / hess_vec, ffm.cpp:537-742) -- test infrastructure.

halves() writes each half as plain matrix products over dense X and Y, so it
shares no code with the oracle or the kernels.  With absolute=True it returns
the same sums with every elementary product replaced by its absolute value
(G_abs, Hv_abs): the scale of the terms a half adds up, which is what a
forward-error bound n * u * sum|terms| is taken against.

Also here: the small shapes the trained-state tests share (CASES) and the
small random state of the one-step regime (small_state).
"""
import numpy as np

import oracle_lib as O
import synth

# ------------------------------------------------------------------ shapes ---
# Smallest sizes that still have multi-segment columns and ragged tails, one
# per padded row width KP (pad_k: 4, 8, 16, 64, 128; 32 has its own tests).
CASES = {
    # config 2's structure, 42 halves
    "kdd12_k16": (dict(seed=31, m=400, n=120, fu=2, fv=4, k=16, mean_pos=3.0), {}),
    # config 4's structure, self-side on: side kernels at 16 lanes per row, k_gram_mfma64
    "outbrain_k64": (dict(seed=32, m=400, n=60, fu=2, fv=2, k=64, mean_pos=1.0), dict(k=64)),
    # several real-valued nodes per field
    "multi_k8": (dict(seed=9, m=150, n=70, fu=3, fv=2, k=8, nnz_user=3, mean_pos=4.0, vals="real"), {}),
    # empty columns, rows without positives, k below KP
    "sparse_k3": (dict(seed=13, m=120, n=90, fu=2, fv=2, k=3, d_user=[300, 7], d_item=[200, 5], mean_pos=0.7), {}),
    # the largest row
    "k128": (dict(seed=14, m=200, n=50, fu=2, fv=1, k=128, mean_pos=3.0), {}),
    # id-like user field, 5- and 3-column fields, heavy columns
    "heavy_k8": (dict(seed=56, m=600, n=40, fu=2, fv=2, k=8, mean_pos=8.0, d_user=[600, 5], d_item=[40, 3]), {}),
    # the --ns cross loop, no side halves in between
    "kdd12_k16_ns": (dict(seed=31, m=400, n=120, fu=2, fv=4, k=16, mean_pos=3.0), dict(self_side=False)),
}


def make_case(name):
    """(data set, keyword arguments for Oracle / problem_from_dataset)."""
    args, kw = CASES[name]
    return synth.general(**args, name=name), dict(kw, with_test=False)


def block_index(f1, f2, f):
    return f2 + (f - 1) * f1 - f1 * (f1 - 1) // 2


def used_blocks(fu, f, self_side=True):
    """[(f1, f2, b12)] in solve-independent (f1, f2) order."""
    return [(f1, f2, block_index(f1, f2, f)) for f1 in range(f) for f2 in range(f1, f)
            if self_side or (f1 < fu <= f2)]


def state_of(src, fu, f, k, self_side=True):
    """a, b and P / Q / W / H by block of anything with get(what, b12)."""
    st = dict(a=src.get("a"), b=src.get("b"), P={}, Q={}, W={}, H={})
    for _, _, b12 in used_blocks(fu, f, self_side):
        for what in "PQWH":
            st[what][b12] = src.get(what, b12).reshape(-1, k)
    return st


def small_state(fu, f, k, sizes, self_side=True, seed=1, sigma=2.0 ** -7):
    """{(what, b12): float32(sigma * standard_normal)} for W and H of every
    used block, drawn in block order, W before H; sizes[(what, b12)] = D * k.
    The values are fp32 numbers, so both precisions load them exactly."""
    rng = np.random.default_rng(seed)
    out = {}
    for _, _, b12 in used_blocks(fu, f, self_side):
        for what in "WH":
            x = (sigma * rng.standard_normal(sizes[(what, b12)])).astype(np.float32)
            out[(what, b12)] = x.astype(np.float64)
    return out


# Smallest lambda of {8, 16, 32, 64, 128} at which every half's CG of one
# oracle epoch from small_state() stops after one step (measured on the
# oracle; test_halves_cpu.py asserts it, and that the next smaller one fails).
# The largest |r|^2 / |g|^2 after that step, over the halves (the CG stops at
# 0.09): kdd12_k16 0.055, outbrain_k64 0.019, multi_k8 0.025, sparse_k3 0.022,
# k128 0.007, heavy_k8 0.072, kdd12_k16_ns < 1e-4 -- none is borderline for
# fp32 sums (relative error ~1e-5).
ONE_STEP_LAMBDA = {"kdd12_k16": 8, "outbrain_k64": 16, "multi_k8": 16, "sparse_k3": 8, "k128": 8,
                   "heavy_k8": 64, "kdd12_k16_ns": 8}
LAMBDAS = (8, 16, 32, 64, 128)


def fresh_oracle(name, **over):
    ds, kw = make_case(name)
    o = O.Oracle(ds, **dict(kw, **over))
    O.lib().orc_srand(1)
    o.init()
    return ds, o


def load_small_state(o):
    """W / H of every used block from small_state(), derived state refreshed."""
    sizes = {(what, b12): o.get(what, b12).size for _, _, b12 in used_blocks(o.fu, o.f, o.self_side)
             for what in "WH"}
    tabs = small_state(o.fu, o.f, o.k, sizes, o.self_side)
    for (what, b12), x in tabs.items():
        o.set(what, b12, x)
    o.refresh()
    return tabs


# ------------------------------------------------------------------ halves ---
def _dense(rows, nfields, dims, absolute):
    X = [np.zeros((rows.m, dims[f])) for f in range(nfields)]
    for i in range(rows.m):
        for p in range(int(rows.xptr[i]), int(rows.xptr[i + 1])):
            v = rows.val[p]
            X[int(rows.fid[p])][i, int(rows.idx[p])] += abs(v) if absolute else v
    return X


def halves(ds, state, params, vs=None, rows=None, absolute=False, reg=True, self_side=True):
    """{(b12, half): (G, Hv)} for every half of every used block.

    state   a, b (vectors) and P, Q, W, H ({b12: rows x k}), as state_of gives.
    params  dict(k, omega, lam, r).
    vs      {(b12, half): D x k} directions; Hv is lam*v + H(v), or None without vs.
    rows    (u0, u1): the sums over users run over this range only, as one
            rank of a row-sharded run forms them (item-side aggregates over
            the local users, user-side rows outside the range dropped).  The
            lam terms belong to the sum of the shards: pass reg=False.
    absolute  every elementary product replaced by its absolute value: the
            residual as |a_i| + |b_j| + sum_c |P_c[i]| . |Q_c[j]| + 1, |r|,
            |x|, |W|, |v|, |Q_c|^T |Q1| for the Grams.
    """
    k, w, lam = params["k"], params["omega"], params["lam"]
    A = np.abs if absolute else (lambda x: x)
    sub = (lambda x, y: x + y) if absolute else (lambda x, y: x - y)
    r = abs(params["r"]) if absolute else params["r"]
    m, n = ds.train.m, ds.item.m
    fu = 1 + int(ds.train.fid.max())
    fv = 1 + int(ds.item.fid.max())
    f = fu + fv
    blocks = used_blocks(fu, f, self_side)
    W = {b: np.asarray(state["W"][b]).reshape(-1, k) for _, _, b in blocks}
    H = {b: np.asarray(state["H"][b]).reshape(-1, k) for _, _, b in blocks}
    P = {b: A(np.asarray(state["P"][b]).reshape(-1, k)) for _, _, b in blocks}
    Q = {b: A(np.asarray(state["Q"][b]).reshape(-1, k)) for _, _, b in blocks}
    dims = {}
    for f1, f2, b in blocks:
        dims[f1], dims[f2] = W[b].shape[0], H[b].shape[0]
    Xu = _dense(ds.train, fu, [dims[fl] for fl in range(fu)], absolute)
    Xv = _dense(ds.item, fv, [dims[fu + fl] for fl in range(fv)], absolute)
    Y = np.zeros((m, n))
    for i in range(m):
        Y[i, ds.train.ycol[int(ds.train.yptr[i]):int(ds.train.yptr[i + 1])].astype(np.int64)] = 1.0
    a, b = A(np.asarray(state["a"])), A(np.asarray(state["b"]))
    u0, u1 = (0, m) if rows is None else rows
    sh = slice(u0, u1)
    cross = [b12 for f1, f2, b12 in blocks if f1 < fu <= f2]
    yt = sub(a[:, None] + b[None, :] + sum(P[c] @ Q[c].T for c in cross), 1.0)
    coef = Y * sub((1 - w) * yt, w * sub(1.0, r))
    sa = sum(P[c] @ Q[c].sum(0) for c in cross)
    sb_loc = sum(Q[c] @ P[c][sh].sum(0) for c in cross)
    out = {}
    for f1, f2, b12 in blocks:
        for half in (0, 1):
            fl = f1 if half == 0 else f2
            user = fl < fu
            X = Xu[fl] if user else Xv[fl - fu]
            Q1 = Q[b12] if half == 0 else P[b12]
            v = None if vs is None else A(np.asarray(vs[(b12, half)]).reshape(-1, k))
            hv = None
            if f1 < fu <= f2:  # cross
                if user:
                    Xs = X[sh]
                    oQ, bQ = Q1.sum(0), b @ Q1
                    T = sum(P[c][sh] @ (Q[c].T @ Q1) for c in cross)
                    g = coef[sh] @ Q1 + w * (T + sub(a[sh], r)[:, None] * oQ + bQ)
                    if v is not None:
                        phi = Xs @ v
                        hv = (1 - w) * (((phi @ Q1.T) * Y[sh]) @ Q1) + w * phi @ (Q1.T @ Q1)
                else:
                    Xs = X
                    P1 = Q1[sh]
                    oQ, bQ = P1.sum(0), a[sh] @ P1
                    T = sum(Q[c] @ (P[c][sh].T @ P1) for c in cross)
                    g = coef[sh].T @ P1 + w * (T + sub(b, r)[:, None] * oQ + bQ)
                    if v is not None:
                        phi = Xs @ v
                        hv = (1 - w) * (((phi @ P1.T) * Y[sh].T) @ P1) + w * phi @ (P1.T @ P1)
            else:  # side
                if user:
                    Xs, q = X[sh], Q1[sh]
                    z = w * (n * sub(a[sh], r) + b.sum() + sa[sh]) + coef[sh].sum(1)
                    d = (1 - w) * Y[sh].sum(1) + w * n
                else:
                    Xs, q = X, Q1
                    z = w * ((u1 - u0) * sub(b, r) + a[sh].sum() + sb_loc) + coef[sh].sum(0)
                    d = (1 - w) * Y[sh].sum(0) + w * (u1 - u0)
                g = z[:, None] * q
                if v is not None:
                    phi = Xs @ v
                    hv = (d * (phi * q).sum(1))[:, None] * q
            G = Xs.T @ g
            Hv = None if hv is None else Xs.T @ hv
            if reg:
                G = G + lam * A(W[b12] if half == 0 else H[b12])
                if Hv is not None:
                    Hv = Hv + lam * v
            out[(b12, half)] = (G, Hv)
    return out
