"""Folding new users in from their history, on the kkbox shape (synth.kkbox(),
k = 32: 3,075 test rows x 100,000 items, 6 cross blocks, d = fv k = 96), in
fp32 and fp64, in one run.

Per precision a problem is trained for one epoch and a model is made from it.
The query rows are the test rows with the listener-id node dropped (the rows
of users the model does not know: only the context field is left), the
history of row i is the train labels of the same user, the fold is on field 0
(the listener id) with the data set's omega, lambda and r.  Timed: the
catalogue aggregates' build ("fold_stats_us", the first fold call after the
catalogue is set); the build-solve-apply launches of a call ("fold_us", between
HIP events) and the rows per second they give; recommend(topn=80) with and
without fold= on the same rows in the same run (median wall time per call,
every call ends with a device sync).  Each time is also given as a ratio to
the same run's plain recommend call.  Quality: evaluate's AUC and nDCG@10 on
the test labels with the history as `seen`, folded and not.  Writes
profiles/fold_bench.json.

Usage: python tools/bench_fold.py [--repeat N] [--warmup N] [--out path]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "one-class-ffm_amd"))

import ocffm  # noqa: E402
import synth  # noqa: E402

TOPN = 80


def wall(fn, warmup, repeat):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeat):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return dict(ms=statistics.median(out), min_ms=min(out), max_ms=max(out))


def query_rows(ds):
    """(the test rows without their field-0 node, the same rows with the train
    labels of the same users as labels)."""
    t, tr = ds.test, ds.train
    keep = t.fid != 0
    cnt = np.add.reduceat(keep.astype(np.uint64), t.xptr[:-1].astype(np.int64))
    xptr = np.zeros(t.m + 1, dtype=np.uint64)
    np.cumsum(cnt, out=xptr[1:])
    X = synth.Rows(xptr, t.fid[keep], t.idx[keep], t.val[keep], t.yptr, t.ycol)
    hp = tr.yptr[:t.m + 1].astype(np.uint64)
    H = synth.Rows(xptr, t.fid[keep], t.idx[keep], t.val[keep], hp, tr.ycol[:int(hp[-1])].astype(np.uint64))
    return X, H


def one(ds, name, precision, warmup, repeat):
    g = ocffm.problem_from_dataset(ds, precision=precision)
    ocffm.srand(1)
    g.init()
    g.one_epoch()
    M = ocffm.Model.from_problem(g)
    U = g._keep[0]
    g.close()
    xr, hr = query_rows(ds)
    X = ocffm.ImpData.from_rows(xr, ds=U.Ds)
    H = ocffm.ImpData.from_rows(hr, ds=U.Ds)
    p = ds.params
    fold = (H, 0, p["w"], p["l"], p["r"])
    delta, nhist = M.fold_in(X, *fold)
    build_ms = M.counter("fold_stats_us") / 1e3
    assert M.counter("fold_stats_builds") == 1
    us = []
    for _ in range(warmup + repeat):
        M.fold_in(X, *fold)
        us.append(M.counter("fold_us") / 1e3)
    us = us[warmup:]
    rows = int(M.counter("fold_rows"))
    plain = wall(lambda: M.recommend(X, topn=TOPN), warmup, repeat)
    folded = wall(lambda: M.recommend(X, topn=TOPN, fold=fold), warmup, repeat)
    e0 = M.evaluate(X, seen=H)
    e1 = M.evaluate(X, seen=H, fold=fold)
    i10 = e0["cuts"].index(10)
    fold_ms = statistics.median(us)
    res = dict(rows=int(X.info["m"]), rows_folded=rows, items=int(M.info["n"]), d=int(delta.shape[1]),
               history_mean=float(nhist.mean()), history_max=int(nhist.max()), topn=TOPN,
               stats_build_ms=build_ms, fold_ms=fold_ms, fold_min_ms=min(us), fold_max_ms=max(us),
               fold_rows_per_s=rows / (fold_ms * 1e-3) if fold_ms > 0 else None,
               recommend=plain, recommend_fold=folded,
               stats_build_over_recommend=build_ms / plain["ms"], fold_over_recommend=fold_ms / plain["ms"],
               recommend_fold_over_recommend=folded["ms"] / plain["ms"],
               unfolded=dict(auc=e0["auc"], ndcg10=float(e0["ndcg"][i10]), labels_ranked=e0["labels_ranked"]),
               folded=dict(auc=e1["auc"], ndcg10=float(e1["ndcg"][i10]), labels_ranked=e1["labels_ranked"]))
    print(f"{name}: aggregates {build_ms:.3f} ms, fold {fold_ms:.3f} ms for {rows} rows "
          f"({res['fold_rows_per_s']:.0f} rows/s), recommend {plain['ms']:.3f} ms, with fold {folded['ms']:.3f} ms; "
          f"AUC {e0['auc']:.4f} -> {e1['auc']:.4f}, nDCG@10 {res['unfolded']['ndcg10']:.4f} -> "
          f"{res['folded']['ndcg10']:.4f}", flush=True)
    M.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fold_bench.json"))
    a = ap.parse_args()
    ds = synth.kkbox()
    out = dict(workload="synth.kkbox() k=32, one epoch; test rows without the listener-id node, history = the same "
                        "users' train labels, fold on field 0, topn=80",
               repeat=a.repeat, warmup=a.warmup,
               timing="stats_build_ms / fold_ms: the model's counters (host clock around the build with its sync; HIP "
                      "events around the build-solve and apply launches); recommend*: median wall ms per call")
    for name, prec in (("fp32", ocffm.FP32), ("fp64", ocffm.FP64)):
        out[name] = one(ds, name, prec, a.warmup, a.repeat)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
