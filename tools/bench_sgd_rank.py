"""Top-N recommendation and ranking evaluation of an SGD-trained model on the
kkbox shape (synth.kkbox(), k = 32: 3,075 test rows x 100,000 items, 6 cross
blocks, depth 6 x 32), against the block Newton-CG problem's fp32
recommend / evaluate on the same rows in the same run.

SGD trainer, after a few epochs: recommend(topn = 80) and evaluate(cuts
5..80) on the data set's test rows, the first call (with the item-side
projection) and the steady state, from the trainer's counters:
rank_kernel_us (sweep, merge and label-score launches between HIP events),
rank_setup_us (host set-up) and rank_item_build_us (the item-side projection,
paid once per model change), with the projection's algorithmic bytes.
Newton problem, fp32, after one epoch: the `recommend` / `evaluate` kernel
families' HIP-event time and the set-up counters.  Medians of repeated calls.
Writes profiles/sgd_rank_bench.json.

Usage: python tools/bench_sgd_rank.py [--epochs N] [--repeat N] [--out path]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "one-class-ffm_amd"))

import ocffm  # noqa: E402
import synth  # noqa: E402

TOPN = 80
CUTS = (5, 10, 20, 40, 80)


def sgd_call(t, fn, repeat):
    """Wall, kernel and set-up ms of repeated calls (medians) and of the first."""
    wall, kern, setup = [], [], []
    for _ in range(repeat + 1):
        t.sync()
        t0 = time.perf_counter()
        fn()
        t.sync()
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(t.counter("rank_kernel_us") / 1e3)
        setup.append(t.counter("rank_setup_us") / 1e3)
    med = statistics.median
    return dict(first=dict(ms_per_call=wall[0], kernel_ms=kern[0], host_setup_ms=setup[0]),
                steady=dict(ms_per_call=med(wall[1:]), kernel_ms=med(kern[1:]), min_kernel_ms=min(kern[1:]),
                            max_kernel_ms=max(kern[1:]), host_setup_ms=med(setup[1:])))


def sgd_side(ds, epochs, repeat):
    U = ocffm.ImpData.from_rows(ds.train)
    V = ocffm.ImpData.from_rows(ds.item)
    X = ocffm.ImpData.from_rows(ds.test, ds=U.Ds)
    t = ocffm.SgdTrainer(U, V, k=ds.k, seed=9)
    loss = [t.epoch() for _ in range(epochs)]
    info = t.info
    fu, fv = int(U.info["f"]), int(V.info["f"])
    n, kp, C = int(V.info["m"]), info["kp"], fu * fv
    nnz_v = int(V.info["nnz_x"])
    rec = sgd_call(t, lambda: t.recommend(X, topn=TOPN), repeat)
    builds = t.counter("rank_item_builds")
    build_ms = t.counter("rank_item_build_us") / 1e3
    t.epoch()  # the model changed: evaluate's first call pays the projection again
    ev = sgd_call(t, lambda: t.evaluate(X, cuts=CUTS), repeat)
    metrics = t.evaluate(X, cuts=CUTS)
    # projection: node lists (j, f, x), one W row per (node, opposite field), tables and side terms out
    bytes_build = nnz_v * 12 + nnz_v * fu * kp * 4 + n * (C * kp + 2) * 4
    out = dict(epochs=epochs, mean_loss=loss, rows=int(X.info["m"]), items=n, kp=kp, cross_blocks=C,
               recommend=rec, evaluate=ev,
               item_build=dict(ms=build_ms, ms_second=t.counter("rank_item_build_us") / 1e3,
                               builds_after_recommend_calls=builds, builds_total=t.counter("rank_item_builds"),
                               alg_bytes=bytes_build, gb_per_s=bytes_build / build_ms / 1e6 if build_ms else None),
               ndcg=[float(x) for x in metrics["ndcg"]], recall=[float(x) for x in metrics["recall"]],
               auc=float(metrics["auc"]))
    t.close()
    return out


def newton_side(ds, repeat):
    g = ocffm.problem_from_dataset(ds, precision=ocffm.FP32)
    ocffm.srand(1)
    g.init()
    g.one_epoch()
    g.sync()
    X = g._keep[1]
    out = {}
    g.set_profiling(True)
    for fam, fn, counter in (("recommend", lambda: g.recommend(X, topn=TOPN), "rec_setup_us"),
                             ("evaluate", lambda: g.evaluate(X, cuts=CUTS), "eval_setup_us")):
        g.set_profile_filter(fam)
        kern, setup = [], []
        for _ in range(repeat + 1):
            g.reset_stats()
            fn()
            kern.append(g.kernel_stats()[fam]["total_ms"])
            setup.append(g.counter(counter) / 1e3)
        out[fam] = dict(kernel_ms=statistics.median(kern[1:]), min_kernel_ms=min(kern[1:]),
                        max_kernel_ms=max(kern[1:]), host_setup_ms=statistics.median(setup[1:]))
    g.set_profiling(False)
    g.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sgd_rank_bench.json"))
    a = ap.parse_args()
    ds = synth.kkbox()
    out = dict(workload=f"synth.kkbox() k=32, test rows, topn={TOPN}, cuts={list(CUTS)}", repeat=a.repeat,
               timing="median over repeated calls; kernel ms between HIP events on the object's stream")
    out["sgd"] = sgd_side(ds, a.epochs, a.repeat)
    out["newton_fp32"] = newton_side(ds, a.repeat)
    for fam in ("recommend", "evaluate"):
        s, nw = out["sgd"][fam]["steady"]["kernel_ms"], out["newton_fp32"][fam]["kernel_ms"]
        out[f"{fam}_sgd_over_newton_kernel"] = s / nw
        print(f"{fam}: SGD kernel {s:.3f} ms (first call {out['sgd'][fam]['first']['kernel_ms']:.3f}), "
              f"Newton fp32 {nw:.3f} ms, ratio {s / nw:.4f}; SGD set-up "
              f"{out['sgd'][fam]['steady']['host_setup_ms']:.3f} ms", flush=True)
    b = out["sgd"]["item_build"]
    print(f"item-side projection: {b['ms']:.3f} ms, {b['alg_bytes'] / 1e6:.1f} MB algorithmic, "
          f"{b['builds_total']} builds in all", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
