"""Ranking evaluation against validate() and recommend() on the kkbox shape
(synth.kkbox(), k = 32: 3,075 test rows x 100,000 items, 6 cross blocks),
after one epoch, in fp32 and fp64, cuts 5..80.

Per precision, in one process and on the same test rows: validate()
(k_scores + k_rank), recommend(topn=80) and evaluate(), each as warm-up calls,
then the median wall time of repeated calls with the device idle before and
after every timed call (all three end with a device sync).  evaluate() is
also timed on the first 4,096 training rows with their own labels (about 70
labels a row, some rows above the 128 labels whose counters fit in LDS).  The
`evaluate` kernel family's HIP-event time (k_eval_label_scores +
k_eval_count) and the call's host-side set-up (layout of X, projections,
label lists: the "eval_setup_us" counter) are reported separately.  Writes
profiles/evaluate_bench.json.

Usage: python tools/bench_evaluate.py [--repeat N] [--warmup N] [--out path]
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

MFMA_PEAK_TF = {"fp32": 157.3, "fp64": 78.6}
CUTS = (5, 10, 20, 40, 80)
TOPN = 80
TRAIN_ROWS = 4096


def timed(g, fn, warmup, repeat):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeat):
        g.sync()
        t = time.perf_counter()
        fn()
        g.sync()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def head_rows(rows, count):
    """The first `count` rows of a synth.Rows, labels included."""
    nx, ny = int(rows.xptr[count]), int(rows.yptr[count])
    return synth.Rows(rows.xptr[:count + 1], rows.fid[:nx], rows.idx[:nx], rows.val[:nx], rows.yptr[:count + 1],
                      rows.ycol[:ny])


def family(g, X, name, repeat):
    """The evaluate family's event time and the host set-up, in calls of their
    own (event timing adds host work to a call)."""
    g.set_profiling(True)
    g.set_profile_filter("evaluate")
    fam_ms, setup_ms, st = [], [], None
    for _ in range(repeat):
        g.reset_stats()
        g.evaluate(X, cuts=CUTS)
        st = g.kernel_stats()["evaluate"]
        fam_ms.append(st["total_ms"])
        setup_ms.append(g.counter("eval_setup_us") / 1e3)
    g.set_profiling(False)
    g.set_profile_filter(None)
    fam = statistics.median(fam_ms)
    return dict(host_setup_ms=statistics.median(setup_ms), family_event_ms=fam, family_launches=int(st["launches"]),
                family_alg_flops=st["alg_flops"], family_alg_bytes=st["alg_bytes"],
                family_tflops=st["alg_flops"] / fam / 1e9,
                mfma_peak_fraction=st["alg_flops"] / fam / 1e9 / MFMA_PEAK_TF[name])


def one(ds, name, precision, warmup, repeat):
    g = ocffm.problem_from_dataset(ds, precision=precision)
    ocffm.srand(1)
    g.init()
    g.one_epoch()
    g.sync()
    U, X = g._keep[0], g._keep[1]
    rows, n = int(X.info["m"]), int(g._keep[2].info["m"])
    Xtr = ocffm.ImpData.from_rows(head_rows(ds.train, TRAIN_ROWS), ds=U.Ds)
    val_ms = timed(g, g.validate, warmup, repeat)
    rec_ms = timed(g, lambda: g.recommend(X, topn=TOPN), warmup, repeat)
    ev_ms = timed(g, lambda: g.evaluate(X, cuts=CUTS), warmup, repeat)
    tr_ms = timed(g, lambda: g.evaluate(Xtr, cuts=CUTS), warmup, repeat)
    e, v0 = g.evaluate(X, cuts=CUTS), g.validate()
    fam_te, fam_tr = family(g, X, name, repeat), family(g, Xtr, name, repeat)
    etr = g.evaluate(Xtr, cuts=CUTS)
    g.close()
    v, r, ev, tr = (statistics.median(x) for x in (val_ms, rec_ms, ev_ms, tr_ms))

    def stat(ms, med, nrows):
        return dict(ms_per_call=med, min_ms=min(ms), max_ms=max(ms), rows_per_s=nrows / med * 1e3,
                    item_scores_per_s=nrows * n / med * 1e3)

    res = dict(
        rows=rows, items=n, cuts=list(CUTS), topn=TOPN,
        validate=stat(val_ms, v, rows), recommend=stat(rec_ms, r, rows),
        evaluate=dict(stat(ev_ms, ev, rows), **fam_te, labels=e["labels"], labels_ranked=e["labels_ranked"],
                      ndcg=list(e["ndcg"]), prec=list(e["prec"]), mrr=e["mrr"], auc=e["auc"],
                      validate_ndcg=list(v0["ndcg"]), validate_prec=list(v0["prec"])),
        evaluate_train_rows=dict(stat(tr_ms, tr, TRAIN_ROWS), **fam_tr, rows=TRAIN_ROWS, labels=etr["labels"],
                                 labels_ranked=etr["labels_ranked"],
                                 max_labels_per_row=int(np.diff(ds.train.yptr[:TRAIN_ROWS + 1].astype(np.int64)).max())),
        evaluate_over_validate=ev / v, evaluate_over_recommend=ev / r,
    )
    print(f"{name}: validate {v:.3f} ms, recommend {r:.3f} ms, evaluate {ev:.3f} ms (x{ev / v:.4f} validate, "
          f"x{ev / r:.2f} recommend); family {fam_te['family_event_ms']:.3f} ms = {fam_te['family_tflops']:.2f} TF "
          f"({100 * fam_te['mfma_peak_fraction']:.1f} % of MFMA peak), host set-up {fam_te['host_setup_ms']:.3f} ms; "
          f"{TRAIN_ROWS} train rows ({etr['labels']} labels): {tr:.3f} ms, family "
          f"{fam_tr['family_event_ms']:.3f} ms, host set-up {fam_tr['host_setup_ms']:.3f} ms", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "evaluate_bench.json"))
    a = ap.parse_args()
    ds = synth.kkbox()
    out = dict(workload="synth.kkbox() k=32, one epoch, test rows (and the first 4096 train rows), cuts 5..80",
               repeat=a.repeat, warmup=a.warmup,
               timing="median wall ms per call, device sync before and after each call",
               mfma_peak_tf=MFMA_PEAK_TF)
    for name, prec in (("fp32", ocffm.FP32), ("fp64", ocffm.FP64)):
        out[name] = one(ds, name, prec, a.warmup, a.repeat)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
