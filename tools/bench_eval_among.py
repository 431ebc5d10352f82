"""Ranking evaluation among per-row candidate lists against the full sweep, on
the kkbox shape (synth.kkbox(), k = 32: 3,075 test rows x 100,000 items, 6
cross blocks), after one epoch: the Newton problem in fp32 and fp64, and the
SGD trainer's model (fp32).

Lists: 100 and 1,000 distinct uniformly random items per row (fixed seed,
tools/bench_rerank.py's).  Per model and list length, from calls with event
timing on: the kernel time of evaluate(candidates=) (family "evaluate":
k_eval_label_scores + k_rerank_count; the trainer's "rank_kernel_us") and the
call's host set-up ("eval_setup_us" / "rank_setup_us": the rows' layout and
the construction of the candidate sets), and the median wall time of repeated
calls; next to full evaluate() and recommend(candidates=, topn=80) on the same
rows in the same run.  Writes profiles/eval_among_bench.json.

Usage: python tools/bench_eval_among.py [--repeat N] [--warmup N] [--out path] [--lengths L[,L...]]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "one-class-ffm_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import ocffm  # noqa: E402
import synth  # noqa: E402
from bench_rerank import TOPN, lists, timed  # noqa: E402

CUTS = (5, 10, 20, 40, 80)


def newton_family(g, name, setup_counter, fn, repeat):
    """Event time of one kernel family and the call's host set-up (medians)."""
    g.set_profiling(True)
    g.set_profile_filter(name)
    fam, setup, st = [], [], None
    for _ in range(repeat):
        g.reset_stats()
        fn()
        st = g.kernel_stats()[name]
        fam.append(st["total_ms"])
        setup.append(g.counter(setup_counter) / 1e3)
    g.set_profiling(False)
    return statistics.median(fam), statistics.median(setup), int(st["launches"])


def sgd_family(t, fn, repeat):
    fam, setup = [], []
    for _ in range(repeat):
        fn()
        fam.append(t.counter("rank_kernel_us") / 1e3)
        setup.append(t.counter("rank_setup_us") / 1e3)
    return statistics.median(fam), statistics.median(setup), None


def measure(model, X, rows, n, lengths, warmup, repeat, family):
    """family(kind, fn) -> (kernel ms, set-up ms, launches) of one call of fn."""
    def entry(kind, fn):
        ms = timed(model, fn, warmup, repeat)
        fam, setup, launches = family(kind, fn)
        d = dict(ms_per_call=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), kernel_ms=fam, host_setup_ms=setup)
        if launches is not None:
            d["family_launches"] = launches
        return d

    res = dict(rows=rows, items=n, evaluate=entry("evaluate", lambda: model.evaluate(X, cuts=CUTS)))
    print(f"  evaluate: {res['evaluate']['ms_per_call']:.3f} ms per call, kernels {res['evaluate']['kernel_ms']:.3f} ms, "
          f"set-up {res['evaluate']['host_setup_ms']:.3f} ms", flush=True)
    for length in lengths:
        cand = lists(rows, n, length, seed=1000 + length)
        ev = entry("evaluate", lambda: model.evaluate(X, cuts=CUTS, candidates=cand))
        rr = entry("rerank", lambda: model.recommend(X, topn=TOPN, candidates=cand))
        ev["kernel_over_evaluate_kernel"] = ev["kernel_ms"] / res["evaluate"]["kernel_ms"]
        ev["call_over_evaluate_call"] = ev["ms_per_call"] / res["evaluate"]["ms_per_call"]
        res[f"lists_{length}"] = dict(pairs=rows * length, evaluate_among=ev, recommend_among=rr)
        print(f"  lists of {length}: evaluate(candidates=) {ev['ms_per_call']:.3f} ms per call, kernels "
              f"{ev['kernel_ms']:.3f} ms ({ev['kernel_over_evaluate_kernel']:.3f} of evaluate's), set-up "
              f"{ev['host_setup_ms']:.3f} ms; recommend(candidates=) {rr['ms_per_call']:.3f} ms, kernels "
              f"{rr['kernel_ms']:.3f} ms, set-up {rr['host_setup_ms']:.3f} ms", flush=True)
    return res


def newton(ds, name, precision, lengths, warmup, repeat):
    g = ocffm.problem_from_dataset(ds, precision=precision)
    ocffm.srand(1)
    g.init()
    g.one_epoch()
    g.sync()
    X = g._keep[1]
    rows, n = int(X.info["m"]), int(g._keep[2].info["m"])
    print(name, flush=True)
    fam = lambda kind, fn: newton_family(g, kind, "eval_setup_us" if kind == "evaluate" else "rec_setup_us", fn,  # noqa: E731
                                         repeat)
    res = measure(g, X, rows, n, lengths, warmup, repeat, fam)
    g.close()
    return res


def sgd(ds, lengths, warmup, repeat):
    U = ocffm.ImpData.from_rows(ds.train)
    V = ocffm.ImpData.from_rows(ds.item)
    X = ocffm.ImpData.from_rows(ds.test, ds=U.Ds)
    t = ocffm.SgdTrainer(U, V, k=ds.k, seed=9)
    t.epoch()
    t.sync()
    rows, n = int(X.info["m"]), int(V.info["m"])
    print("sgd", flush=True)
    res = measure(t, X, rows, n, lengths, warmup, repeat, lambda kind, fn: sgd_family(t, fn, repeat))
    t.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lengths", default="100,1000")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eval_among_bench.json"))
    a = ap.parse_args()
    lengths = [int(s) for s in a.lengths.split(",")]
    ds = synth.kkbox()
    out = dict(workload="synth.kkbox() k=32, one epoch, test rows; lists of distinct uniformly random items; "
                        "cuts 5,10,20,40,80; recommend topn=80",
               repeat=a.repeat, warmup=a.warmup,
               timing="median wall ms per call, device sync before and after each call; kernel times are HIP events "
                      "around the call's launches; host_setup_ms is the call's set-up counter")
    for name, prec in (("fp32", ocffm.FP32), ("fp64", ocffm.FP64)):
        out[name] = newton(ds, name, prec, lengths, a.warmup, a.repeat)
    out["sgd_fp32"] = sgd(ds, lengths, a.warmup, a.repeat)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
