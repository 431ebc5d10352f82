"""Serving from a saved model against serving from a problem, on the kkbox
shape (synth.kkbox(), k = 32: 3,075 test rows x 100,000 items, 6 cross blocks),
in fp32 and fp64, in one run.

Per precision a problem is trained for one epoch and writes its binary
snapshot.  Then, timed: Model.load_binary of that file; Model.set_items of the
100,000-item catalogue (wall time, and the "project_us" counter: the fused
projection launch with its sync); and recommend(topn=80) and evaluate() on the
test split through the model and through a second problem that loaded the same
snapshot: the median wall time of repeated calls (every call ends with a
device sync), the serving kernels' time, and the host set-up counters
("rec_setup_us" / "eval_setup_us"), which hold each host's projection of the
query rows: one k_project_side launch in the model, one k_utx launch per cross
block plus three launches and a sync per side block in the problem.  The
kernel times are not measured alike: the problem's are event pairs carried by
the dispatch packets (its kernel_stats), the model's plain events around the
launches ("rank_kernel_us"), which include the gaps between them.  The results
of the two hosts are compared bit for bit.  Writes profiles/model_bench.json.

Usage: python tools/bench_model.py [--repeat N] [--warmup N] [--out path]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
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


def popularity(U):
    _, ycol = U.labels()
    cnt = np.bincount(ycol.astype(np.int64), minlength=int(U.info["n"])).astype(np.float64)
    return cnt / cnt.sum()


def serve_problem(g, X, warmup, repeat):
    out = {}
    for name, family, counter, fn in (("recommend", "recommend", "rec_setup_us", lambda: g.recommend(X, topn=TOPN)),
                                      ("evaluate", "evaluate", "eval_setup_us", lambda: g.evaluate(X))):
        res = wall(fn, warmup, repeat)
        g.set_profiling(True)
        g.set_profile_filter(family)
        fam, setup = [], []
        for _ in range(repeat):
            g.reset_stats()
            fn()
            fam.append(g.kernel_stats()[family]["total_ms"])
            setup.append(g.counter(counter) / 1e3)
        g.set_profiling(False)
        res.update(kernel_ms=statistics.median(fam), setup_ms=statistics.median(setup), setup_min_ms=min(setup),
                   setup_max_ms=max(setup))
        out[name] = res
    return out


def serve_model(M, X, warmup, repeat):
    out = {}
    for name, counter, fn in (("recommend", "rec_setup_us", lambda: M.recommend(X, topn=TOPN)),
                              ("evaluate", "eval_setup_us", lambda: M.evaluate(X))):
        res = wall(fn, warmup, repeat)
        fam, setup = [], []
        for _ in range(repeat):
            fn()
            fam.append(M.counter("rank_kernel_us") / 1e3)
            setup.append(M.counter(counter) / 1e3)
        res.update(kernel_ms=statistics.median(fam), setup_ms=statistics.median(setup), setup_min_ms=min(setup),
                   setup_max_ms=max(setup))
        out[name] = res
    return out


def one(ds, name, precision, warmup, repeat, tmp):
    g = ocffm.problem_from_dataset(ds, precision=precision)
    ocffm.srand(1)
    g.init()
    g.one_epoch()
    path = os.path.join(tmp, f"kkbox_{name}.bin")
    g.save_binary(path)
    g.close()
    g2 = ocffm.problem_from_dataset(ds, precision=precision)
    t = time.perf_counter()
    g2.load_binary(path)
    g2.sync()
    problem_load_ms = (time.perf_counter() - t) * 1e3
    U, X, V = g2._keep
    loads = []
    for _ in range(max(3, repeat)):
        t = time.perf_counter()
        M = ocffm.Model.load_binary(path, precision)
        loads.append((time.perf_counter() - t) * 1e3)
        M.close()
    M = ocffm.Model.load_binary(path, precision)
    sets, proj = [], []
    for _ in range(warmup + repeat):
        t = time.perf_counter()
        M.set_items(V)
        sets.append((time.perf_counter() - t) * 1e3)
        proj.append(M.counter("project_us") / 1e3)
    sets, proj = sets[warmup:], proj[warmup:]
    M.set_popularity(popularity(U))
    a, b = g2.recommend(X, topn=TOPN), M.recommend(X, topn=TOPN)
    same = bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
    ea, eb = g2.evaluate(X), M.evaluate(X)
    same = same and all(np.array_equal(np.asarray(ea[k]), np.asarray(eb[k])) for k in ea)
    res = dict(rows=int(X.info["m"]), items=int(V.info["m"]), topn=TOPN, file_bytes=os.path.getsize(path),
               model_load_ms=statistics.median(loads), model_load_min_ms=min(loads), model_load_max_ms=max(loads),
               problem_load_binary_ms=problem_load_ms,
               set_items_ms=statistics.median(sets), set_items_min_ms=min(sets), set_items_max_ms=max(sets),
               project_ms=statistics.median(proj), project_min_ms=min(proj), project_max_ms=max(proj),
               results_identical=same,
               problem=serve_problem(g2, X, warmup, repeat), model=serve_model(M, X, warmup, repeat))
    for call in ("recommend", "evaluate"):
        res[call + "_setup_model_over_problem"] = res["model"][call]["setup_ms"] / res["problem"][call]["setup_ms"]
    print(f"{name}: load {res['model_load_ms']:.2f} ms, set_items {res['set_items_ms']:.2f} ms (project "
          f"{res['project_ms']:.3f} ms), identical {same}", flush=True)
    for call in ("recommend", "evaluate"):
        p, m = res["problem"][call], res["model"][call]
        print(f"  {call}: problem {p['ms']:.3f} ms (kernels {p['kernel_ms']:.3f}, set-up {p['setup_ms']:.3f}), "
              f"model {m['ms']:.3f} ms (kernels {m['kernel_ms']:.3f}, set-up {m['setup_ms']:.3f})", flush=True)
    M.close()
    g2.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "model_bench.json"))
    a = ap.parse_args()
    ds = synth.kkbox()
    out = dict(workload="synth.kkbox() k=32, one epoch, binary snapshot; test rows, topn=80, cuts 5..80",
               repeat=a.repeat, warmup=a.warmup,
               timing="median wall ms per call (every call ends with a device sync); kernel_ms: problem = "
                      "dispatch-carried event pairs of the family, model = plain events around the launches")
    with tempfile.TemporaryDirectory() as tmp:
        for name, prec in (("fp32", ocffm.FP32), ("fp64", ocffm.FP64)):
            out[name] = one(ds, name, prec, a.warmup, a.repeat, tmp)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
