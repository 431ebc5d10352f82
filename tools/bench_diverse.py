"""Diversified top-N against recommend on the kkbox-shape catalogue
(synth.kkbox(), k = 32: 100,000 items, 6 cross blocks, depth 192), after one
epoch, on a model taken from the problem, the 3,075 rows of the test split, in
fp32 and fp64, all in one process.

Per precision:
  recommend_40 / recommend_128   Model.recommend(topn = pool): the yardstick,
                                 the sweep and merge the diverse call runs too
  diverse_10_40 / diverse_80_128 Model.recommend_diverse(topn, pool) at theta 0.3
Each call is warmed up, then repeated: the median wall time per call (every
entry ends with a device sync), the median of the call's launches between HIP
events ("rank_kernel_us"; for the diverse calls it includes k_mmr) and k_mmr's
own share ("div_kernel_us"), each with [min, max] over the repeats.  The ratio
written is the diverse call's kernel time over the yardstick's at the same
pool, from the same run.  Writes profiles/diverse_bench.json.

Usage: python tools/bench_diverse.py [--repeat N] [--warmup N] [--out path]
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

THETA = 0.3
SHAPES = ((10, 40), (80, 128))  # (topn, pool)


def timed(M, fn, counters, warmup, repeat):
    """wall ms and the named counters (ms) of `repeat` calls after `warmup`."""
    for _ in range(warmup):
        fn()
    wall, cnt = [], {c: [] for c in counters}
    for _ in range(repeat):
        t = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t) * 1e3)
        for c in counters:
            cnt[c].append(M.counter(c) / 1e3)
    return wall, cnt


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def one(ds, name, precision, warmup, repeat):
    g = ocffm.problem_from_dataset(ds, precision=precision)
    ocffm.srand(1)
    g.init()
    g.one_epoch()
    g.sync()
    X = g._keep[1]
    M = ocffm.Model.from_problem(g)
    rows = int(X.info["m"])
    i = M.info
    res = dict(items=int(i["n"]), depth=int(i["fu"]) * int(i["fv"]) * int(i["kp"]), rows=rows, theta=THETA)
    M.item_similarity([0], [1])  # the norm build is paid once per catalogue, outside the timed calls
    res["norm_build_ms"] = M.counter("sim_norm_us") / 1e3
    for topn, pool in SHAPES:
        wall, c = timed(M, lambda: M.recommend(X, topn=pool), ["rank_kernel_us", "rec_setup_us"], warmup, repeat)
        y = dict(call_ms=spread(wall), rank_kernel_ms=spread(c["rank_kernel_us"]),
                 host_setup_ms=spread(c["rec_setup_us"]))
        res[f"recommend_{pool}"] = y
        wall, c = timed(M, lambda: M.recommend_diverse(X, topn=topn, theta=THETA, pool=pool),
                        ["rank_kernel_us", "div_kernel_us", "div_setup_us"], warmup, repeat)
        d = dict(topn=topn, pool=pool, call_ms=spread(wall), rank_kernel_ms=spread(c["rank_kernel_us"]),
                 div_kernel_ms=spread(c["div_kernel_us"]), host_setup_ms=spread(c["div_setup_us"]))
        d["kernel_over_yardstick"] = d["rank_kernel_ms"]["median"] / y["rank_kernel_ms"]["median"]
        d["div_over_yardstick_kernel"] = d["div_kernel_ms"]["median"] / y["rank_kernel_ms"]["median"]
        d["call_over_yardstick"] = d["call_ms"]["median"] / y["call_ms"]["median"]
        res[f"diverse_{topn}_{pool}"] = d
        print(f"{name} pool {pool}: recommend {y['call_ms']['median']:.3f} ms (kernels "
              f"{y['rank_kernel_ms']['median']:.3f} [{y['rank_kernel_ms']['min']:.3f}, {y['rank_kernel_ms']['max']:.3f}]); "
              f"diverse topn {topn}: {d['call_ms']['median']:.3f} ms (kernels {d['rank_kernel_ms']['median']:.3f} "
              f"[{d['rank_kernel_ms']['min']:.3f}, {d['rank_kernel_ms']['max']:.3f}], k_mmr "
              f"{d['div_kernel_ms']['median']:.3f} [{d['div_kernel_ms']['min']:.3f}, {d['div_kernel_ms']['max']:.3f}]); "
              f"kernels over yardstick {d['kernel_over_yardstick']:.3f}, k_mmr over yardstick "
              f"{d['div_over_yardstick_kernel']:.3f}", flush=True)
    M.close()
    g.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "diverse_bench.json"))
    a = ap.parse_args()
    ds = synth.kkbox()
    out = dict(workload="synth.kkbox() k=32, one epoch, Model.from_problem; the test split's rows; theta 0.3; "
                        "recommend(topn=pool) against recommend_diverse(topn, pool) for (10, 40) and (80, 128)",
               repeat=a.repeat, warmup=a.warmup,
               timing="median [min, max] over calls; call_ms: wall, every entry ends with a device sync; "
                      "rank_kernel_ms: the call's launches between HIP events; div_kernel_ms: k_mmr's share of them")
    for name, prec in (("fp32", ocffm.FP32), ("fp64", ocffm.FP64)):
        out[name] = one(ds, name, prec, a.warmup, a.repeat)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
