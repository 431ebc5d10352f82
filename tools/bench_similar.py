"""Similar items against recommend on the kkbox-shape catalogue (synth.kkbox(),
k = 32: 100,000 items, 6 cross blocks, depth 192), after one epoch, on a model
taken from the problem, in fp32 and fp64, topn = 10.

Per precision, in one process:
  recommend      Model.recommend on 4,096 user rows (the yardstick: the same sweep)
  similar_4096   Model.similar_items of 4,096 query items
  similar_all    Model.similar_items of all 100,000 items (chunks of 4,096 queries)
  norm_build     the catalogue's inverse norms ("sim_norm_us": launch to sync, on
                 the first similarity call after set_items)
  gather         the query gathers of the similar_4096 call ("sim_gather_us")
Each call is warmed up, then repeated: the median wall time per call with the
device idle before and after (every entry ends with a device sync), the
median of the call's launches between HIP events ("rank_kernel_us": the sweep,
the merge and, for similar_items, the gather) and the item-scores per second
those give.  Writes profiles/similar_bench.json.

Usage: python tools/bench_similar.py [--repeat N] [--warmup N] [--out path]
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

TOPN = 10
ROWS = 4096


def timed(M, fn, counters, warmup, repeat):
    """wall ms and the named counters (us) of `repeat` calls after `warmup`."""
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


def summary(wall, kernel, pairs):
    k = statistics.median(kernel)
    return dict(ms_per_call=statistics.median(wall), min_ms=min(wall), max_ms=max(wall),
                kernel_ms=k, kernel_min_ms=min(kernel), kernel_max_ms=max(kernel),
                g_item_scores_per_s=pairs / k / 1e6,
                g_item_scores_per_s_min=pairs / max(kernel) / 1e6, g_item_scores_per_s_max=pairs / min(kernel) / 1e6)


def one(ds, name, precision, warmup, repeat):
    g = ocffm.problem_from_dataset(ds, precision=precision)
    ocffm.srand(1)
    g.init()
    g.one_epoch()
    g.sync()
    U, _, V = g._keep
    M = ocffm.Model.from_problem(g)
    g.close()
    i = M.info
    n, depth = int(i["n"]), int(i["fu"]) * int(i["fv"]) * int(i["kp"])
    esz = 4 if name == "fp32" else 8
    rng = np.random.default_rng(5)
    q = rng.choice(n, size=ROWS, replace=False).astype(np.uint32)
    res = dict(items=n, depth=depth, topn=TOPN, rows=ROWS)
    wall, c = timed(M, lambda: M.recommend(U, topn=TOPN, row0=0, rows=ROWS), ["rank_kernel_us", "rec_setup_us"],
                    warmup, repeat)
    res["recommend"] = summary(wall, c["rank_kernel_us"], ROWS * n)
    res["recommend"]["host_setup_ms"] = statistics.median(c["rec_setup_us"])
    wall, c = timed(M, lambda: M.similar_items(q, topn=TOPN), ["rank_kernel_us", "sim_setup_us", "sim_gather_us"],
                    warmup, repeat)
    res["similar_4096"] = summary(wall, c["rank_kernel_us"], ROWS * n)
    res["similar_4096"]["host_setup_ms"] = statistics.median(c["sim_setup_us"])
    gus = statistics.median(c["sim_gather_us"])
    gbytes = ROWS * (2 * depth * esz + esz + 4)
    res["gather"] = dict(ms_per_chunk=gus, min_ms=min(c["sim_gather_us"]), max_ms=max(c["sim_gather_us"]),
                         alg_bytes=gbytes, gb_per_s=gbytes / gus / 1e6)
    allq = np.arange(n, dtype=np.uint32)
    wall, c = timed(M, lambda: M.similar_items(allq, topn=TOPN), ["rank_kernel_us"], 1, max(3, repeat // 2))
    res["similar_all"] = summary(wall, c["rank_kernel_us"], n * n)
    res["similar_all"]["queries"] = n
    # the norm build: once per catalogue, so every sample sets the catalogue again
    nus = []
    for _ in range(repeat):
        M.set_items(V)
        M.item_similarity(q[:1], q[1:2])
        nus.append(M.counter("sim_norm_us") / 1e3)
    nbytes = n * (depth * esz + esz)
    res["norm_build"] = dict(ms=statistics.median(nus), min_ms=min(nus), max_ms=max(nus), alg_bytes=nbytes,
                             gb_per_s=nbytes / statistics.median(nus) / 1e6, builds=M.counter("sim_norm_builds"))
    r, s = res["recommend"], res["similar_4096"]
    res["similar_over_recommend_kernel_rate"] = s["g_item_scores_per_s"] / r["g_item_scores_per_s"]
    res["similar_all_over_recommend_kernel_rate"] = res["similar_all"]["g_item_scores_per_s"] / r["g_item_scores_per_s"]
    M.close()
    print(f"{name}: recommend {r['ms_per_call']:.3f} ms (kernels {r['kernel_ms']:.3f} ms, "
          f"{r['g_item_scores_per_s']:.1f} G/s [{r['g_item_scores_per_s_min']:.1f}, {r['g_item_scores_per_s_max']:.1f}]); "
          f"similar_items 4096: {s['ms_per_call']:.3f} ms (kernels {s['kernel_ms']:.3f} ms, "
          f"{s['g_item_scores_per_s']:.1f} G/s [{s['g_item_scores_per_s_min']:.1f}, {s['g_item_scores_per_s_max']:.1f}]), "
          f"ratio {res['similar_over_recommend_kernel_rate']:.4f}; all {n}: {res['similar_all']['ms_per_call']:.1f} ms "
          f"(kernels {res['similar_all']['kernel_ms']:.1f} ms, {res['similar_all']['g_item_scores_per_s']:.1f} G/s); "
          f"norms {res['norm_build']['ms']:.3f} ms ({res['norm_build']['gb_per_s']:.0f} GB/s); "
          f"gather {gus:.3f} ms ({res['gather']['gb_per_s']:.0f} GB/s)", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "similar_bench.json"))
    a = ap.parse_args()
    ds = synth.kkbox()
    out = dict(workload="synth.kkbox() k=32, one epoch, Model.from_problem; topn=10; 4,096 rows / query items, and all items",
               repeat=a.repeat, warmup=a.warmup,
               timing="median over calls; ms_per_call: wall, every entry ends with a device sync; kernel_ms: the "
                      "call's launches between HIP events (rank_kernel_us); [min, max] over the repeats is the spread")
    for name, prec in (("fp32", ocffm.FP32), ("fp64", ocffm.FP64)):
        out[name] = one(ds, name, prec, a.warmup, a.repeat)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
