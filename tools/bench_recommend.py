"""Top-N recommendation against validate() on the kkbox shape (synth.kkbox(),
k = 32: 3,075 test rows x 100,000 items, 6 cross blocks), after one epoch,
in fp32 and fp64, topn = 80, on the data set's own test rows.

Per precision: validate() (k_scores + k_rank, unchanged by the recommend
path: the baseline) and recommend() over the same rows, each as warm-up
calls, then the median wall time of repeated calls with the device idle
before and after every timed call (both calls end with a device sync).  The
`recommend` kernel family's HIP-event time (k_rec_topn + k_rec_merge) and
the call's host-side set-up (layout of X, projections, uploads: the
"rec_setup_us" counter) are reported separately.  Writes
profiles/recommend_bench.json.

Usage: python tools/bench_recommend.py [--repeat N] [--warmup N] [--out path]
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

MFMA_PEAK_TF = {"fp32": 157.3, "fp64": 78.6}
TOPN = 80


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


def one(ds, name, precision, warmup, repeat):
    g = ocffm.problem_from_dataset(ds, precision=precision)
    ocffm.srand(1)
    g.init()
    g.one_epoch()
    g.sync()
    X = g._keep[1]
    rows, n = int(X.info["m"]), int(g._keep[2].info["m"])
    val_ms = timed(g, g.validate, warmup, repeat)
    rec_ms = timed(g, lambda: g.recommend(X, topn=TOPN), warmup, repeat)
    # the family's event time and the host set-up, in calls of their own
    # (event timing adds host work to a call)
    g.set_profiling(True)
    g.set_profile_filter("recommend")
    fam_ms, setup_ms, st = [], [], None
    for _ in range(repeat):
        g.reset_stats()
        g.recommend(X, topn=TOPN)
        st = g.kernel_stats()["recommend"]
        fam_ms.append(st["total_ms"])
        setup_ms.append(g.counter("rec_setup_us") / 1e3)
    g.set_profiling(False)
    g.close()
    v, r, fam = statistics.median(val_ms), statistics.median(rec_ms), statistics.median(fam_ms)
    flops = st["alg_flops"]
    res = dict(
        rows=rows, items=n, topn=TOPN,
        validate=dict(ms_per_call=v, min_ms=min(val_ms), max_ms=max(val_ms), rows_per_s=rows / v * 1e3,
                      item_scores_per_s=rows * n / v * 1e3),
        recommend=dict(ms_per_call=r, min_ms=min(rec_ms), max_ms=max(rec_ms), rows_per_s=rows / r * 1e3,
                       item_scores_per_s=rows * n / r * 1e3,
                       host_setup_ms=statistics.median(setup_ms),
                       family_event_ms=fam, family_launches=int(st["launches"]),
                       family_alg_flops=flops, family_alg_bytes=st["alg_bytes"],
                       family_tflops=flops / fam / 1e9,
                       mfma_peak_fraction=flops / fam / 1e9 / MFMA_PEAK_TF[name]),
        recommend_over_validate=r / v,
    )
    print(f"{name}: validate {v:.3f} ms, recommend {r:.3f} ms (ratio {r / v:.4f}); family {fam:.3f} ms = "
          f"{res['recommend']['family_tflops']:.2f} TF ({100 * res['recommend']['mfma_peak_fraction']:.1f} % of "
          f"MFMA peak), host set-up {res['recommend']['host_setup_ms']:.3f} ms", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "recommend_bench.json"))
    a = ap.parse_args()
    ds = synth.kkbox()
    out = dict(workload="synth.kkbox() k=32, one epoch, test rows, topn=80", repeat=a.repeat, warmup=a.warmup,
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
