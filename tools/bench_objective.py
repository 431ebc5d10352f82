"""Cost of the closed-form training objective against the epoch it reports on,
on the kkbox shape (synth.kkbox(), k = 32: 30,755 x 100,000, 6 cross blocks),
in fp32 and fp64.

Per precision, on one problem after a warm-up epoch: the median wall time of
repeated one_epoch() calls and of repeated objective() calls, each with the
device idle before and after every timed call (both end with a device sync),
and their ratio.  The `objective` kernel family's HIP-event time, its
algorithmic flops and bytes, and the achieved fraction of the MFMA peak (the
pair-Gram passes carry all the flops) come from calls of their own, since event
timing adds host work to a call.  Writes profiles/objective_bench.json.

Usage: python tools/bench_objective.py [--repeat N] [--warmup N] [--out path]
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
    g = ocffm.problem_from_dataset(ds, precision=precision, with_test=False)
    ocffm.srand(1)
    g.init()
    g.one_epoch()
    g.sync()
    ep_ms = timed(g, g.one_epoch, warmup, repeat)
    ob_ms = timed(g, g.objective, warmup, repeat)
    value = g.objective()
    g.set_profiling(True)
    g.set_profile_filter("objective")
    fam_ms, st = [], None
    for _ in range(repeat):
        g.reset_stats()
        g.objective()
        st = g.kernel_stats()["objective"]
        fam_ms.append(st["total_ms"])
    g.set_profiling(False)
    g.close()
    e, o, fam = statistics.median(ep_ms), statistics.median(ob_ms), statistics.median(fam_ms)
    res = dict(
        rows=int(value["m"]), items=int(value["n"]), labels=int(value["labels"]), value=value["value"],
        epoch=dict(ms_per_call=e, min_ms=min(ep_ms), max_ms=max(ep_ms)),
        objective=dict(ms_per_call=o, min_ms=min(ob_ms), max_ms=max(ob_ms),
                       family_event_ms=fam, family_launches=int(st["launches"]),
                       family_alg_flops=st["alg_flops"], family_alg_bytes=st["alg_bytes"],
                       family_tflops=st["alg_flops"] / fam / 1e9,
                       mfma_peak_fraction=st["alg_flops"] / fam / 1e9 / MFMA_PEAK_TF[name]),
        objective_over_epoch=o / e,
    )
    print(f"{name}: epoch {e:.3f} ms, objective {o:.3f} ms (ratio {o / e:.4f}); family {fam:.3f} ms over "
          f"{res['objective']['family_launches']} launches = {res['objective']['family_tflops']:.2f} TF "
          f"({100 * res['objective']['mfma_peak_fraction']:.1f} % of MFMA peak)", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "objective_bench.json"))
    a = ap.parse_args()
    ds = synth.kkbox()
    out = dict(workload="synth.kkbox() k=32, after warm-up epochs, no test set", repeat=a.repeat, warmup=a.warmup,
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
