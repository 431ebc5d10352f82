"""Top-N among per-row candidate lists against the full sweep, on the kkbox
shape (synth.kkbox(), k = 32: 3,075 test rows x 100,000 items, 6 cross
blocks), after one epoch, in fp32 and fp64, topn = 80.

Lists: 100, 1,000 and 10,000 distinct uniformly random items per row (fixed
seed).  Baseline: recommend(topn=80) over all items on the same rows in the
same run, which is what a caller had before.  Per precision and list length:
the median wall time of repeated calls with the device idle before and after
every timed call, and, from calls of their own with event timing on, the
`rerank` kernel family's HIP-event time (k_rerank + k_rerank_merge), the
host-side set-up ("rec_setup_us"), pairs/s and gathered bytes/s (pairs x C x
KP x sizeof(real) over the family time), next to the random-row gather rates
measured for this chip.  score() of the 1,000-item lists' pairs is timed the
same way.  Writes profiles/rerank_bench.json.

Usage: python tools/bench_rerank.py [--repeat N] [--warmup N] [--out path]
                                    [--seg LEN[,LEN...]] [--lengths L[,L...]]
--seg runs every setting of OCFFM_REC_SEG given (0 = the default) on a
problem of its own; the first one is the one reported at the top level.
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
# chip-wide rates of uniformly random whole-row gathers (1,152-B rows): from a
# 38 MB table, from a 151 MB table, and into registers from a buffer far
# larger than the last-level cache
GATHER_TBS = {"38MB_table": 8.6, "151MB_table": 7.4, "beyond_cache_registers": 5.5}


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


def family(g, name, fn, repeat):
    """Event time of one kernel family and the call's host set-up (medians)."""
    g.set_profiling(True)
    g.set_profile_filter(name)
    fam, setup, st = [], [], None
    for _ in range(repeat):
        g.reset_stats()
        fn()
        st = g.kernel_stats()[name]
        fam.append(st["total_ms"])
        setup.append(g.counter("rec_setup_us") / 1e3)
    g.set_profiling(False)
    return statistics.median(fam), statistics.median(setup), st


_LISTS = {}


def lists(rows, n, length, seed):
    """`length` distinct uniformly random items per row."""
    if (rows, n, length, seed) in _LISTS:
        return _LISTS[(rows, n, length, seed)]
    rng = np.random.default_rng(seed)
    ccol = np.empty((rows, length), dtype=np.uint32)
    for i in range(rows):
        ccol[i] = rng.choice(n, size=length, replace=False)
    _LISTS[(rows, n, length, seed)] = (np.arange(rows + 1, dtype=np.uint64) * np.uint64(length), ccol.reshape(-1))
    return _LISTS[(rows, n, length, seed)]


def one(ds, name, precision, seg, lengths, warmup, repeat):
    if seg:
        os.environ["OCFFM_REC_SEG"] = str(seg)
    else:
        os.environ.pop("OCFFM_REC_SEG", None)
    g = ocffm.problem_from_dataset(ds, precision=precision)
    ocffm.srand(1)
    g.init()
    g.one_epoch()
    g.sync()
    X = g._keep[1]
    rows, n = int(X.info["m"]), int(g._keep[2].info["m"])
    depth_bytes = 6 * 32 * (4 if precision == ocffm.FP32 else 8)  # C x KP x sizeof(real)
    rec_ms = timed(g, lambda: g.recommend(X, topn=TOPN), warmup, repeat)
    rec_fam, rec_setup, _ = family(g, "recommend", lambda: g.recommend(X, topn=TOPN), repeat)
    res = dict(rows=rows, items=n, topn=TOPN, seg=seg or "default",
               recommend=dict(ms_per_call=statistics.median(rec_ms), min_ms=min(rec_ms), max_ms=max(rec_ms),
                              family_event_ms=rec_fam, host_setup_ms=rec_setup))
    print(f"{name} seg={seg or 'default'}: recommend {res['recommend']['ms_per_call']:.3f} ms, family "
          f"{rec_fam:.3f} ms, set-up {rec_setup:.3f} ms", flush=True)
    for length in lengths:
        cand = lists(rows, n, length, seed=1000 + length)
        call = lambda: g.recommend(X, topn=TOPN, candidates=cand)  # noqa: E731
        ms = timed(g, call, warmup, repeat)
        fam, setup, st = family(g, "rerank", call, repeat)
        pairs = rows * length
        r = dict(pairs=pairs, ms_per_call=statistics.median(ms), min_ms=min(ms), max_ms=max(ms),
                 family_event_ms=fam, family_launches=int(st["launches"]), host_setup_ms=setup,
                 family_alg_bytes=st["alg_bytes"], family_alg_flops=st["alg_flops"],
                 pairs_per_s=pairs / fam * 1e3, gathered_tb_per_s=pairs * depth_bytes / fam / 1e9,
                 family_over_recommend_family=fam / rec_fam)
        if length == 1000:
            prow = np.repeat(np.arange(rows, dtype=np.uint32), length)
            sc = lambda: g.score(X, prow, cand[1])  # noqa: E731
            sms = timed(g, sc, warmup, repeat)
            sfam, ssetup, _ = family(g, "rerank", sc, repeat)
            r["score"] = dict(ms_per_call=statistics.median(sms), family_event_ms=sfam, host_setup_ms=ssetup,
                              gathered_tb_per_s=2 * pairs * depth_bytes / sfam / 1e9)
        res[f"lists_{length}"] = r
        print(f"{name} seg={seg or 'default'} lists of {length}: {r['ms_per_call']:.3f} ms per call, family "
              f"{fam:.3f} ms ({fam / rec_fam:.3f} of recommend's), set-up {setup:.3f} ms, "
              f"{r['pairs_per_s'] / 1e9:.2f} G pairs/s, {r['gathered_tb_per_s']:.2f} TB/s gathered", flush=True)
    g.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seg", default="0")
    ap.add_argument("--lengths", default="100,1000,10000")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rerank_bench.json"))
    a = ap.parse_args()
    segs = [int(s) for s in a.seg.split(",")]
    lengths = [int(s) for s in a.lengths.split(",")]
    ds = synth.kkbox()
    out = dict(workload="synth.kkbox() k=32, one epoch, test rows, topn=80; lists of distinct uniformly random items",
               repeat=a.repeat, warmup=a.warmup,
               timing="median wall ms per call, device sync before and after each call; family times are HIP events",
               random_row_gather_tb_per_s=GATHER_TBS)
    for name, prec in (("fp32", ocffm.FP32), ("fp64", ocffm.FP64)):
        runs = [one(ds, name, prec, seg, lengths, a.warmup, a.repeat) for seg in segs]
        out[name] = runs[0]
        if len(runs) > 1:
            out[name + "_seg_sweep"] = runs[1:]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
