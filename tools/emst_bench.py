#!/usr/bin/env python3
"""The exact MST from points on the device (device.emst, ghs_emst_device) next to one k-NN sweep on the same
points, and device.hdbscan_points(exact=True) next to exact=False and to scikit-learn, all in one process.

Per shape (n, d) and variant (plain: Euclidean MST; cores: mutual reachability with min_samples = 5), one entry:
  emst_ms          ghs_emst_result_t.ms_total of device.emst (the host wall time of the call; every round ends
                   in a stream synchronise); warmed up, repeated; median, min, max
  rounds           Boruvka rounds (the same in every repeat: the result is a function of the input)
  components       the components left after each round (ghs_emst_rounds)
  scan_ms          per round, the median over the repeats of the HIP-event time of the round's sweep
  scan_share       the sum of those medians over the median of emst_ms: what is left is the small kernels, the
                   host syncs, the sort and the events themselves
  knn1_ms          in the same run, ghs_knn_result_t.ms_total of device.knn(k = 1) on the same points: the
                   yardstick for one sweep (the same arithmetic, a k = 1 list selection)
  scan0_over_knn1  round 0's sweep median over the knn1 median
With --hdbscan LOG2N: wall times (ending in a device synchronise) of device.hdbscan_points at n = 2^LOG2N,
d = 16, min_cluster_size = min_samples = 5: exact=True, and exact=False at k = 15.
With --sklearn: scikit-learn's HDBSCAN(algorithm="brute") on the host at n = 2^10, 2^11, ... (d = 16) while a run
stays under --sklearn-budget seconds; the largest n that finished under a minute is reported with its time.

    python tools/emst_bench.py --out profiles/r19/emst_bench.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(1 << 14, 2), (1 << 14, 16), (1 << 14, 64), (1 << 17, 2), (1 << 17, 16), (1 << 17, 64)]
MIN_SAMPLES = 5


def spread(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "repeats": len(ts)}


def points(n, d, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn((n, d), dtype=torch.float32, device="cuda", generator=g)


def bench_shape(n, d, cores, seed, warmup, repeats):
    from distributed_ghs_implementation_amd import _native, device
    L = _native.load()
    x = points(n, d, seed)
    core2 = device.knn(x, MIN_SAMPLES - 1, metric="sqeuclidean").dist[:, MIN_SAMPLES - 2].contiguous() if cores else None
    ms, scans, comps, t = [], [], None, None
    L.ghs_emst_rounds(1, 0, None, None, None)
    for i in range(warmup + repeats):
        t = device.emst(x, core2=core2)
        r, c, s = ctypes.c_uint32(0), (ctypes.c_uint32 * 32)(), (ctypes.c_double * 32)()
        L.ghs_emst_rounds(1, 32, c, s, ctypes.byref(r))
        if i >= warmup:
            ms.append(t.info["ms_total"])
            scans.append(list(s)[:r.value])
            comps = list(c)[:r.value]
    L.ghs_emst_rounds(0, 0, None, None, None)
    k1 = []
    for i in range(warmup + repeats):
        nn = device.knn(x, 1)
        if i >= warmup:
            k1.append(nn.info["ms_total"])
    ours, knn1 = spread(ms), spread(k1)
    scan = [statistics.median(col) for col in zip(*scans)]
    return {"n": n, "d": d, "variant": "cores" if cores else "plain", "min_samples": MIN_SAMPLES if cores else None,
            "emst_ms": ours, "rounds": t.info["rounds"], "components": comps, "scan_ms": scan,
            "scan_share": sum(scan) / ours["median_ms"], "knn1_ms": knn1, "scan0_over_knn1": scan[0] / knn1["median_ms"],
            "info": {f: t.info[f] for f in ("slices", "query_tiles", "zero_edges", "pairs")}}


def bench_hdbscan(n, d, seed, repeats):
    import torch

    from distributed_ghs_implementation_amd import device
    x = points(n, d, seed)
    out = {"n": n, "d": d, "min_cluster_size": MIN_SAMPLES, "min_samples": MIN_SAMPLES}
    for name, kw in (("exact", {"exact": True}), ("knn_k15", {"k": 15})):
        ts, h = [], None
        for i in range(1 + repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h = device.hdbscan_points(x, min_cluster_size=MIN_SAMPLES, min_samples=MIN_SAMPLES, **kw)
            torch.cuda.synchronize()
            if i >= 1:
                ts.append((time.perf_counter() - t0) * 1e3)
        out[name] = {"wall_ms": spread(ts), "forest_trees": int(h.dendrogram.info["num_trees"]),
                     "clusters": {f: h.clusters.info[f] for f in ("num_selected", "num_noise")}}
    return out


def bench_sklearn(d, seed, budget_s, max_log2_n):
    import numpy as np
    try:
        from sklearn.cluster import HDBSCAN
    except ImportError:
        return {"measured": False, "why": "scikit-learn is not installed"}
    runs = []
    for lg in range(10, max_log2_n + 1):
        X = np.random.default_rng(seed).normal(size=(1 << lg, d))
        t0 = time.perf_counter()
        HDBSCAN(min_cluster_size=MIN_SAMPLES, min_samples=MIN_SAMPLES, algorithm="brute").fit(X)
        s = time.perf_counter() - t0
        runs.append({"n": 1 << lg, "seconds": s})
        if 4 * s > budget_s:          # brute force is quadratic: the next size takes about four times as long
            break
    under = [r for r in runs if r["seconds"] < 60]
    return {"measured": True, "d": d, "runs": runs, "largest_under_a_minute": under[-1] if under else None,
            "stopped_by": "budget" if runs and 4 * runs[-1]["seconds"] > budget_s else "max n"}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--max-log2-n", type=int, default=17, help="leave out the shapes above 2^N points")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--hdbscan", type=int, nargs="*", default=[17], metavar="LOG2N", help="log2 n of the hdbscan_points runs (d = 16)")
    ap.add_argument("--sklearn", action="store_true", help="time scikit-learn's brute HDBSCAN on the host too")
    ap.add_argument("--sklearn-budget", type=float, default=60.0, help="seconds the next scikit-learn run may be expected to take")
    ap.add_argument("--sklearn-max-log2-n", type=int, default=15)
    ap.add_argument("--out", type=str, default=None, help="JSON file to write")
    args = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "emst_bench needs a GPU (no fallback)"
    out = {"device": torch.cuda.get_device_name(0), "shapes": [], "hdbscan_points": [], "sklearn_brute": {"measured": False}}
    for n, d in SHAPES:
        if n > (1 << args.max_log2_n):
            continue
        for cores in (False, True):
            line = bench_shape(n, d, cores, args.seed, args.warmup, args.repeats)
            out["shapes"].append(line)
            print(json.dumps(line), flush=True)
    for lg in args.hdbscan:
        line = bench_hdbscan(1 << lg, 16, args.seed, 3)
        out["hdbscan_points"].append(line)
        print(json.dumps(line), flush=True)
    if args.sklearn:
        out["sklearn_brute"] = bench_sklearn(16, args.seed, args.sklearn_budget, args.sklearn_max_log2_n)
        print(json.dumps(out["sklearn_brute"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
