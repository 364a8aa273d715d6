#!/usr/bin/env python3
"""The brute-force k-NN search on the device (device.knn, ghs_knn_device) next to the same answer from the
torch formulation (chunked torch.cdist + topk), and the split of device.hdbscan_points, all in one process.

Per shape (n, d, k), one entry:
  knn_ms           ghs_knn_result_t.ms_total of device.knn (the host wall time of the call, which ends in a
                   stream synchronise); warmed up, repeated; median, min, max
  torch_ms         wall time (ending in a device synchronise) of: for chunks of rows, torch.cdist against all
                   points, the diagonal set to inf, topk(k, largest=False); the chunk sized so that its
                   distance block stays under --chunk-bytes
  knn_over_torch   the ratio of the medians
  agree            the fraction of (row, rank) entries where both give the same index (the torch formulation
                   rounds differently and breaks ties its own way: below 1 is no error of either)
  fp32_rate        3 n^2 d / knn median: one subtraction and one fused multiply-add per pair and dimension, the
                   fma counted as two, over the whole call; and its share of the fp32 vector peak (157.3
                   TFLOP/s). The kernel issues two vector instructions for those three operations, so its
                   ceiling by instruction issue is 0.75 of that peak.
  info             slices, query_tiles, zero_neighbours
With --hdbscan: the split of device.hdbscan_points (min_cluster_size = min_samples = k) at the given shapes:
knn / canonicalise (knn_graph without the search) / the rest (device.hdbscan), each ending in a synchronise.

    python tools/knn_bench.py --out profiles/r18/knn_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP32_PEAK = 157.3e12   # MI355X fp32 vector peak, FLOP/s
SHAPES = [(1 << 14, 2, 15), (1 << 14, 16, 15), (1 << 14, 64, 15), (1 << 17, 2, 15), (1 << 17, 16, 15), (1 << 17, 64, 15),
          (1 << 17, 16, 5), (1 << 17, 16, 64), (1 << 20, 2, 15), (1 << 20, 16, 15), (1 << 20, 64, 15)]


def spread(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "repeats": len(ts)}


def torch_knn(x, k, chunk_bytes):
    import torch
    n = x.shape[0]
    rows = max(1, min(n, chunk_bytes // (4 * n)))
    idx = torch.empty((n, k), dtype=torch.int64, device=x.device)
    dist = torch.empty((n, k), dtype=torch.float32, device=x.device)
    for lo in range(0, n, rows):
        hi = min(n, lo + rows)
        d = torch.cdist(x[lo:hi], x)
        d[torch.arange(hi - lo, device=x.device), torch.arange(lo, hi, device=x.device)] = float("inf")
        dist[lo:hi], idx[lo:hi] = torch.topk(d, k, dim=1, largest=False)
    return idx, dist


def wall(fn, warmup, repeats):
    import torch
    ts, out = [], None
    for i in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return spread(ts), out


def bench_shape(n, d, k, seed, warmup, repeats, torch_repeats, chunk_bytes):
    import torch

    from distributed_ghs_implementation_amd import device
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((n, d), dtype=torch.float32, device="cuda", generator=g)
    ms, r = [], None
    for i in range(warmup + repeats):
        r = device.knn(x, k)
        if i >= warmup:
            ms.append(r.info["ms_total"])
    ours = spread(ms)
    line = {"n": n, "d": d, "k": k, "knn_ms": ours, "info": {f: r.info[f] for f in ("slices", "query_tiles", "zero_neighbours")}}
    flops = 3.0 * n * n * d
    rate = flops / (ours["median_ms"] * 1e-3)
    line["fp32_rate"] = {"flop": flops, "tflops": rate / 1e12, "share_of_vector_peak": rate / FP32_PEAK,
                         "bound": "fp32 vector issue (two instructions per three operations: ceiling 0.75)"}
    if torch_repeats > 0:
        tm, (ti, _) = wall(lambda: torch_knn(x, k, chunk_bytes), 1, torch_repeats)
        line["torch_ms"] = tm
        line["knn_over_torch"] = ours["median_ms"] / tm["median_ms"]
        line["agree"] = float((ti == (r.idx.to(torch.int64) & 0xFFFFFFFF)).float().mean())
        del ti
    return line


def bench_hdbscan(n, d, k, seed, warmup, repeats):
    import torch

    from distributed_ghs_implementation_amd import device
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((n, d), dtype=torch.float32, device="cuda", generator=g)
    parts = {"knn": [], "canonicalise": [], "rest": [], "total": []}
    h = None
    for i in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nn = device.knn(x, k)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ru = torch.arange(n, dtype=torch.int32, device="cuda").repeat_interleave(k)
        edges = device.canonicalize_device(n, ru, nn.idx.reshape(-1), nn.dist.reshape(-1), rank_weights=True)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        h = device.hdbscan(edges, min_cluster_size=max(k, 2), min_samples=k, include_self=True)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if i >= warmup:
            for name, a, b in (("knn", t0, t1), ("canonicalise", t1, t2), ("rest", t2, t3), ("total", t0, t3)):
                parts[name].append((b - a) * 1e3)
    return {"n": n, "d": d, "k": k, "m": edges.m, "split_ms": {name: spread(ts) for name, ts in parts.items()},
            "clusters": {f: h.clusters.info[f] for f in ("num_clusters", "num_selected", "num_noise")},
            "forest_trees": int(h.dendrogram.info["num_trees"])}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--max-log2-n", type=int, default=20, help="leave out the shapes above 2^N points")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--torch-repeats", type=int, default=7, help="0: leave the torch formulation out")
    ap.add_argument("--chunk-bytes", type=int, default=1 << 31, help="the torch formulation's distance block")
    ap.add_argument("--hdbscan", type=int, nargs="*", default=[17, 20], metavar="LOG2N",
                    help="log2 n of the hdbscan_points splits (d = 16, k = 15)")
    ap.add_argument("--out", type=str, default=None, help="JSON file to write")
    args = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "knn_bench needs a GPU (no fallback)"
    out = {"device": torch.cuda.get_device_name(0), "fp32_vector_peak_tflops": FP32_PEAK / 1e12, "shapes": [], "hdbscan_points": []}
    for n, d, k in SHAPES:
        if n > (1 << args.max_log2_n):
            continue
        line = bench_shape(n, d, k, args.seed, args.warmup, args.repeats, args.torch_repeats, args.chunk_bytes)
        out["shapes"].append(line)
        print(json.dumps(line), flush=True)
    for lg in args.hdbscan:
        if lg > args.max_log2_n:
            continue
        line = bench_hdbscan(1 << lg, 16, 15, args.seed, 1, 3)
        out["hdbscan_points"].append(line)
        print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
