#!/usr/bin/env python3
"""Batched solve against a loop of single solves, same process, same GPU.

Two points:
  a  B = 65 536 Erdos-Renyi graphs of 6-20 vertices at p = 0.5, weights 1..10 — the shape of the
     reference's experiment loop (ghs_implementation.py main(), create_random_graph)
  b  B = 2 048 graphs of n = 1000 at p = 0.01 — the cgf_n1000_p001 fixture's shape
For each point: minimum_spanning_forest_batch over all B graphs (host arrays in, flags out: pack,
one ghs_mst_batch_host call, unpack) against a Python loop of minimum_spanning_forest over a
256-graph subset, its time scaled by B / 256. Both are host-clock times around calls that end in a
device synchronise, warmed up, repeated; the median and the min / max are reported. Also timed:
device.batch_mst on the device-resident batch (enqueue + sync + the results' D2H, no packing).
The subset's batch flags are compared with the loop's, graph by graph.

    python tools/batch_bench.py --point a --out profiles/r07/batch_bench.json
    python tools/batch_bench.py --point b --out profiles/r07/batch_bench.json   (merges into the file)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SUBSET = 256


def graphs_point_a(B, seed):
    """6-20 vertices, p = 0.5, integer weights 1..10; canonical by construction."""
    from distributed_ghs_implementation_amd import CanonicalGraph
    rng = np.random.default_rng(seed)
    pairs = {n: np.triu_indices(n, 1) for n in range(6, 21)}  # row-major = canonical order
    out = []
    for n in rng.integers(6, 21, B).tolist():
        a, b = pairs[n]
        keep = rng.random(len(a)) < 0.5
        out.append(CanonicalGraph(n, a[keep], b[keep], rng.integers(1, 11, int(keep.sum()))))
    return out


def graphs_point_b(B, seed, n=1000, p=0.01):
    from distributed_ghs_implementation_amd import CanonicalGraph
    rng = np.random.default_rng(seed)
    a, b = np.triu_indices(n, 1)
    out = []
    for _ in range(B):
        m = int(rng.binomial(len(a), p))
        idx = np.unique(rng.integers(0, len(a), m + m // 8 + 16))
        idx = np.sort(rng.permutation(idx)[:m])  # m distinct pairs, uniformly
        out.append(CanonicalGraph(n, a[idx], b[idx], rng.integers(1, 11, len(idx))))
    return out


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def spread(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "repeats": len(ts)}


def run_point(name, B, seed, warmup, repeats):
    import torch

    from distributed_ghs_implementation_amd import minimum_spanning_forest, minimum_spanning_forest_batch
    from distributed_ghs_implementation_amd.device import DeviceBatch, batch_mst
    assert torch.cuda.is_available(), "batch_bench needs a GPU (no fallback)"
    graphs = graphs_point_a(B, seed) if name == "a" else graphs_point_b(B, seed)
    edges = sum(g.m for g in graphs)
    sub = graphs[:: max(1, B // SUBSET)][:SUBSET]
    # the subset's flags: batch == loop
    bs = minimum_spanning_forest_batch(sub)
    ls = [minimum_spanning_forest(g) for g in sub]
    same = all(np.array_equal(x.in_mst, y.in_mst) and x.total_weight == y.total_weight for x, y in zip(bs, ls))
    assert same, "batch and single solves disagree"
    t_batch = timed(lambda: minimum_spanning_forest_batch(graphs), warmup, repeats)
    t_loop = timed(lambda: [minimum_spanning_forest(g) for g in sub], warmup, repeats)
    dev = DeviceBatch.from_graphs(graphs)
    torch.cuda.synchronize()
    t_dev = timed(lambda: batch_mst(dev), warmup, repeats)
    scale = B / len(sub)
    mb, ml, md = (statistics.median(t) for t in (t_batch, t_loop, t_dev))
    return {
        "point": name, "num_graphs": B, "edges": edges, "seed": seed, "loop_subset": len(sub),
        "batch_host": dict(spread(t_batch), graphs_per_s=B / mb, edges_per_s=edges / mb),
        "loop_subset_time": spread(t_loop),
        "loop_scaled": {"median_s": ml * scale, "min_s": min(t_loop) * scale, "max_s": max(t_loop) * scale,
                        "graphs_per_s": B / (ml * scale), "edges_per_s": edges / (ml * scale),
                        "per_solve_us": ml / len(sub) * 1e6},
        "batch_device_resident": dict(spread(t_dev), graphs_per_s=B / md, edges_per_s=edges / md),
        "ratio_loop_over_batch": ml * scale / mb,
        "ratio_loop_over_batch_worst": min(t_loop) * scale / max(t_batch),
        "subset_flags_equal": bool(same),
    }


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--point", choices=["a", "b"], required=True)
    ap.add_argument("--graphs", type=int, default=None, help="B (default: 65536 for a, 2048 for b)")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", type=str, default=None, help="JSON file to merge the point into")
    args = ap.parse_args(argv)
    B = args.graphs if args.graphs is not None else (65536 if args.point == "a" else 2048)
    rec = run_point(args.point, B, args.seed, args.warmup, args.repeats)
    print(json.dumps(rec))
    if args.out:
        doc = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                doc = json.load(f)
        doc[args.point] = rec
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=2, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
