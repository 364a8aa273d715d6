#!/usr/bin/env python3
"""Vertex labels of the engine's forest (device.forest_labels) next to the solve that made it, same process.

Per graph, one JSON line:
  labels_ms        per cut mode, ghs_labels_result_t.ms_total of DeviceMST.labels() on the engine's flags
                   (the host wall time of the call, which ends in a stream synchronise): warmed up,
                   repeated; median, min, max. Modes: none (the graph's connected components),
                   count (num_clusters = --clusters), weight (max_weight = the median weight of the
                   flagged edges, so about half of the forest is kept)
  labels_python_wall_ms
                   the same calls timed around the Python entry (workspace allocation included)
  engine_ms        ghs_result_t.ms_total of DeviceMST.run() on the same device-resident list, same way
  info             per mode, the call's result fields (flagged / kept / dropped edges, clusters, rounds)
  checks           what the numbers must satisfy whatever they are: no cut gives n - num_mst_edges
                   clusters, the count cut max(k, components), both cuts on a forest stay forests
  model            HBM bytes the passes move, from the shapes alone (DESIGN.md "Vertex labels and forest
                   cuts"), and the time they would take at the measured copy rate: a lower bound from a
                   byte count, not a measurement — the passes gather and hook through atomics

    python tools/labels_bench.py --graph rmat --scale 20 --out profiles/r10/labels_bench.json
    python tools/labels_bench.py --graph grid --scale 4096 --out profiles/r10/labels_bench.json   (merges)
    python tools/labels_bench.py --graph rmat --scale 24 --out profiles/r10/labels_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_COPY_TBS = 6.29  # measured copy rate of the micro-architecture notes


def spread(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "repeats": len(ts)}


def model_bytes(n, m, flagged, kept, mode):
    """Bytes per pass from the shapes (no measurement). The rounds are counted for round 1 only (the
    live list shrinks geometrically after it)."""
    b = {
        "check_canonical": 8 * m,                                   # u, v
        "flag_count": m + (4 * flagged if mode == "weight" else 0),  # the flags (+ w gathered per flagged edge)
        "init": 8 * n,                                              # par, marks
        "write_edges": m + kept * (8 + 8) + (4 * flagged if mode != "none" else 0) + (8 * flagged if mode == "count" else 0),
        "round1_hook_jump_compact": kept * (8 + 4) + kept * (8 + 8) + kept * (8 + 8 + 8),
        "final_jump_rank_labels": n * (4 + 4) + n * 4 + n * (4 + 4) + n * (4 + 4 + 4),
    }
    if mode == "count":
        b["select_and_cut"] = 8 * 8 * flagged + flagged * (8 + 8) + kept * 8
    total = sum(b.values())
    return {"bytes": b, "total_bytes_lower_bound": total, "bound_ms_at_copy_rate": total / (HBM_COPY_TBS * 1e12) * 1e3}


def run(graph, scale, seed, warmup, repeats, clusters):
    import torch

    from distributed_ghs_implementation_amd.device import DeviceMST, flags_to_eids, generate_grid, generate_rmat
    assert torch.cuda.is_available(), "labels_bench needs a GPU (no fallback)"
    e = generate_rmat(scale, 16, seed=seed, wseed=seed + 1) if graph == "rmat" else generate_grid(scale, 0, wseed=seed + 1)
    name = f"rmat-s{scale}-ef16" if graph == "rmat" else f"grid-{scale}x{scale}"
    eng = DeviceMST(e)
    eng_ms = []
    for i in range(warmup + repeats):
        res, _ = eng.run()
        torch.cuda.synchronize()
        if i >= warmup:
            eng_ms.append(res.ms_total)
    eids = flags_to_eids(eng.in_mst, 0, e.m)
    wmed = int((e.w[eids].to(torch.int64) & 0xFFFFFFFF).median()) if eids.numel() else 0
    del eids
    cuts = {"none": {}, "count": {"num_clusters": clusters}, "weight": {"max_weight": wmed}}
    line = {"graph": name, "n": e.n, "m": e.m, "engine_ms": spread(eng_ms), "engine_rounds": res.rounds,
            "engine_totals": {"num_mst_edges": res.num_mst_edges, "total_weight": res.total_weight},
            "clusters_asked": clusters, "median_flagged_weight": wmed,
            "labels_ms": {}, "labels_python_wall_ms": {}, "info": {}, "model": {}, "labels_over_engine": {}}
    comps = e.n - res.num_mst_edges
    for mode, cut in cuts.items():
        ms, wall = [], []
        for i in range(warmup + repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            labels, info = eng.labels(**cut)
            dt = (time.perf_counter() - t0) * 1e3
            if i >= warmup:
                ms.append(info["ms_total"])
                wall.append(dt)
        line["labels_ms"][mode] = spread(ms)
        line["labels_python_wall_ms"][mode] = spread(wall)
        line["info"][mode] = {k: info[k] for k in ("flagged_edges", "kept_edges", "dropped_edges", "num_clusters",
                                                   "rounds", "is_forest")}
        line["model"][mode] = model_bytes(e.n, e.m, info["flagged_edges"], info["kept_edges"], mode)
        line["labels_over_engine"][mode] = line["labels_ms"][mode]["median_ms"] / line["engine_ms"]["median_ms"]
        distinct = int(labels.max()) + 1 if e.n else 0
        assert distinct == info["num_clusters"] and int(labels[0]) == 0, (mode, distinct, info)
        del labels
    inf = line["info"]
    line["checks"] = {
        "none_clusters_equal_components": inf["none"]["num_clusters"] == comps,
        "count_clusters_equal_max_k_components": inf["count"]["num_clusters"] == max(min(clusters, e.n), comps),
        "weight_clusters_equal_n_minus_kept": inf["weight"]["num_clusters"] == e.n - inf["weight"]["kept_edges"],
        "all_forests": all(inf[k]["is_forest"] for k in inf),
    }
    assert all(line["checks"].values()), line["checks"]
    return line


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--graph", choices=["rmat", "grid"], default="rmat")
    ap.add_argument("--scale", type=int, default=20, help="R-MAT scale (2^scale vertices) / grid side k")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--clusters", type=int, default=1000, help="k of the count cut")
    ap.add_argument("--out", type=str, default=None, help="JSON file to merge the line into, keyed by graph")
    args = ap.parse_args(argv)
    line = run(args.graph, args.scale, args.seed, args.warmup, args.repeats, args.clusters)
    print(json.dumps(line), flush=True)
    if args.out:
        merged = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                merged = json.load(f)
        merged[line["graph"]] = line
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(merged, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
