#!/usr/bin/env python3
"""Replacement edges of the engine's forest (device.forest_replacements) next to the path query, same process.

Per graph, one JSON line:
  forest           what forest_root found: trees, max depth (the index has K = max(1, bit_length) levels)
  solve_ms         ghs_result_t.ms_total of DeviceMST.run(): warmed up, repeated; median, min, max
  replace          workspace bytes, the counts of ghs_replace_result_t, total_ms (its ms_total: the host wall
                   time of the call, which ends in a stream synchronise) and, from HIP events recorded around
                   the phases of the same calls (ghs_forest_replace_phases): init_ms (the memsets), cover_ms,
                   push_down_ms (K - 1 launches), finish_ms
  query_edges_ms   ghs_paths_query_result_t.ms_total of PathIndex.query on the same index with the graph's own
                   m edges as pairs: the cover pass is that walk plus at most four lifts and four atomics per
                   edge, so this is its yardstick
  cover_over_query median cover_ms / median query_edges_ms: a ratio to report, not a gate
  checks           asserted whatever the times are: no replacement lighter than its MSF edge, every edge counted
                   once, two runs byte-equal

    python tools/replace_bench.py --graph rmat --scale 24 --out profiles/r13/replace_bench.json
    python tools/replace_bench.py --graph grid --scale 4096 --mode 0 --out profiles/r13/replace_bench.json   (merges)
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "repeats": len(ts)}


def run(graph, scale, mode, seed, warmup, repeats):
    import torch

    from distributed_ghs_implementation_amd import _native
    from distributed_ghs_implementation_amd.device import DeviceMST, forest_paths, generate_grid, generate_rmat
    assert torch.cuda.is_available(), "replace_bench needs a GPU (no fallback)"
    L = _native.load()
    e = generate_rmat(scale, 16, seed=seed, wseed=seed + 1) if graph == "rmat" else generate_grid(scale, mode, wseed=seed + 1)
    name = f"rmat-s{scale}-ef16" if graph == "rmat" else f"grid-{scale}x{scale}-mode{mode}"
    eng = DeviceMST(e)
    solve = []
    for i in range(warmup + repeats):
        res, _ = eng.run()
        if i >= warmup:
            solve.append(res.ms_total)
    rooted, rinfo = eng.rooted(order=False)
    assert rinfo["is_forest"] and rinfo["num_trees"] == e.n - res.num_mst_edges, rinfo
    line = {"graph": name, "n": e.n, "m": e.m, "solve_ms": spread(solve),
            "forest": {"num_trees": rinfo["num_trees"], "max_depth": rinfo["max_depth"], "root_ms": rinfo["ms_total"]}}
    index, info = forest_paths(e, rooted=rooted, max_depth=rinfo["max_depth"])
    line["index"] = {"levels": info["levels"], "index_bytes": info["index_bytes"], "create_ms": info["ms_total"]}
    ms = (ctypes.c_double * 4)()
    phases = {k: [] for k in ("init_ms", "cover_ms", "push_down_ms", "finish_ms")}
    total, first = [], None
    L.ghs_forest_replace_phases(1, None)
    for i in range(warmup + repeats):
        rep, xinfo = index.replacements(e)
        L.ghs_forest_replace_phases(1, ms)
        if first is None:
            first = (rep.key.clone(), rep.eid_by_edge.clone())
        else:
            assert torch.equal(rep.key, first[0]) and torch.equal(rep.eid_by_edge, first[1]), "runs differ"
        if i >= warmup:
            total.append(xinfo["ms_total"])
            for k, t in zip(phases, ms):
                phases[k].append(t)
        del rep
    L.ghs_forest_replace_phases(0, None)
    assert xinfo["improving"] == 0 and xinfo["best_delta"] >= 0, xinfo
    assert xinfo["tree_edges"] == res.num_mst_edges, xinfo
    assert xinfo["tree_edges"] + xinfo["covering_edges"] + xinfo["cross_edges"] == e.m, xinfo
    line["replace"] = {"workspace_bytes": int(L.ghs_forest_replace_workspace_bytes(e.n, rinfo["max_depth"])),
                       "counts": {k: v for k, v in xinfo.items() if k != "ms_total"}, "total_ms": spread(total),
                       **{k: spread(v) for k, v in phases.items()}}
    q = []
    for i in range(warmup + repeats):
        ans = index.query(e.u, e.v)
        if i >= warmup:
            q.append(ans.info["ms_total"])
    assert ans.info["connected"] == e.m
    line["query_edges_ms"] = spread(q)
    line["cover_over_query"] = line["replace"]["cover_ms"]["median_ms"] / line["query_edges_ms"]["median_ms"]
    line["checks"] = {"no_improving_replacement": True, "every_edge_counted_once": True, "runs_byte_equal": True}
    index.close()
    return line


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--graph", choices=["rmat", "grid"], default="rmat")
    ap.add_argument("--scale", type=int, default=20, help="R-MAT scale (2^scale vertices) / grid side k")
    ap.add_argument("--mode", type=int, default=0, help="grid weight mode (1: the road-like forest)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", type=str, default=None, help="JSON file to merge the line into, keyed by graph")
    args = ap.parse_args(argv)
    line = run(args.graph, args.scale, args.mode, args.seed, args.warmup, args.repeats)
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
