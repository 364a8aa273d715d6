#!/usr/bin/env python3
"""The engine's forest's single-linkage dendrogram on the device (device.forest_dendrogram) next to the
solve that made the forest and to forest_root on the same flags, same process.

Per graph, one JSON line:
  dendro_ms        ghs_dendro_result_t.ms_total of DeviceMST.dendrogram() on the engine's flags (the host
                   wall time of the call, which ends in a stream synchronise): warmed up, repeated; median,
                   min, max. Modes: full (children and sizes), parents (both left out)
  dendro_python_wall_ms
                   the same calls timed around the Python entry (output and workspace allocation included)
  root_ms          ghs_root_result_t.ms_total of DeviceMST.rooted() (all five arrays), same way: comparable
                   sort plus doubling work on the same forest
  engine_ms        ghs_result_t.ms_total of DeviceMST.run() on the same device-resident list, same way
  host_ms          what a user does without the call: flags_d2h (the flags copied to the host), and
                   kruskal_c (the serial C sort + union-find of the checker over the forest's edges alone,
                   which finds the merge order but builds no dendrogram arrays); --host-repeats runs
  info             per mode, the call's result fields (flagged edges, trees, height, levels, rounds)
  checks           asserted whatever the times are: num_trees == n - num_mst_edges, is_forest, every
                   size the sum of its children's
  ratios           dendro (full) over root, over the engine, and the host's kruskal_c over dendro (full)

    python tools/dendro_bench.py --graph rmat --scale 24 --out profiles/r15/dendro_bench.json
    python tools/dendro_bench.py --graph grid --scale 4096 --mode 1 --out profiles/r15/dendro_bench.json   (merges)
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "repeats": len(ts)}


def run(graph, scale, mode, seed, warmup, repeats, host_repeats):
    import numpy as np
    import torch

    from distributed_ghs_implementation_amd import _native
    from distributed_ghs_implementation_amd.device import DeviceMST, generate_grid, generate_rmat
    assert torch.cuda.is_available(), "dendro_bench needs a GPU (no fallback)"
    e = generate_rmat(scale, 16, seed=seed, wseed=seed + 1) if graph == "rmat" else generate_grid(scale, mode, wseed=seed + 1)
    name = f"rmat-s{scale}-ef16" if graph == "rmat" else f"grid-{scale}x{scale}-mode{mode}"
    eng = DeviceMST(e)
    eng_ms = []
    for i in range(warmup + repeats):
        res, _ = eng.run()
        torch.cuda.synchronize()
        if i >= warmup:
            eng_ms.append(res.ms_total)
    line = {"graph": name, "n": e.n, "m": e.m, "engine_ms": spread(eng_ms), "engine_rounds": res.rounds,
            "engine_totals": {"num_mst_edges": res.num_mst_edges, "total_weight": res.total_weight},
            "workspace_bytes": int(_native.load().ghs_forest_dendro_workspace_bytes(e.n, e.m)),
            "dendro_ms": {}, "dendro_python_wall_ms": {}, "info": {}}
    root_ms = []
    for i in range(warmup + repeats):
        rooted, rinfo = eng.rooted()
        if i >= warmup:
            root_ms.append(rinfo["ms_total"])
    del rooted
    line["root_ms"] = spread(root_ms)
    line["root_info"] = {k: rinfo[k] for k in ("flagged_edges", "num_trees", "max_depth", "rounds", "is_forest")}
    for label, full in (("full", True), ("parents", False)):
        ms, wall = [], []
        for i in range(warmup + repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d = eng.dendrogram(children=full, sizes=full)
            dt = (time.perf_counter() - t0) * 1e3
            if i >= warmup:
                ms.append(d.info["ms_total"])
                wall.append(dt)
        info = d.info
        assert info["num_trees"] == e.n - res.num_mst_edges and info["is_forest"], info
        if full:
            csize = torch.cat([torch.ones(e.n, dtype=torch.int64, device=e.device), d.size.long() & 0xFFFFFFFF])
            kids = csize[d.child_a.long() & 0xFFFFFFFF] + csize[d.child_b.long() & 0xFFFFFFFF]
            assert bool((kids == csize[e.n:]).all()), "a size is not the sum of its children's"
        line["dendro_ms"][label] = spread(ms)
        line["dendro_python_wall_ms"][label] = spread(wall)
        line["info"][label] = {k: info[k] for k in ("flagged_edges", "num_trees", "max_height", "levels", "rounds", "is_forest")}
        del d
    # the host's way: copy the flags, sort the forest's edges and run a serial union-find over them
    from oracle import oracle
    d2h, kr = [], []
    for _ in range(host_repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        flags = eng.in_mst[: e.m].cpu().numpy()
        d2h.append((time.perf_counter() - t0) * 1e3)
    g = e.to_host()
    T = np.flatnonzero(flags)
    tu, tv, tw = (np.ascontiguousarray(x[T]) for x in (g.u, g.v, g.w))
    for _ in range(host_repeats):
        t0 = time.perf_counter()
        _, _, k = oracle.kruskal_c(g.n, tu, tv, tw)
        kr.append((time.perf_counter() - t0) * 1e3)
        assert k == len(T)
    line["host_ms"] = {"flags_d2h": spread(d2h), "kruskal_c": spread(kr)}
    full = line["dendro_ms"]["full"]["median_ms"]
    line["ratios"] = {"dendro_over_root": full / line["root_ms"]["median_ms"],
                      "dendro_over_engine": full / line["engine_ms"]["median_ms"],
                      "host_kruskal_c_over_dendro": line["host_ms"]["kruskal_c"]["median_ms"] / full}
    line["checks"] = {"num_trees_equal_n_minus_mst_edges": True, "is_forest": True, "sizes_sum_of_children": True}
    return line


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--graph", choices=["rmat", "grid"], default="rmat")
    ap.add_argument("--scale", type=int, default=20, help="R-MAT scale (2^scale vertices) / grid side k")
    ap.add_argument("--mode", type=int, default=0, help="grid weight mode (1: the road-like, deep forest)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", type=str, default=None, help="JSON file to merge the line into, keyed by graph")
    args = ap.parse_args(argv)
    line = run(args.graph, args.scale, args.mode, args.seed, args.warmup, args.repeats, args.host_repeats)
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
