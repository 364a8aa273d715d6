#!/usr/bin/env python3
"""Path queries on the engine's forest (device.forest_paths) next to the verifier, same process.

Per graph, one JSON line:
  forest           what forest_root found: trees, max depth (the index has K = max(1, bit_length) levels)
  index            K, index bytes, and create_ms: ghs_paths_result_t.ms_total of forest_paths on the rooted
                   arrays (the host wall time of the call, which ends in a stream synchronise): warmed up,
                   repeated; median, min, max
  query            per batch (2^20 and 2^24 uniform random pairs, and the graph's own m edges as pairs):
                   query_ms = ghs_paths_query_result_t.ms_total the same way, queries per second from its
                   median, and the number of connected pairs
  verify_ms        ghs_verify_result_t.ms_total of DeviceMST.verify() on the same graph: its query kernel
                   answers the same m path-max questions over its Boruvka tree
  edges_over_verify  median query_ms of the m edges / median verify_ms: a ratio to report, not a gate
  checks           asserted whatever the times are: every tree edge answers itself, every other edge a
                   smaller key, every edge's ends connected

    python tools/paths_bench.py --graph rmat --scale 24 --out profiles/r12/paths_bench.json
    python tools/paths_bench.py --graph grid --scale 4096 --mode 1 --out profiles/r12/paths_bench.json   (merges)
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "repeats": len(ts)}


def run(graph, scale, mode, seed, warmup, repeats):
    import torch

    from distributed_ghs_implementation_amd.device import DeviceMST, forest_paths, generate_grid, generate_rmat
    assert torch.cuda.is_available(), "paths_bench needs a GPU (no fallback)"
    e = generate_rmat(scale, 16, seed=seed, wseed=seed + 1) if graph == "rmat" else generate_grid(scale, mode, wseed=seed + 1)
    name = f"rmat-s{scale}-ef16" if graph == "rmat" else f"grid-{scale}x{scale}-mode{mode}"
    eng = DeviceMST(e)
    res, _ = eng.run()
    rooted, rinfo = eng.rooted(order=False)
    assert rinfo["is_forest"] and rinfo["num_trees"] == e.n - res.num_mst_edges, rinfo
    line = {"graph": name, "n": e.n, "m": e.m,
            "forest": {"num_trees": rinfo["num_trees"], "max_depth": rinfo["max_depth"], "root_ms": rinfo["ms_total"]}}
    create_ms, index = [], None
    for i in range(warmup + repeats):
        if index is not None:
            index.close()
        del index
        index, info = forest_paths(e, rooted=rooted, max_depth=rinfo["max_depth"])
        if i >= warmup:
            create_ms.append(info["ms_total"])
    assert info["num_trees"] == rinfo["num_trees"] and info["max_depth"] == rinfo["max_depth"], info
    line["index"] = {"levels": info["levels"], "index_bytes": info["index_bytes"], "create_ms": spread(create_ms)}
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    batches = []
    for lg in (20, 24):
        q = 1 << lg
        batches.append((f"random_2^{lg}", torch.randint(0, e.n, (q,), generator=gen, device="cuda", dtype=torch.int32),
                        torch.randint(0, e.n, (q,), generator=gen, device="cuda", dtype=torch.int32)))
    batches.append(("graph_edges", e.u, e.v))
    line["query"] = {}
    for label, a, b in batches:
        ms = []
        for i in range(warmup + repeats):
            ans = index.query(a, b)
            if i >= warmup:
                ms.append(ans.info["ms_total"])
        s = spread(ms)
        line["query"][label] = {"pairs": int(a.numel()), "connected": ans.info["connected"], "query_ms": s,
                                "queries_per_second": a.numel() / (s["median_ms"] * 1e-3)}
    # the last batch's answers: the cycle property of the engine's forest
    own = ((e.w.to(torch.int64) & 0xFFFFFFFF) << 32) | torch.arange(e.m, device="cuda", dtype=torch.int64)
    tree = eng.in_mst[: e.m] != 0
    high = torch.tensor(-(1 << 63), dtype=torch.int64, device="cuda")  # unsigned order on int64 bits
    assert bool((ans.key[tree] == own[tree]).all()) and bool(((ans.key[~tree] ^ high) < (own[~tree] ^ high)).all())
    assert ans.info["connected"] == e.m
    line["checks"] = {"tree_edges_answer_themselves": True, "other_edges_answer_smaller_keys": True,
                      "every_edge_connected": True}
    vms = []
    for i in range(warmup + repeats):
        v = eng.verify()
        if i >= warmup:
            vms.append(v["ms_total"])
    assert v["ok"], v
    line["verify_ms"] = spread(vms)
    line["edges_over_verify"] = line["query"]["graph_edges"]["query_ms"]["median_ms"] / line["verify_ms"]["median_ms"]
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
