#!/usr/bin/env python3
"""Tree distances on the engine's forest (device.forest_distances and friends) next to PathIndex.query,
same process, same pairs.

Per graph, one JSON line:
  forest           what forest_root found: trees, max depth; the index's K
  wdepth_ms        the weighted depth built from scratch (PathIndex.wdepth with its cache cleared): host
                   wall time around the call, which ends in a stream synchronise; K launches over n
  distances        2^24 uniform random pairs through PathIndex.distances: ghs_dist_query_result_t.ms_total
                   (the host wall time of the call, ending in a stream synchronise), pairs per second,
                   connected pairs, the largest distance
  query            the same pairs through PathIndex.query (key, lca and hops written), measured the same
                   way in the same process: the yardstick
  dist_over_query  median distances ms / median query ms on those pairs: the ratio to quote
  edge_distances   the graph's own m edges through PathIndex.edge_distances (per-edge array written), with
                   the exact sums; query_edges is PathIndex.query on the same m pairs, edges_over_query the ratio
  diameters        PathIndex.diameters (eccentricities written): ghs_diameter_result_t.ms_total, and what it found
  checks           asserted whatever the times are: hop distances equal the path query's hop counts on
                   the random pairs, every tree edge has dist == w, no edge crosses two trees, every
                   eccentricity lies between half the diameter of its tree and that diameter
Every time is warmed up and repeated: median, min, max of --repeats (default 7).

    python tools/dist_bench.py --graph rmat --scale 24 --out profiles/r14/dist_bench.json
    python tools/dist_bench.py --graph grid --scale 4096 --mode 1 --out profiles/r14/dist_bench.json   (merges)
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


def timed(fn, warmup, repeats):
    """fn() -> (value, ms); the spread of ms after the warm-up calls, and the last value."""
    ms, val = [], None
    for i in range(warmup + repeats):
        val, t = fn()
        if i >= warmup:
            ms.append(t)
    return spread(ms), val


def run(graph, scale, mode, seed, warmup, repeats, log_pairs):
    import torch

    from distributed_ghs_implementation_amd.device import DeviceMST, forest_paths, generate_grid, generate_rmat
    assert torch.cuda.is_available(), "dist_bench needs a GPU (no fallback)"
    e = generate_rmat(scale, 16, seed=seed, wseed=seed + 1) if graph == "rmat" else generate_grid(scale, mode, wseed=seed + 1)
    name = f"rmat-s{scale}-ef16" if graph == "rmat" else f"grid-{scale}x{scale}-mode{mode}"
    eng = DeviceMST(e)
    res, _ = eng.run()
    rooted, rinfo = eng.rooted(order=False)
    assert rinfo["is_forest"] and rinfo["num_trees"] == e.n - res.num_mst_edges, rinfo
    index, info = forest_paths(e, rooted=rooted, max_depth=rinfo["max_depth"])
    del rooted
    line = {"graph": name, "n": e.n, "m": e.m,
            "forest": {"num_trees": rinfo["num_trees"], "max_depth": rinfo["max_depth"], "levels": info["levels"]}}

    def build():
        index._wdepth.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        wd = index.wdepth()
        return wd, (time.perf_counter() - t0) * 1e3
    line["wdepth_ms"], wd = timed(build, warmup, repeats)
    line["max_wdepth"] = int(wd.view(torch.int64).max())

    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    q = 1 << log_pairs
    a = torch.randint(0, e.n, (q,), generator=gen, device="cuda", dtype=torch.int32)
    b = torch.randint(0, e.n, (q,), generator=gen, device="cuda", dtype=torch.int32)

    def dist_of(x, y, hops=False):
        def fn():
            d = index.distances(x, y, hops=hops)
            return d, index.last_distance_info["ms_total"]
        return fn

    def query_of(x, y):
        def fn():
            ans = index.query(x, y)
            return ans, ans.info["ms_total"]
        return fn
    ds, d = timed(dist_of(a, b), warmup, repeats)
    dinfo = dict(index.last_distance_info)
    qs, ans = timed(query_of(a, b), warmup, repeats)
    line["distances"] = {"pairs": q, "connected": dinfo["connected"], "max_dist": dinfo["max_dist"], "dist_ms": ds,
                         "pairs_per_second": q / (ds["median_ms"] * 1e-3)}
    line["query"] = {"pairs": q, "connected": ans.info["connected"], "query_ms": qs,
                     "pairs_per_second": q / (qs["median_ms"] * 1e-3)}
    line["dist_over_query"] = ds["median_ms"] / qs["median_ms"]
    hd = index.distances(a, b, hops=True).view(torch.int64)
    assert bool((hd == ans.hops.to(torch.int64)).all())  # -1 on both sides for different trees
    assert dinfo["connected"] == ans.info["connected"]
    del d, hd, ans

    def edges():
        ed = index.edge_distances(e)
        return ed, ed.info["ms_total"]
    es, ed = timed(edges, warmup, repeats)
    qes, eans = timed(query_of(e.u, e.v), warmup, repeats)
    einfo = {k: v for k, v in ed.info.items() if k != "ms_total"}
    tree = eng.in_mst[: e.m] != 0
    dist = ed.dist.view(torch.int64)
    assert bool((dist[tree] == (e.w[tree].to(torch.int64) & 0xFFFFFFFF)).all()) and einfo["cross_edges"] == 0
    assert einfo["tight_edges"] >= int(tree.sum())
    line["edge_distances"] = {**einfo, "sum_dist": str(einfo["sum_dist"]), "average_stretch": ed.average_stretch(), "edges_ms": es}
    line["query_edges"] = {"query_ms": qes}
    line["edges_over_query"] = es["median_ms"] / qes["median_ms"]
    del ed, eans, dist

    def diam():
        tm = index.diameters()
        return tm, tm.info["ms_total"]
    ts, tm = timed(diam, warmup, repeats)
    tinfo = {k: v for k, v in tm.info.items() if k != "ms_total"}
    ecc = tm.ecc.view(torch.int64)
    widest = tm.diameter.view(torch.int64)[tm.root_of.to(torch.int64) & 0xFFFFFFFF]  # per vertex: its tree's diameter
    assert bool((ecc <= widest).all()) and bool((2 * ecc >= widest).all())
    assert tinfo["num_trees"] == rinfo["num_trees"]
    line["diameters"] = {**tinfo, "diam_ms": ts}
    line["checks"] = {"hop_distances_equal_query_hops": True, "tree_edges_have_dist_w": True, "no_edge_crosses_trees": True,
                      "ecc_between_half_and_whole_diameter": True}
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
    ap.add_argument("--log-pairs", type=int, default=24, help="2^LOG random pairs")
    ap.add_argument("--out", type=str, default=None, help="JSON file to merge the line into, keyed by graph")
    args = ap.parse_args(argv)
    line = run(args.graph, args.scale, args.mode, args.seed, args.warmup, args.repeats, args.log_pairs)
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
