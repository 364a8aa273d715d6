#!/usr/bin/env python3
"""The engine's forest rooted on the device (device.forest_root) next to the solve that made it, same process.

Per graph, one JSON line:
  root_ms          ghs_root_result_t.ms_total of DeviceMST.rooted() on the engine's flags (the host wall
                   time of the call, which ends in a stream synchronise): warmed up, repeated; median,
                   min, max. Modes: order (all five arrays), no_order (pre and size left out)
  root_python_wall_ms
                   the same calls timed around the Python entry (workspace allocation included)
  engine_ms        ghs_result_t.ms_total of DeviceMST.run() on the same device-resident list, same way
  info             per mode, the call's result fields (flagged edges, trees, max depth, rounds)
  splitters        two-hop minima of the forest (local minima that are also the smallest neighbour of
                   each of their neighbours) + the hashed 1-in-64 sample of the arcs (counted here with
                   torch, not returned by the call)
  checks           asserted whatever the times are: num_trees == n - num_mst_edges and is_forest
  model            HBM bytes the passes move, from the shapes alone (DESIGN.md "Rooted forest"), and the
                   time they would take at the measured copy rate: a lower bound from a byte count, not a
                   measurement — the walks and the doubling rounds are dependent gathers

    python tools/root_bench.py --graph rmat --scale 20 --out profiles/r11/root_bench.json
    python tools/root_bench.py --graph grid --scale 4096 --mode 1 --out profiles/r11/root_bench.json   (merges)
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


def model_bytes(n, m, T, S, rounds, order):
    """Bytes per pass from the shapes (no measurement): T tree edges, A = 2 T arcs, S splitters."""
    A = 2 * T
    bits = max(1, (max(n, 2) - 1).bit_length())
    b = {
        "check_canonical": 8 * m,                             # u, v
        "flag_count": m,
        "gather_edges": m + T * (8 + 12),                     # flags again; u, v read, (u, v, eid) written
        "sort_by_v": -(-bits // 8) * 16 * T,                  # per radix pass: keys + values in and out
        "clear_adjacency_sizes": 21 * n,
        "inverse_and_bounds": 8 * T + 2 * (4 * T + 8 * min(T, n)),
        "demote_local_minima": 8 * T,                         # u, v streamed; the gathers hit only at local minima
        "successors_and_splitter_bits": A * (12 + 24 + 8) + A // 4,
        "splitter_list": A // 8 + 4 * S,
        "walk_measure": A * 8 + S * (4 + 40),
        "doubling_rounds": rounds * S * 36,                   # 16 + 16 + 16 B (min) / 8 + 8 + 8 B (rank) per node
        "tree_sizes_and_root_scan": S * 12 + n * (16 + 4 + 8) + n * 24 + n * 28,
        "clear_marks": 8 * A,
        "walk_place": A * (8 + 4) + S * 20,
        "mark_down": T * (12 + 8),
        "scan_marks": A * 24,
        "outputs": T * (12 + 8 + 8) + T * (20 if order else 12),
    }
    total = sum(b.values())
    return {"bytes": b, "total_bytes_lower_bound": total, "bound_ms_at_copy_rate": total / (HBM_COPY_TBS * 1e12) * 1e3}


def count_splitters(e, in_mst):
    import torch

    from distributed_ghs_implementation_amd.device import flags_to_eids
    eids = flags_to_eids(in_mst, 0, e.m).long()
    tu, tv = e.u[eids].long() & 0xFFFFFFFF, e.v[eids].long() & 0xFFFFFFFF
    has_larger = torch.zeros(e.n, dtype=torch.bool, device=e.device)
    has_smaller = torch.zeros(e.n, dtype=torch.bool, device=e.device)
    has_larger[tu] = True
    has_smaller[tv] = True
    local_min = has_larger & ~has_smaller
    # a local minimum stays a splitter when it is also the smallest neighbour of each of its neighbours
    min_nbr = torch.full((e.n,), 1 << 40, dtype=torch.int64, device=e.device)
    min_nbr.scatter_reduce_(0, tv, tu, "amin")
    demoted = torch.zeros(e.n, dtype=torch.bool, device=e.device)
    demoted[tu[min_nbr[tv] < tu]] = True
    return {"local_minima": int(local_min.sum()), "two_hop_minima": int((local_min & ~demoted).sum()),
            "hashed_sample_expected": 2 * int(eids.numel()) // 64}


def run(graph, scale, mode, seed, warmup, repeats):
    import torch

    from distributed_ghs_implementation_amd.device import DeviceMST, generate_grid, generate_rmat
    assert torch.cuda.is_available(), "root_bench needs a GPU (no fallback)"
    e = generate_rmat(scale, 16, seed=seed, wseed=seed + 1) if graph == "rmat" else generate_grid(scale, mode, wseed=seed + 1)
    name = f"rmat-s{scale}-ef16" if graph == "rmat" else f"grid-{scale}x{scale}-mode{mode}"
    eng = DeviceMST(e)
    eng_ms = []
    for i in range(warmup + repeats):
        res, _ = eng.run()
        torch.cuda.synchronize()
        if i >= warmup:
            eng_ms.append(res.ms_total)
    spl = count_splitters(e, eng.in_mst)
    line = {"graph": name, "n": e.n, "m": e.m, "engine_ms": spread(eng_ms), "engine_rounds": res.rounds,
            "engine_totals": {"num_mst_edges": res.num_mst_edges, "total_weight": res.total_weight},
            "splitters": spl, "root_ms": {}, "root_python_wall_ms": {}, "info": {}, "model": {}, "root_over_engine": {}}
    for label, order in (("order", True), ("no_order", False)):
        ms, wall = [], []
        for i in range(warmup + repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rooted, info = eng.rooted(order=order)
            dt = (time.perf_counter() - t0) * 1e3
            if i >= warmup:
                ms.append(info["ms_total"])
                wall.append(dt)
        assert info["num_trees"] == e.n - res.num_mst_edges and info["is_forest"], info
        assert int(rooted.parent[0]) == -1
        line["root_ms"][label] = spread(ms)
        line["root_python_wall_ms"][label] = spread(wall)
        line["info"][label] = {k: info[k] for k in ("flagged_edges", "num_trees", "max_depth", "rounds", "is_forest")}
        S = spl["two_hop_minima"] + spl["hashed_sample_expected"]
        line["model"][label] = model_bytes(e.n, e.m, info["flagged_edges"], S, info["rounds"], order)
        line["root_over_engine"][label] = line["root_ms"][label]["median_ms"] / line["engine_ms"]["median_ms"]
        del rooted
    line["checks"] = {"num_trees_equal_n_minus_mst_edges": True, "is_forest": True}
    return line


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--graph", choices=["rmat", "grid"], default="rmat")
    ap.add_argument("--scale", type=int, default=20, help="R-MAT scale (2^scale vertices) / grid side k")
    ap.add_argument("--mode", type=int, default=0, help="grid weight mode (1: the road-like, deep forest)")
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
