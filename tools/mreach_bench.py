#!/usr/bin/env python3
"""Core distances and mutual reachability on the device (device.mutual_reachability) next to the solve on
the original weights, the solve on the re-weighted list and the whole device.hdbscan, same process.

Per input and k (min_samples), one JSON line:
  mreach_ms        ghs_mreach_result_t.ms_total of mutual_reachability(short_rows="clamp"): the host wall
                   time of the call, which ends in a stream synchronise; warmed up, repeated; median, min, max
  stage_ms         HIP-event times of the call's three stages (ghs_mutual_reach_phases), medians of the same
                   runs: rows (the pairs sort by v and the two lower bounds per vertex), select, reweight
  stage_bytes      what each stage must move at least: rows 16 B per edge (the sort reads and writes (v, w)
                   once per radix pass: `sort_passes` of them) + 8 B per vertex; select 8 B per edge (every
                   weight once from each end) + 12 B per vertex; reweight 16 B per edge (u, v, w in, w out)
                   + the core gathers; and the GB/s each stage reached against that floor
  info             short_rows, isolated, raised_edges, max_degree, block_rows, grid_rows
  engine_ms        ghs_result_t.ms_total of DeviceMST.run() on the original weights
  engine_reweighted_ms
                   the same on the re-weighted list, with its rounds next to the original's
  hdbscan_wall_ms  the whole device.hdbscan (min_cluster_size = k) timed around the Python call
  ratios           mreach over the engine; the re-weighted solve over the original solve
Weights of 0 are raised to 1 before anything is timed: 0 is no valid merge height for the clusters.

    python tools/mreach_bench.py --input rmat --scale 24 --k 5 15 --out profiles/r17/mreach_bench.json
    python tools/mreach_bench.py --input grid --scale 4096 --out profiles/r17/mreach_bench.json
    python tools/mreach_bench.py --input road --scale 4096 --out profiles/r17/mreach_bench.json
    python tools/mreach_bench.py --input star --scale 24 --out profiles/r17/mreach_bench.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

INFO = ("short_rows", "isolated", "raised_edges", "max_degree", "block_rows", "grid_rows")


def spread(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "repeats": len(ts)}


def make(kind, scale, seed):
    import torch

    from distributed_ghs_implementation_amd.device import DeviceEdges, generate_grid, generate_rmat
    if kind == "rmat":
        e, name = generate_rmat(scale, 16, seed=seed, wseed=seed + 1), f"rmat-s{scale}-ef16"
    elif kind in ("grid", "road"):
        mode = 1 if kind == "road" else 0
        e, name = generate_grid(scale, mode, wseed=seed + 1), f"grid-{scale}x{scale}-mode{mode}"
    else:  # a star: vertex 0 joined to 2^scale leaves, random weights
        leaves = 1 << scale
        g = torch.Generator(device="cuda").manual_seed(seed)
        w = torch.randint(1, 1 << 31, (leaves,), dtype=torch.int32, device="cuda", generator=g)
        e = DeviceEdges(leaves + 1, torch.zeros(leaves, dtype=torch.int32, device="cuda"),
                        torch.arange(1, leaves + 1, dtype=torch.int32, device="cuda"), w)
        name = f"star-2^{scale}"
    e.w[e.w == 0] = 1
    return e, name


def timed_engine(e, warmup, repeats):
    import torch

    from distributed_ghs_implementation_amd.device import DeviceMST
    eng = DeviceMST(e)
    ms = []
    for i in range(warmup + repeats):
        res, _ = eng.run()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(res.ms_total)
    return spread(ms), int(res.rounds), int(res.total_weight)


def run(kind, scale, seed, warmup, repeats, ks, with_hdbscan):
    import torch

    from distributed_ghs_implementation_amd import _native
    from distributed_ghs_implementation_amd.device import hdbscan, mutual_reachability
    assert torch.cuda.is_available(), "mreach_bench needs a GPU (no fallback)"
    L = _native.load()
    e, name = make(kind, scale, seed)
    n, m = e.n, e.m
    engine, rounds, _ = timed_engine(e, warmup, repeats)
    lines = []
    for k in ks:
        ms, stages = [], [[], [], []]
        L.ghs_mutual_reach_phases(1, None)
        for i in range(warmup + repeats):
            mr = mutual_reachability(e, min_samples=k, short_rows="clamp")
            ph = (ctypes.c_double * 3)()
            L.ghs_mutual_reach_phases(1, ph)
            if i >= warmup:
                ms.append(mr.info["ms_total"])
                for s in range(3):
                    stages[s].append(ph[s])
        L.ghs_mutual_reach_phases(0, None)
        w_new = mr.edges.w.to(torch.int64) & 0xFFFFFFFF
        w_old = e.w.to(torch.int64) & 0xFFFFFFFF
        cu, cv = (mr.core.to(torch.int64) & 0xFFFFFFFF)[e.u.long()], (mr.core.to(torch.int64) & 0xFFFFFFFF)[e.v.long()]
        assert bool((w_new == torch.maximum(torch.maximum(cu, cv), w_old)).all()), "w_out is not max(core, core, w)"
        assert int((w_new > w_old).sum()) == mr.info["raised_edges"]
        del w_new, w_old, cu, cv
        bits = max(n - 1, 1).bit_length()
        passes = -(-bits // 8)  # an estimate: rocPRIM picks its own digit widths
        floor = {"rows": 16 * m * passes + 8 * n, "select": 8 * m + 12 * n, "reweight": 16 * m + 4 * n}
        med = {s: statistics.median(stages[i]) for i, s in enumerate(("rows", "select", "reweight"))}
        line = {"input": name, "k": k, "n": n, "m": m, "mreach_ms": spread(ms), "stage_ms": med,
                "stage_bytes": floor, "sort_passes": passes,
                "stage_GBps": {s: floor[s] / (med[s] * 1e6) if med[s] > 0 else None for s in med},
                "info": {f: mr.info[f] for f in INFO},
                "workspace_bytes": int(L.ghs_mutual_reach_workspace_bytes(n, m)),
                "engine_ms": engine, "engine_rounds": rounds}
        re_ms, re_rounds, _ = timed_engine(mr.edges, warmup, repeats)
        line["engine_reweighted_ms"], line["engine_reweighted_rounds"] = re_ms, re_rounds
        line["ratios"] = {"mreach_over_engine": line["mreach_ms"]["median_ms"] / engine["median_ms"],
                          "reweighted_solve_over_original": re_ms["median_ms"] / engine["median_ms"]}
        del mr
        if with_hdbscan:
            wall = []
            for i in range(1 + 3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                h = hdbscan(e, min_cluster_size=max(k, 2), min_samples=k, short_rows="clamp")
                torch.cuda.synchronize()
                if i >= 1:
                    wall.append((time.perf_counter() - t0) * 1e3)
            line["hdbscan_wall_ms"] = spread(wall)
            line["hdbscan_info"] = {f: h.clusters.info[f] for f in ("num_clusters", "num_selected", "num_noise")}
            del h
        lines.append(line)
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--input", choices=["rmat", "grid", "road", "star"], default="rmat")
    ap.add_argument("--scale", type=int, default=20, help="R-MAT scale / grid side / log2 of the star's leaves")
    ap.add_argument("--k", type=int, nargs="+", default=[5], help="min_samples values")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-hdbscan", action="store_true", help="leave the end-to-end call out")
    ap.add_argument("--out", type=str, default=None, help="JSON file to merge the lines into, keyed by input and k")
    args = ap.parse_args(argv)
    lines = run(args.input, args.scale, args.seed, args.warmup, args.repeats, args.k, not args.no_hdbscan)
    for line in lines:
        print(json.dumps(line), flush=True)
    if args.out:
        merged = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                merged = json.load(f)
        for line in lines:
            merged[f"{line['input']}-k{line['k']}"] = line
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(merged, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
