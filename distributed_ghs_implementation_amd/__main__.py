"""CLI mirroring `mpiexec -n N python ghs_implementation_mpi.py --graph-dir D`
(ghs_implementation_mpi.py:884-954) and the thread path's result JSON.

    python -m distributed_ghs_implementation_amd --graph-dir graph_data
        reads graph_metadata.json (or node_<id>.json files), runs the HIP engine on one GPU,
        writes <graph-dir>/ghs_mst.json in the mst_result_mpi.json schema
        ({"mst_edges", "total_weight", "num_edges", "algorithm"}), prints a summary.
    --mpi-compat   also write <graph-dir>/mst_result_mpi.json (same content)
    --graph FILE   read an .mstbin binary graph instead of a directory
    --output FILE  result path (default <graph-dir>/ghs_mst.json)
    --check        verify the result after the run (verify.py: forest, spans every component,
                   weight vs NetworkX when available — the reference's check_mst.py)
    --check-device verify the result on the GPU, exactly, at any size (verify.verify_forest_device:
                   the flags equal canonical Kruskal's under the key (w, eid)); prints the counts
                   and CORRECT / INCORRECT, exit status 1 when not ok
    --check-result FILE
                   verify an existing result JSON against the graph; no GPU, no solve
    --labels OUT.npy
                   after the solve, write every vertex's cluster as a numpy uint32 array (the forest's
                   components labelled on the GPU, clusters ordered by their smallest vertex); with
                   --clusters K the heaviest forest edges are dropped until K clusters remain, with
                   --max-weight T only forest edges of weight <= T are kept (single linkage)
    --rooted OUT.npz
                   after the solve, write the forest rooted at every tree's smallest vertex: numpy
                   uint32 arrays parent, parent_eid (0xffffffff for a root), depth, pre (DFS preorder)
                   and size (subtree sizes), computed on the GPU
    --dendrogram OUT.npz
                   after the solve, write the single-linkage dendrogram of the forest, computed on the
                   GPU: merge j is the j-th lightest forest edge, vertex v is node v and merge j node
                   n + j (scipy's ids); leaf_parent per vertex, and per merge merge_eid, merge_parent,
                   child_a, child_b, size (uint32, 0xffffffff: none) and height (its weight)
    --clusters OUT.npz --min-cluster-size K [--cluster-method eom|leaf] [--allow-single-cluster]
                   after the solve, HDBSCAN cluster extraction from that dendrogram on the GPU (a
                   --clusters value that is no integer is this output file): label (int32 per vertex,
                   -1: noise; a value that parses as an integer always means K, so name a file ./123), probability, point_cluster, point_lambda, and per cluster of the
                   condensed tree cluster_head, cluster_parent, cluster_size, cluster_birth,
                   cluster_stability, cluster_selected, with the counts num_clusters, num_selected,
                   num_noise, num_top, cluster_height; a forest edge of weight 0 is an error
    --mutual-reachability OUT.npz [--min-samples K] [--short-rows error|clamp]
                   the weights HDBSCAN wants, of the graph's own edges, on the GPU: core (per vertex the
                   K-th smallest weight among its edges, default K = 5) and w (per canonical edge
                   max(core[u], core[v], w)), with the counts short_rows, isolated, raised_edges,
                   max_degree, block_rows, grid_rows, k; a vertex with fewer than K edges is an error
                   unless --short-rows clamp
    --hdbscan OUT.npz [--min-samples K] [--min-cluster-size K] [--cluster-method eom|leaf]
              [--allow-single-cluster] [--short-rows error|clamp]
                   HDBSCAN of the graph's own edges (a k-NN graph, a sparse distance matrix) end to end
                   on the GPU: mutual reachability, the solve on those weights, the dendrogram, the
                   clusters; the arrays of --clusters OUT.npz plus core and in_mst (the flags of the
                   mutual-reachability forest); --min-cluster-size defaults to 5, --min-samples to it
    --paths OUT.npz --pairs PAIRS.npy
                   after the solve, answer path queries on the forest on the GPU: PAIRS.npy is an
                   integer array of shape (Q, 2); OUT.npz holds a, b, eid (the heaviest edge between
                   a and b on the forest, 0xffffffff where there is none), weight (its weight: the
                   minimax distance of a and b in the graph), lca and hops (0xffffffff for different
                   components)
    --replacements OUT.npz
                   after the solve, what takes each forest edge's place when it fails, on the GPU:
                   eid_by_edge (uint32 per canonical edge: the lightest edge that reconnects the two
                   halves, 0xffffffff for a bridge and for non-forest edges), key (uint64 per vertex:
                   the replacement's w << 32 | eid of the edge to its parent in the rooted forest), and
                   the counts tree_edges, covering_edges, cross_edges, bridges, improving, best_delta,
                   best_out_eid, best_in_eid
    --distances OUT.npz --pairs PAIRS.npy
                   after the solve, how far it is from a to b along the forest, on the GPU: OUT.npz
                   holds a, b, dist (uint64: the sum of the weights on the path, 0 for a == b,
                   2^64 - 1 for different components) and lca; --pairs as for --paths
    --diameters OUT.npz
                   after the solve, every tree's diameter on the GPU: root_of, diameter / end_a / end_b
                   (indexed by root), ecc (every vertex's distance to the farthest vertex of its tree),
                   roots, and num_trees, max_diameter, max_root, min_ecc, center
    --stretch OUT.npz
                   after the solve, the forest distance between the ends of every graph edge (dist,
                   uint64 per canonical edge) and its summary: sum_dist (as a decimal string: it can
                   pass 64 bits), sum_w, max_dist, max_eid, cross_edges, tight_edges
    --hops         with --distances / --diameters: count edges instead of summing weights (required
                   for rank-mapped weights, whose sums mean nothing)

    --batch-dir ROOT
                   many small graphs in one launch: every immediate subdirectory of ROOT holding
                   graph_metadata.json or node_<id>.json files and every ROOT/*.mstbin is one graph
                   (sorted order); writes each graph's ghs_mst.json next to its input and
                   ROOT/ghs_experiments.json (the reference's experiment records); with --check the
                   exit status is 1 if any record fails

    --gpus N       one process drives N GPUs of this node (RCCL clique, ghs_mst_multi)
    --generator {rmat,grid} --scale S --seed X
                   solve a synthetic BASELINE graph generated on the GPU instead of reading one
                   (R-MAT 2^S vertices, edgefactor 16; grid: --scale is the side k)

Multi-GPU, one process per GPU:
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 \
        -m distributed_ghs_implementation_amd --graph-dir D
"""
import argparse
import os
import sys
import time


def discover_batch(root):
    """The graphs of a --batch-dir tree in sorted order: [(name, kind, path)] with kind "dir" (an
    immediate subdirectory holding graph_metadata.json or node_<id>.json files) or "mstbin"."""
    from .graph import _NODE_RE
    found = []
    for name in sorted(os.listdir(root)):
        p = os.path.join(root, name)
        if os.path.isdir(p):
            files = os.listdir(p)
            if "graph_metadata.json" in files or any(_NODE_RE.match(f) for f in files):
                found.append((name, "dir", p))
        elif name.endswith(".mstbin"):
            found.append((name, "mstbin", p))
    return found


def batch_output_path(kind, path):
    """Where a batch graph's ghs_mst.json goes: next to its input."""
    if kind == "dir":
        return os.path.join(path, "ghs_mst.json")
    return path[: -len(".mstbin")] + ".ghs_mst.json"


def run_batch_dir(args):
    """--batch-dir ROOT: every graph under ROOT solved in one batch (the reference main()'s
    six-experiment loop, ghs_implementation.py:779-833, as one call); writes each graph's ghs_mst.json
    and ROOT/ghs_experiments.json (a list of verify.experiment_record entries)."""
    import json

    from . import graph as G
    from .mst import minimum_spanning_forest_batch
    from .verify import experiment_record
    t0 = time.perf_counter()
    items = discover_batch(args.batch_dir)
    if not items:
        raise FileNotFoundError(f"no graph directories or .mstbin files in {args.batch_dir}")
    graphs = [G.read_graph_dir(p) if kind == "dir" else G.read_mstbin(p) for _, kind, p in items]
    t_read = time.perf_counter() - t0
    results = minimum_spanning_forest_batch(graphs)
    records = []
    for (name, kind, p), g, r in zip(items, graphs, results):
        triples = r.triples()
        G.write_result(batch_output_path(kind, p), triples)
        records.append(experiment_record(name, g, triples))
    exp = os.path.join(args.batch_dir, "ghs_experiments.json")
    with open(exp, "w") as f:
        json.dump(records, f, indent=2)
    bad = [r["experiment"] for r in records if not r["is_correct"]]
    if not args.quiet:
        print("=" * 70)
        print("Boruvka MST on MI355X (HIP) — batched solve")
        print("=" * 70)
        print(f"Graphs: {len(graphs)}  Edges: {sum(g.m for g in graphs)}  "
              f"engine time: {results[0].ms_total:.3f} ms  read: {t_read * 1e3:.1f} ms")
        for rec in records:
            print(f"  {rec['experiment']}: n={rec['num_nodes']} m={rec['num_edges']} MST edges={rec['edges_found']} "
                  f"weight={rec['mst_weight']} {'CORRECT' if rec['is_correct'] else 'INCORRECT'}")
        print(f"Results saved to: {exp}")
    return 1 if (args.check and bad) else 0


def run_points(args):
    """--points X.npy: the k-NN graph (--knn-graph), the exact MST (--emst) and / or HDBSCAN from points
    (--hdbscan, with --exact on the exact MST)."""
    import numpy as np

    t0 = time.perf_counter()
    X = np.load(args.points)
    t_read = time.perf_counter() - t0
    metric = args.metric or "euclidean"
    if args.knn_graph is not None:
        import torch

        from .device import knn_graph
        if X.ndim != 2 or X.dtype == np.float64:
            raise ValueError("--points: an (n, d) array of float32 / float16 / integer points expected "
                             "(float64 is never narrowed silently)")
        g = knn_graph(torch.from_numpy(np.ascontiguousarray(X if X.dtype.kind != "u" else X.astype(np.int64))).to("cuda"),
                      args.knn, metric=metric)
        e = g.edges
        np.savez(args.knn_graph, idx=g.knn.idx.cpu().numpy().view(np.uint32), dist=g.knn.dist.cpu().numpy(),
                 u=e.u.cpu().numpy().view(np.uint32), v=e.v.cpu().numpy().view(np.uint32), w=e.weights.cpu().numpy())
        if not args.quiet:
            print(f"Points: {X.shape[0]} x {X.shape[1]}  k = {args.knn}  k-NN graph edges: {e.m}  "
                  f"zero distances: {g.knn.info['zero_neighbours']}  knn: {g.knn.info['ms_total']:.3f} ms  "
                  f"read: {t_read * 1e3:.1f} ms")
            print(f"k-NN graph saved to: {args.knn_graph}")
    if args.emst is not None:
        from .mst import emst_points
        out, info = emst_points(X, min_samples=args.min_samples, metric=metric, return_info=True)
        np.savez(args.emst, **{k: v for k, v in out.items() if v is not None})
        if not args.quiet:
            what = "Euclidean" if args.min_samples is None else f"mutual-reachability (min_samples = {args.min_samples})"
            print(f"Points: {X.shape[0]} x {X.shape[1]}  exact {what} MST: {info['num_edges']} edges  "
                  f"rounds: {info['rounds']}  zero edges: {info['zero_edges']}  emst: {info['ms_total']:.3f} ms  "
                  f"read: {t_read * 1e3:.1f} ms")
            print(f"Exact MST saved to: {args.emst}")
    if args.hdbscan is not None:
        from .mst import hdbscan_points
        mcs = 5 if args.min_cluster_size is None else args.min_cluster_size
        out, info = hdbscan_points(X, min_cluster_size=mcs, min_samples=args.min_samples, k=args.knn, metric=metric,
                                   method=args.cluster_method, allow_single_cluster=args.allow_single_cluster,
                                   return_info=True, exact=args.exact)
        np.savez(args.hdbscan, **out)
        if not args.quiet:
            how = f"exact MST, {info['emst']['rounds']} rounds" if args.exact else f"k = {info['knn']['k']}"
            print(f"HDBSCAN from points: {info['cluster']['num_selected']} clusters, {info['cluster']['num_noise']} noise "
                  f"points of {X.shape[0]} ({how}, {metric})")
            print(f"HDBSCAN saved to: {args.hdbscan}")
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description="MI355X Boruvka MST (drop-in for ghs_implementation_mpi.py)")
    ap.add_argument("--batch-dir", type=str, default=None,
                    help="solve every graph under this directory (subdirectories, *.mstbin) in one batch")
    ap.add_argument("--graph-dir", type=str, default="graph_data", help="Graph data directory (default: graph_data)")
    ap.add_argument("--graph", type=str, default=None, help=".mstbin graph file")
    ap.add_argument("--output", type=str, default=None)
    ap.add_argument("--mpi-compat", action="store_true")
    ap.add_argument("--quiet", action="store_true")
    ap.add_argument("--check", action="store_true", help="verify the result (check_mst.py)")
    ap.add_argument("--check-device", action="store_true",
                    help="verify the result on the GPU: exact optimality at any size (device verifier)")
    ap.add_argument("--check-result", type=str, default=None, help="verify an existing result JSON only")
    ap.add_argument("--labels", type=str, default=None, metavar="OUT.npy",
                    help="write the vertices' cluster labels (uint32 .npy) after the solve")
    ap.add_argument("--clusters", type=str, default=None, metavar="K | OUT.npz",
                    help="an integer, with --labels: single linkage into K clusters; anything else is a file name: "
                         "write the HDBSCAN clusters of the forest's dendrogram (needs --min-cluster-size). A value "
                         "that parses as an integer always means K: name an output file ./123, not 123")
    ap.add_argument("--min-cluster-size", type=int, default=None, metavar="K",
                    help="with --clusters OUT.npz: the smallest cluster HDBSCAN keeps (>= 2)")
    ap.add_argument("--cluster-method", choices=["eom", "leaf"], default="eom",
                    help="with --clusters OUT.npz: excess of mass (default) or the leaves of the condensed tree")
    ap.add_argument("--allow-single-cluster", action="store_true",
                    help="with --clusters OUT.npz: a lone tree top may be selected")
    ap.add_argument("--hdbscan", type=str, default=None, metavar="OUT.npz",
                    help="write HDBSCAN of the graph's own edges (mutual reachability, the solve on it, the clusters); "
                         "takes --min-samples, --min-cluster-size (default 5), --cluster-method, --allow-single-cluster, "
                         "--short-rows")
    ap.add_argument("--mutual-reachability", type=str, default=None, metavar="OUT.npz",
                    help="write the core distances (core) and the mutual-reachability weights (w) of the graph's edges")
    ap.add_argument("--min-samples", type=int, default=None, metavar="K",
                    help="with --hdbscan / --mutual-reachability: the neighbour whose distance is the core distance "
                         "(default: --min-cluster-size with --hdbscan, 5 with --mutual-reachability)")
    ap.add_argument("--short-rows", choices=["error", "clamp"], default="error",
                    help="with --hdbscan / --mutual-reachability: a vertex with fewer than --min-samples edges is an "
                         "error (default) or takes its largest weight")
    ap.add_argument("--max-weight", type=float, default=None,
                    help="with --labels: keep forest edges of weight <= T (single linkage at distance T)")
    ap.add_argument("--rooted", type=str, default=None, metavar="OUT.npz",
                    help="write the rooted forest (parent, parent_eid, depth, pre, size: uint32) after the solve")
    ap.add_argument("--dendrogram", type=str, default=None, metavar="OUT.npz",
                    help="write the single-linkage dendrogram (leaf_parent, merge_eid, merge_parent, child_a, child_b, "
                         "size, height) after the solve")
    ap.add_argument("--paths", type=str, default=None, metavar="OUT.npz",
                    help="write the path queries' answers (a, b, eid, weight, lca, hops) after the solve; needs --pairs")
    ap.add_argument("--pairs", type=str, default=None, metavar="PAIRS.npy",
                    help="with --paths: the vertex pairs to query, an integer array of shape (Q, 2)")
    ap.add_argument("--replacements", type=str, default=None, metavar="OUT.npz",
                    help="write every forest edge's replacement (eid_by_edge, key) and the bridge / best-swap counts")
    ap.add_argument("--distances", type=str, default=None, metavar="OUT.npz",
                    help="write the forest distances (a, b, dist, lca) of the --pairs after the solve")
    ap.add_argument("--diameters", type=str, default=None, metavar="OUT.npz",
                    help="write every tree's diameter, far ends and eccentricities after the solve")
    ap.add_argument("--stretch", type=str, default=None, metavar="OUT.npz",
                    help="write the forest distance of every graph edge (dist) and the stretch summary after the solve")
    ap.add_argument("--hops", action="store_true", help="with --distances / --diameters: count edges, not weights")
    ap.add_argument("--points", type=str, default=None, metavar="X.npy",
                    help="an (n, d) array of points instead of a graph (float32 / float16 / integers): the exact k-NN "
                         "graph is built on the device; takes --knn, --metric, --knn-graph, --emst, --hdbscan and --exact")
    ap.add_argument("--knn", type=int, default=None, metavar="K",
                    help="with --points: neighbours per point (default with --hdbscan: --min-samples)")
    ap.add_argument("--metric", choices=["euclidean", "sqeuclidean"], default=None,
                    help="with --points: the distance written and clustered on (default euclidean)")
    ap.add_argument("--knn-graph", type=str, default=None, metavar="OUT.npz",
                    help="with --points: write the k-NN table (idx, dist) and the symmetrised canonical graph (u, v, w)")
    ap.add_argument("--emst", type=str, default=None, metavar="OUT.npz",
                    help="with --points: write the exact minimum spanning tree of the complete graph on the points "
                         "(u, v, w): Euclidean, or with --min-samples K the mutual-reachability tree (and core)")
    ap.add_argument("--exact", action="store_true",
                    help="with --points --hdbscan: cluster on the exact mutual-reachability MST, not the k-NN graph's "
                         "forest (--knn is ignored)")
    ap.add_argument("--gpus", type=int, default=1, help="GPUs driven by this one process (RCCL clique)")
    ap.add_argument("--generator", choices=["rmat", "grid"], default=None, help="synthetic graph instead of a file")
    ap.add_argument("--scale", type=int, default=16, help="R-MAT scale (2^scale vertices) / grid side k")
    ap.add_argument("--seed", type=int, default=1, help="generator seed (weights: seed + 1)")
    args = ap.parse_args(argv)
    args.cluster_out = None
    if args.clusters is not None:
        try:
            args.clusters = int(args.clusters)
        except ValueError:
            args.cluster_out, args.clusters = args.clusters, None
    if args.cluster_out is not None and (args.min_cluster_size is None or args.min_cluster_size < 2):
        ap.error("--clusters OUT.npz needs --min-cluster-size K with K >= 2")
    if args.cluster_out is None and args.hdbscan is None and args.min_cluster_size is not None:
        ap.error("--min-cluster-size needs --clusters OUT.npz")
    if args.hdbscan is not None and args.min_cluster_size is not None and args.min_cluster_size < 2:
        ap.error("--hdbscan OUT.npz takes --min-cluster-size K with K >= 2")
    if args.min_samples is not None and args.hdbscan is None and args.mutual_reachability is None and args.emst is None:
        ap.error("--min-samples needs --hdbscan OUT.npz or --mutual-reachability OUT.npz (or --points X.npy --emst OUT.npz)")
    if args.min_samples is not None and args.min_samples < 1:
        ap.error("--min-samples K needs K >= 1")
    if args.clusters is not None and args.max_weight is not None:
        ap.error("--clusters and --max-weight exclude each other")
    if (args.clusters is not None or args.max_weight is not None) and not args.labels:
        ap.error("--clusters / --max-weight need --labels OUT.npy")
    if (args.paths is not None and args.pairs is None) or (args.pairs is not None and args.paths is None
                                                           and args.distances is None):
        ap.error("--paths OUT.npz and --pairs PAIRS.npy go together")
    if args.distances is not None and args.pairs is None:
        ap.error("--distances OUT.npz needs --pairs PAIRS.npy")
    if args.points is None and (args.knn is not None or args.metric is not None or args.knn_graph is not None):
        ap.error("--knn / --metric / --knn-graph need --points X.npy")
    if args.points is None and (args.emst is not None or args.exact):
        ap.error("--emst / --exact need --points X.npy")
    if args.points is not None:
        if args.graph is not None or args.generator is not None or args.batch_dir is not None:
            ap.error("--points excludes --graph, --generator and --batch-dir")
        if args.knn_graph is None and args.hdbscan is None and args.emst is None:
            ap.error("--points X.npy needs --knn-graph OUT.npz or --hdbscan OUT.npz or --emst OUT.npz")
        if args.exact and args.hdbscan is None:
            ap.error("--exact needs --hdbscan OUT.npz")
        if args.knn is not None and not 1 <= args.knn <= 128:
            ap.error("--knn K needs 1 <= K <= 128")
        if args.knn_graph is not None and args.knn is None:
            ap.error("--knn-graph OUT.npz needs --knn K")
        others = ("labels", "cluster_out", "clusters", "mutual_reachability", "rooted", "dendrogram", "paths",
                  "replacements", "distances", "diameters", "stretch", "check_result")
        if any(getattr(args, o) is not None for o in others) or args.check or args.check_device:
            ap.error("--points takes --knn-graph OUT.npz and --hdbscan OUT.npz only, and --emst OUT.npz (the graph outputs "
                     "need a graph)")
        return run_points(args)
    if args.batch_dir is not None:
        return run_batch_dir(args)

    from . import graph as G

    t0 = time.perf_counter()
    if args.generator:
        from .device import generate_grid, generate_rmat
        e = (generate_rmat(args.scale, 16, seed=args.seed, wseed=args.seed + 1) if args.generator == "rmat"
             else generate_grid(args.scale, 0, wseed=args.seed + 1))
        g = e.to_host()
        del e
    else:
        g = G.read_mstbin(args.graph) if args.graph else G.read_graph_dir(args.graph_dir)
    t_read = time.perf_counter() - t0

    if args.check_result:
        import json

        from .verify import format_report, verify_forest
        with open(args.check_result) as f:
            triples = [tuple(e) for e in json.load(f)["mst_edges"]]
        rep = verify_forest(g, triples)
        print(format_report(rep, triples))
        return 0 if rep["ok"] else 1

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1:
        import torch
        import torch.distributed as dist

        from .device import DeviceEdges
        from .distributed import DistributedMST
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group("nccl")
        edges = DeviceEdges.from_host(g)
        d = DistributedMST(edges)
        res, _ = d.run()
        in_mst = d.in_mst_host()
        triples = g.edge_triples(in_mst)
        rounds, ms = res.rounds, res.ms_total
        flags = in_mst
        dist.barrier()
        dist.destroy_process_group()
    else:
        from .mst import minimum_spanning_forest
        r = minimum_spanning_forest(g, num_gpus=args.gpus)
        triples, rounds, ms = r.triples(), r.rounds, r.ms_total
        flags = r.in_mst
    if rank != 0:
        return 0
    if args.output:
        out = args.output
    elif args.generator:
        out = "ghs_mst.json"
    else:
        out = os.path.join(args.graph_dir if not args.graph else os.path.dirname(args.graph) or ".", "ghs_mst.json")
    res = G.write_result(out, triples)
    if args.mpi_compat:
        G.write_result(os.path.join(os.path.dirname(out), "mst_result_mpi.json"), triples)
    if not args.quiet:
        print("=" * 70)
        print("Boruvka MST on MI355X (HIP) — drop-in for the GHS MPI path")
        print("=" * 70)
        print(f"Nodes: {g.n}  Edges: {g.m}  GPUs: {max(world, args.gpus)}")
        print(f"MST edges: {res['num_edges']}  Total MST weight: {res['total_weight']}")
        print(f"Rounds (GHS levels): {rounds}  engine time: {ms:.3f} ms  read: {t_read * 1e3:.1f} ms")
        if res["num_edges"] == g.n - 1:
            print("Spanning tree: n-1 edges")
        else:
            print(f"Spanning forest: {g.n - res['num_edges']} components")
        print(f"Results saved to: {out}")
    if args.labels:
        import numpy as np

        from .mst import MSTResult
        lr = MSTResult(g, np.asarray(flags), 0, rounds, [], ms)
        t = args.max_weight
        if t is not None and g.weights is None:
            # integer engine weights: floor(T), and a negative T keeps nothing (as n clusters do)
            t = None if t < 0 else int(min(t, float((1 << 32) - 1)))
        if args.max_weight is not None and t is None:
            labels, info = lr.labels(num_clusters=max(g.n, 1), return_info=True)
        else:
            labels, info = lr.labels(max_weight=t, num_clusters=args.clusters, return_info=True)
        np.save(args.labels, labels)
        if not args.quiet:
            print(f"Clusters: {info['num_clusters']} (kept {info['kept_edges']} of {info['flagged_edges']} forest edges)")
            print(f"Labels saved to: {args.labels}")
    if args.rooted:
        import numpy as np

        from .mst import MSTResult
        rooted, rinfo = MSTResult(g, np.asarray(flags), 0, rounds, [], ms).rooted(return_info=True)
        np.savez(args.rooted, **rooted)
        if not args.quiet:
            print(f"Rooted forest: {rinfo['num_trees']} trees, max depth {rinfo['max_depth']}")
            print(f"Rooted forest saved to: {args.rooted}")
    if args.dendrogram:
        import numpy as np

        from .mst import MSTResult
        dg, dinfo = MSTResult(g, np.asarray(flags), 0, rounds, [], ms).dendrogram(return_info=True)
        np.savez(args.dendrogram, **dg)
        if not args.quiet:
            print(f"Dendrogram: {dinfo['flagged_edges']} merges, {dinfo['num_trees']} trees, height {dinfo['max_height']}")
            print(f"Dendrogram saved to: {args.dendrogram}")
    if args.cluster_out:
        import numpy as np

        from .mst import MSTResult
        cl, cinfo = MSTResult(g, np.asarray(flags), 0, rounds, [], ms).clusters(
            min_cluster_size=args.min_cluster_size, method=args.cluster_method,
            allow_single_cluster=args.allow_single_cluster, return_info=True)
        np.savez(args.cluster_out, **cl, **{k: np.asarray(v) for k, v in cinfo.items() if k != "ms_total"})
        if not args.quiet:
            print(f"Clusters: {cinfo['num_selected']} selected of {cinfo['num_clusters']} in the condensed tree "
                  f"(height {cinfo['cluster_height']}), {cinfo['num_noise']} noise vertices")
            print(f"Clusters saved to: {args.cluster_out}")
    if args.mutual_reachability or args.hdbscan:
        import numpy as np
        import torch

        from .device import DeviceEdges, hdbscan, mutual_reachability
        de = DeviceEdges.from_host(g)
        if g.weights is not None:
            de.weights = torch.from_numpy(np.ascontiguousarray(g.weights)).to(de.device)
        if args.mutual_reachability:
            mr = mutual_reachability(de, min_samples=5 if args.min_samples is None else args.min_samples,
                                     short_rows=args.short_rows)
            w_new = mr.edges.w.cpu().numpy().view(np.uint32) if g.weights is None else mr.edges.weights.cpu().numpy()
            counts = {k: np.asarray(v) for k, v in mr.info.items() if k != "ms_total"}
            np.savez(args.mutual_reachability, core=mr.core_values().cpu().numpy(), w=w_new, **counts)
            if not args.quiet:
                print(f"Mutual reachability: k = {mr.info['k']}, {mr.info['raised_edges']} of {g.m} edges raised, "
                      f"{mr.info['short_rows']} short rows, {mr.info['isolated']} isolated vertices, "
                      f"max degree {mr.info['max_degree']}")
                print(f"Mutual reachability saved to: {args.mutual_reachability}")
        if args.hdbscan:
            mcs = 5 if args.min_cluster_size is None else args.min_cluster_size
            h = hdbscan(de, min_cluster_size=mcs, min_samples=args.min_samples, method=args.cluster_method,
                        allow_single_cluster=args.allow_single_cluster, short_rows=args.short_rows)
            c = h.clusters
            arrays = {k: getattr(c, k).cpu().numpy() for k in (
                "label", "probability", "point_cluster", "point_lambda", "cluster_head", "cluster_parent", "cluster_size",
                "cluster_birth", "cluster_stability", "cluster_selected")}
            for k in ("point_cluster", "cluster_head", "cluster_parent", "cluster_size"):
                arrays[k] = arrays[k].view(np.uint32)
            counts = {k: np.asarray(v) for k, v in c.info.items() if k != "ms_total"}
            np.savez(args.hdbscan, core=h.reach.core_values().cpu().numpy(), in_mst=h.mst.in_mst_host(), **arrays, **counts)
            if not args.quiet:
                print(f"HDBSCAN: {c.info['num_selected']} clusters selected of {c.info['num_clusters']} in the condensed "
                      f"tree, {c.info['num_noise']} noise vertices ({h.reach.info['raised_edges']} of {g.m} edges raised)")
                print(f"HDBSCAN saved to: {args.hdbscan}")
    if args.paths:
        import numpy as np

        from .mst import MSTResult
        pairs = np.load(args.pairs)
        if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.dtype.kind not in "iu":
            raise ValueError(f"{args.pairs}: an integer array of shape (Q, 2) expected, got {pairs.dtype} {pairs.shape}")
        ans, pinfo = MSTResult(g, np.asarray(flags), 0, rounds, [], ms).paths(pairs[:, 0], pairs[:, 1], return_info=True)
        np.savez(args.paths, a=pairs[:, 0], b=pairs[:, 1], eid=ans["eid"], weight=ans["weight"], lca=ans["lca"],
                 hops=ans["hops"])
        if not args.quiet:
            heaviest = ans["weight"][ans["has_edge"]].max() if ans["has_edge"].any() else "none"
            print(f"Path queries: {len(pairs)} pairs, {int(ans['connected'].sum())} connected, max bottleneck {heaviest}")
            print(f"Path answers saved to: {args.paths}")
    if args.replacements:
        import numpy as np

        from .mst import MSTResult
        rep, pinfo = MSTResult(g, np.asarray(flags), 0, rounds, [], ms).replacements(return_info=True, per_vertex=True)
        counts = {k: np.asarray(v) for k, v in pinfo.items() if k != "ms_total"}
        np.savez(args.replacements, eid_by_edge=rep["eid"], key=rep["key"], **counts)
        if not args.quiet:
            swap = (f"best swap {pinfo['best_out_eid']} -> {pinfo['best_in_eid']} ({pinfo['best_delta']:+d})"
                    if pinfo["best_out_eid"] != 0xFFFFFFFF else "no swap")
            print(f"Replacements: {pinfo['tree_edges']} forest edges, {pinfo['bridges']} bridges, {swap}")
            print(f"Replacements saved to: {args.replacements}")
    if args.distances:
        import numpy as np

        from .mst import MSTResult
        pairs = np.load(args.pairs)
        if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.dtype.kind not in "iu":
            raise ValueError(f"{args.pairs}: an integer array of shape (Q, 2) expected, got {pairs.dtype} {pairs.shape}")
        dist, lca, dinfo = MSTResult(g, np.asarray(flags), 0, rounds, [], ms).distances(
            pairs[:, 0], pairs[:, 1], hops=args.hops, return_lca=True, return_info=True)
        np.savez(args.distances, a=pairs[:, 0], b=pairs[:, 1], dist=dist, lca=lca)
        if not args.quiet:
            print(f"Distances: {len(pairs)} pairs, {dinfo['connected']} connected, max distance {dinfo['max_dist']}")
            print(f"Distances saved to: {args.distances}")
    if args.diameters:
        import numpy as np

        from .mst import MSTResult
        tm, tinfo = MSTResult(g, np.asarray(flags), 0, rounds, [], ms).diameters(hops=args.hops, return_info=True)
        np.savez(args.diameters, **tm, **{k: np.asarray(v) for k, v in tinfo.items() if k != "ms_total"})
        if not args.quiet:
            print(f"Diameters: {tinfo['num_trees']} trees, max diameter {tinfo['max_diameter']} (root {tinfo['max_root']}), "
                  f"centre {tinfo['center']} at radius {tinfo['min_ecc']}")
            print(f"Diameters saved to: {args.diameters}")
    if args.stretch:
        import numpy as np

        from .mst import MSTResult
        sd = MSTResult(g, np.asarray(flags), 0, rounds, [], ms).edge_distances()
        summary = {k: np.asarray(-1 if v is None else v) for k, v in sd.items() if k not in ("dist", "stretch", "sum_dist")}
        np.savez(args.stretch, dist=sd["dist"], sum_dist=np.asarray(str(sd["sum_dist"])), **summary)
        if not args.quiet:
            avg = sd["sum_dist"] / sd["sum_w"] if sd["sum_w"] else float("nan")
            print(f"Stretch: {g.m} edges, sum dist {sd['sum_dist']}, sum w {sd['sum_w']} (average {avg:.6g}), "
                  f"max dist {sd['max_dist']} at edge {sd['max_eid']}, {sd['tight_edges']} tight")
            print(f"Stretch saved to: {args.stretch}")
    status = 0
    if args.check:
        from .verify import format_report, verify_forest
        rep = verify_forest(g, triples)
        print(format_report(rep, triples))
        status = 0 if rep["ok"] else 1
    if args.check_device:
        from .verify import format_device_report, verify_forest_device
        drep = verify_forest_device(g, flags)
        print(format_device_report(drep))
        status = status if drep["ok"] else 1
    return status


if __name__ == "__main__":
    sys.exit(main())
