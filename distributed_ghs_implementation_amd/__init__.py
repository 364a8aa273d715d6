"""MI355X-native MST engine — the GHS fragment-merging hot path of
Trisanu-007/Distributed_GHS_Implementation rebuilt as a level-synchronous Boruvka fragment
contraction in hand-written gfx950 HIP kernels (libghs_mst.so, C-ABI in include/ghs_mst.h).

Entry points mirroring the reference:
  GHSAlgorithm(num_nodes, edges).run()      ghs_implementation.py:416-490
  python -m distributed_ghs_implementation_amd --graph-dir D
                                            ghs_implementation_mpi.py:884-954 (CLI)
Array level: graph.canonicalize -> mst.minimum_spanning_forest (many small graphs in one launch:
mst.minimum_spanning_forest_batch; raw edge arrays canonicalized on the device:
mst.minimum_spanning_forest_edges); device level: device.DeviceMST, device.batch_mst,
device.canonicalize_device; the forest's vertex labels (connected components, single-linkage cuts by
weight or cluster count): device.forest_labels, DeviceMST.labels, MSTResult.labels, CLI --labels;
the forest rooted (parent, parent edge, depth, DFS preorder, subtree size per vertex):
device.forest_root, DeviceMST.rooted, MSTResult.rooted, CLI --rooted;
path queries on it (heaviest edge between a and b = the minimax distance, lowest common ancestor,
hop count): device.forest_paths, DeviceMST.paths, MSTResult.paths, CLI --paths / --pairs;
replacement edges (what takes a forest edge's place when it fails, the bridges, the best swap):
device.forest_replacements, PathIndex.replacements, DeviceMST.replacements, MSTResult.replacements,
CLI --replacements;
tree distances (how far it is from a to b along the forest, the stretch of every graph edge over it,
every tree's diameter, far ends, eccentricities and centre): device.forest_distances /
forest_edge_distances / forest_diameters, PathIndex.wdepth / distances / edge_distances / diameters,
DeviceMST.distances / edge_distances / diameters, MSTResult.distances / edge_distances / diameters,
CLI --distances / --pairs, --diameters, --stretch (--hops counts edges: the only metric for rank-mapped
weights);
the single-linkage dendrogram (the whole merge order, scipy's linkage matrix): device.forest_dendrogram,
DeviceMST.dendrogram, MSTResult.dendrogram, CLI --dendrogram;
HDBSCAN cluster extraction from it (the condensed tree for a min_cluster_size, stabilities, the
excess-of-mass or leaf selection, labels with noise and membership probabilities):
device.forest_clusters, Dendrogram.clusters, DeviceMST.clusters, MSTResult.clusters,
CLI --clusters OUT.npz --min-cluster-size K;
the weights HDBSCAN wants (core distances: the min_samples-th smallest weight at every vertex; mutual
reachability: max(core[u], core[v], w) on every edge) and HDBSCAN end to end on a k-NN graph or a
sparse distance matrix: device.mutual_reachability, DeviceEdges.mutual_reachability, device.hdbscan,
DeviceEdges.hdbscan, mst.hdbscan_edges, CLI --mutual-reachability OUT.npz, --hdbscan OUT.npz;
where the graph comes from (the exact brute-force k nearest neighbours of float32 points, the symmetrised
k-NN graph as a canonical list, HDBSCAN from points end to end): device.knn, device.knn_graph,
device.hdbscan_points, mst.hdbscan_points, CLI --points X.npy --knn K --knn-graph OUT.npz / --hdbscan OUT.npz;
the exact MST of the complete graph on points (Euclidean or mutual-reachability) and HDBSCAN exact from
points to labels: device.emst, device.hdbscan_points(exact=True), mst.emst_points,
mst.hdbscan_points(exact=True), CLI --points X.npy --emst OUT.npz / --hdbscan OUT.npz --exact;
multi-GPU: distributed.DistributedMST. Float, negative and 64-bit
weights: rank-mapped by graph.canonicalize on the host, or on the device with rank_weights=True
(minimum_spanning_forest_edges, DeviceEdges.from_raw, canonicalize_device; device.weight_ranks).
"""
from .graph import (CanonicalGraph, canonicalize, read_graph_dir, read_mstbin, write_graph_dir, write_mstbin,
                    write_result)
from .mst import (GHSAlgorithm, MSTResult, hdbscan_edges, hdbscan_points, minimum_spanning_forest, minimum_spanning_forest_batch,
                  minimum_spanning_forest_edges)

__all__ = [
    "CanonicalGraph", "canonicalize", "read_graph_dir", "read_mstbin", "write_graph_dir", "write_mstbin",
    "write_result", "GHSAlgorithm", "MSTResult", "minimum_spanning_forest", "minimum_spanning_forest_batch",
    "minimum_spanning_forest_edges", "hdbscan_edges", "hdbscan_points",
]
