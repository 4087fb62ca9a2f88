"""numpy and scipy model of RULE K (include/cwipc_util_amd/hip_ext.h): Euclidean clusters and the cluster filter, written from the
rule's text.

Candidate pairs come from scipy.spatial.cKDTree.query_pairs at a slightly larger radius (the tree's own arithmetic decides nothing);
the rule's float64 d2 < r2 and the tile test cut them; scipy.sparse.csgraph.connected_components follows, renumbered by smallest
index.  brute_force_labels is the O(n^2) sequential union the model is checked against (tests/test_cluster_model.py)."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

NONE = 0xFFFFFFFF


def _d2(a, b):
    """(dx*dx + dy*dy) + dz*dz in float64, every operation rounded on its own; a, b: float32 (m, 3)"""
    d = a.astype(np.float64) - b.astype(np.float64)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def links(xyz, radius, tiles=None):
    """The rule's links among the points with finite coordinates: (i, j) index pairs, i < j."""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    r2 = np.float64(radius) * np.float64(radius)
    finite = np.flatnonzero(np.isfinite(xyz).all(axis=1))
    if len(finite) < 2:
        return np.zeros((0, 2), dtype=np.int64)
    pts = xyz[finite]
    reach = float(radius) * (1.0 + 1e-6) + 1e-30
    if not np.isfinite(reach):
        reach = np.finfo(np.float64).max
    pairs = cKDTree(pts.astype(np.float64)).query_pairs(reach, output_type="ndarray")
    if len(pairs) == 0:
        return np.zeros((0, 2), dtype=np.int64)
    keep = _d2(pts[pairs[:, 0]], pts[pairs[:, 1]]) < r2
    pairs = finite[pairs[keep]]
    if tiles is not None:
        tiles = np.asarray(tiles)
        pairs = pairs[tiles[pairs[:, 0]] == tiles[pairs[:, 1]]]
    return pairs


def _renumber(component, finite, n):
    """component ids of the finite points -> (labels, sizes): clusters numbered by their smallest index"""
    labels = np.full(n, NONE, dtype=np.uint32)
    if len(finite) == 0:
        return labels, np.zeros(0, dtype=np.uint32)
    component = np.unique(component, return_inverse=True)[1].reshape(-1)   # (the graph's other nodes, the non-finite points, left ids behind)
    ncomp = int(component.max()) + 1
    first = np.full(ncomp, n, dtype=np.int64)
    np.minimum.at(first, component, finite)
    order = np.argsort(first, kind="stable")          # component ids in ascending order of their smallest index
    number = np.empty(ncomp, dtype=np.int64)
    number[order] = np.arange(ncomp)
    labels[finite] = number[component].astype(np.uint32)
    sizes = np.bincount(number[component], minlength=ncomp).astype(np.uint32)
    return labels, sizes


def cluster_labels(xyz, radius, tiles=None):
    """(labels uint32 (n,), sizes uint32 (C,)) by RULE K; tiles: the tile bytes for CWIPC_HIP_CLUSTER_SAME_TILE, None without it."""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    n = len(xyz)
    finite = np.flatnonzero(np.isfinite(xyz).all(axis=1))
    pairs = links(xyz, radius, tiles)
    graph = coo_matrix((np.ones(len(pairs), dtype=np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    _, comp = connected_components(graph, directed=False)
    return _renumber(comp[finite], finite, n)


def ranks(sizes):
    """rank[c] by (size descending, number ascending)"""
    order = np.lexsort((np.arange(len(sizes)), -sizes.astype(np.int64)))
    rank = np.empty(len(sizes), dtype=np.int64)
    rank[order] = np.arange(len(sizes))
    return rank


def keep_mask(labels, sizes, min_points=1, max_clusters=0):
    """The filter's keep mask from labels and sizes."""
    labelled = labels != NONE
    ok = sizes.astype(np.int64) >= int(min_points)
    if max_clusters:
        ok &= ranks(sizes) < int(max_clusters)
    keep = np.zeros(len(labels), dtype=bool)
    keep[labelled] = ok[labels[labelled]]
    return keep


def cluster_filter(points, radius, min_points=1, max_clusters=0, same_tile=False):
    """points: the structured cwipc point array; -> the kept points, in input order"""
    xyz = np.stack([points["x"], points["y"], points["z"]], axis=1)
    labels, sizes = cluster_labels(xyz, radius, points["tile"] if same_tile else None)
    return points[keep_mask(labels, sizes, min_points, max_clusters)]


def brute_force_labels(xyz, radius, tiles=None):
    """O(n^2) sequential union over every pair, the rule's arithmetic; for small n."""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    n = len(xyz)
    r2 = np.float64(radius) * np.float64(radius)
    finite = np.isfinite(xyz).all(axis=1)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    for i in range(n):
        if not finite[i]:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            near = np.flatnonzero(_d2(np.broadcast_to(xyz[i], (i, 3)), xyz[:i]) < r2) if i else []
        for j in near:
            if not finite[j] or (tiles is not None and tiles[i] != tiles[j]):
                continue
            a, b = find(i), find(int(j))
            if a != b:
                parent[max(a, b)] = min(a, b)
    roots = np.array([find(i) if finite[i] else -1 for i in range(n)], dtype=np.int64)
    labels = np.full(n, NONE, dtype=np.uint32)
    uniq = np.unique(roots[roots >= 0])               # ascending roots: the cluster numbers
    labels[roots >= 0] = np.searchsorted(uniq, roots[roots >= 0]).astype(np.uint32)
    sizes = np.array([(roots == r).sum() for r in uniq], dtype=np.uint32)
    return labels, sizes
