"""RULE K without a GPU: the numpy and scipy model (tests/cluster_model.py) against an O(n^2) sequential union, the model's own
edge cases, and the new symbols exported, bound, declared and registered."""
import ctypes
import os
import re

import numpy as np
import pytest

import cluster_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_cloud(n, seed, bad=2):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    for k, v in zip(rng.choice(n, bad, replace=False), (np.nan, np.inf, -np.inf)):
        xyz[k, rng.integers(0, 3)] = v
    return xyz


@pytest.mark.parametrize("radius", [0.02, 0.05, 0.08, 0.2])
def test_model_against_brute_force(radius):
    """1 500 random points, two of them non-finite: from nearly all singletons to one cluster."""
    xyz = random_cloud(1500, 1500)
    tiles = np.random.default_rng(3).integers(1, 3, 1500).astype(np.uint8)
    for t in (None, tiles):
        labels, sizes = cm.cluster_labels(xyz, radius, t)
        blabels, bsizes = cm.brute_force_labels(xyz, radius, t)
        assert np.array_equal(labels, blabels) and np.array_equal(sizes, bsizes)
        assert (labels == cm.NONE).sum() == 2 and sizes.sum() == 1498
        # numbered by first appearance: a cluster's first member comes after those of every lower number
        firsts = [np.flatnonzero(labels == c)[0] for c in range(len(sizes))]
        assert firsts == sorted(firsts)
    counts = [len(cm.cluster_labels(xyz, r)[1]) for r in (0.02, 0.2)]
    assert counts[0] > 1000 and counts[1] == 1


def test_model_is_strict_at_the_radius():
    g = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32) * np.float32(0.25)
    labels, sizes = cm.cluster_labels(g, 0.25)
    assert len(sizes) == 64 and np.array_equal(labels, np.arange(64))
    labels, sizes = cm.cluster_labels(g, np.nextafter(0.25, 1))
    assert sizes.tolist() == [64] and not labels.any()


def test_model_small_clouds_and_duplicates():
    assert [a.tolist() for a in cm.cluster_labels(np.zeros((0, 3)), 1.0)] == [[], []]
    assert [a.tolist() for a in cm.cluster_labels(np.zeros((1, 3)), 1.0)] == [[0], [1]]
    assert [a.tolist() for a in cm.cluster_labels(np.float32([[0, 0, 0], [0.5, 0, 0]]), 1.0)] == [[0, 0], [2]]
    assert [a.tolist() for a in cm.cluster_labels(np.float32([[0, 0, 0], [1.5, 0, 0]]), 1.0)] == [[0, 1], [1, 1]]
    assert [a.tolist() for a in cm.cluster_labels(np.tile(np.float32([[0.5, 0.25, 0.75]]), (64, 1)), 1e-6)] == [[0] * 64, [64]]
    labels, sizes = cm.cluster_labels(np.float32([[np.nan, 0, 0], [0, 0, 0], [0, np.inf, 0], [0.1, 0, 0]]), 1.0)
    assert labels.tolist() == [cm.NONE, 0, cm.NONE, 0] and sizes.tolist() == [2]


def test_model_ranking_and_keep_mask():
    sizes = np.uint32([3, 5, 5, 1, 3])
    assert cm.ranks(sizes).tolist() == [2, 0, 1, 4, 3]
    labels = np.uint32([0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 3, 4, 4, 4, cm.NONE])
    assert cm.keep_mask(labels, sizes).tolist() == [True] * 17 + [False]
    assert cm.keep_mask(labels, sizes, min_points=3).sum() == 16 and cm.keep_mask(labels, sizes, min_points=4).sum() == 10
    assert np.flatnonzero(cm.keep_mask(labels, sizes, max_clusters=1)).tolist() == [3, 4, 5, 6, 7]          # equal sizes: the lower number
    assert cm.keep_mask(labels, sizes, max_clusters=3).sum() == 13 and cm.keep_mask(labels, sizes, max_clusters=5).sum() == 17
    assert cm.keep_mask(labels, sizes, min_points=5, max_clusters=3).sum() == 10


def test_new_symbols_are_exported_bound_and_declared(cwipc):
    from cwipc_util_amd.util import _SIGNATURES
    dll = cwipc.cwipc_util_dll_load()
    header = open(os.path.join(ROOT, "include", "cwipc_util_amd", "hip_ext.h")).read()
    assert "RULE K." in header
    assert "#define CWIPC_HIP_CLUSTER_SAME_TILE 1" in header and cwipc.CWIPC_HIP_CLUSTER_SAME_TILE == 1
    for name in ("cwipc_hip_clusters", "cwipc_hip_cluster_filter", "cwipc_hip_cluster_link_stats", "cwipc_hip_cluster_rank_keep"):
        assert hasattr(dll, name) and name in _SIGNATURES, name
        assert re.search(r"_CWIPC_UTIL_EXPORT[^;]*\b%s\(" % name, header), name
    for public in ("cwipc_cluster_labels", "cwipc_cluster_filter", "cwipc_hip_cluster_link_stats", "cwipc_hip_cluster_rank_keep", "CWIPC_HIP_CLUSTER_SAME_TILE"):
        assert public in cwipc.util.__all__ and hasattr(cwipc, public), public
    pc_p = _SIGNATURES["cwipc_hip_direction_filter"][0][0]
    # the header's parameter lists against the wrapper's argument types
    params = re.search(r"cwipc_hip_clusters\(([^)]*)\)", header).group(1)
    assert [p.strip().rsplit(" ", 1)[0] for p in params.split(",")] == ["cwipc_pointcloud", "double", "int", "uint32_t", "uint32_t", "size_t", "uint32_t"]
    assert _SIGNATURES["cwipc_hip_clusters"] == ([pc_p, ctypes.c_double, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                                   ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int)
    params = re.search(r"cwipc_hip_cluster_filter\(([^)]*)\)", header).group(1)
    assert [p.strip().rsplit(" ", 1)[0] for p in params.split(",")] == ["cwipc_pointcloud", "double", "int", "uint64_t", "uint32_t"]
    assert _SIGNATURES["cwipc_hip_cluster_filter"] == ([pc_p, ctypes.c_double, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32], pc_p)
    params = re.search(r"cwipc_hip_cluster_rank_keep\(([^)]*)\)", header).group(1)
    assert [p.strip().rsplit(" ", 1)[0] for p in params.split(",")] == ["const uint32_t", "size_t", "uint64_t", "uint32_t", "uint8_t"]
    assert _SIGNATURES["cwipc_hip_cluster_rank_keep"] == ([ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p], ctypes.c_int)


def test_factory_entry(cwipc):
    from cwipc_util_amd import filters
    from cwipc_util_amd.filters import cluster
    f = filters.factory("cluster(0.02, 100, 1)")
    assert isinstance(f, cluster.ClusterFilter) and f.filtername == "cluster"
    assert (f.radius, f.min_points, f.max_clusters, f.same_tile) == (0.02, 100, 1, False)
    g = filters.factory("cluster(0.05)")
    assert (g.min_points, g.max_clusters) == (1, 0)
    assert cluster in filters.all_filters and "cluster" in filters.__doc__
    assert callable(f.filter) and callable(f.statistics)


def test_refusals_need_no_gpu(cwipc):
    """Bad arguments are turned away before the device is asked for: -1 / NULL with an ERROR logged."""
    dll = cwipc.cwipc_util_dll_load()
    labels = np.zeros(4, dtype=np.uint32)
    n = ctypes.c_uint32(7)
    assert dll.cwipc_hip_clusters(None, 0.1, 0, labels.ctypes.data, None, 4, ctypes.byref(n)) == -1
    assert not dll.cwipc_hip_cluster_filter(None, 0.1, 0, 1, 0)
    assert dll.cwipc_hip_cluster_link_stats(None, 0.1, 0, None) == -1
    keep = np.full(4, 7, dtype=np.uint8)
    assert dll.cwipc_hip_cluster_rank_keep(None, 4, 1, 0, keep.ctypes.data) == -1
    assert dll.cwipc_hip_cluster_rank_keep(labels.ctypes.data, 4, 1, 0, None) == -1
    assert dll.cwipc_hip_cluster_rank_keep(labels.ctypes.data, 0, 1, 0, keep.ctypes.data) == 0 and np.all(keep == 7)     # no cluster: nothing written


def test_edge_case_constructions_do_what_their_names_say():
    """The inputs of tests/test_gpu_cluster_edges.py's three-flow cases, built and held to their purpose by the model alone: the
    bridge of another tile cuts the chain, twins at identical coordinates fall apart by tile, the far outliers are the clusters the
    rule's arithmetic gives, the translated cloud's coordinates tie.  A wrong generator fails here, without a GPU."""
    import test_gpu_cluster_edges as edges
    cases, want = edges.edge_answers()
    assert set(cases) == set(want) and len(cases) == 19
    assert sum(same for _, _, same in cases.values()) == 7


def test_scale_case_is_as_large_as_its_purpose():
    """1 061 208 points (more than 4096 workgroups of 256 hold) in more than 262 144 clusters (more than the histogram's launch holds)."""
    import test_gpu_cluster_edges as edges
    pts, radius, labels, sizes, _ = edges.scale_case()
    assert len(pts) > 4096 * 256 and len(sizes) > 262144 and sizes.sum() == len(pts) and labels.max() == len(sizes) - 1
