"""The numpy model of RULE Q (tests/quality_model.py) held to things that do not come from it -- a case worked out by hand, its own
brute force, the PSNR formulas' edges -- and, without a GPU, the boundary: the library exports cwipc_hip_distortion, the header, the
wrapper and the struct agree, cwipc_util_amd.quality has its names, and a call without a device fails loudly.

A NOTE ON "A PAIR WITHOUT A NORMAL".  RULE Q gives reference point j of the forward pass the normal nA[idxBA[j]], none when idxBA[j]
is none.  Through the entry point a MATCHED forward pair never meets that case: if original point a is matched to degraded point b,
then d2(a, b) < max_distance^2 with both finite, d2(b, a) is the same f64 number (a negated difference squares to the same bits), so
b has at least a as a candidate in the backward pass and idxBA[b] is an index.  Hence forward n_plane == n whenever normals are
used -- test_forward_pairs_always_inherit_a_normal holds the model to that on a bounded search -- and the branch is the kernel's
guard against an index that is no address.  The model's one_pass takes the index array as an argument, so the hand-worked case
below feeds it one with a hole."""
import math
import os
import re

import numpy as np
import pytest

import quality_model as qm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = qm.NONE

# the hand-worked case: three original points with colours and normals, two degraded points
A = qm.make_cloud([[0, 0, 0], [2, 0, 0], [10, 0, 0]], [[10, 20, 30], [200, 100, 50], [0, 0, 0]])
NA = np.float32([[0, 0, 1], [1, 0, 0], [0, 0, 1]])
B = qm.make_cloud([[1, 0, 0.5], [10, 0, 3]], [[12, 20, 30], [5, 5, 5]])


def test_hand_worked_case_with_a_tie_and_a_bound():
    """max_distance 2.  b0 = (1, 0, 0.5) is 1.25 from a0 AND from a1 (squared): the tie goes to a0, the smaller index, whose colour
    differs from b0's by (2, 0, 0) -- a1's would differ by (-188, -80, -20).  b1 is 9 from a2: beyond the bound, no match.  Forward,
    a0 and a1 both match b0, which carries a0's normal (0, 0, 1) -- a1's own (1, 0, 0) would give r = 1, not -0.5; a2 matches nothing."""
    fwd, bwd = qm.distortion(A, B, 2.0, NA)
    assert bwd["idx"].tolist() == [0, NONE] and fwd["idx"].tolist() == [0, 0, NONE]
    s = qm.sums(bwd)
    assert (bwd["n_source"], bwd["n"], bwd["n_plane"], bwd["max_d2"]) == (2, 1, 1, 1.25)
    assert s["sum_d2"] == 1.25 and s["sum_r2"] == 0.25 and s["sum_rgb2"] == [4, 0, 0]
    assert s["sum_yuv2"] == pytest.approx([0.18079504, 0.05253264, 1.0], rel=1e-14)
    s = qm.sums(fwd)
    assert (fwd["n_source"], fwd["n"], fwd["n_plane"], fwd["max_d2"]) == (3, 2, 2, 1.25)
    assert s["sum_d2"] == 2.5 and s["sum_r2"] == 0.5 and s["sum_rgb2"] == [4 + 35344, 6400, 400]
    assert s["sum_yuv2"] == pytest.approx([0.18079504 + 9727.64018944, 0.05253264 + 1795.79317824, 1.0 + 3220.335504], rel=1e-14)
    # at exactly the bound a pair is out: strictly closer only (b1 is 3 from a2)
    assert qm.distortion(A, B, 3.0, NA)[1]["idx"].tolist() == [0, NONE] and qm.distortion(A, B, 3.0000001, NA)[1]["idx"].tolist() == [0, 2]
    fwd, bwd = qm.distortion(A, B, 1.0, NA)
    assert (fwd["n"], bwd["n"]) == (0, 0) and fwd["max_d2"] == 0.0 and qm.sums(fwd)["sum_rgb2"] == [0, 0, 0]
    # without a bound b1 matches a2: r = (b1 - a2) . (0, 0, 1) = 3
    fwd, bwd = qm.distortion(A, B, np.inf, NA)
    assert bwd["idx"].tolist() == [0, 2] and qm.sums(bwd)["sum_r2"] == 0.25 + 9.0 and bwd["max_d2"] == 9.0
    # no normals at all
    fwd, bwd = qm.distortion(A, B, np.inf, None)
    assert (fwd["n_plane"], bwd["n_plane"]) == (0, 0) and qm.sums(fwd)["sum_r2"] == 0.0 and fwd["n"] == 3


def test_hand_worked_pair_without_an_inherited_normal():
    """one_pass with an index array that has a hole (see the note at the top): a0 -> b0, which carries a0's normal, and a1 -> b1',
    which carries none; a2 unmatched.  n_plane counts one pair, sum r^2 has one term, every other sum has two."""
    B2 = qm.make_cloud([[1, 0, 0.5], [2, 0, 1]], [[12, 20, 30], [200, 100, 49]])
    idx, d2 = np.array([0, 1, NONE], dtype=np.uint32), np.array([1.25, 1.0, np.inf])
    one = qm.one_pass(A, B2, idx, d2, NA, np.array([0, NONE], dtype=np.uint32))
    s = qm.sums(one)
    assert (one["n"], one["n_plane"], one["max_d2"]) == (2, 1, 1.25)
    assert s["sum_d2"] == 2.25 and s["sum_r2"] == 0.25 and s["sum_rgb2"] == [4, 0, 1]
    assert one["terms"][:, 1].tolist() == [1.0, 0.0] and one["terms"][:, 3].tolist() == [0.25, 0.0]
    both = qm.one_pass(A, B2, idx, d2, NA, np.array([0, 1], dtype=np.uint32))
    assert both["n_plane"] == 2 and qm.sums(both)["sum_r2"] == 0.25 + 0.0      # (a1 - b1') . (1, 0, 0) = 0


def lattice(n, shift, rng):
    """an n^3 lattice of pitch 0.25 from -1 (every coordinate and every half pitch a short binary fraction) with distinct colours"""
    g = np.arange(n) * 0.25 - 1.0
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + np.asarray(shift)
    colours = rng.permutation(256 ** 3)[:len(pts)]
    return qm.make_cloud(pts, np.stack([colours & 255, (colours >> 8) & 255, colours >> 16], axis=1))


@pytest.mark.parametrize("axes", [1, 2, 3])
def test_tree_equals_brute_force_on_a_lattice_with_ties(axes):
    rng = np.random.default_rng(40 + axes)
    a = lattice(6, (0, 0, 0), rng)
    b = lattice(6, [0.125] * axes + [0.0] * (3 - axes), rng)
    assert qm.tied_queries(b, a) >= 100
    normals = rng.normal(size=(len(a), 3)).astype(np.float32)
    for maxd in (np.inf, 0.25):
        brute, tree = qm.distortion(a, b, maxd, normals), qm.distortion(a, b, maxd, normals, tree=True)
        for x, y in zip(brute, tree):
            assert np.array_equal(x["idx"], y["idx"]) and x["terms"].tobytes() == y["terms"].tobytes() and x["max_d2"] == y["max_d2"]
            assert x["n"] > 100


def test_forward_pairs_always_inherit_a_normal():
    """The note at the top, on a bounded search that leaves many points of either side unmatched."""
    rng = np.random.default_rng(44)
    a = qm.make_cloud(rng.uniform(0, 1, (1500, 3)), rng.integers(0, 256, (1500, 3)))
    b = qm.make_cloud(rng.uniform(0, 1, (1200, 3)), rng.integers(0, 256, (1200, 3)))
    fwd, bwd = qm.distortion(a, b, 0.04, rng.normal(size=(1500, 3)).astype(np.float32))
    assert 100 < fwd["n"] < 1400 and 100 < bwd["n"] < 1100
    assert (bwd["idx"] == NONE).sum() > 100            # degraded points without a normal exist ...
    assert fwd["n_plane"] == fwd["n"] and bwd["n_plane"] == bwd["n"]     # ... and no matched pair meets one


def test_psnr_edges_and_the_symmetric_rule():
    assert qm.psnr(1.0, 0.0) == math.inf and math.isnan(qm.psnr(1.0, float("nan"))) and qm.psnr(100.0, 1.0) == 20.0
    fwd, bwd = qm.distortion(A, B, np.inf, NA)
    r = qm.results(fwd, bwd, 10.0)
    for key in ("mse_d1", "mse_d2", "hausdorff"):
        assert r["symmetric"][key] == max(r["forward"][key], r["backward"][key])
    assert r["forward"]["mse_d1"] != r["backward"]["mse_d1"]
    assert r["symmetric"]["mse_yuv"] == tuple(max(x, y) for x, y in zip(r["forward"]["mse_yuv"], r["backward"]["mse_yuv"]))
    assert r["psnr_d1"] == 10 * math.log10(300.0 / r["symmetric"]["mse_d1"])
    assert r["psnr_y"] == 10 * math.log10(65025.0 / r["symmetric"]["mse_yuv"][0])
    # the very same cloud: every mse 0, every PSNR +inf
    fwd, bwd = qm.distortion(A, A, np.inf, NA)
    r = qm.results(fwd, bwd, 10.0)
    assert r["symmetric"]["mse_d1"] == 0.0 and all(r[k] == math.inf for k in ("psnr_d1", "psnr_d2", "psnr_y", "psnr_u", "psnr_v"))
    # n = 0: NaN everywhere, also where only one direction has none
    empty = qm.make_cloud(np.zeros((0, 3)), np.zeros((0, 3)))
    fwd, bwd = qm.distortion(A, empty, np.inf, NA)
    r = qm.results(fwd, bwd, 10.0)
    assert fwd["n"] == 0 and bwd["n"] == 0 and bwd["n_source"] == 0 and fwd["n_source"] == 3
    assert all(math.isnan(r[k]) for k in ("psnr_d1", "psnr_d2", "psnr_y", "psnr_u", "psnr_v")) and r["forward"]["hausdorff"] == 0.0
    fwd, bwd = qm.distortion(A, B, np.inf, None)     # no normals: D2 is NaN, D1 is not
    r = qm.results(fwd, bwd, 10.0)
    assert math.isnan(r["psnr_d2"]) and math.isfinite(r["psnr_d1"])


def test_the_python_layer_computes_what_the_model_computes(cwipc):
    """cwipc_util_amd.quality from sums (no GPU): DistortionResults of the model's sums equals the model's results, field for field."""
    from cwipc_util_amd import quality
    for maxd, normals, b in ((np.inf, NA, B), (2.0, NA, B), (np.inf, None, B), (np.inf, NA, A), (np.inf, NA, B[:0])):
        structs = []
        passes = qm.distortion(A, b, maxd, normals)
        for one in passes:
            s = qm.sums(one)
            st = cwipc.cwipc_hip_distortion_sums(one["n_source"], one["n"], one["n_plane"], s["sum_d2"], one["max_d2"], s["sum_r2"])
            for c in range(3):
                st.sum_rgb2[c], st.sum_yuv2[c] = s["sum_rgb2"][c], s["sum_yuv2"][c]
            structs.append(st)
        got = quality.DistortionResults(structs[0], structs[1], 10.0).as_dict()
        want = qm.results(passes[0], passes[1], 10.0)
        got.pop("peak")
        assert repr(got) == repr(want)
    assert quality.psnr(1.0, 0.0) == math.inf and math.isnan(quality.psnr(1.0, float("nan")))


def test_new_symbol_is_exported_and_declared(cwipc):
    import ctypes
    from cwipc_util_amd.util import _SIGNATURES
    from cwipc_util_amd import quality
    dll = cwipc.cwipc_util_dll_load()
    header = open(os.path.join(ROOT, "include", "cwipc_util_amd", "hip_ext.h")).read()
    name = "cwipc_hip_distortion"
    assert hasattr(dll, name) and name in _SIGNATURES
    for public in (name, "cwipc_hip_distortion_sums", "CWIPC_HIP_DISTORTION_NO_PLANE"):
        assert public in cwipc.util.__all__ and hasattr(cwipc, public), public
    assert "#define CWIPC_HIP_DISTORTION_NO_PLANE 1" in header and cwipc.CWIPC_HIP_DISTORTION_NO_PLANE == 1
    # the signature: the header's parameter list against the wrapper's argument types
    decl = re.search(r"_CWIPC_UTIL_EXPORT int cwipc_hip_distortion\(([^;]*)\);", header).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    assert params == ["cwipc_pointcloud *original", "cwipc_pointcloud *degraded", "double max_distance", "const float *normals", "float radius",
                      "int max_nn", "int flags", "cwipc_hip_distortion_sums out[2]"]
    argtypes, restype = _SIGNATURES[name]
    pc_p = _SIGNATURES["cwipc_hip_icp_plane_sums"][0][0]
    assert argtypes == [pc_p, pc_p, ctypes.c_double, ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_void_p] and restype is ctypes.c_int
    # the struct: the header's fields, in order, against the ctypes fields
    body = re.search(r"typedef struct cwipc_hip_distortion_sums \{(.*?)\} cwipc_hip_distortion_sums;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for ctype, names in re.findall(r"(uint64_t|double)\s+([^;]+);", body):
        for field in names.split(","):
            m = re.fullmatch(r"\s*(\w+)(?:\[(\d+)\])?\s*", field)
            base = ctypes.c_uint64 if ctype == "uint64_t" else ctypes.c_double
            declared.append((m.group(1), base * int(m.group(2)) if m.group(2) else base))
    assert [f[0] for f in declared] == ["n_source", "n", "n_plane", "sum_d2", "max_d2", "sum_r2", "sum_rgb2", "sum_yuv2"]
    fields = cwipc.cwipc_hip_distortion_sums._fields_
    assert [(f[0], ctypes.sizeof(f[1]), f[1]._type_ if hasattr(f[1], "_length_") else f[1]) for f in fields] == \
           [(f[0], ctypes.sizeof(f[1]), f[1]._type_ if hasattr(f[1], "_length_") else f[1]) for f in declared]
    assert ctypes.sizeof(cwipc.cwipc_hip_distortion_sums) == 96
    for public in ("DirectionalDistortion", "DistortionResults", "cloud_distortion", "codec_distortion", "rate_distortion"):
        assert public in quality.__all__ and hasattr(quality, public), public


def test_bad_arguments_and_a_missing_device_fail_loudly(cwipc):
    """Every scalar argument is refused before a device is looked for (-1, out zeroed); without a GPU a good call raises."""
    import ctypes
    from conftest import make_cloud
    dll = cwipc.cwipc_util_dll_load()
    a, b = make_cloud(cwipc, A), make_cloud(cwipc, B)
    out = (cwipc.cwipc_hip_distortion_sums * 2)()
    planes = np.ascontiguousarray(NA.T)
    bad = planes.copy()
    bad[1, 2] = np.nan

    def call(original=a, degraded=b, maxd=np.inf, normals=planes, radius=0.02, max_nn=30, flags=0, result=out):
        out[0].n_source = out[1].n = 77
        return dll.cwipc_hip_distortion(original.as_cwipc_p() if original else None, degraded.as_cwipc_p() if degraded else None, maxd,
                                        None if normals is None else normals.ctypes.data, radius, max_nn, flags, ctypes.addressof(result) if result else None)
    refused = [dict(original=None), dict(degraded=None), dict(maxd=0.0), dict(maxd=-1.0), dict(maxd=float("nan")), dict(flags=2), dict(flags=-1),
               dict(normals=bad), dict(normals=None, radius=0.0), dict(normals=None, radius=float("inf")), dict(normals=None, max_nn=0),
               dict(normals=None, max_nn=129)]
    for kw in refused:
        assert call(**kw) == -1, kw
        assert bytes(out) == bytes(96 * 2), kw
    assert call(result=None) == -1
    if cwipc.cwipc_hip_device_count() == 0:
        assert call() == -1 and call(flags=1, normals=bad) == -1 and bytes(out) == bytes(96 * 2)
        with pytest.raises(cwipc.CwipcError, match="cwipc_hip_distortion"):
            cwipc.cwipc_hip_distortion(a, b)
        from cwipc_util_amd import quality
        with pytest.raises(cwipc.CwipcError):
            quality.cloud_distortion(a, b, peak=1.0)
