"""Cloud distortion on the GPU (cwipc_hip_distortion: DistortionPair of kernels_icp.hip, quality_terms.hpp; cwipc_util_amd.quality)
against the numpy model of RULE Q (tests/quality_model.py, checked on the CPU by tests/test_quality_model.py and, for the per-pair
arithmetic, tests/test_quality_terms_host.py).

Bars:
  * n_source, n, n_plane, sum_rgb2[3] and max_d2 EQUAL the model's: counts and sums of integers below 2^53 are exact in f64 in any
    order, a maximum is order-free;
  * sum_d2, sum_r2 and sum_yuv2[3] within (n + 3) * 2^-53 * sum |term| of math.fsum over the model's terms -- the worst case of any
    summation order; the terms themselves are the model's bit for bit (the host test): derived, not measured;
  * every output byte-equal over two calls.

INHERITED NORMALS.  A matched forward pair always has a normal (the note at the top of tests/test_quality_model.py: if a is matched
to b then b, in the backward pass, has at least a as a candidate), so forward n_plane == n like backward's; what the tests can and
do show is that the normal is the one inherited through the backward index and not the source's own -- random normals, equal sums."""
import ctypes
import gc
import math

import numpy as np
import pytest

from conftest import make_cloud
import codec_model as cm
import icp_model as im
import quality_model as qm

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SIZES = [0, 1, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2500]
NONE = qm.NONE


def sums_within_bound(got, terms, n, label):
    """got: the library's sums of the columns of `terms` ((n, k)); each within (n + 3) * 2^-53 * sum |term| of math.fsum."""
    want = np.array([math.fsum(terms[:, v]) for v in range(terms.shape[1])])
    bound = (n + 3) * U * np.abs(terms).sum(axis=0)
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    print("%s: n %d, largest error over bound %.3f" % (label, n, float(np.max(err / np.maximum(bound, 1e-300))) if n else 0.0))
    assert np.all(err <= bound), (label, err, bound)


def compare(got, want, label):
    """one direction: a cwipc_hip_distortion_sums against the model's one_pass"""
    t = want["terms"]
    exact = (int(got.n_source), int(got.n), int(got.n_plane), [int(v) for v in got.sum_rgb2], float(got.max_d2))
    assert exact == (want["n_source"], want["n"], want["n_plane"], qm.sums(want)["sum_rgb2"], want["max_d2"]), label
    sums_within_bound([got.sum_d2, got.sum_r2] + list(got.sum_yuv2), t[:, [2, 3, 7, 8, 9]], want["n"], label)


def check(gpu, A, B, maxd=np.inf, normals=None, plane=True, tree=False, label=""):
    """Both directions of one call against the model, and a second call byte for byte.  normals None with plane: the test passes none."""
    a, b = make_cloud(gpu, A), make_cloud(gpu, B)
    got = gpu.cwipc_hip_distortion(a, b, maxd, normals, plane=plane)
    again = gpu.cwipc_hip_distortion(a, b, maxd, normals, plane=plane)
    assert bytes(got[0]) == bytes(again[0]) and bytes(got[1]) == bytes(again[1]), label
    want = qm.distortion(A, B, maxd, normals if plane else None, tree=tree)
    for g, w, name in zip(got, want, ("forward", "backward")):
        compare(g, w, "%s %s" % (label, name))
    return got, want


def coloured(rng, xyz):
    return qm.make_cloud(xyz, rng.integers(0, 256, (len(xyz), 3)))


@pytest.fixture(scope="module")
def pools():
    """2500 original points on the surface, as many degraded ones (a permuted, jittered copy) and the original's random normals: a
    test takes the first na and nb of them.  Read only."""
    rng = np.random.default_rng(500)
    base = im.surface(rng, 2500)
    A = coloured(rng, base)
    B = coloured(rng, base[rng.permutation(2500)] + rng.normal(0, 0.004, (2500, 3)).astype(np.float32))
    normals = rng.normal(size=(2500, 3)).astype(np.float32)
    for arr in (A, B, normals):
        arr.setflags(write=False)
    return A, B, normals


# ---------------------------------------------------------------------------
# sizes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("na", SIZES)
def test_sizes(gpu, pools, na):
    """Every pair of counts: a partial four-point step, a partial wave, a partial workgroup, more than one chunk; both passes in one call."""
    A, B, normals = pools
    for nb in SIZES:
        got, want = check(gpu, A[:na], B[:nb], np.inf, normals[:na], label="%d x %d" % (na, nb))
        if na and nb:
            assert got[0].n == na and got[1].n == nb and got[0].n_plane == na and got[1].n_plane == nb
        else:
            assert got[0].n == 0 and got[1].n == 0 and (got[0].n_source, got[1].n_source) == (na, nb)
            assert bytes(got[0])[8:] == bytes(88) and bytes(got[1])[8:] == bytes(88)


def test_bounded_search(gpu, pools):
    A, B, normals = pools
    got, want = check(gpu, A, B, 0.006, normals, label="bounded")
    assert 200 < got[0].n < 2300 and 200 < got[1].n < 2300


# ---------------------------------------------------------------------------
# ties
# ---------------------------------------------------------------------------
def lattice(rng, shift):
    g = np.arange(9) * 0.25 - 1.0
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + np.asarray(shift)
    colours = rng.permutation(256 ** 3)[:len(pts)]
    return qm.make_cloud(pts, np.stack([colours & 255, (colours >> 8) & 255, colours >> 16], axis=1))


@pytest.mark.parametrize("axes", [1, 2, 3])
def test_ties_go_to_the_smallest_index(gpu, axes):
    """A 9 x 9 x 9 lattice of pitch 1/4 and the same lattice shifted by 1/8 along one, two, three axes (short binary fractions:
    the distances are equal in f64): 2-, 4-, 8-way ties in both passes, every point its own colour, so a wrong winner changes sum_rgb2."""
    rng = np.random.default_rng(600 + axes)
    A = lattice(rng, (0, 0, 0))
    B = lattice(rng, [0.125] * axes + [0.0] * (3 - axes))[rng.permutation(729)]
    assert len(np.unique(np.stack([A['r'], A['g'], A['b']], axis=1), axis=0)) == 729
    assert qm.tied_queries(B, A) >= 100 and qm.tied_queries(A, B) >= 100
    normals = rng.normal(size=(729, 3)).astype(np.float32)
    for maxd in (np.inf, 0.25):
        got, want = check(gpu, A, B, maxd, normals, label="ties %d" % axes)
        assert got[0].n == 729 and got[1].n == 729 and got[1].max_d2 == axes * 0.015625


# ---------------------------------------------------------------------------
# normals
# ---------------------------------------------------------------------------
def test_inherited_normals(gpu, pools):
    """Caller-supplied random normals on A, a bound that leaves points of either side without a match: the forward sums are the
    model's, whose pairs take A's normal at idxBA of the matched B point; negating the normals changes no bit."""
    A, B, normals = pools
    rng = np.random.default_rng(700)
    far = coloured(rng, rng.uniform(3, 4, (300, 3)))
    B = np.concatenate([B[:1200], far, B[1200:2000]])
    got, want = check(gpu, A, B, 0.008, normals, label="inherited")
    fwd, bwd = want
    assert (bwd["idx"] == NONE).sum() >= 300 and (fwd["idx"] == NONE).sum() >= 10        # B points without a normal exist; so do unmatched A points
    own = qm.one_pass(A, B, fwd["idx"], np.where(fwd["idx"] == NONE, np.inf, 0.0), normals, np.arange(len(B)) % len(A))
    assert fwd["n_plane"] >= 10 and abs(qm.sums(own)["sum_r2"] - qm.sums(fwd)["sum_r2"]) > 1e-3 * qm.sums(fwd)["sum_r2"]   # another normal would show
    assert got[0].n_plane == got[0].n and got[1].n_plane == got[1].n and got[0].n < got[0].n_source
    a, b = make_cloud(gpu, A), make_cloud(gpu, B)
    flipped = normals.copy()
    flipped[::3] = -flipped[::3]
    for other in (-normals, flipped):
        neg = gpu.cwipc_hip_distortion(a, b, 0.008, other)
        assert bytes(neg[0]) == bytes(got[0]) and bytes(neg[1]) == bytes(got[1])


def test_estimated_normals(gpu):
    """normals=None gives byte for byte what the call gives when handed cwipc_hip_estimate_normals' output."""
    rng = np.random.default_rng(710)
    base = im.surface(rng, 4000)
    A, B = coloured(rng, base), coloured(rng, base[:3000] + rng.normal(0, 0.003, (3000, 3)).astype(np.float32))
    a, b = make_cloud(gpu, A), make_cloud(gpu, B)
    for radius, max_nn in ((0.05, 30), (0.1, 12)):
        normals = gpu.cwipc_hip_estimate_normals(a, radius, max_nn)[0]
        assert np.isfinite(normals).all()
        inside = gpu.cwipc_hip_distortion(a, b, 0.05, None, radius, max_nn)
        passed = gpu.cwipc_hip_distortion(a, b, 0.05, normals)
        assert bytes(inside[0]) == bytes(passed[0]) and bytes(inside[1]) == bytes(passed[1])
        assert inside[0].n_plane == inside[0].n > 3000 and inside[0].sum_r2 > 0
    for g, w, name in zip(passed, qm.distortion(A, B, 0.05, normals, tree=True), ("forward", "backward")):
        compare(g, w, "estimated " + name)


def test_no_plane(gpu, pools):
    A, B, normals = pools
    a, b = make_cloud(gpu, A), make_cloud(gpu, B)
    plain = gpu.cwipc_hip_distortion(a, b, 0.01, normals)
    bare = check(gpu, A, B, 0.01, normals, plane=False, label="no plane")[0]
    for p, q in zip(plain, bare):
        assert q.n_plane == 0 and q.sum_r2 == 0.0 and p.n_plane == p.n > 0 and p.sum_r2 > 0
        for name, _ in gpu.cwipc_hip_distortion_sums._fields_:
            if name not in ("n_plane", "sum_r2"):
                x, y = getattr(p, name), getattr(q, name)
                assert (list(x), ) == (list(y), ) if hasattr(x, "__len__") else x == y, name
    # a non-finite caller normal is refused only without the flag
    dll = gpu.util.cwipc_util_dll_load()
    bad = np.ascontiguousarray(normals.T).copy()
    bad[2, 1234] = np.inf
    out = (gpu.cwipc_hip_distortion_sums * 2)()
    assert dll.cwipc_hip_distortion(a.as_cwipc_p(), b.as_cwipc_p(), 0.01, bad.ctypes.data, 0.02, 30, 0, ctypes.addressof(out)) == -1
    assert dll.cwipc_hip_distortion(a.as_cwipc_p(), b.as_cwipc_p(), 0.01, bad.ctypes.data, 0.0, 0, gpu.CWIPC_HIP_DISTORTION_NO_PLANE, ctypes.addressof(out)) == 0
    assert bytes(out[0]) == bytes(bare[0]) and bytes(out[1]) == bytes(bare[1])


# ---------------------------------------------------------------------------
# non-finite points, the same cloud
# ---------------------------------------------------------------------------
def test_non_finite_points(gpu, pools):
    """NaN and inf coordinates on both sides of index 256 and of index 1024, in both clouds: counted in n_source, never matched,
    never matched to; the inputs' bytes are what they were."""
    A, B, normals = pools
    A, B = A[:1500].copy(), B[:1400].copy()
    bad = [np.nan, np.inf, -np.inf]
    for k, i in enumerate((254, 255, 256, 257, 1022, 1023, 1024, 1025)):
        A[("x", "y", "z")[k % 3]][i] = bad[k % 3]
        B[("z", "x", "y")[k % 3]][i + (1 if i < 1000 else -1)] = bad[(k + 1) % 3]
    a, b = make_cloud(gpu, A), make_cloud(gpu, B)
    before = a.get_numpy_array().tobytes(), b.get_numpy_array().tobytes()
    got, want = check(gpu, A, B, np.inf, normals[:1500], label="non-finite")
    assert (got[0].n_source, got[0].n, got[1].n_source, got[1].n) == (1500, 1492, 1400, 1392)
    got, want = check(gpu, A, B, 0.01, normals[:1500], label="non-finite, bounded")
    assert got[0].n < 1492
    direct = gpu.cwipc_hip_distortion(a, b, 0.01, normals[:1500])
    assert bytes(direct[0]) == bytes(got[0]) and bytes(direct[1]) == bytes(got[1])
    assert (a.get_numpy_array().tobytes(), b.get_numpy_array().tobytes()) == before


def test_the_very_same_cloud(gpu, pools):
    from cwipc_util_amd import quality
    A, _, normals = pools
    A = A.copy()
    A['x'][[300, 1024]] = np.nan
    a = make_cloud(gpu, A)
    fwd, bwd = gpu.cwipc_hip_distortion(a, a, np.inf, normals)
    for one in (fwd, bwd):
        assert (one.n_source, one.n, one.n_plane) == (2500, 2498, 2498)
        assert bytes(one)[24:] == bytes(72)                 # every sum and the maximum: 0
    r = quality.cloud_distortion(a, a, normals=normals)
    assert r.peak > 1.0 and all(v == math.inf for v in (r.psnr_d1, r.psnr_d2, r.psnr_y, r.psnr_u, r.psnr_v))
    assert r.forward == r.backward and r.symmetric.mse_d1 == 0.0 and r.forward.hausdorff == 0.0
    compare(fwd, qm.distortion(A, A, np.inf, normals)[0], "same cloud")


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def test_refusals_launch_nothing(gpu, pools):
    """Each bad argument returns -1; the profiling counters, which see every launch of the library, stay empty, and the pool does not grow."""
    A, B, normals = pools
    a, b = make_cloud(gpu, A), make_cloud(gpu, B)
    dll = gpu.util.cwipc_util_dll_load()
    planes = np.ascontiguousarray(normals.T)
    bad = planes.copy()
    bad[0, 2499] = np.nan
    out = (gpu.cwipc_hip_distortion_sums * 2)()

    def call(original=a, degraded=b, maxd=0.01, nrm=planes, radius=0.02, max_nn=30, flags=0, result=out):
        return dll.cwipc_hip_distortion(original.as_cwipc_p() if original else None, degraded.as_cwipc_p() if degraded else None, maxd,
                                        None if nrm is None else nrm.ctypes.data, radius, max_nn, flags, ctypes.addressof(result) if result else None)
    assert call() == 0 and out[0].n > 0                       # both clouds are on the device, the pool is warm
    good = bytes(out)
    dll.cwipc_hip_synchronize()
    pool = dll.cwipc_hip_pool_bytes()
    refused = [dict(original=None), dict(degraded=None), dict(maxd=0.0), dict(maxd=-0.01), dict(maxd=float("nan")), dict(flags=2), dict(flags=3),
               dict(flags=-2), dict(nrm=bad), dict(nrm=None, radius=0.0), dict(nrm=None, radius=-1.0), dict(nrm=None, radius=float("nan")),
               dict(nrm=None, radius=float("inf")), dict(nrm=None, max_nn=0), dict(nrm=None, max_nn=129), dict(result=None)]
    with gpu.cwipc_hip_profile() as prof:
        for kw in refused:
            assert call(**kw) == -1, kw
            if "result" not in kw:
                assert bytes(out) == bytes(2 * 96), kw
    assert prof.kernels == {} and dll.cwipc_hip_pool_bytes() == pool
    with gpu.cwipc_hip_profile() as prof:                     # the counters do see a call that runs
        assert call() == 0 and bytes(out) == good
    assert "distortion_sums_partial" in prof.kernels and "distortion_sums_final" in prof.kernels and "icp_correspond" in prof.kernels
    with pytest.raises(ValueError):
        gpu.cwipc_hip_distortion(a, b, 0.01, normals[:100])
    with pytest.raises(gpu.CwipcError):
        gpu.cwipc_hip_distortion(a, b, -1.0)


# ---------------------------------------------------------------------------
# through the codec
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def codec_runs(gpu):
    """A 20 000-point coloured surface through the codec at 6, 8 and 10 bits, once: bits -> (results, bytes, packet, decoded host array)."""
    import cwipc_util_amd.codec as codec
    from cwipc_util_amd import quality
    rng = np.random.default_rng(800)
    xyz = im.surface(rng, 20000)
    pts = qm.make_cloud(xyz, np.clip(128 + 100 * np.sin(7 * xyz) + rng.normal(0, 6, xyz.shape), 0, 255))
    pc = make_cloud(gpu, pts)
    runs = {}
    for bits in (6, 8, 10):
        result, nbytes = quality.codec_distortion(pc, octree_bits=bits, jpeg_quality=85)
        enc = codec.cwipc_new_encoder(octree_bits=bits, jpeg_quality=85)
        enc.feed(pc)
        assert enc.available(True)
        packet = bytes(enc.get_bytes())
        dec = codec.cwipc_new_decoder()
        dec.feed(packet)
        assert dec.available(True)
        runs[bits] = (result, nbytes, packet, dec.get())
    return pts, pc, runs


def test_codec_distortion_is_bounded_by_the_cell(gpu, codec_runs):
    import cwipc_util_amd.codec as codec
    pts, pc, runs = codec_runs
    mn, side = cm.cube(cm.finite_points(pts))
    spacing = float(np.spacing(np.abs(qm.xyz(pts))).astype(np.float64).max())
    previous = math.inf
    for bits in (6, 8, 10):
        r, nbytes, packet, decoded = runs[bits]
        per_axis = (side / (1 << bits)) / 2 + 2 * spacing          # the bound tests/test_codec_model.py holds the codec to, per axis
        print("bits %d: %d bytes, hausdorff %.6f / %.6f, bound %.6f, psnr d1 %.2f d2 %.2f y %.2f" % (
            bits, nbytes, r.forward.hausdorff, r.backward.hausdorff, math.sqrt(3) * per_axis, r.psnr_d1, r.psnr_d2, r.psnr_y))
        assert 0 < r.forward.hausdorff <= math.sqrt(3) * per_axis and 0 < r.backward.hausdorff <= math.sqrt(3) * per_axis
        assert r.forward.n == r.forward.n_source == 20000 and r.backward.n == r.backward.n_source
        assert nbytes == len(packet) and r.backward.n_source == codec.packet_info(packet)["nleaves"] == decoded.count()
        assert r.symmetric.mse_d1 <= previous
        previous = r.symmetric.mse_d1
        assert r.forward.n_plane == 20000 and math.isfinite(r.psnr_d2) and math.isfinite(r.psnr_y)
    assert runs[10][0].psnr_d1 > runs[6][0].psnr_d1 + 12       # four octree levels: a cell 16 times smaller


def test_entropy_coded_packets_cost_less_and_lose_the_same(gpu, codec_runs):
    from cwipc_util_amd import quality
    pts, pc, runs = codec_runs
    for bits in (6, 8, 10):
        r, nbytes = quality.codec_distortion(pc, entropy=True, octree_bits=bits, jpeg_quality=85)
        assert r == runs[bits][0] and repr(r.as_dict()) == repr(runs[bits][0].as_dict())
        assert nbytes <= runs[bits][1]


def test_rate_distortion_rows(gpu, codec_runs):
    from cwipc_util_amd import quality
    pts, pc, runs = codec_runs
    settings = [dict(octree_bits=6, jpeg_quality=85), dict(octree_bits=8, jpeg_quality=85), dict(octree_bits=10, jpeg_quality=85),
                dict(octree_bits=10, jpeg_quality=85, entropy=True)]
    rows = quality.rate_distortion(pc, settings)
    assert [row["settings"] for row in rows] == settings
    for row, bits in zip(rows, (6, 8, 10, 10)):
        r, nbytes = runs[bits][0], runs[bits][1]
        assert row["bytes"] == nbytes or (row["settings"].get("entropy") and row["bytes"] <= nbytes)
        assert row["bits_per_input_point"] == 8.0 * row["bytes"] / 20000
        for key in ("psnr_d1", "psnr_d2", "psnr_y", "psnr_u", "psnr_v"):
            assert row[key] == getattr(r, key), (bits, key)
    assert quality.rate_distortion(pc, []) == []


@pytest.mark.parametrize("bits", [6, 8, 10])
def test_codec_distortion_equals_the_model(gpu, codec_runs, bits):
    """The model on get_numpy_array() of the two clouds (the only place where the decoded cloud becomes a host array)."""
    from cwipc_util_amd import quality
    pts, pc, runs = codec_runs
    r, _, _, decoded = runs[bits]
    host = decoded.get_numpy_array()
    assert pc.get_numpy_array().tobytes() == pts.tobytes()
    normals = gpu.cwipc_hip_estimate_normals(pc, 0.02, 30)[0]
    got = gpu.cwipc_hip_distortion(pc, decoded)
    want = qm.distortion(pts, host, np.inf, normals, tree=True)
    for g, w, name in zip(got, want, ("forward", "backward")):
        compare(g, w, "codec %d %s" % (bits, name))
    assert quality.DistortionResults(got[0], got[1], r.peak) == r
    box = qm.xyz(pts)
    assert r.peak == float(np.max(box.max(axis=0).astype(np.float64) - box.min(axis=0).astype(np.float64)))
    gc.collect()
