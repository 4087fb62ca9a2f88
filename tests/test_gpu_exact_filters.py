"""The exact filters of the HIP path at the sizes, alignments and values where their kernels can go wrong, against the numpy
model of tests/exact_model.py (which tests/test_exact_model.py validates against the oracle on the CPU).

Their bar is bit-exact bytes, count and order: every comparison is tobytes() equality of the whole
result, and every result's timestamp and cellsize are checked.  What each test aims at is a path of csrc/kernels_basic.hip or
csrc/filters.cpp: the LDS staging of the scatter kernel (head / 16-byte quads / tail), the three exits of compact(), the
workgroup sums of the big-cloud scatter, results whose plane spacing is not their own size, the ragged lanes of the maps,
both forms of join_copy, the crop predicate on non-finite values, the tile sets, the per-tile outlier loop, the affine kernel
and the camera assignment on edge inputs.
"""
import fractions
import itertools

import numpy as np
import pytest

import exact_model as model
from conftest import make_cloud

pytestmark = pytest.mark.gpu

SMALL_CLOUD = 262144          # csrc/kernels_basic.hip: up to here a workgroup compacts 1024 points, beyond 4096 in four steps


def same(a, b):
    return len(a) == len(b) and a.tobytes() == b.tobytes()


def check(out, exp, ts, cs, what=None):
    got = out.get_numpy_array()
    assert len(got) == len(exp), (what, len(got), len(exp))
    if got.tobytes() != exp.tobytes():
        bad = np.flatnonzero((got.view(np.uint8).reshape(-1, 16) != exp.view(np.uint8).reshape(-1, 16)).any(axis=1))
        raise AssertionError((what, "differing points", len(bad), bad[:8].tolist()))
    assert out.count() == len(exp), what
    assert out.timestamp() == ts and out.cellsize() == cs, (what, out.timestamp(), out.cellsize())


def planes(gpu, pc):
    return gpu.cwipc_hip_device_planes(pc)[:4]


def spacing(gpu, pc):
    """Points between the starts of the x and the y plane: the plane spacing (`stride`) of the device cloud."""
    p = gpu.cwipc_hip_device_planes(pc)
    return (p[1] - p[0]) // 4


def round_up(n):
    return max((n + 255) // 256, 1) * 256


def indexed_cloud(rng, n):
    """z is the index (stability), colours random; x, y and the tile are the test's to set."""
    pts = model.empty(n)
    pts['z'] = np.arange(n, dtype=np.float32)
    pts['r'], pts['g'], pts['b'] = rng.integers(0, 256, n), rng.integers(0, 256, n), rng.integers(0, 256, n)
    return pts


def through_the_three_filters(gpu, base, keep, what):
    """The points of `keep` through cwipc_tilefilter, the masked filter and a crop that encode the same set."""
    pts = base.copy()
    n = len(pts)
    pts['tile'] = np.where(keep, 1, 2)
    pts['x'] = keep.astype(np.float32)
    pc = make_cloud(gpu, pts, 0.25, 99)
    exp = pts[keep]
    outs = {"tilefilter": gpu.cwipc_tilefilter(pc, 1), "masked": gpu.cwipc_tilefilter_masked(pc, 1),
            "crop": gpu.cwipc_crop(pc, [0.5, 1.5, -1.0, 1.0, -1.0, float(n + 1)])}
    for name, out in outs.items():
        check(out, exp, 99, pc.cellsize(), (what, name))
        if keep.all():
            assert planes(gpu, out) == planes(gpu, pc), (what, name)       # every point kept: the input's planes, nothing copied
        elif len(exp):
            assert planes(gpu, out)[0] != planes(gpu, pc)[0], (what, name)
    return pc, outs


# ---------------------------------------------------------------------------------------------------------------------
# scatter kernel: chosen kept sets
# ---------------------------------------------------------------------------------------------------------------------
SCATTER_SIZES = [1025, 4099, 262145 + 4096 + 3]
WAVE_COUNTS = (1, 2, 3, 4, 5, 7, 8, 255, 256)
MORE_WAVE_COUNTS = (6, 10)     # a three-point tail behind a three-point head, without and with a quad between them


def wave_classes(keep):
    """Per wave step (256 consecutive points): where its run of the output starts modulo four, how many points it keeps, and the
    head / quads / tail the staged copy splits them into (compact_scatter_kernel)."""
    n = len(keep)
    chunks = (n + 255) // 256
    padded = np.zeros(chunks * 256, dtype=bool)
    padded[:n] = keep
    total = padded.reshape(chunks, 256).sum(axis=1)
    pos0 = np.concatenate([[0], np.cumsum(total)[:-1]])
    head = np.minimum(total, (4 - (pos0 & 3)) & 3)
    quads = (total - head) // 4
    tail = total - head - 4 * quads
    return set(zip((pos0 & 3).tolist(), total.tolist())), set(zip((pos0 & 3).tolist(), head.tolist(), (quads > 0).tolist(), tail.tolist()))


def keep_per_wave(n, c, first):
    """Exactly c points of every wave step, the first at index `first` of the step (as far as c leaves room), the others spread over
    the rest; step 0 keeps `first` points only, so that the runs behind it start at every alignment."""
    keep = np.zeros(n, dtype=bool)
    lo = min(first, 256 - c)
    inside = lo + (np.arange(c) * (256 - lo)) // c
    for chunk in range((n + 255) // 256):
        at = chunk * 256 + (np.array([5, 100, 255][:first], dtype=np.int64) if chunk == 0 else inside)
        keep[at[at < n]] = True
    return keep


@pytest.mark.parametrize("n", SCATTER_SIZES)
def test_scatter_single_points_and_all_but_one(gpu, n):
    """One kept point, and all points but one (kept == n - 1: not the input's planes), in the first, a middle and the last lane of the
    first, a middle and the last workgroup."""
    base = indexed_cloud(np.random.default_rng(n), n)
    tile = 1024 if n <= SMALL_CLOUD else 4096
    groups = (n + tile - 1) // tile
    where = set()
    for g in (0, groups // 2, groups - 1):
        lo, hi = g * tile, min((g + 1) * tile, n)
        where |= {lo, min(lo + tile // 2 + 1, hi - 1), hi - 1, max(hi - 4, lo)}
    for i in sorted(where):
        keep = np.zeros(n, dtype=bool)
        keep[i] = True
        through_the_three_filters(gpu, base, keep, ("only", i))
        through_the_three_filters(gpu, base, ~keep, ("all but", i))


@pytest.mark.parametrize("n", SCATTER_SIZES)
def test_scatter_every_head_quad_tail_class(gpu, n):
    """Exactly c kept points in every wave step for c = 1, 2, 3, 4, 5, 7, 8, 255, 256, the output run of a wave starting at every
    alignment: every (start modulo four, kept points) pair must occur, which the test checks of its own patterns."""
    base = indexed_cloud(np.random.default_rng(n + 1), n)
    pairs, splits = set(), set()
    for c in WAVE_COUNTS + MORE_WAVE_COUNTS:
        for first in range(4):
            keep = keep_per_wave(n, c, first)
            p, s = wave_classes(keep)
            pairs |= p
            splits |= s
            through_the_three_filters(gpu, base, keep, ("per wave", c, first))
    missing = [(a, c) for c in WAVE_COUNTS for a in range(4) if (a, c) not in pairs]
    assert not missing, missing
    print("n = %d: (start & 3, head, has quads, tail) classes reached: %s" % (n, sorted(splits)))
    for a in range(4):   # the head that aligns the run, with and without quads behind it, and every length of tail
        reached = {s[1:] for s in splits if s[0] == a}
        assert {h for h, _, _ in reached} >= set(range(1, ((4 - a) & 3) + 1)), (a, reached)
        assert {q for _, q, _ in reached} == {False, True} and {t for _, _, t in reached} == {0, 1, 2, 3}, (a, reached)


def test_scatter_one_step_of_the_four_step_tile(gpu):
    """Big flow: kept points in step s of every workgroup's four steps only."""
    n = SCATTER_SIZES[-1]
    base = indexed_cloud(np.random.default_rng(5), n)
    for s in range(4):
        through_the_three_filters(gpu, base, (np.arange(n) % 4096) // 1024 == s, ("step", s))


@pytest.mark.parametrize("n", SCATTER_SIZES)
def test_scatter_alternating_runs(gpu, n):
    base = indexed_cloud(np.random.default_rng(n + 2), n)
    for run in (1, 63, 64, 65, 1024):
        keep = (np.arange(n) // run) % 2 == 0
        through_the_three_filters(gpu, base, keep, ("runs", run))
        through_the_three_filters(gpu, base, ~keep, ("runs, the others", run))


# ---------------------------------------------------------------------------------------------------------------------
# the exits of compact(), and their results as inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4096, 300000])
def test_compact_exits_and_their_results_as_inputs(gpu, n):
    """kept == n hands the input's planes on; kept * 16 >= n keeps the input's plane spacing with a smaller count; below that the
    result is copied to planes of its own size.  Both sizes are multiples of 16, so kept = n // 16 - 1, n // 16, n // 16 + 1
    satisfy kept * 16 < n, == n and > n (4096: 255, 256, 257; 300000: 18749, 18750, 18751).  Every result then feeds a join with
    itself, a tilemap, a second crop and the download."""
    assert n % 16 == 0
    rng = np.random.default_rng(n)
    base = indexed_cloud(rng, n)
    base['y'] = rng.random(n).astype(np.float32)
    reverse = bytes(range(255, -1, -1))
    for kept in (0, 1, n // 16 - 1, n // 16, n // 16 + 1, n - 1, n):
        keep = np.zeros(n, dtype=bool)
        keep[rng.permutation(n)[:kept]] = True
        pc, outs = through_the_three_filters(gpu, base, keep, ("kept", kept))
        exp = model.crop(model.tilefilter(base_with(base, keep), 1), [0.5, 1.5, -1, 1, -1, n + 1])
        assert len(exp) == kept
        for name, out in outs.items():
            what = (n, kept, name)
            if kept == n:
                assert planes(gpu, out) == planes(gpu, pc), what
            else:
                assert planes(gpu, out)[0] != planes(gpu, pc)[0], what
                assert spacing(gpu, out) == (round_up(n) if kept * 16 >= n else round_up(kept)), (what, spacing(gpu, out))
            cs = pc.cellsize()
            check(gpu.cwipc_join(out, out), model.join(exp, exp), 99, cs, (what, "join"))
            mapped = gpu.cwipc_tilemap(out, reverse)
            check(mapped, model.tilemap(exp, reverse), 99, cs, (what, "tilemap"))
            assert planes(gpu, mapped)[:3] == planes(gpu, out)[:3], what
            box = [-1.0, 2.0, 0.25, 0.75, float(n // 4), float(3 * (n // 4))]
            check(gpu.cwipc_crop(out, box), model.crop(exp, box), 99, cs, (what, "crop"))
            check(gpu.cwipc_tilefilter_masked(out, 1), exp, 99, cs, (what, "keep all of it"))
            check(out, exp, 99, cs, (what, "download"))


def base_with(base, keep):
    pts = base.copy()
    pts['tile'] = np.where(keep, 1, 2)
    pts['x'] = keep.astype(np.float32)
    return pts


def test_remove_outliers_and_downsample_take_a_strided_result(gpu):
    """A compaction result whose plane spacing is the input's feeds the outlier filter and the voxel downsample: the same clouds as
    from a fresh upload of the same points.  This is a check of layout invariance and nothing more: it compares the library with
    itself, so an error that both layouts share goes unseen here (tests/test_gpu_parity.py holds both filters to the oracle)."""
    rng = np.random.default_rng(8)
    n = 20000
    pts = model.empty(n)
    pts['x'], pts['y'] = rng.random(n), rng.random(n)
    pts['z'] = 0.05 * np.sin(pts['x'] * 5)
    pts['tile'] = np.where(rng.random(n) < 0.3, 1, 2)
    strided = gpu.cwipc_tilefilter(make_cloud(gpu, pts, 0.0, 3), 1)
    fresh = make_cloud(gpu, model.tilefilter(pts, 1), 0.0, 3)
    assert spacing(gpu, strided) == round_up(n) != spacing(gpu, fresh)
    assert same(gpu.cwipc_remove_outliers(strided, 8, 1.0, False).get_numpy_array(), gpu.cwipc_remove_outliers(fresh, 8, 1.0, False).get_numpy_array())
    for cell in (0.02, -0.02):
        assert same(gpu.cwipc_downsample(strided, cell).get_numpy_array(), gpu.cwipc_downsample(fresh, cell).get_numpy_array()), cell


# ---------------------------------------------------------------------------------------------------------------------
# the workgroup sums of the big-cloud scatter beyond 256 workgroups
# ---------------------------------------------------------------------------------------------------------------------
def test_scatter_sums_beyond_256_workgroups(gpu):
    """1,048,576 + 3 * 4096 + 5 points are 260 workgroups: the loop in which a workgroup adds up the counts in front of it runs twice.
    A random predicate, and one that keeps points in workgroups 0, 255, 256, 257 and the last only."""
    n = 1048576 + 4096 * 3 + 5
    rng = np.random.default_rng(260)
    pts = indexed_cloud(rng, n)
    pts['x'] = rng.random(n).astype(np.float32)
    pts['tile'] = np.where(rng.random(n) < 0.5, 1, 2)
    groups = (n + 4095) // 4096
    assert groups == 260
    sparse = np.zeros(n, dtype=bool)
    for g in (0, 255, 256, 257, groups - 1):
        at = g * 4096 + np.array([0, 1, 777, 2048, 4095])
        sparse[at[at < n]] = True
    pts['tile'][sparse] = 4
    pts['tile'][~sparse & (pts['tile'] == 4)] = 2
    pc = make_cloud(gpu, pts, 0.5, 11)
    check(gpu.cwipc_tilefilter(pc, 1), model.tilefilter(pts, 1), 11, pc.cellsize(), "random half")
    check(gpu.cwipc_tilefilter_masked(pc, 3), model.tilefilter_masked(pts, 3), 11, pc.cellsize(), "all but the sparse ones")
    check(gpu.cwipc_tilefilter(pc, 4), pts[sparse], 11, pc.cellsize(), "sparse")
    check(gpu.cwipc_tilefilter_masked(pc, 4), pts[sparse], 11, pc.cellsize(), "sparse, masked")
    box = [0.25, 0.75, -1.0, 1.0, 4096.0 * 200, float(n)]
    check(gpu.cwipc_crop(pc, box), model.crop(pts, box), 11, pc.cellsize(), "crop")


# ---------------------------------------------------------------------------------------------------------------------
# map kernels at ragged sizes, on fresh uploads and on strided results
# ---------------------------------------------------------------------------------------------------------------------
MAP_SIZES = [1, 2, 3, 4, 5, 6, 7, 255, 256, 257, 1023, 1025]


def fresh_and_strided(gpu, pts, ts=21, cs=0.125):
    """The same points as an upload and as the result of a compaction that keeps every second point of a cloud twice the size
    (kept * 16 >= n: the result keeps the spacing of the wider input)."""
    n = len(pts)
    assert np.isfinite(pts['x']).all() and np.isfinite(pts['z']).all()
    wide = model.empty(2 * n)
    wide[0::2] = pts
    wide[1::2] = pts[::-1]
    wide['y'][1::2] = 5.0
    wide['y'][0::2] = 0.0
    narrow = wide[0::2].copy()
    strided = gpu.cwipc_crop(make_cloud(gpu, wide, cs, ts), [-np.inf, np.inf, -1.0, 1.0, -np.inf, np.inf])
    return narrow, [("fresh", make_cloud(gpu, narrow, cs, ts)), ("strided", strided)]


@pytest.mark.parametrize("n", MAP_SIZES)
def test_maps_at_ragged_sizes(gpu, oracle, n):
    rng = np.random.default_rng(n)
    pts = model.edge_cloud(rng, n, special=0.3, finite=True)
    pts['tile'] = (np.arange(n) * 37 + n) % 256
    pts, sources = fresh_and_strided(gpu, pts)
    assert n < 256 or len(model.tiles_used(pts)) == 256
    maps = {"identity": bytes(range(256)), "constant": bytes([9]) * 256, "reversal": bytes(range(255, -1, -1)),
            "permutation": bytes(rng.permutation(256).astype(np.uint8))}
    lut = np.random.default_rng(77).random((256, 3))
    some = np.ones(256, dtype=np.uint8)
    some[::3] = 0
    for kind, pc in sources:
        assert kind == "fresh" or (spacing(gpu, pc) == round_up(2 * n) and pc.count() == n)
        check(pc, pts, 21, 0.125, (kind, "source"))
        for name, m in maps.items():
            out = gpu.cwipc_tilemap(pc, m)
            check(out, model.tilemap(pts, m), 21, 0.125, (kind, "tilemap", name))
            assert planes(gpu, out)[:3] == planes(gpu, pc)[:3] and planes(gpu, out)[3] != planes(gpu, pc)[3]
        for clear, setb in model.COLORMAP_MASKS:
            out = gpu.cwipc_colormap(pc, clear, setb)
            check(out, model.colormap(pts, clear, setb), 21, 0.125, (kind, "colormap", hex(clear), hex(setb)))
            assert planes(gpu, out)[:3] == planes(gpu, pc)[:3] and planes(gpu, out)[3] != planes(gpu, pc)[3]
        for weight, valid in ((0.0, np.ones(256, dtype=np.uint8)), (1.0, np.ones(256, dtype=np.uint8)), (0.5, np.ones(256, dtype=np.uint8)), (0.5, some)):
            out = gpu.cwipc_hip_colorize(pc, weight, lut, valid)
            check(out, oracle.colorize(pts, weight, lut, valid), 21, 0.125, (kind, "colorize", weight, int(valid.sum())))
            assert planes(gpu, out)[:3] == planes(gpu, pc)[:3] and planes(gpu, out)[3] != planes(gpu, pc)[3]
        assert gpu.get_tiles_used(pc) == model.tiles_used(pts)


# ---------------------------------------------------------------------------------------------------------------------
# join
# ---------------------------------------------------------------------------------------------------------------------
JOIN_SIZES = (0, 1, 2, 3, 4, 5, 255, 256, 257, 1000)


@pytest.fixture(scope="module")
def join_parts(gpu):
    rng = np.random.default_rng(33)
    parts = {}
    for i, n in enumerate(JOIN_SIZES):
        pts = model.edge_cloud(rng, n, special=0.3)
        ts, cs = 500 - 7 * i + (i % 3) * 40, [0.5, 0.25, 1.0, 0.125][i % 4]
        parts[n] = (pts, ts, cs, make_cloud(gpu, pts, cs, ts))
    return parts


def check_join(gpu, parts, what):
    exp = model.join(*[p[0] for p in parts])
    ts, cs = model.join_metadata([(p[1], p[2]) for p in parts])
    fold = parts[0][3]
    for p in parts[1:]:
        fold = gpu.cwipc_join(fold, p[3])
    check(fold, exp, ts, cs, (what, "folded"))
    check(gpu.cwipc_join_multi([p[3] for p in parts]), exp, ts, cs, (what, "n-ary"))


def test_join_every_pair_of_sizes(gpu, join_parts):
    for a in JOIN_SIZES:
        for b in JOIN_SIZES:
            check_join(gpu, [join_parts[a], join_parts[b]], (a, b))


def test_join_sampled_triples_of_sizes(gpu, join_parts):
    triples = list(itertools.product(JOIN_SIZES, repeat=3))
    for i in np.random.default_rng(34).permutation(len(triples))[:200]:
        check_join(gpu, [join_parts[n] for n in triples[i]], triples[i])


def test_join_special_cases(gpu, join_parts):
    pts, ts, cs, pc = join_parts[257]
    check(gpu.cwipc_join(pc, pc), model.join(pts, pts), ts, cs, "a cloud with itself")
    check(gpu.cwipc_join_multi([pc, pc, pc]), model.join(pts, pts, pts), ts, cs, "a cloud with itself, three times")
    recoloured = gpu.cwipc_colormap(pc, 0x00ffffff, 0x00102030)
    assert planes(gpu, recoloured)[:3] == planes(gpu, pc)[:3]
    check(gpu.cwipc_join(recoloured, pc), model.join(model.colormap(pts, 0x00ffffff, 0x00102030), pts), ts, cs, "parts that share coordinate planes")
    check(gpu.cwipc_join(pc, recoloured), model.join(pts, model.colormap(pts, 0x00ffffff, 0x00102030)), ts, cs, "parts that share coordinate planes")
    # 17 parts, an empty one first, in the middle and last
    for hole in (0, 8, 16):
        sizes = [(1, 2, 3, 5, 255, 257, 1000, 4)[i % 8] for i in range(17)]
        sizes[hole] = 0
        check_join(gpu, [join_parts[n] for n in sizes], ("17 parts", hole))
    check_join(gpu, [join_parts[0]] * 17, "17 empty parts")
    check_join(gpu, [join_parts[0]] * 8 + [join_parts[3]] + [join_parts[0]] * 8, "all points in one part of 17")


@pytest.mark.parametrize("front", [1, 2, 3, 4, 5])
def test_join_takes_strided_results_at_every_offset(gpu, join_parts, front):
    """A compaction result that keeps its input's plane spacing behind `front` points (destination offset modulo four 1, 2, 3:
    the four-bytes-per-lane copy; 0: the 16-byte one with its tail) and in front of them."""
    rng = np.random.default_rng(front)
    for n in (6, 257, 1023):
        pts = model.edge_cloud(rng, n, special=0.3, finite=True)   # (the crop that makes the strided cloud keeps finite points only)
        pts, sources = fresh_and_strided(gpu, pts, 300, 0.75)
        strided = (pts, 300, 0.75, sources[1][1])
        assert spacing(gpu, strided[3]) == round_up(2 * n)
        check_join(gpu, [join_parts[front], strided], (front, n, "behind"))
        check_join(gpu, [strided, join_parts[front]], (front, n, "in front"))
        check_join(gpu, [join_parts[front], strided, strided, join_parts[2]], (front, n, "twice"))


# ---------------------------------------------------------------------------------------------------------------------
# the crop predicate on non-finite values, signed zeros, denormals and bounds float32 cannot hold
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flow", ["small", "big"])
def test_crop_on_edge_values(gpu, flow):
    """The count kernel and the scatter kernel evaluate the box along two code paths; both have to give the reference's
    `lo <= v && v < hi` on NaN, infinities, -0.0, denormals, the bounds and their neighbours -- or the ranks are wrong."""
    rng = np.random.default_rng(71)
    pts = model.edge_cloud(rng, 2001, model.CROP_BOUNDS)
    if flow == "big":
        reps = SMALL_CLOUD // len(pts) + 1
        pts = np.tile(pts, reps)
        pts['r'], pts['g'] = rng.integers(0, 256, len(pts)), rng.integers(0, 256, len(pts))
        assert SMALL_CLOUD < len(pts) < SMALL_CLOUD + 4096
    pc = make_cloud(gpu, pts, 0.5, 13)
    kept = {}
    for name, box in model.crop_boxes():
        exp = model.crop(pts, box)
        kept[name] = len(exp)
        check(gpu.cwipc_crop(pc, box), exp, 13, pc.cellsize(), name)
    assert kept["inverted"] == kept["all NaN"] == kept["degenerate zero"] == 0 and kept["ordinary"] > 0
    assert 0 < kept["everything finite"] < len(pts) and kept["zero and up"] > 0 and kept["denormal bounds"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# model-based random chains
# ---------------------------------------------------------------------------------------------------------------------
class DeviceBackend:
    def __init__(self, gpu):
        self.gpu = gpu
        self.shortcuts = 0

    def upload(self, pts, ts, cs):
        return make_cloud(self.gpu, pts, cs, ts)

    def census(self, cloud, used):
        assert self.gpu.get_tiles_used(cloud.dev) == used

    def apply(self, op, args, ins, new, shortcut):
        g, dev = self.gpu, ins[0].dev
        if op == "tilefilter":
            out = g.cwipc_tilefilter(dev, args[0])
        elif op == "masked":
            out = g.cwipc_tilefilter_masked(dev, args[0])
        elif op == "crop":
            out = g.cwipc_crop(dev, args[0])
        elif op == "tilemap":
            out = g.cwipc_tilemap(dev, args[0])
        elif op == "colormap":
            out = g.cwipc_colormap(dev, *args)
        elif op == "join":
            out = g.cwipc_join(ins[0].dev, ins[1].dev)
        else:
            out = g.cwipc_transform(dev, np.eye(4))
        what = (op, args if op != "tilemap" else "map", [len(c.pts) for c in ins])
        got = out.get_numpy_array()
        assert same(got, new.pts), (what, len(got), len(new.pts))
        assert out.timestamp() == new.ts, what
        if len(new.pts) or op != "masked":   # (the reference's empty masked result is a new cloud without a cellsize)
            assert out.cellsize() == new.cs, what
        # what the tile set allows to answer without a kernel is answered that way: the input itself, or nothing
        if shortcut == 'all':
            assert planes(g, out) == planes(g, dev), what
            self.shortcuts += 1
        elif shortcut == 'none':
            assert out.count() == 0 and len(ins[0].pts) > 0, what
            self.shortcuts += 1
        return out


@pytest.mark.parametrize("block", range(model.CHAIN_SEEDS // model.CHAIN_BIG_EVERY))
def test_model_based_random_chains(gpu, block):
    """200 seeds in blocks of 20 (the first of a block draws a cloud just above 262,144 points): after every one of a chain's eight
    operations the device cloud's bytes, timestamp and cellsize are the model's."""
    backend = DeviceBackend(gpu)
    total = {}
    for seed in range(block * model.CHAIN_BIG_EVERY, (block + 1) * model.CHAIN_BIG_EVERY):
        for key, v in model.run_chain(seed, backend).items():
            total[key] = total.get(key, 0) + v
    assert backend.shortcuts == total["shortcut_all"] + total["shortcut_none"]
    print("chains %d-%d: %s" % (block * model.CHAIN_BIG_EVERY, (block + 1) * model.CHAIN_BIG_EVERY - 1, total))


# ---------------------------------------------------------------------------------------------------------------------
# per-tile outlier removal
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", model.OUTLIER_CLOUDS)
def test_remove_outliers_pertile_exactly(gpu, oracle, name):
    """1. Within the library: the per-tile result is, byte for byte, the join over the tiles in first-appearance order of
    remove_outliers(tilefilter(pc, t)) -- tile value 0 acting as the wildcard it is in the reference's loop
    (src/cwipc_filters.cpp:251-256).  2. Against the oracle by the rule of check_sor: per tile d_i bit for bit, the mask the
    library's own threshold applied; the clouds are chosen so that no d_i lies within 1e-6 of the oracle's threshold in any
    tile (tests/test_exact_model.py checks that on the CPU), so the oracle's cloud is the only right one: plain byte equality."""
    k, mul = model.OUTLIER_K, model.OUTLIER_MUL
    pts, order, exp, d_oracle = model.pertile_expectation(oracle, name)
    pc = make_cloud(gpu, pts, 0.125, 61)
    out = gpu.cwipc_remove_outliers(pc, k, mul, True)
    got = out.get_numpy_array()
    assert out.timestamp() == 61 and out.cellsize() == pc.cellsize()
    pieces = []
    for t, d_exp in zip(order, d_oracle):
        sub = gpu.cwipc_tilefilter(pc, t)
        sub_pts = model.tilefilter(pts, t)
        d_got, thr_got = gpu.cwipc_hip_knn_mean_dist(sub, k, mul)
        assert (d_got == d_exp).all(), (name, t, np.flatnonzero(d_got != d_exp)[:5])
        piece = gpu.cwipc_remove_outliers(sub, k, mul, False)
        assert same(piece.get_numpy_array(), sub_pts[~(d_got.astype(np.float64) > thr_got)]), (name, t)
        pieces.append(piece)
    composed = pieces[0] if len(pieces) == 1 else gpu.cwipc_join_multi(pieces)
    assert same(got, composed.get_numpy_array()), (name, len(got), composed.count())
    assert same(got, exp), (name, len(got), len(exp))
    if name == "wildcard":
        # every point once for the wildcard's turn and once more for its own tile's, less what each pass removed
        own = [len(oracle.remove_outliers(model.tilefilter(pts, t), k, mul, False)) for t in (1, 2)]
        assert order == [1, 0, 2] and len(got) == own[0] + len(oracle.remove_outliers(pts, k, mul, False)) + own[1] > len(pts)


# ---------------------------------------------------------------------------------------------------------------------
# the affine kernel on edge inputs
# ---------------------------------------------------------------------------------------------------------------------
def differences_but_for_nan_payloads(got, exp, src):
    """Byte equality of the clouds, except that a NaN coordinate equals any NaN: the reference computes them in numpy on the
    CPU, whose NaN payloads and signs are those of its instruction set -- nothing a port can or should reproduce.  Returns
    the first differences (empty: none)."""
    if len(got) != len(exp) or any((got[f] != exp[f]).any() for f in ('r', 'g', 'b', 'tile')):
        return ["length or colour / tile bytes"]
    diff = []
    for f in ('x', 'y', 'z'):
        nan = np.isnan(exp[f])
        bad = (np.isnan(got[f]) != nan) | (~nan & (got[f].view(np.uint32) != exp[f].view(np.uint32)))
        diff += [(f, int(i), tuple(float(src[c][i]) for c in ('x', 'y', 'z')), float(got[f][i]), float(exp[f][i])) for i in np.flatnonzero(bad)[:4]]
    return diff


@pytest.mark.parametrize("n", [1, 3, 257, 10000])
def test_affine_on_edge_inputs(gpu, oracle, n):
    rng = np.random.default_rng(n)
    pts = model.edge_cloud(rng, n, bounds=(3e38, -3e38, 1.0), special=0.5)
    pc = make_cloud(gpu, pts, 0.5, 17)
    ang = 0.7
    rot = np.eye(4)
    rot[:3, :3] = [[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]
    rot[:3, 3] = [0.25, -1.5, 3.0]
    broken = rot.copy()
    broken[1, 2] = np.nan
    matrices = {"identity": np.eye(4), "rotation": rot, "scale 1e30": np.diag([1e30, 1e30, 1e30, 1.0]),
                "scale 1e-45": np.diag([1e-45, 1e-45, 1e-45, 1.0]), "NaN entry": broken}
    with np.errstate(all='ignore'):
        for name, m in matrices.items():
            out = gpu.cwipc_transform(pc, m)
            diff = differences_but_for_nan_payloads(out.get_numpy_array(), oracle.transform(pts, m), pts)
            assert not diff, (n, name, diff)
            assert out.timestamp() == 17 and out.cellsize() == pc.cellsize() and planes(gpu, out)[3] == planes(gpu, pc)[3]
        for args in ((0.1, -1.0, 2.5, 1.7), (0.0, 0.0, 0.0, 1.0), (1e30, -1e30, 0.0, 1e30), (0.0, 0.0, 0.0, 1e-45), (float('nan'), 0.0, float('inf'), 1.0)):
            out = gpu.cwipc_offset_scale(pc, *args)
            got = out.get_numpy_array()
            diff = differences_but_for_nan_payloads(got, model.offset_scale(pts, *args), pts) + differences_but_for_nan_payloads(got, oracle.offset_scale(pts, *args), pts)
            assert not diff, (n, args, diff)
            assert out.timestamp() == 17 and out.cellsize() == float(np.float32(np.float64(pc.cellsize()) * args[3]))


# ---------------------------------------------------------------------------------------------------------------------
# simulated cameras, hard assignment
# ---------------------------------------------------------------------------------------------------------------------
def camera_vectors(ncam):
    cams = np.zeros((ncam, 3), dtype=float)
    for c in range(ncam):
        cams[c, 0], cams[c, 2] = np.cos(2 * np.pi * c / ncam), np.sin(2 * np.pi * c / ncam)
    return cams


def fma(a, b, c):
    """a * b + c rounded once (exact rational arithmetic; float() of a Fraction rounds to nearest even)."""
    return float(fractions.Fraction(a) * fractions.Fraction(b) + fractions.Fraction(c))


def assigned_tiles(pts, centroid, cams):
    """reference python/cwipc/filters/simulatecams.py:47-58, 70: position minus centroid in float32, numpy.dot of that float32
    vector with a float64 camera vector -- fl(x * cx), the y term 0, then one fused multiply-add for z * cz -- and the last
    index of a stable ascending sort: of equal dot products the higher camera index."""
    vx = (pts['x'] - np.float32(centroid[0])).astype(np.float32)
    vz = (pts['z'] - np.float32(centroid[2])).astype(np.float32)
    tiles = np.zeros(len(pts), dtype=np.uint8)
    for i in range(len(pts)):
        dots = np.array([fma(float(vz[i]), float(cz), float(vx[i]) * float(cx)) for cx, _, cz in cams])
        tiles[i] = 1 << int(np.argsort(dots, kind="stable")[-1])
    return tiles


def check_cameras(gpu, pts, centroid, ncam, what):
    cams = camera_vectors(ncam)
    pc = make_cloud(gpu, pts, 0.125, 77)
    out = gpu.cwipc_hip_simulatecams(pc, cams, np.asarray(centroid, dtype=np.float32))
    exp = pts.copy()
    exp['tile'] = assigned_tiles(pts, centroid, cams)
    check(out, exp, 77, 0.125, what)
    assert planes(gpu, out)[:3] == planes(gpu, pc)[:3]
    return exp['tile']


@pytest.mark.parametrize("ncam", [1, 2, 7, 8])
def test_simulatecams_ties_and_random_points(gpu, ncam):
    rng = np.random.default_rng(ncam)
    # every point on the centroid's x and z: every dot product is 0, the highest camera index wins
    pts = model.edge_cloud(rng, 300, special=0.0)
    pts['x'], pts['z'] = np.float32(0.3), np.float32(-1.7)
    tiles = check_cameras(gpu, pts, (np.float32(0.3), 0.0, np.float32(-1.7)), ncam, ("on the centroid", ncam))
    assert (tiles == 1 << (ncam - 1)).all()
    pts = model.edge_cloud(rng, 600, special=0.1, finite=True)
    tiles = check_cameras(gpu, pts, (np.float32(0.1), 0.0, np.float32(-0.2)), ncam, ("random", ncam))
    assert len(np.unique(tiles)) == ncam


def test_simulatecams_points_on_the_bisectors(gpu):
    """Four cameras, points at equal angles from two of them (|x| == |z| around the centroid)."""
    rng = np.random.default_rng(4)
    t = np.concatenate([2.0 ** np.arange(-20, 4), rng.random(76) * 3]).astype(np.float32)
    pts = model.empty(4 * len(t))
    pts['x'] = np.concatenate([t, -t, -t, t])
    pts['z'] = np.concatenate([t, t, -t, -t])
    pts['y'] = rng.random(len(pts))
    pts['tile'] = 200
    tiles = check_cameras(gpu, pts, (0.0, 0.0, 0.0), 4, "bisectors")
    assert set(np.unique(tiles)) <= {1, 2, 4, 8} and len(np.unique(tiles)) >= 2
