"""The numpy model of the exact filters (tests/exact_model.py) against the CPU oracle and against the recorded outputs of the
reference's own functions (tests/golden/helper_vectors.npz), on random clouds that hold the edge values the GPU tests use.
No GPU: this is what entitles tests/test_gpu_exact_filters.py to take the model as its reference.

Where model and oracle could disagree the reference source decides (src/cwipc_filters.cpp:281-418).  They did not: both
restate `tile == 0 || tile == pt.a` with the int comparison (values outside 0..255 keep nothing) and the six float32
comparisons `lo <= v && v < hi` (NaN never inside, -0.0 inside [0, ...))."""
import os

import numpy as np
import pytest

import exact_model as model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def same(a, b):
    return len(a) == len(b) and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def clouds():
    rng = np.random.default_rng(2026)
    out = [model.empty(0)]
    for n in (1, 2, 3, 5, 257, 2000):
        out.append(model.edge_cloud(rng, n, model.CROP_BOUNDS))
        out.append(model.edge_cloud(rng, n, model.CROP_BOUNDS, tiles=[0, 1, 2, 128, 255]))
    return out


def test_model_dtype_is_the_oracles(oracle):
    assert model.POINT_DTYPE == oracle.POINT_DTYPE


def test_edge_cloud_holds_the_edge_values():
    pts = model.edge_cloud(np.random.default_rng(1), 2000, model.CROP_BOUNDS)
    x = pts['x']
    assert np.isnan(x).any() and (x == np.inf).any() and (x == -np.inf).any()
    assert ((x == 0) & np.signbit(x)).any() and ((x == 0) & ~np.signbit(x)).any()
    assert ((x != 0) & (np.abs(x) < np.finfo(np.float32).tiny)).any()
    assert (np.abs(x) == np.finfo(np.float32).max).any()
    bounds = np.asarray(model.CROP_BOUNDS, dtype=np.float32)
    # every bound of every box, the ones float32 cannot hold and the negative ones included
    assert {-1.0, 1.0, 0.25, -np.inf, np.inf, model.FLT_MAX, -model.FLT_MAX} <= set(bounds.tolist())
    for v in (0.1, 1.0000000001, -1.0000000001, -16777217.0, 16777217.0, -1e-39, 1e-45, -1e-45):
        assert np.float32(v) in bounds, v
    for b in bounds:
        with np.errstate(over='ignore'):
            lo, hi = np.nextafter(b, np.float32(-np.inf)), np.nextafter(b, np.float32(np.inf))
        assert (x == b).any() and (x == hi).any() and (x == lo).any(), b


def test_tilefilter_model(oracle, clouds):
    for pts in clouds:
        for tile in (0, 1, 2, 3, 128, 255, 256, 257, 511, -1, -255, 65536 + 1):
            assert same(model.tilefilter(pts, tile), oracle.tilefilter(pts, tile)), (len(pts), tile)


def test_masked_tilefilter_model(oracle, clouds):
    for pts in clouds:
        for mask in (0, 1, 2, 3, 6, 128, 129, 255):
            assert same(model.tilefilter_masked(pts, mask), oracle.tilefilter_masked(pts, mask)), (len(pts), mask)


def test_crop_model(oracle, clouds):
    for pts in clouds:
        for name, box in model.crop_boxes():
            with np.errstate(over='ignore', invalid='ignore'):
                exp = oracle.crop(pts, box)
            got = model.crop(pts, box)
            assert same(got, exp), (len(pts), name)
            assert not (np.isnan(got['x']) | np.isnan(got['y']) | np.isnan(got['z'])).any()


def test_crop_model_known_answers():
    """The answers the reference's comparisons define, spelled out (src/cwipc_filters.cpp:348-350)."""
    pts = model.empty(8)
    pts['x'] = [-0.0, 0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, np.finfo(np.float32).max]
    inf = float('inf')
    free = [-inf, inf, -inf, inf]
    assert model.crop(pts, [0.0, inf] + free)['x'].tobytes() == pts['x'][[0, 1, 5, 7]].tobytes()     # -0.0 inside [0, ...), inf is not < inf
    assert len(model.crop(pts, [-inf, inf] + free)) == 6                                             # -inf <= -inf; NaN and +inf out
    assert len(model.crop(pts, [float('nan'), inf] + free)) == 0 and len(model.crop(pts, [1.0, -1.0] + free)) == 0
    assert len(model.crop(pts, [0.0, 0.0] + free)) == 0
    assert len(model.crop(pts, [-1e-45, 1e-45] + free)) == 3                                         # -denormal, -0.0, 0.0
    assert len(model.crop(pts, [-1e39, 1e39] + free)) == 6                                           # bounds round to infinities


def test_tilemap_model(oracle, clouds):
    rng = np.random.default_rng(3)
    maps = [bytes(range(256)), bytes([7]) * 256, bytes(range(255, -1, -1)), bytes(rng.permutation(256).astype(np.uint8)),
            bytes(rng.integers(0, 4, 256).astype(np.uint8))]
    for pts in clouds:
        for m in maps:
            assert same(model.tilemap(pts, m), oracle.tilemap(pts, m)), len(pts)


def test_colormap_model(oracle, clouds):
    for pts in clouds:
        for clear, setb in model.COLORMAP_MASKS:
            assert same(model.colormap(pts, clear, setb), oracle.colormap(pts, clear, setb)), (len(pts), hex(clear), hex(setb))


def test_join_and_tiles_used_model(oracle, clouds):
    for a in clouds:
        assert model.tiles_used(a) == oracle.tiles_used(a) if len(a) else model.tiles_used(a) == []
        for b in clouds[:6]:
            assert same(model.join(a, b), oracle.join(a, b)), (len(a), len(b))
    a, b, c = clouds[3], clouds[5], clouds[0]
    assert same(model.join(a, c, b, a), oracle.join(oracle.join(oracle.join(a, c), b), a))
    assert model.join_metadata([(50, 0.5), (40, 0.75), (45, 0.25)]) == (40, 0.25)


def test_offset_scale_model(oracle, clouds):
    with np.errstate(all='ignore'):
        for pts in clouds:
            for args in ((0.1, -1.0, 2.5, 1.7), (0.0, 0.0, 0.0, 1.0), (1e30, -1e30, 0.0, 1e30), (0.0, 0.0, 0.0, 1e-45), (float('nan'), 0.0, 0.0, 1.0)):
                got, exp = model.offset_scale(pts, *args), oracle.offset_scale(pts, *args)
                for f in ('x', 'y', 'z'):
                    nan = np.isnan(exp[f])
                    assert (np.isnan(got[f]) == nan).all() and got[f][~nan].tobytes() == exp[f][~nan].tobytes(), (len(pts), args, f)


def test_model_against_the_reference_functions_own_outputs(oracle):
    """tests/golden/helper_vectors.npz holds what the reference's cwipc_tilefilter_masked, get_tiles_used and TransformFilter
    returned: the model gives the same arrays."""
    d = np.load(os.path.join(GOLDEN, "helper_vectors.npz"))
    for i in range(6):
        pts = d["masked%d_in" % i]
        assert model.tiles_used(pts) == d["masked%d_tiles_used" % i].tolist()
        for m in (0, 1, 2, 3, 4, 8, 15, 128, 255):
            assert same(model.tilefilter_masked(pts, m), d["masked%d_mask%d_out" % (i, m)]), (i, m)
    pts = d["offsetscale_in"]
    for i in range(4):
        x, y, z, scale = d["offsetscale%d_params" % i]
        assert same(model.offset_scale(pts, x, y, z, scale), d["offsetscale%d_out" % i]), i
    pts = d["transform_in"]
    assert same(model.identity_transform(pts), d["transform_identity_out"])


def test_tile_set_rules():
    """The model's knowledge of tile sets never claims more than the points show."""
    rng = np.random.default_rng(4)
    for trial in range(50):
        alphabet = rng.integers(0, 256, rng.integers(1, 5))
        pts = model.edge_cloud(rng, 200, tiles=alphabet, finite=True)
        ts = model.TileSet(model.tiles_used(pts))
        m = bytes(rng.integers(0, 256, 256).astype(np.uint8))
        clear, setb = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32))
        assert set(model.tiles_used(model.tilemap(pts, m))) <= ts.after_tilemap(m).values
        assert set(model.tiles_used(model.colormap(pts, clear, setb))) <= ts.after_colormap(clear, setb).values
        t = int(alphabet[0])
        assert ts.tilefilter_shortcut(t, len(pts)) == ('all' if set(alphabet.tolist()) == {t} else None) or t == 0
        assert ts.tilefilter_shortcut(256, len(pts)) is None and model.TileSet(None).tilefilter_shortcut(5, 10) is None
        other = next(v for v in range(1, 256) if v not in ts.values)
        assert ts.tilefilter_shortcut(other, len(pts)) == 'none' and len(model.tilefilter(pts, other)) == 0
    u = model.TileSet.after_join([(model.TileSet([1]), 5), (model.TileSet(None), 0), (model.TileSet([2, 3]), 1)])
    assert u.values == {1, 2, 3}
    assert not model.TileSet.after_join([(model.TileSet([1]), 5), (model.TileSet(None), 2)]).known()


# ---------------------------------------------------------------------------------------------------------------------
# the per-tile outlier clouds: nothing sits on the oracle's threshold
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", model.OUTLIER_CLOUDS)
def test_pertile_outlier_clouds_have_an_empty_threshold_band(oracle, name):
    pts, order, exp, _ = model.pertile_expectation(oracle, name)
    assert 3000 <= len(pts) <= 20000 or name == "late_tile"
    assert 0 < len(exp)
    if name == "wildcard":
        # tile value 0 between the others: once for its own turn, as the wildcard, every point; and every point of tiles 1 and 2 again
        assert order == [1, 0, 2] and len(exp) > len(pts)
    if name == "tiles256":
        assert sorted(order) == list(range(256))
    if name == "late_tile":
        assert int(np.flatnonzero(pts['tile'] == 9)[0]) > 262144
    if name == "last_point_tile":
        assert order == [1, 7] and pts['tile'][-1] == 7 and (pts['tile'][:-1] == 1).all()
    if name == "small_tiles":
        counts = [int((pts['tile'] == t).sum()) for t in (20, 21, 22, 23, 24)]
        assert counts == [1, 1, 3, 5, 7] and max(counts) < model.OUTLIER_K


def test_chain_generator_reaches_the_shortcuts():
    """The random chains of tests/test_gpu_exact_filters.py, run on the model alone: of their cwipc_tilefilter steps at least a
    tenth are ones a tile set answers without a kernel (the input itself, or an empty cloud from a non-empty input), not counting
    tile 0."""
    total = {}
    for seed in range(model.CHAIN_SEEDS):
        for key, v in model.run_chain(seed).items():
            total[key] = total.get(key, 0) + v
    print(total)
    assert total["steps"] == model.CHAIN_SEEDS * model.CHAIN_STEPS
    by_set = total["shortcut_all"] - total["shortcut_all_tile0"] + total["shortcut_none"]
    assert 10 * by_set >= total["tilefilter_steps"], total
    assert total["shortcut_all"] > total["shortcut_all_tile0"] > 0 and total["shortcut_none"] > 0
