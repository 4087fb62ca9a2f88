"""A plain numpy model of the exact per-point filters (TEST INFRASTRUCTURE).

Restates, on the structured point dtype, what the reference's loops do (src/cwipc_filters.cpp:281-418,
python/cwipc/registration/util.py:98-112 and 285-293, python/cwipc/filters/transform.py:38-52).  No C, no oracle library:
tests/test_exact_model.py checks it against the oracle and the recorded outputs of the reference's own functions, which is
what entitles tests/test_gpu_exact_filters.py to compare the HIP kernels with it.

Besides the model the file holds what the CPU and the GPU tests share: the edge-value clouds and crop boxes, the clouds of
the per-tile outlier tests, what the library may know about a cloud's tile values without looking at a point (`TileSet`, so
that a test can tell which cwipc_tilefilter calls have to be answered without a kernel), and the driver of the random chains.
"""
from __future__ import annotations

import numpy as np

POINT_DTYPE = np.dtype([('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('r', 'u1'), ('g', 'u1'), ('b', 'u1'), ('tile', 'u1')])


def empty(n: int) -> np.ndarray:
    return np.zeros(n, dtype=POINT_DTYPE)


def tilefilter(pts: np.ndarray, tile: int) -> np.ndarray:
    """keep iff tile == 0 || tile == pt.a (:296): 0 keeps all; an int outside 0..255 equals no uint8."""
    if tile == 0:
        return pts.copy()
    if not 0 <= tile <= 255:
        return pts[:0].copy()
    return pts[pts['tile'] == np.uint8(tile)].copy()


def tilefilter_masked(pts: np.ndarray, mask: int) -> np.ndarray:
    """(tile & mask) != 0, in input order (registration/util.py:105-107).  Masks are tile masks: 0..255."""
    assert 0 <= mask <= 255
    return pts[(pts['tile'] & np.uint8(mask)) != 0].copy()


def crop(pts: np.ndarray, bbox) -> np.ndarray:
    """lo <= v && v < hi on every axis in float32 (:348-350); the C ABI takes float[6], so the bounds are rounded first."""
    with np.errstate(over='ignore', invalid='ignore'):
        b = np.asarray(bbox, dtype=np.float64).astype(np.float32)
    assert b.shape == (6,)
    with np.errstate(invalid='ignore'):
        keep = ((b[0] <= pts['x']) & (pts['x'] < b[1]) & (b[2] <= pts['y']) & (pts['y'] < b[3]) &
                (b[4] <= pts['z']) & (pts['z'] < b[5]))
    return pts[keep].copy()


def tilemap(pts: np.ndarray, mapping) -> np.ndarray:
    m = np.frombuffer(bytes(mapping), dtype=np.uint8)
    assert m.size == 256
    out = pts.copy()
    out['tile'] = m[pts['tile']]
    return out


def colormap(pts: np.ndarray, clear_bits: int, set_bits: int) -> np.ndarray:
    """word = (word & ~clear) | set on PCL's a << 24 | r << 16 | g << 8 | b, a being the tile (:377-378)."""
    clear_bits &= 0xffffffff
    set_bits &= 0xffffffff
    word = ((pts['tile'].astype(np.uint32) << 24) | (pts['r'].astype(np.uint32) << 16) | (pts['g'].astype(np.uint32) << 8) |
            pts['b'].astype(np.uint32))
    word = (word & np.uint32(~clear_bits & 0xffffffff)) | np.uint32(set_bits)
    out = pts.copy()
    out['tile'], out['r'], out['g'], out['b'] = (word >> 24) & 0xff, (word >> 16) & 0xff, (word >> 8) & 0xff, word & 0xff
    return out


def join(*parts: np.ndarray) -> np.ndarray:
    """All points of the first, then of the second, ... (:403-409; the n-ary form is the left fold)."""
    return np.concatenate([np.ascontiguousarray(p, dtype=POINT_DTYPE) for p in parts]) if parts else empty(0)


def tiles_used(pts: np.ndarray):
    return sorted(np.unique(pts['tile']).tolist())


def offset_scale(pts: np.ndarray, x: float, y: float, z: float, scale: float) -> np.ndarray:
    """(p + offset) * scale in Python floats, stored into a c_float: widened, two float64 operations, one rounding."""
    out = pts.copy()
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        for f, o in (('x', x), ('y', y), ('z', z)):
            out[f] = ((pts[f].astype(np.float64) + np.float64(o)) * np.float64(scale)).astype(np.float32)
    return out


def identity_transform(pts: np.ndarray) -> np.ndarray:
    """cwipc_transform with the identity matrix on finite coordinates: every coordinate plus +0.0 (-0.0 becomes +0.0)."""
    out = pts.copy()
    for f in ('x', 'y', 'z'):
        assert np.isfinite(pts[f]).all()
        out[f] = pts[f] + np.float32(0.0)
    return out


def join_metadata(clouds_ts_cs):
    """timestamp and cellsize of a join: the minimum of each (:411-414), folded from the left as std::min does."""
    ts, cs = clouds_ts_cs[0]
    for t, c in clouds_ts_cs[1:]:
        ts = min(ts, t)
        cs = c if c < cs else cs
    return ts, cs


class TileSet:
    """What can be known about the tile values of a cloud without looking at its points: None (nothing: a fresh upload),
    or a frozenset of the values that may occur.  The rules are the ones a correct implementation may use, stated on sets.

    This mirrors, rule for rule, the bookkeeping of csrc/filters.cpp (DeviceSoA::tiles, only_tile, may_have_tile, the union in
    join, the images in tilemap, the mask arithmetic in colormap), and run_chain() below mirrors which results share one
    object with their input.  The chain test asserts that every shortcut the mirror allows is taken, so a change to what the
    library knows about tiles has to be made here as well."""

    def __init__(self, values=None):
        self.values = None if values is None else frozenset(int(v) for v in values)

    def known(self) -> bool:
        return self.values is not None

    # -- producers ---------------------------------------------------------------------------------------------------
    def after_tilefilter(self, tile: int) -> "TileSet":
        if tile == 0:
            return TileSet(self.values)
        return TileSet([tile & 255])

    def after_subset(self) -> "TileSet":          # crop, masked filter: what could not occur still cannot
        return TileSet(self.values)

    def after_tilemap(self, mapping) -> "TileSet":
        m = bytes(mapping)
        return TileSet({m[t] for t in (range(256) if self.values is None else self.values)})

    def after_colormap(self, clear_bits: int, set_bits: int) -> "TileSet":
        if self.values is None:
            return TileSet(None)
        c, s = (clear_bits >> 24) & 255, (set_bits >> 24) & 255
        return TileSet({(t & ~c & 255) | s for t in self.values})

    @staticmethod
    def after_join(parts) -> "TileSet":
        """parts: (TileSet, npoints) pairs.  Parts without points say nothing and change nothing."""
        full = [(s, n) for s, n in parts if n]
        if len(full) == 1:
            return TileSet(full[0][0].values)
        if not full or any(not s.known() for s, _ in full):
            return TileSet(None)
        return TileSet(set().union(*[s.values for s, _ in full]))

    def after_census(self, used) -> "TileSet":
        return TileSet(self.values) if self.known() else TileSet(used)

    # -- the shortcut a tile filter may take -------------------------------------------------------------------------
    def tilefilter_shortcut(self, tile: int, npoints: int):
        """'all' (the result is the input), 'none' (empty without a kernel) or None (the points have to be looked at)."""
        if tile == 0:
            return 'all'
        if not npoints or not self.known() or not 0 <= tile <= 255:
            return None
        if self.values == frozenset([tile]):
            return 'all'
        if tile not in self.values:
            return 'none'
        return None


# ---------------------------------------------------------------------------------------------------------------------
# inputs shared by tests/test_exact_model.py (CPU) and tests/test_gpu_exact_filters.py
# ---------------------------------------------------------------------------------------------------------------------
FLT_MAX = float(np.finfo(np.float32).max)
DENORMALS = (1e-45, 1e-39)        # the smallest float32 denormal (rounds to 1.4e-45) and a larger one


def edge_values(bounds=()):
    """The float32 values at which a comparison or a copy can go wrong: NaN, infinities, signed zeros, denormals, the
    largest finite values, and every bound with its two neighbours."""
    v = [np.nan, np.inf, -np.inf, 0.0, -0.0, FLT_MAX, -FLT_MAX]
    for d in DENORMALS:
        v += [d, -d]
    with np.errstate(over='ignore', invalid='ignore'):
        for b in np.asarray(list(bounds), dtype=np.float64).astype(np.float32):
            v += [b, np.nextafter(b, np.float32(np.inf)), np.nextafter(b, np.float32(-np.inf))]
        return np.asarray(v, dtype=np.float64).astype(np.float32)


def edge_cloud(rng, n, bounds=(), special=0.5, tiles=None, finite=False):
    """n points whose coordinates are edge values with probability `special`, ordinary values in [-2, 2) otherwise."""
    pts = empty(n)
    ev = edge_values(bounds)
    if finite:
        ev = ev[np.isfinite(ev)]
    for f in ('x', 'y', 'z'):
        plain = (rng.random(n) * 4 - 2).astype(np.float32)
        pts[f] = np.where(rng.random(n) < special, ev[rng.integers(0, len(ev), n)], plain)
    pts['r'], pts['g'], pts['b'] = rng.integers(0, 256, n), rng.integers(0, 256, n), rng.integers(0, 256, n)
    pts['tile'] = rng.integers(0, 256, n) if tiles is None else np.asarray(tiles, dtype=np.uint8)[rng.integers(0, len(tiles), n)]
    return pts


def crop_boxes():
    """(name, box): ordinary, degenerate, inverted, bounded by infinities, by NaN, and with bounds float32 cannot represent."""
    inf, nan = float('inf'), float('nan')
    return [
        ("ordinary", [-1.0, 1.0, -1.0, 1.0, -1.0, 1.0]),
        ("everything finite", [-inf, inf, -inf, inf, -inf, inf]),
        ("zero and up", [0.0, inf, 0.0, inf, 0.0, inf]),
        ("below zero", [-inf, 0.0, -inf, 0.0, -inf, 0.0]),
        ("minus zero as bound", [-0.0, 1.0, -0.0, 1.0, -0.0, 1.0]),
        ("degenerate x", [0.25, 0.25, -inf, inf, -inf, inf]),
        ("degenerate zero", [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]),
        ("inverted", [1.0, -1.0, -inf, inf, -inf, inf]),
        ("inverted infinities", [inf, -inf, inf, -inf, inf, -inf]),
        ("NaN low bound", [nan, 1.0, -inf, inf, -inf, inf]),
        ("NaN high bound on z", [-inf, inf, -inf, inf, -1.0, nan]),
        ("all NaN", [nan] * 6),
        ("largest finite", [-FLT_MAX, FLT_MAX, -FLT_MAX, FLT_MAX, -FLT_MAX, FLT_MAX]),
        ("up to the largest finite", [-inf, FLT_MAX, -inf, FLT_MAX, -inf, FLT_MAX]),
        ("denormal bounds", [-1e-45, 1e-45, -inf, inf, -1e-39, inf]),
        ("not representable", [0.1, 1.0000000001, -1.0000000001, 0.1, -16777217.0, 16777217.0]),
        ("beyond float32", [-1e39, 1e39, -1e39, 1e39, -1e39, 1e39]),
        ("one axis only", [-inf, inf, 0.1, 0.25, -inf, inf]),
    ]


def crop_bounds():
    """Every bound of crop_boxes() but NaN, as the float32 the C ABI makes of it, once each (by bit pattern: both zeros).  A
    crop cloud gets each of them and its two float32 neighbours as coordinates (edge_values)."""
    with np.errstate(over='ignore'):
        b = np.asarray([v for _, box in crop_boxes() for v in box], dtype=np.float64).astype(np.float32)
    b = b[~np.isnan(b)]
    _, first = np.unique(b.view(np.uint32), return_index=True)
    return tuple(b[np.sort(first)])


CROP_BOUNDS = crop_bounds()

COLORMAP_MASKS = [(0xffffffff, 0x010203), (0, 0), (0xff000000, 0x07000000), (0x00ff0000, 0x00800000), (0x000000ff, 0x00000011), (0x0000ff00, 0),
                  (0x12345678, 0x9abcdef0)]


OUTLIER_K, OUTLIER_MUL = 8, 1.0
OUTLIER_CLOUDS = ("interleaved5", "tiles256", "last_point_tile", "late_tile", "small_tiles", "wildcard")
_OUTLIER_SEED = {"interleaved5": 11, "tiles256": 12, "last_point_tile": 13, "late_tile": 14, "small_tiles": 15, "wildcard": 16}


def outlier_cloud(name):
    """The clouds of the per-tile outlier tests: a wavy sheet with a few far points, tiles laid out as the name says.  The
    seeds are chosen so that in every tile no d_i lies within 1e-6 (relative) of the oracle's threshold -- checked on the
    CPU by tests/test_exact_model.py -- so the oracle's result is the only right one, byte for byte."""
    rng = np.random.default_rng(_OUTLIER_SEED[name])
    n = {"interleaved5": 5000, "tiles256": 19968, "last_point_tile": 3000, "late_tile": 270000, "small_tiles": 3000, "wildcard": 4000}[name]
    pts = empty(n)
    side = float(np.sqrt(n / 5000.0))
    pts['x'], pts['y'] = rng.random(n) * side, rng.random(n) * side * 0.5
    pts['z'] = 0.03 * np.sin(pts['x'] * 6.0) + rng.normal(0, 0.002, n)
    far = rng.integers(0, n, max(n // 200, 5))
    pts['z'][far] += rng.normal(0, 0.3, len(far)).astype(np.float32)
    pts['r'], pts['g'], pts['b'] = rng.integers(0, 256, n), rng.integers(0, 256, n), rng.integers(0, 256, n)
    idx = np.arange(n)
    if name == "interleaved5":
        pts['tile'] = 1 + idx % 5
    elif name == "tiles256":
        pts['tile'] = rng.permutation(n) % 256             # every value, 0 (the wildcard) included, in random order
        # (78 points per tile on a thin strip: the oracle's shell search through so few points scattered over a sheet takes a tenth of
        # a second per tile, and the library's search through a dozen points 24 ms)
        pts['y'] = rng.random(n) * 0.002
        pts['z'] = 0.001 * np.sin(pts['x'] * 40.0)
        pts['x'][far] += rng.normal(0, 0.3, len(far)).astype(np.float32)
    elif name == "last_point_tile":
        pts['tile'] = 1
        pts['tile'][-1] = 7
    elif name == "late_tile":
        pts['tile'] = np.where(idx < 265000, 3, 9)
    elif name == "small_tiles":
        pts['tile'] = 1
        at = rng.permutation(n)[:17]
        for t, (a, b) in zip((20, 21, 22, 23, 24), ((0, 1), (1, 2), (2, 5), (5, 10), (10, 17))):   # 1, 1, 3, 5, 7 points: fewer than k
            pts['tile'][at[a:b]] = t
    else:
        pts['tile'] = np.where(idx < n // 3, 1, np.where(idx < 2 * n // 3, 0, 2))
    return pts


def first_appearance(tiles):
    _, first = np.unique(tiles, return_index=True)
    return [int(tiles[i]) for i in np.sort(first)]


_pertile_cache = {}


def pertile_expectation(oracle, name):
    """(cloud, tiles in first-appearance order, the expected per-tile result, the oracle's d_i tile by tile), computed once for
    the CPU and the GPU test alike.  `oracle` is the CPU oracle of the caller (the one place here that uses it).  Asserts that the
    1e-6 band around the oracle's threshold is empty in every tile, so that the join of the oracle's per-tile results is the only
    right answer, and that the oracle's own per-tile call returns that very cloud."""
    if name not in _pertile_cache:
        pts = outlier_cloud(name)
        order = first_appearance(pts['tile'])
        parts, dists = [], []
        for t in order:
            kept, d, thr = oracle.remove_outliers(tilefilter(pts, t), OUTLIER_K, OUTLIER_MUL, False, want_stats=True)
            band = np.abs(d.astype(np.float64) - thr) <= 1e-6 * abs(thr)
            assert not band.any(), (name, t, int(band.sum()))
            parts.append(kept)
            dists.append(d)
        exp = join(*parts)
        whole = oracle.remove_outliers(pts, OUTLIER_K, OUTLIER_MUL, True)
        assert len(whole) == len(exp) and whole.tobytes() == exp.tobytes(), (name, len(whole), len(exp))
        _pertile_cache[name] = (pts, order, exp, dists)
    return _pertile_cache[name]


# ---------------------------------------------------------------------------------------------------------------------
# model-based random chains
# ---------------------------------------------------------------------------------------------------------------------
CHAIN_SEEDS = 200
CHAIN_STEPS = 8
CHAIN_BIG_EVERY = 20            # every 20th seed draws a cloud just above the small-cloud limit of the compaction (262,144)


class ModelCloud:
    """A cloud as the model sees it: points, timestamp, cellsize, what is known of its tiles; `dev` is the device cloud of
    the backend that runs the chain on the GPU (None in a model-only run)."""

    def __init__(self, pts, ts, cs, tiles, dev=None):
        self.pts, self.ts, self.cs, self.tiles, self.dev = pts, ts, cs, tiles, dev


def run_chain(seed, backend=None):
    """Chain `seed`: two uploads, then CHAIN_STEPS random operations, each applied to the model and -- if there is a backend --
    to the device, where backend.apply(op, args, inputs, expected) runs the operation and compares.  The draws depend on the
    seed and the model alone, so a model-only run sees the steps a GPU run takes.  Returns the counts of the tile-filter steps
    and of those a tile set answers without a kernel."""
    rng = np.random.default_rng(1000 + seed)
    big = seed % CHAIN_BIG_EVERY == 0
    n = 262145 + int(rng.integers(0, 5000)) if big else int(rng.integers(0, 6001))
    if rng.random() < 0.3:
        alphabet = [int(rng.integers(1, 256))]
    else:
        alphabet = sorted(set(int(v) for v in rng.integers(0 if rng.random() < 0.2 else 1, 256, int(rng.integers(2, 5)))))
    outside = [v for v in range(1, 256) if v not in alphabet]
    stats = {"tilefilter_steps": 0, "shortcut_all": 0, "shortcut_all_tile0": 0, "shortcut_none": 0, "steps": 0}

    def upload(m, ts, cs):
        pts = edge_cloud(rng, m, special=0.2, tiles=alphabet, finite=True)
        c = ModelCloud(pts, ts, cs, TileSet(None))
        if backend:
            c.dev = backend.upload(pts, ts, cs)
        return c

    clouds = [upload(int(rng.integers(0, 300)), 700 + seed, 0.25), upload(n, 900 + seed, 0.5)]
    cur = clouds[-1]
    for step in range(CHAIN_STEPS):
        op = ("tilefilter", "tilefilter", "masked", "crop", "tilemap", "colormap", "join", "census", "transform")[int(rng.integers(0, 9))]
        ins, args, shortcut, new = [cur], (), None, None
        if op == "tilefilter":
            kind = rng.random()
            tile = (int(rng.choice(alphabet)) if kind < 0.45 else int(rng.choice(outside)) if kind < 0.7 else 0 if kind < 0.85
                    else 256 + int(rng.choice(alphabet)))
            args = (tile,)
            shortcut = cur.tiles.tilefilter_shortcut(tile, len(cur.pts))
            stats["tilefilter_steps"] += 1
            if shortcut:
                stats["shortcut_" + shortcut] += 1
                stats["shortcut_all_tile0"] += 1 if tile == 0 else 0
            # (a result that IS the input -- tile 0, or the only tile there is -- shares what is known with it, a later census included)
            tiles = cur.tiles if shortcut == 'all' else cur.tiles.after_tilefilter(tile)
            new = ModelCloud(tilefilter(cur.pts, tile), cur.ts, cur.cs, tiles)
        elif op == "masked":
            mask = int(rng.integers(1, 256)) if rng.random() < 0.5 else int(rng.choice(alphabet)) & -int(rng.choice(alphabet)) or 1
            args = (mask,)
            new = ModelCloud(tilefilter_masked(cur.pts, mask), cur.ts, cur.cs, cur.tiles.after_subset())
        elif op == "crop":
            lo, hi = sorted((rng.random(2) * 5 - 2.5).tolist())
            box = [lo, hi, -np.inf, np.inf, -np.inf, np.inf] if rng.random() < 0.75 else [-np.inf, np.inf, -3.0, 3.0, -np.inf, FLT_MAX]
            args = (box,)
            new = ModelCloud(crop(cur.pts, box), cur.ts, cur.cs, cur.tiles.after_subset())
        elif op == "tilemap":
            if rng.random() < 0.3:
                m = bytes([int(rng.choice(alphabet))]) * 256
            else:
                table = list(range(256))
                for a in alphabet:
                    table[a] = int(rng.choice(alphabet))
                m = bytes(table)
            args = (m,)
            new = ModelCloud(tilemap(cur.pts, m), cur.ts, cur.cs, cur.tiles.after_tilemap(m))
        elif op == "colormap":
            clear, setb = int(rng.integers(0, 1 << 24)), int(rng.integers(0, 1 << 24))
            if rng.random() < 0.3:
                clear, setb = clear | 0xff000000, setb | (int(rng.choice(alphabet)) << 24)
            args = (clear, setb)
            new = ModelCloud(colormap(cur.pts, clear, setb), cur.ts, cur.cs, cur.tiles.after_colormap(clear, setb))
        elif op == "join":
            other = clouds[int(rng.integers(0, len(clouds)))]
            ins = [cur, other] if rng.random() < 0.5 else [other, cur]
            ts, cs = join_metadata([(c.ts, c.cs) for c in ins])
            whole = [c for c in ins if len(c.pts) and len(c.pts) == sum(len(d.pts) for d in ins)]
            tiles = whole[0].tiles if whole else TileSet.after_join([(c.tiles, len(c.pts)) for c in ins])   # (one part holds all: it IS the result)
            new = ModelCloud(join(*[c.pts for c in ins]), ts, cs, tiles)
        elif op == "census":
            used = tiles_used(cur.pts)
            if backend:
                backend.census(cur, used)
            if len(cur.pts) and not cur.tiles.known():
                cur.tiles.values = frozenset(used)
            stats["steps"] += 1
            continue
        else:
            new = ModelCloud(identity_transform(cur.pts), cur.ts, cur.cs, TileSet(cur.tiles.values))
        if backend:
            new.dev = backend.apply(op, args, ins, new, shortcut)
        stats["steps"] += 1
        clouds.append(new)
        # an empty cloud ends nothing: the chain goes on from an earlier one that still has points, if there is one
        alive = [c for c in clouds if len(c.pts)]
        cur = new if len(new.pts) or not alive else alive[int(rng.integers(0, len(alive)))]
    return stats
