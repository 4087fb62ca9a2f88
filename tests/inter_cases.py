"""Streams for the inter-frame codec (RULE P) with CHOSEN leaf sets: the cases of test_inter_cases.py (the model alone),
test_gpu_inter_edges.py (the kernels) and test_inter_host.py (the host code).  Pure numpy.

The lattice construction.  The GOP's cube is binary-exact: MN = (-1, -1, -1), SIDE = 4.  The first frame of every stream is anchor(),
three points whose box is [0, 2]^3; with exp_factor 2.0 the grown cube is exactly (MN, SIDE).  Every later "lattice" frame is the cloud
frame_of(X) = cm.decode(X)[0] of a cwao packet X built over any chosen key set, stored colours and tiles in that cube: its points are
cell centres, which float32 holds exactly at every depth up to 16, so the frame lies in the cube (a delta), the encoder's intra packet
of it is X byte for byte, and its delta is im.diff(X, the frame before, gop_index).  Frames that are not decode outputs (several
points in a leaf, non-finite points, points on the cube's faces) take their expected bytes from im.Encoder alone.

A case is built when it is first asked for; cases() itself only names them.  A frame's `pins` say what the case is there for
(nleaves, nadded, ...): test_inter_cases.py holds the model's output to them, so a case cannot drift off its path unnoticed."""
import functools

import numpy as np

import codec_model as cm
import inter_model as im

MN = (-1.0, -1.0, -1.0)
SIDE = 4.0
EXP_FACTOR = 2.0
COUNTS = (1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 512, 513)      # the wave, the workgroup, the keep byte
QUALITY = {4: 10, 5: 30, 6: 60, 7: 80, 8: 95}                        # colour bits -> a jpeg_quality that gives them


def timestamp(index):
    """Of frame `index` of a stream (the anchor is frame 0)."""
    return 1000 + 33 * index


@functools.lru_cache(maxsize=None)
def anchor():
    pts = cm.make_cloud([[0.0, 0.0, 0.0], [2.0, 2.0, 2.0], [1.0, 0.5, 1.5]], [[10, 20, 30], [200, 100, 50], [255, 0, 128]], tile=1)
    pts.setflags(write=False)
    return pts


def frame_of(packet):
    pts = cm.decode(packet)[0]
    pts.setflags(write=False)
    return pts


def lattice_packet(seed, keys, bits, cb, index, tile="plane", stored=None):
    """The cwao packet of the leaves `keys` in the cube (MN, SIDE) with the timestamp of frame `index`.  Colours: `stored`, else drawn.
    tile: "plane" (drawn from 1, 2, 4) or one value.  The tile mode is the encoder's own choice (0 when all tiles are equal), so that
    the packet is the one an encoder gives for its decoded cloud even where a drawn plane comes out uniform (one leaf, two leaves)."""
    rng = np.random.default_rng(seed)
    keys = np.unique(np.asarray(keys, dtype=np.uint64))
    n = len(keys)
    drawn = rng.integers(0, 1 << cb, (n, 3))
    tiles = rng.choice(np.array([1, 2, 4], dtype=np.uint8), n) if tile == "plane" else np.full(n, tile, dtype=np.uint8)
    return cm.build_packet(keys, drawn if stored is None else stored, tiles, np.asarray(MN, dtype=np.float32), SIDE, bits, cb, timestamp(index))


def centres(keys, bits):
    """float32 [n, 3]: the cell centres of the keys (ascending), in the cube (MN, SIDE)."""
    pts = cm.decode(lattice_packet(0, keys, bits, 8, 0, tile=1))[0]
    return np.stack([pts['x'], pts['y'], pts['z']], axis=1)


def crowd(seed, keys, counts, bits):
    """A cloud with counts[i] points at the centre of the cell keys[i] (ascending), colours and tiles drawn per point, shuffled."""
    rng = np.random.default_rng(seed)
    xyz = np.repeat(centres(keys, bits), counts, axis=0)
    pts = cm.make_cloud(xyz, rng.integers(0, 256, (len(xyz), 3)))
    pts['tile'] = rng.choice(np.array([1, 2, 4], dtype=np.uint8), len(xyz))
    return pts[rng.permutation(len(pts))]


def non_finite(n, seed=0):
    """n points that RULE C drops: NaN, +inf or -inf in one coordinate, the other two far outside any cube."""
    rng = np.random.default_rng(seed)
    xyz = np.empty((n, 3), dtype=np.float32)
    for i in range(n):
        xyz[i] = (np.float32(1e9), np.float32(-1e30), np.float32(1e9))[i % 3], np.float32(-1e30 if i % 2 else 1e9), np.float32(1e9 if i % 5 else -1e30)
        xyz[i, i % 3] = (np.nan, np.inf, -np.inf)[(i // 3) % 3]
    pts = cm.make_cloud(xyz, rng.integers(0, 256, (n, 3)))
    pts['tile'] = 8
    return pts


# ---------------------------------------------------------------------------
# a case
# ---------------------------------------------------------------------------
class Case:
    """octree_bits, jpeg_quality, gop_size, entropy; frames: the clouds after the anchor; lattice[i]: the packet frames[i] was made
    from, or None; pins[i]: what frame i + 1 of the stream is there for; kinds: the stream's pattern, anchor included ("K", "d");
    model(): (packets, intra packets, kinds) of im.Encoder over anchor + frames."""

    def __init__(self, bits, quality, build, gop=64, entropy=False, kinds=None):
        self.octree_bits, self.jpeg_quality, self.gop_size, self.entropy = bits, quality, gop, entropy
        self.colour_bits = 8 - cm.colour_shift(quality)
        self._build, self._kinds = build, kinds

    @property
    def _made(self):
        key = (self._build, self.octree_bits, self.colour_bits)
        if key not in _built:
            made = _Frames(self.octree_bits, self.colour_bits)
            self._build(made)
            for f in made.frames:
                f.setflags(write=False)
            _built[key] = made
        return _built[key]

    frames = property(lambda self: self._made.frames)
    lattice = property(lambda self: self._made.lattice)
    pins = property(lambda self: self._made.pins)
    kinds = property(lambda self: self._kinds or "K" + "d" * len(self.frames))

    def stream(self):
        return [anchor()] + list(self.frames)

    def model(self):
        key = (self._build, self.octree_bits, self.jpeg_quality, self.gop_size, self.entropy)
        if key not in _models:
            enc = im.Encoder(self.gop_size, EXP_FACTOR, self.octree_bits, self.jpeg_quality, self.entropy)
            packets, intra = [], []
            for i, f in enumerate(self.stream()):
                packets.append(enc.feed(f, timestamp(i)))
                intra.append(enc.intra)
            _models[key] = (packets, intra, "".join("Kd"[k] for k in enc.kinds))
        return _models[key]

    def boundaries(self):
        """at_gop_boundary() before each feed of the stream and after the last, by the rule's state machine over the model's output."""
        _, intra, kinds = self.model()
        g, have, out = 0, False, []
        for k, p in zip(kinds, intra):
            out.append(g == 0 or not have)
            g = 0 if k == "K" else g
            have = cm.parse(p)["nleaves"] > 0
            g = (g + 1) % self.gop_size
        return out + [g == 0 or not have]

    def gop_indices(self):
        g, out = 0, []
        for k in self.model()[2]:
            g = 0 if k == "K" else g
            out.append(g)
            g = (g + 1) % self.gop_size
        return out


_built, _models = {}, {}


class _Frames:
    def __init__(self, bits, cb):
        self.bits, self.cb = bits, cb
        self.frames, self.lattice, self.pins = [], [], []

    def leaves(self, seed, keys, tile="plane", stored=None, extra=None, **pins):
        """A lattice frame; extra: points appended to it (non-finite ones: the packet stays the frame's)."""
        X = lattice_packet(seed, keys, self.bits, self.cb, len(self.frames) + 1, tile, stored)
        pts = frame_of(X)
        if extra is not None:
            pts = extra(pts)
        self.frames.append(pts)
        self.lattice.append(X)
        self.pins.append(dict(nleaves=len(np.unique(np.asarray(keys, dtype=np.uint64))), **pins))

    def points(self, pts, **pins):
        self.frames.append(np.ascontiguousarray(pts))
        self.lattice.append(None)
        self.pins.append(pins)


def _pool(seed, bits):
    """All keys of a shallow tree in a drawn order."""
    return np.random.default_rng(seed).permutation(1 << (3 * bits)).astype(np.uint64)


def _draw(rng, n, bits):
    """n distinct keys of a tree of any depth (a permutation of 2^48 keys is not to be had)."""
    k = np.unique(rng.integers(0, 1 << (3 * bits), 2 * n + 16, dtype=np.uint64))
    assert len(k) >= n
    return rng.permutation(k)[:n]


# ---------------------------------------------------------------------------
# leaf counts at the wave, the workgroup and the keep byte (bits 6)
# ---------------------------------------------------------------------------
SECOND_START = (9, 64, 255, 512)         # P takes R's leaves 1, 3, 5, ... here, 0, 2, 4, ... elsewhere: R's last leaf kept and not, at nR % 8 == 0 and != 0


def _count_nR(f):
    pool, at = _pool(101, 6), 0
    new = pool[4000:]
    for i, nr in enumerate(COUNTS):
        R = np.sort(pool[at:at + nr])
        at += nr
        start = 1 if nr in SECOND_START else 0
        f.leaves(200 + i, R)
        f.leaves(300 + i, np.concatenate([R[start::2], new[5 * i:5 * i + 5]]), nR=nr, nadded=5, last_kept=(nr - 1 - start) % 2 == 0)


def _count_nP(f):
    pool = _pool(102, 6)
    rng = np.random.default_rng(103)
    R, new = np.sort(pool[:300]), pool[1000:]
    for i, n in enumerate(COUNTS):
        kept = min(n // 2, 300)
        f.leaves(400 + i, R, tile=2 if i % 2 else "plane")
        f.leaves(500 + i, np.concatenate([R[rng.choice(300, kept, replace=False)], new[600 * i:600 * i + n - kept]]), nR=300, nadded=n - kept)


def _count_added(f):
    pool = _pool(104, 6)
    R, new = np.sort(pool[:20]), pool[1000:]                   # 20 leaves: three keep bytes
    for i, n in enumerate(COUNTS):
        f.leaves(600 + i, R)
        f.leaves(700 + i, np.concatenate([R[::2], new[600 * i:600 * i + n]]), nR=20, nadded=n)


# ---------------------------------------------------------------------------
# past one scan round (bits 7): more than 256 workgroups of 256 leaves
# ---------------------------------------------------------------------------
def _big_added(f):
    pool = _pool(105, 7)
    rng = np.random.default_rng(106)
    R = np.sort(pool[:65793])
    f.leaves(800, R)
    f.leaves(801, np.concatenate([R[rng.choice(65793, 256, replace=False)], pool[65793:65793 + 65537]]), nR=65793, nadded=65537)


def _big_dropped(f):
    R = np.sort(_pool(107, 7)[:65537])
    stored = np.random.default_rng(108).integers(0, 1 << f.cb, (65537, 3))
    keep = np.arange(65537) % 3 != 2
    f.leaves(802, R, stored=stored)
    f.leaves(803, R[keep], stored=stored[keep], nR=65537, nadded=0)     # a still scene: the colour residuals are 0 and get coded


# ---------------------------------------------------------------------------
# key positions (bits 6), key 0 and the all-sevens key (any depth)
# ---------------------------------------------------------------------------
def _positions(f):
    pool = _pool(109, 6)
    low, mid, high = (np.sort(pool[(pool >= a) & (pool < b)][:n]) for a, b, n in ((0, 900, 200), (1000, 2000, 300), (3000, 4000, 250)))
    f.leaves(900, mid)
    f.leaves(901, low, nR=300, nadded=200)                    # P entirely before R's first key: every predictor is leaf 0
    f.leaves(902, mid)
    f.leaves(903, high, nR=300, nadded=250)                   # P entirely behind R's last key: every predictor is the last leaf
    f.leaves(904, np.arange(0, 600, 2))
    f.leaves(905, np.arange(1, 600, 2), nR=300, nadded=300)   # even cells in R, odd cells in P


RUN = np.arange(5000, 5600, dtype=np.uint64)                  # 75 whole nodes of the last depth, three workgroups of added leaves


def _run_of_600(f):
    pool = _pool(110, 6)
    R = np.sort(pool[(pool < 4000) | (pool >= 6000)][:400])
    f.leaves(910, R)
    f.leaves(911, np.concatenate([R, RUN]), nR=400, nadded=600, last_depth=bytes([0xff]) * 75)


def _first_and_last_key(f):
    rng = np.random.default_rng(111 + f.bits)
    last = np.uint64((1 << (3 * f.bits)) - 1)
    mids = _draw(rng, 80, f.bits)
    mids = mids[(mids != 0) & (mids != last)]
    a, b = mids[:40], mids[20:60]
    both = np.array([0, last], dtype=np.uint64)
    f.leaves(920, np.concatenate([a, both]), holds=(True, True))
    f.leaves(921, np.concatenate([b, both]), holds=(True, True), nadded=20)              # both kept
    f.leaves(922, a, holds=(False, False), nadded=20)                                    # both dropped
    f.leaves(923, np.concatenate([b, both]), holds=(True, True), nadded=22)              # both added
    f.leaves(924, np.concatenate([b, both[:1]]), holds=(True, False), nadded=0)          # key 0 kept, the last dropped
    f.leaves(925, np.concatenate([a, both[1:]]), holds=(False, True), nadded=21)         # key 0 dropped, the last added
    f.leaves(926, np.concatenate([a, both]), holds=(True, True), nadded=1)               # key 0 added, the last kept


# ---------------------------------------------------------------------------
# depth
# ---------------------------------------------------------------------------
def _shallow(f):
    """bits 1 and 2: all leaves, single ones, halves, complements, subsets and supersets, then drawn subsets."""
    total = 1 << (3 * f.bits)
    every = np.arange(total)
    rng = np.random.default_rng(120 + f.bits)
    shapes = [every, [0], [total - 1], [0, total - 1], every[1:-1], every, every[::2], every[1::2], every, [total // 2], [total // 2, total // 2 + 1], every,
              every[:total // 2], every[total // 2:], every[:total // 2], every[:total // 2]]
    shapes += [every[rng.random(total) < p] for p in (0.5, 0.5, 0.2, 0.8, 0.5, 0.9, 0.1, 0.5) * 3]
    before = None
    for i, keys in enumerate(shapes):
        keys = np.asarray(keys, dtype=np.uint64)
        if len(keys) == 0:
            continue
        pins = {} if before is None else dict(nR=len(before), nadded=len(np.setdiff1d(keys, before)))
        f.leaves(1000 + i, keys, tile="plane" if i % 3 else 4, **pins)
        before = keys


def _sparse(f):
    rng = np.random.default_rng(130 + f.bits)
    last = np.uint64((1 << (3 * f.bits)) - 1)
    k = _draw(rng, 460, f.bits)
    k = k[(k != 0) & (k != last)]
    both = np.array([0, last], dtype=np.uint64)
    f.leaves(1100, np.concatenate([k[:298], both]))
    f.leaves(1101, np.concatenate([k[:148], k[298:448], both]), nR=300, nadded=150)
    f.leaves(1102, np.concatenate([k[100:398]]), nR=300, nadded=150)


def _dense_16(f):
    rng = np.random.default_rng(140)
    top = np.uint64(int(rng.integers(1, 1 << 39)) << 9)                  # 13 triples shared, the last three take every value
    dense = top | np.arange(512, dtype=np.uint64)
    sparse = _draw(rng, 300, 16)
    sparse = sparse[(sparse >> np.uint64(9)) != (top >> np.uint64(9))]
    f.leaves(1200, sparse)
    f.leaves(1201, dense, nR=len(sparse), nadded=512, nodes_added=[1] * 13 + [8, 64, 512])
    f.leaves(1202, np.concatenate([dense[::2], sparse[:100]]), nR=512, nadded=100)
    f.leaves(1203, np.concatenate([dense, sparse[:100]]), nR=356, nadded=256)


# ---------------------------------------------------------------------------
# colours and tiles (bits 5)
# ---------------------------------------------------------------------------
def _colour(f):
    """The kept leaves' stored colours from 0 to the maximum and back: the residual wraps both ways; the other leaves drawn."""
    pool = _pool(150, 5)
    rng = np.random.default_rng(151 + f.cb)
    top = (1 << f.cb) - 1
    R = np.sort(pool[:200])
    low, high = rng.integers(0, top + 1, (200, 3)), rng.integers(0, top + 1, (200, 3))
    low[:100], high[:100] = 0, top
    low[100:150, 1], high[100:150, 1] = 0, top              # and one channel alone
    f.leaves(1300, R, stored=low)
    f.leaves(1301, np.concatenate([R, pool[200:260]]), stored=_stored(R, high, pool[200:260], rng, top), nR=200, nadded=60)
    f.leaves(1302, R, stored=low, nR=260, nadded=0)
    f.leaves(1303, R[:150], stored=high[:150], nR=200, nadded=0)


def _stored(R, colours, more, rng, top):
    """Colours in key order for the leaves R (ascending, with `colours`) and `more` (drawn)."""
    keys = np.concatenate([R, more])
    col = np.concatenate([colours, rng.integers(0, top + 1, (len(more), 3))])
    return col[np.argsort(keys, kind="stable")]


def _tiles(f):
    pool = _pool(160, 5)
    a, b = np.sort(pool[:300]), np.sort(np.concatenate([pool[:150], pool[300:420]]))
    f.leaves(1400, a, tile=1, tile_mode=0)                   # uniform after the anchor's uniform 1: the same value
    f.leaves(1401, b, tile="plane", tile_mode=1)             # uniform -> plane
    f.leaves(1402, a, tile="plane", tile_mode=1)             # plane -> plane
    f.leaves(1403, b, tile=2, tile_mode=0)                   # plane -> uniform
    f.leaves(1404, a, tile=4, tile_mode=0)                   # uniform -> uniform with another value
    f.leaves(1405, b, tile=4, tile_mode=0)
    f.leaves(1406, a, tile="plane", tile_mode=1)


# ---------------------------------------------------------------------------
# frames that are no decoder's output: crowded leaves, non-finite points, the wide frame, the cube's faces
# ---------------------------------------------------------------------------
def _crowded(f):
    pool = _pool(170, 6)
    three = np.sort(pool[:3])
    f.points(crowd(171, three, [1, 700, 1], 6), nleaves=3, points=702)              # two workgroups and more without a leaf start
    f.points(crowd(172, np.sort(pool[3:260]), [2] * 257, 6), nleaves=257, points=514)
    f.points(crowd(173, three, [1, 513, 1], 6), nleaves=3, points=515, nadded=3)
    f.points(np.concatenate([crowd(174, three, [1, 700, 1], 6), non_finite(50)]), nleaves=3, points=752, nadded=0)
    f.points(crowd(175, np.sort(pool[:40]), [300] + [1] * 38 + [520], 6), nleaves=40, points=858, nadded=37)     # the crowds at both ends


def _non_finite(f):
    pool = _pool(180, 6)
    bad = non_finite(30)
    a, b = np.sort(pool[:50]), np.sort(pool[25:75])
    f.leaves(1500, a, extra=lambda pts: np.concatenate([bad, pts]))                                    # first in input order
    f.leaves(1501, b, extra=lambda pts: np.concatenate([pts, bad]), nR=50, nadded=25)                  # last
    f.leaves(1502, a, extra=lambda pts: _scatter(pts, bad), nR=50, nadded=25)                          # scattered
    f.leaves(1503, b, extra=lambda pts: np.concatenate([non_finite(600, 1), pts]), nR=50, nadded=25)   # two whole workgroups of the bounds kernel hold none that counts
    f.points(bad, nleaves=0)                                  # nothing finite: an empty frame, a key that leaves no reference
    f.points(frame_of(lattice_packet(1504, b, 6, f.cb, 6)))  # a key again, in a cube of its own
    f.points(_scatter(_recoloured(f.frames[-1][::2], 181), bad), nadded=0)


def _scatter(pts, bad):
    """The points `bad` spread evenly over the input order, the first and the last place included."""
    out = np.empty(len(pts) + len(bad), dtype=cm.POINT_DTYPE)
    taken = np.zeros(len(out), dtype=bool)
    taken[np.linspace(0, len(out) - 1, len(bad)).astype(np.int64)] = True
    out[taken], out[~taken] = bad, pts
    return out


def _recoloured(pts, seed):
    out = pts.copy()
    rgb = np.random.default_rng(seed).integers(0, 256, (len(out), 3))
    out['r'], out['g'], out['b'] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    return out


WIDE = 140000            # above 131 072 points the bounds kernel's grid is capped and its lanes stride


def _wide(f):
    rng = np.random.default_rng(190)
    pts = cm.random_cloud(rng, WIDE, 1.9, (1.0, 1.0, 1.0), tiles=(1, 2))          # inside [-0.9, 2.9]^3
    f.points(pts, points=WIDE)
    bad = _recoloured(pts, 191)
    bad['x'][-1], bad['y'][-1], bad['z'][-1] = np.nan, 1e9, -1e30
    f.points(bad, points=WIDE, nadded=0)                      # the last point in input order is non-finite and far away: a delta
    out = _recoloured(pts, 192)
    out['x'][-1] = 3.5
    f.points(out, points=WIDE)                                # the last point alone leaves the cube: a key
    f.points(pts, points=WIDE)
    low = _recoloured(pts, 193)
    low['x'][512 * 256 - 1] = -4.0                            # the grown cube starts at -3.1: the last lane of the last workgroup's first trip
    f.points(low, points=WIDE)


def _face(axis, second):
    """A frame with a point on the cube's top face and one on its bottom face (a delta, the clamp cell and cell 0), then one a
    float32 step past the top ("past") or below the bottom ("below"): a key; then the first again, a delta in the new cube."""
    def build(f):
        inner = np.sort(_pool(195, 6)[:20])

        def with_points(*values):
            def extra(pts):
                more = cm.make_cloud([[1.0, 1.0, 1.0]] * len(values), [[9, 99, 199]] * len(values), tile=2)
                more['xyz'[axis]][:] = values
                return np.concatenate([pts, more])
            return extra
        top, bottom = np.float32(MN[axis] + SIDE), np.float32(MN[axis])
        on = frame_of(lattice_packet(1600, inner, 6, f.cb, 1))
        f.points(with_points(top, bottom)(on), nleaves=22, nadded=22, cells=(0, 63))
        step = np.nextafter(top, np.float32(np.inf)) if second == "past" else np.nextafter(bottom, np.float32(-np.inf))
        f.points(with_points(step)(on))
        f.points(with_points(top, bottom)(on))
    return build


_FACES = {(a, s): _face(a, s) for a in range(3) for s in ("past", "below")}


# ---------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    """{name: Case}.  Every group of the list in test_inter_cases.py's docstring; nothing is built here."""
    out = {}
    out["counts: nR"] = Case(6, QUALITY[7], _count_nR)
    out["counts: nP"] = Case(6, QUALITY[6], _count_nP)
    out["counts: added"] = Case(6, QUALITY[8], _count_added)
    for entropy in (False, True):
        tail = ", entropy" if entropy else ""
        out["two scan rounds: added" + tail] = Case(7, QUALITY[5], _big_added, entropy=entropy)
        out["two scan rounds: dropped" + tail] = Case(7, QUALITY[5], _big_dropped, entropy=entropy)
    out["positions"] = Case(6, QUALITY[7], _positions)
    out["run of 600 added"] = Case(6, QUALITY[7], _run_of_600)
    out["key 0 and the last key, bits 6"] = Case(6, QUALITY[8], _first_and_last_key)
    out["key 0 and the last key, bits 16"] = Case(16, QUALITY[8], _first_and_last_key)
    out["bits 1"] = Case(1, QUALITY[7], _shallow)
    out["bits 2"] = Case(2, QUALITY[6], _shallow)
    for bits in (11, 12, 13, 14, 15, 16):
        out[f"bits {bits}, sparse"] = Case(bits, QUALITY[4 + bits % 5], _sparse, entropy=bits % 2 == 0)
    out["bits 16, dense"] = Case(16, QUALITY[7], _dense_16)
    for cb in (4, 5, 6, 7, 8):
        out[f"colour bits {cb}"] = Case(5, QUALITY[cb], _colour)
    out["tiles"] = Case(5, QUALITY[6], _tiles)
    out["crowded leaves"] = Case(6, QUALITY[8], _crowded)
    out["non-finite points"] = Case(6, QUALITY[7], _non_finite, kinds="KddddKKd")
    out["wide frame"] = Case(5, QUALITY[6], _wide, kinds="KddKdK")
    for (axis, second), build in _FACES.items():
        out[f"face {'xyz'[axis]}: {second}"] = Case(6, QUALITY[8], build, kinds="KdKd")
    return out


CROWDED = ("crowded leaves", "non-finite points", "wide frame")                 # given again in another point order
# every frame fed before the first packet is taken: leaf counts, tile modes and kinds that change from frame to frame
QUEUED = ("counts: nR", "bits 1", "tiles", "non-finite points")
BIG, TINY, MID = "two scan rounds: added", "counts: added", "run of 600 added"
