"""Trees for transform colour coding (RULE T) and level-of-detail cuts (RULE L) with CHOSEN leaf keys: the cases of
test_tree_cases.py (the models alone), test_gpu_transform_edges.py and test_gpu_lod_edges.py (the kernels), test_transform_host.py and
test_lod_host.py (the host code).  Pure numpy.

A case is a set of ascending leaf keys with an 8-bit colour and a tile a leaf.  Its "cwao" packet P is cm.build_packet of them in the
cube mn = 0, side = 1.  Its CLOUD has one point a leaf at the cell's centre (q + 0.5) / 2^bits, which float32 holds exactly up to 16
bits; the points of the first and the last cell are moved to the cube's corners (0, 0, 0) and (1, 1, 1), which pins the cube.  Every
case therefore holds cell 0 and the all-ones cell (a case of one leaf holds cell 0 alone), and cm.encode(cloud, bits, quality of its
colour bits) is P byte for byte (test_tree_cases.py holds every case to that).

A case names the jpeg qualities its transform runs at (`qualities`) and the cuts its level-of-detail runs take (`cuts`), and `pins`:
what it is there for (counts, scan rounds, launches, escapes, weights, run lengths and places).  test_tree_cases.py works the pins
out again from the models and the keys, so a case cannot drift off its path unnoticed.  A case is built when it is first used."""
import functools
import struct

import numpy as np

import codec_model as cm
import entropy_model as em
import transform_model as tm

TIMESTAMP = 4711
QUALITY_OF = {4: 10, 5: 30, 6: 60, 7: 80, 8: 100}                    # colour bits -> a jpeg_quality that stores them
LANES, WAVE = 256, 64                                                # a workgroup of the kernels, a wave


def last_key(bits):
    return (1 << (3 * bits)) - 1


def with_corners(keys, bits):
    return np.unique(np.concatenate([np.asarray(keys, dtype=np.uint64), np.array([0, last_key(bits)], dtype=np.uint64)]))


def draw(rng, n, bits, below=None):
    """n distinct keys, ascending, cell 0 and the all-ones cell among them (n == 1: cell 0).  below: the other keys lie under it."""
    if n == 1:
        return np.zeros(1, dtype=np.uint64)
    top = last_key(bits) if below is None else below
    if top <= 1 << 24:
        inner = rng.choice(top - 1, n - 2, replace=False).astype(np.uint64) + np.uint64(1)
    else:
        inner = np.unique(rng.integers(1, top, 2 * n + 16, dtype=np.uint64))
        inner = rng.permutation(inner)[:n - 2]
    return with_corners(inner, bits)


def smooth(n):
    """Colours that change slowly along the key order: most coefficients are small, the lossy qualities differ."""
    i = np.arange(n) / max(n, 1)
    return np.clip(np.stack([128 + 100 * np.sin(11 * i), 128 + 90 * np.cos(7 * i + 1), 128 + 80 * np.sin(23 * i)], axis=1), 0, 255).astype(np.int64)


class Case:
    """octree_bits, colour_bits, qualities, cuts, pins; keys, stored [n, 3] (below 2^colour_bits), tiles; packet, cloud."""

    def __init__(self, bits, build, qualities=(), cuts=(), colour_bits=8, **pins):
        self.octree_bits, self.colour_bits, self.qualities, self.cuts, self.pins = bits, colour_bits, tuple(qualities), tuple(cuts), pins
        self._build = build

    @functools.cached_property
    def _made(self):
        keys, stored, tiles = self._build(self)
        keys = np.asarray(keys, dtype=np.uint64)
        n = len(keys)
        assert n >= 1 and int(keys[0]) == 0 and (n == 1 or int(keys[-1]) == last_key(self.octree_bits)) and (keys[1:] > keys[:-1]).all()
        stored = np.broadcast_to(np.asarray(stored, dtype=np.int64), (n, 3)).copy()
        tiles = np.broadcast_to(np.asarray(tiles, dtype=np.uint8), (n,)).copy()
        for a in (keys, stored, tiles):
            a.setflags(write=False)
        return keys, stored, tiles

    keys = property(lambda self: self._made[0])
    stored = property(lambda self: self._made[1])
    tiles = property(lambda self: self._made[2])
    quality = property(lambda self: QUALITY_OF[self.colour_bits])

    @functools.cached_property
    def packet(self):
        return cm.build_packet(self.keys, self.stored, self.tiles, np.zeros(3, dtype=np.float32), 1.0, self.octree_bits, self.colour_bits, TIMESTAMP)

    @functools.cached_property
    def cloud(self):
        pts = cm.decode(self.packet)[0].copy()
        for f in "xyz":
            pts[f][0] = 0.0
            if len(pts) > 1:
                pts[f][-1] = 1.0
        pts.setflags(write=False)
        return pts


def leaves(n, seed, colours="random", tiles="mixed", below=None):
    """A builder: n drawn leaves."""
    def build(case):
        rng = np.random.default_rng(seed)
        keys = draw(rng, n, case.octree_bits, below)
        return keys, paint(rng, len(keys), colours, case.colour_bits), tile_plane(rng, len(keys), tiles)
    return build


def paint(rng, n, colours, cb=8):
    if isinstance(colours, str):
        return rng.integers(0, 1 << cb, (n, 3)) if colours == "random" else smooth(n) >> (8 - cb)
    return np.broadcast_to(np.asarray(colours, dtype=np.int64), (n, 3))


def tile_plane(rng, n, tiles):
    return rng.choice(np.array([1, 2, 4], dtype=np.uint8), n) if isinstance(tiles, str) else np.full(n, tiles, dtype=np.uint8)


def of(keys_of, seed, colours="random", tiles="mixed"):
    """A builder: the keys of keys_of(rng, bits), painted."""
    def build(case):
        rng = np.random.default_rng(seed)
        keys = np.asarray(keys_of(rng, case.octree_bits), dtype=np.uint64)
        col = colours(keys, rng) if callable(colours) else paint(rng, len(keys), colours, case.colour_bits)
        return keys, col, tile_plane(rng, len(keys), tiles)
    return build


# ---------------------------------------------------------------------------
# counts: leaves, coefficients, inner nodes
# ---------------------------------------------------------------------------
def inner_nodes(count):
    """A 4-bit tree of exactly `count` inner nodes: the root, 8, 64 and count - 73 nodes of depth 3."""
    def keys_of(rng, bits):
        assert bits == 4 and 73 + 65 <= count <= 73 + 512
        must = np.concatenate([np.arange(64) * 8, [511]])
        rest = np.setdiff1d(np.arange(512), must)
        prefixes = np.sort(np.concatenate([must, rng.choice(rest, count - 73 - len(must), replace=False)])).astype(np.uint64)
        take = rng.random((len(prefixes), 8)) < 0.4
        take[0, 0] = take[-1, 7] = True
        take[~take.any(axis=1), 3] = True
        node, child = np.nonzero(take)
        return (prefixes[node] << np.uint64(3)) | child.astype(np.uint64)
    return keys_of


def past_inner(limit):
    """The fewest leaves of a drawn order at 16 bits whose tree has more than `limit` inner nodes."""
    def keys_of(rng, bits):
        pool = rng.permutation(np.unique(rng.integers(1, last_key(bits), limit // 7, dtype=np.uint64)))
        lo, hi = 2, len(pool)                         # inner(lo) <= limit < inner(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if inner_count(with_corners(pool[:mid], bits), bits) > limit:
                hi = mid
            else:
                lo = mid
        return with_corners(pool[:hi], bits)
    return keys_of


def inner_count(keys, bits):
    return 1 + sum(len(np.unique(keys >> np.uint64(3 * (bits - 1 - d)))) for d in range(bits - 1))


# ---------------------------------------------------------------------------
# depth widths
# ---------------------------------------------------------------------------
def chains(m):
    """m leaves of an 8-bit tree whose paths part at depth 4 at the latest: the depths below hold m nodes each."""
    def keys_of(rng, bits):
        assert bits == 8
        heads = np.concatenate([[0, 4095], rng.choice(4094, m - 2, replace=False) + 1]).astype(np.uint64)
        tails = rng.integers(0, 4096, m).astype(np.uint64)
        tails[0], tails[1] = 0, 4095
        return np.sort((heads << np.uint64(12)) | tails)
    return keys_of


# ---------------------------------------------------------------------------
# weights and values
# ---------------------------------------------------------------------------
def block_keys(origin, edge, bits):
    r = np.arange(edge)
    q = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3) + np.asarray(origin)
    return np.sort(cm.keys(q, bits))


def cells_of(keys, bits):
    """q [n, 3] of keys."""
    keys = np.asarray(keys, dtype=np.uint64)
    q = np.zeros((len(keys), 3), dtype=np.int64)
    for level in range(bits):
        triple = ((keys >> np.uint64(3 * (bits - 1 - level))) & np.uint64(7)).astype(np.int64)
        for a in range(3):
            q[:, a] = (q[:, a] << 1) | ((triple >> (2 - a)) & 1)
    return q


def full_block(rng, bits):
    return np.arange(1 << (3 * bits), dtype=np.uint64)


def lone_beside_blocks(rng, bits):
    """6 bits: cell 0 beside the full block [16, 32)^3 (1 against 4096, the light side first) and the full block [32, 48)^3 beside the
    all-ones cell (4096 against 1)."""
    assert bits == 6
    return with_corners(np.concatenate([block_keys((16, 16, 16), 16, 6), block_keys((32, 32, 32), 16, 6)]), 6)


def checkerboard(keys, rng):
    q = cells_of(keys, 5)
    return np.where((q.sum(axis=1) & 1)[:, None] == 0, [[255, 0, 0]], [[0, 0, 255]])


def sibling_pairs(npairs, bits=4):
    """npairs pairs of z siblings (children 0 and 1 of drawn nodes of the last inner depth), the pair of cell 0 and the pair of the
    all-ones cell among them.  Coefficients npairs - 1 .. 2 npairs - 2 are the pairs', in key order."""
    def keys_of(rng, b):
        assert b == bits
        total = 1 << (3 * (bits - 1))
        prefixes = np.sort(np.concatenate([[0, total - 1], rng.choice(total - 2, npairs - 2, replace=False) + 1])).astype(np.uint64)
        keys = np.stack([(prefixes << np.uint64(3)), (prefixes << np.uint64(3)) | np.uint64(1)], axis=1).reshape(-1)
        keys[-2:] = [last_key(bits) - 1, last_key(bits)]
        return keys
    return keys_of


def grey_pairs(pairs):
    """Colours for sibling_pairs: pair k is grey (pairs[k][0], pairs[k][1]); Y alone carries coefficients."""
    def colours(keys, rng):
        v = np.asarray([pairs(k) for k in range(len(keys) // 2)], dtype=np.int64).reshape(-1)
        return np.stack([v, v, v], axis=1)
    return colours


def escaping_pairs(quiet):
    """Every pair's |d| is 128 or more (an escape at step 1) but pair `quiet`'s; every pair's merged value is 128."""
    return grey_pairs(lambda k: (100, 156) if k == quiet else ((0, 255) if k % 2 else (255, 0)) if k % 3 else (64, 192))


BORDER = ((0, 127), (128, 0), (0, 128), (127, 0), (1, 128), (200, 72), (3, 131), (128, 255))      # d: 127, -128, 128, -127, 127, -128, 128, 127


# ---------------------------------------------------------------------------
# runs of RULE L
# ---------------------------------------------------------------------------
RUN_LENGTHS = {3: (1, 63, 64, 65, 255, 256, 257, 511, 512), 4: (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4096)}
RUN_STARTS = (0, 63, 64, 100)        # within the workgroup: its first lane, a wave's last lane, a wave's first lane, mid-wave


def plan_runs(lengths, order):
    """[run lengths] of consecutive nodes: every length of `lengths` at every start of RUN_STARTS (a filler run in front of it where
    the place needs one), in the order `order` of the lengths."""
    out, at = [], 0
    for start in RUN_STARTS:
        for n in order(lengths):
            gap = (start - at) % LANES
            if gap:
                out.append(gap)
            out.append(n)
            at += gap + n
    return out


def runs(lengths, below):
    """A builder of keys: node j of depth bits - below holds lengths[j] drawn leaves; cell 0 is in the first run, and the all-ones
    cell is a run of one at the end."""
    def keys_of(rng, bits):
        t, width = bits - below, 1 << (3 * below)
        assert len(lengths) < 1 << (3 * t) and max(lengths) <= width
        out = []
        for j, n in enumerate(lengths):
            low = np.sort(rng.choice(width, n, replace=False))
            if j == 0:
                low[0] = 0
            out.append((np.uint64(j) << np.uint64(3 * below)) | low.astype(np.uint64))
        return with_corners(np.concatenate(out), bits)
    return keys_of


def run_lengths(keys, bits, t):
    """(starts, lengths) of the runs that a cut at t makes of ascending keys."""
    prefix = np.asarray(keys, dtype=np.uint64) >> np.uint64(3 * (bits - t))
    starts = np.concatenate([[0], 1 + np.nonzero(prefix[1:] != prefix[:-1])[0]])
    return starts, np.diff(np.concatenate([starts, [len(prefix)]]))


MEAN_RUNS = (2, 4, 64, 256, 2, 6, 3, 65, 255, 1, 8, 8)       # the last two: all 0 and all the largest value


def mean_colours(below):
    """Per run (of the cut at bits - below) and channel a base value v; red: v + 1 on n / 2 leaves (the mean is v + 1 / 2 exactly and
    rounds up), green: on n / 2 - 1 leaves (just below the half: down), blue: on n - 1 leaves (up).  Odd runs: (n - 1) / 2 and
    (n + 1) / 2 leaves in red and green.  The last two runs of MEAN_RUNS are all 0 and all the largest value."""
    def colours(keys, rng):
        bits = 6
        top = 255
        starts, lengths = run_lengths(keys, bits, bits - below)
        out = np.zeros((len(keys), 3), dtype=np.int64)
        for j, (a, n) in enumerate(zip(starts.tolist(), lengths.tolist())):
            if j >= len(MEAN_RUNS) - 2:
                out[a:a + n] = 0 if j == len(MEAN_RUNS) - 2 else top
                continue
            base = rng.integers(0, top, 3)
            more = (n // 2, max(n // 2 - 1, 0) if n % 2 == 0 else (n + 1) // 2, n - 1)
            for ch in range(3):
                out[a:a + n, ch] = base[ch]
                out[a + rng.choice(n, more[ch], replace=False), ch] += 1
        return out
    return colours


def tile_or(rng, bits):
    """A run of 200 leaves from place 40 on (four waves of one workgroup); then a run of 200 from place 248 on (two workgroups)."""
    return runs([40, 200, 8, 200, 30], 3)(rng, bits)


def one_bit_tiles(keys):
    tiles = np.ones(len(keys), dtype=np.uint8)
    tiles[40 + 150] |= 0x80          # the third wave of the first long run
    tiles[248 + 199] |= 0x40         # the last leaf of the second, alone in its wave with 0x40
    tiles[248] |= 0x20               # its first leaf, in the workgroup before
    return tiles


def _tile_or_build(case):
    rng = np.random.default_rng(4100)
    keys = tile_or(rng, case.octree_bits)
    return keys, rng.integers(0, 256, (len(keys), 3)), one_bit_tiles(keys)


def straddling(cb):
    """The fewest leaves from 300 on whose last leaf's colour bits lie in two 32-bit words."""
    n = 300
    while (3 * cb * (n - 1)) % 32 + 3 * cb <= 32:
        n += 1
    return n


# ---------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------
BIG = "two scan rounds: 70 000 leaves at 9 bits"
BIG_RUN = "runs: one run of 70 000 leaves"
COUNTS = (1, 2, 3, 9, 256, 257, 258, 513, 4096, 4097)
ALL_QUALITIES = (0, 1, 49, 50, 99, 100)


def ascending(lengths):
    return list(lengths)


def descending(lengths):
    return list(lengths)[::-1]


@functools.lru_cache(maxsize=None)
def cases():
    """{name: Case}; nothing is built here."""
    out = {}
    for n in COUNTS:
        lossy = (24,) if n in (2, 257, 4097) else (85,) if n in (9, 4096) else ()
        out[f"counts: {n} leaves"] = Case(9, leaves(n, 1000 + n, tiles="mixed" if n % 2 else 3), (100,) + lossy, (1, 8) if n in (1, 3, 257, 4097) else (),
                                          nleaves=n, ncoef=n - 1)
    out["counts: 256 inner nodes"] = Case(4, of(inner_nodes(256), 1100), (100, 50), (3,), inner=256, first_blocks=1)
    out["counts: 257 inner nodes"] = Case(4, of(inner_nodes(257), 1101), (100, 50), (3,), inner=257, first_blocks=2)
    # scans past one round of 256 block counts
    out[BIG] = Case(9, leaves(70000, 1200), (100,), (1, 5, 8), first_rounds=4, escape_rounds=2, coded_tokens=True)
    out["two scan rounds: coefficients alone"] = Case(6, leaves(65538, 1201, colours="smooth"), (100,), (5,), ncoef=65537, first_rounds=1, escape_rounds=2)
    out["two scan rounds: inner nodes alone"] = Case(16, of(past_inner(65536), 1202), (100,), (15,), first_rounds=2, escape_rounds=1, just_past_inner=65536)
    out["two scan rounds: three of inner nodes"] = Case(16, of(past_inner(131072), 1203), (100,), (15,), first_rounds=3, escape_rounds=1, just_past_inner=131072)
    # depth widths
    for m in (255, 256, 257):
        out[f"depths: {m} chains"] = Case(8, of(chains(m), 1300 + m), (100, 50), (4, 7), nleaves=m, widths_from_3=[m] * 5, own_launches=0 if m <= 256 else 4)
    out["depths: 1 bit, all eight"] = Case(1, of(full_block, 1310), (100, 24), (1,), nleaves=8, own_launches=0)
    out["depths: 1 bit, the corners"] = Case(1, leaves(2, 1311), (100, 0), (), nleaves=2)
    out["depths: 2 bits"] = Case(2, leaves(9, 1312), (100, 50), (1,), nleaves=9)
    out["depths: 3 bits"] = Case(3, leaves(40, 1313, tiles=7), (100, 1), (1, 2), nleaves=40)
    out["depths: 16 bits, siblings of the last triple"] = Case(16, of(lambda rng, b: [0, 1, last_key(16)], 1314), (100, 50), (1, 15), widths=[2] * 15 + [3])
    out["depths: 16 bits, 3000 leaves"] = Case(16, leaves(3000, 1315), (100, 24), (1, 15, 16), own_launches=13)
    # weights
    out["weights: the full 32^3 block"] = Case(5, of(full_block, 1400), (100, 0), (2, 4), nleaves=32768, butterflies=[(8 ** k, 8 ** k) for k in range(1, 5)] + [(16384, 16384)])
    out["weights: 1 against 4096"] = Case(6, of(lone_beside_blocks, 1401), (100, 0), (2,), nleaves=8194, butterflies=[(1, 4096), (4096, 1), (4097, 4097)])
    out["weights: 1 and 2"] = Case(2, of(lambda rng, b: [0, 8, 9, 63], 1402, colours=lambda k, rng: [[10] * 3, [110] * 3, [150] * 3, [200] * 3], tiles=1), (100, 0), (1,),
                                   butterflies=[(1, 2), (1, 1), (3, 1)])
    # values
    out["values: checkerboard"] = Case(5, of(full_block, 1500, colours=checkerboard, tiles=1), (100, 0), (),
                                       nescapes={100: [0, 16384, 0], 0: [0, 0, 0]}, max_zz={100: 1020, 0: 12}, dc={100: [63, 0, -127]}, exact=True)
    for name, colour, dc in (("0", (0, 0, 0), [0, 0, 0]), ("255", (255, 255, 255), [255, 0, 0]), ("blue", (0, 0, 255), [63, -255, -127]), ("green", (0, 255, 0), [127, 0, 255])):
        out[f"values: constant {name}"] = Case(9, leaves(300, 1510, colours=colour), (100, 0), (4,) if name in ("0", "255") else (), dc={100: dc, 0: dc}, max_zz={100: 0, 0: 0})
    out["values: every coefficient escapes"] = Case(1, of(lambda rng, b: [0, 7], 1520, colours=lambda k, rng: [[255, 0, 0], [0, 255, 255]], tiles=1), (100,), (), nescapes={100: [1, 1, 1]})
    out["values: a block of 256 escapes, then none"] = Case(4, of(sibling_pairs(257), 1530, colours=escaping_pairs(256)), (100,), (), escape_blocks={100: [0, 256, 0]})
    out["values: none, then 256 escapes"] = Case(4, of(sibling_pairs(257), 1531, colours=escaping_pairs(0)), (100,), (), escape_blocks={100: [0, 255, 1]})
    out["values: zigzag 254, 255, 256"] = Case(4, of(sibling_pairs(len(BORDER)), 1540, colours=grey_pairs(lambda k: BORDER[k])), (100,), (), zz_has={100: [253, 254, 255, 256]})
    # quality and tiles
    out["quality: 5000 smooth leaves"] = Case(9, leaves(5000, 1600, colours="smooth"), ALL_QUALITIES, ())
    out["tiles: uniform"] = Case(9, leaves(5000, 1601, colours="smooth", tiles=5), (100, 50), (4,), tile_mode=0)
    out["tiles: mixed"] = Case(9, leaves(5000, 1602, colours="smooth"), (100, 50), (4,), tile_mode=1)
    # runs of RULE L
    for below, bits, order in ((3, 6, ascending), (3, 6, descending), (4, 7, ascending)):
        lengths = plan_runs(RUN_LENGTHS[below], order)
        name = f"runs: b - t = {below}, {order.__name__}"
        out[name] = Case(bits, of(runs(lengths, below), 4000 + below), (100,) if order is descending else (), (3, 1, bits - 1) if order is ascending else (3,),
                         placed=(3, RUN_LENGTHS[below]))
    out["runs: 512 runs of one"] = Case(7, of(runs([1] * 511, 3), 4010), (), (4,), run_set=(4, [1]), nleaves=512)
    out["runs: 513 runs of one"] = Case(7, of(runs([1] * 512, 3), 4011), (100,), (4,), run_set=(4, [1]), nleaves=513)
    out[BIG_RUN] = Case(7, leaves(70001, 4012, below=1 << 18), (100,), (1, 6), run_list=(1, [70000, 1]))
    out["runs: the full 16^3 block cut to waves"] = Case(5, of(lambda rng, b: with_corners(block_keys((0, 0, 0), 16, 5), 5), 4013), (100,), (3, 1, 4, 5, 6), run_list=(3, [64] * 64 + [1]))
    for cb in (4, 5, 7, 8):
        out[f"runs: {cb} colour bits"] = Case(5, leaves(straddling(cb), 4020 + cb), (), (1, 3, 4), colour_bits=cb, last_leaf_straddles=True)
    out["means: halves"] = Case(6, of(runs(list(MEAN_RUNS), 3), 4030, colours=mean_colours(3)), (), (3,), run_list=(3, list(MEAN_RUNS) + [1]), halves=True)
    out["tile or: one leaf's bit"] = Case(6, _tile_or_build, (), (3,), run_list=(3, [40, 200, 8, 200, 30, 1]), tile_bits=(3, [1, 0x81, 1, 0x61, 1, 1]))
    return out


def transform_runs():
    """[(name, quality)] of every transform run."""
    return [(name, q) for name, c in cases().items() for q in c.qualities]


def lod_runs():
    """[(name, t)] of every cut."""
    return [(name, t) for name, c in cases().items() for t in c.cuts]


# every small case again after the large ones
SMALL = [name for name in cases() if not name.startswith("two scan rounds") and name != BIG_RUN and "32^3" not in name and "checkerboard" not in name]


# ---------------------------------------------------------------------------
# hostile but valid "cwat" packets (decoder only)
# ---------------------------------------------------------------------------
def hostile_packet(plain, dc=(255, -255, 255)):
    """The "cwat" packet over the tree and tiles of the cwao packet `plain` with every token 255, every escape 0xffff, Q16 1024: every
    coefficient is the largest the container can say."""
    p = bytes(plain)
    info = cm.parse(p)
    n, b = info["nleaves"], info["octree_bits"]
    assert n - 1 < em.BLOCK                      # raw streams only
    values = dict(zip([(k, w) for k, w, _ in em.streams_of(info)], em.stream_values(p, info)))
    directory, payloads = [], []
    for kind, which, count in tm.streams_of(info, [n - 1] * 3):
        if kind == "escape":
            payload = b"\xff\xff" * count
            payload += bytes(cm.pad4(len(payload)) - len(payload))
        else:
            payload = em.raw_payload(kind, np.full(count, 255) if kind == "token" else values[(kind, which)], 8)
        directory.append(struct.pack("<II", 0, len(payload)))
        payloads.append(payload)
    fixed = struct.pack("<H3h3I", 1024, *dc, n - 1, n - 1, n - 1)
    return tm.MAGIC + struct.pack("<I", 1) + p[8:48 + 4 * b] + fixed + struct.pack("<I", len(payloads)) + b"".join(directory) + b"".join(payloads)


@functools.lru_cache(maxsize=None)
def hostile():
    """{name: cwat packet}"""
    chain = (0o1234567012345670 >> 3) << 3
    rng = np.random.default_rng(1700)
    two = tm.leaves_packet([chain | 1, chain | 6], [[1, 2, 3], [4, 5, 6]], 16, timestamp=TIMESTAMP)
    keys = draw(rng, 300, 9)
    many = tm.leaves_packet(keys, rng.integers(0, 256, (300, 3)), 9, tile_plane(rng, 300, "mixed"), timestamp=TIMESTAMP)
    return {"hostile: 2 leaves at 16 bits": hostile_packet(two), "hostile: 300 leaves at 9 bits": hostile_packet(many),
            "hostile: 300 leaves, dc the other way": hostile_packet(many, (-255, 255, -255))}
