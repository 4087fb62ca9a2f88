"""The numpy model of RULE S (include/cwipc_util_amd/hip_ext.h): plane segmentation by random-sample consensus.  CPU only.

Everything the rule states in float64 operations "rounded on their own, in the order written" is written here as numpy float64
expressions in that order (numpy evaluates one IEEE operation per operator), the integers as uint64 / int64 / Python integers:
the splitmix64 draws, the index rule, the hypothesis table, the counts, the best hypothesis, the refit's integer sums, the exact
matrix M as Python integers rounded to float once.  The eigenvector comes from a line-by-line Python port of
csrc/smallest_eigvec.hpp (IEEE doubles, the same operations in the same order, so the SAME BITS as the library), and
numpy.linalg.eigh stands beside it as the independent check of its direction.  brute_force() is a pure-Python statement of the same
rule with loops and Python numbers, for clouds of a few hundred points: tests/test_plane_model.py holds the model to it.
"""
import math
import struct

import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
TAG_PLANE = 0x706c616e65
MASK = (1 << 64) - 1
FIX = 16.0
MAX_OFFSET = 262144.0
MAX_CNT = 1 << 26
REFINE = 1
KEEP_INLIERS, KEEP_REST, BELOW_IS_INLIER = 1, 2, 4
RESULT_FORMAT = "<4d4d10q6dI3IIIIiii"   # cwipc_hip_plane_result


# ---------------------------------------------------------------------------
# draws
# ---------------------------------------------------------------------------
def splitmix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z ^ (z >> np.uint64(30)); z = z * np.uint64(0xBF58476D1CE4E5B9)
        z = z ^ (z >> np.uint64(27)); z = z * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def splitmix64_int(z):
    z &= MASK
    z ^= z >> 30; z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27; z = (z * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def triples(seed, H, n):
    """(H, 3) uint32: i_k = ((x_k >> 32) * n) >> 32 with x_k = draw(base, 3 h + k)"""
    base = splitmix64_int((int(seed) + TAG_PLANE) & MASK)
    k = np.arange(3 * H, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = splitmix64(np.uint64(base) + (k + np.uint64(1)) * np.uint64(GOLDEN))
        idx = ((x >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)
    return idx.astype(np.uint32).reshape(H, 3)


def constrained(axis, min_abs_cos):
    return min_abs_cos > 0.0 and any(float(a) != 0.0 for a in axis)


def dot3(n, a):
    """(n_x a_x + n_y a_y) + n_z a_z on the last axis of n"""
    return (n[..., 0] * a[0] + n[..., 1] * a[1]) + n[..., 2] * a[2]


# ---------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------
def table(xyz, H, seed, axis=(0.0, 0.0, 0.0), min_abs_cos=0.0):
    """xyz: (n, 3) float32.  Returns planes (H, 4) float64 (four +0.0 for an invalid row), valid (H,) bool, triples (H, 3) uint32."""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    n = len(xyz)
    tri = triples(seed, H, n)
    planes = np.zeros((H, 4), dtype=np.float64)
    valid = (tri[:, 0] != tri[:, 1]) & (tri[:, 0] != tri[:, 2]) & (tri[:, 1] != tri[:, 2])
    if n == 0:
        return planes, np.zeros(H, dtype=bool), tri
    P = xyz.astype(np.float64)
    p0, p1, p2 = P[tri[:, 0]], P[tri[:, 1]], P[tri[:, 2]]
    with np.errstate(all="ignore"):
        valid &= np.isfinite(p0).all(axis=1) & np.isfinite(p1).all(axis=1) & np.isfinite(p2).all(axis=1)
        u, v = p1 - p0, p2 - p0
        c = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
        l2 = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
        valid &= np.isfinite(l2) & (l2 > 0.0)
        nrm = c / np.sqrt(l2)[:, None]
        if constrained(axis, min_abs_cos):
            a = np.asarray(axis, dtype=np.float64)
            valid &= np.abs(dot3(nrm, a)) >= min_abs_cos
        d = -dot3(nrm, p0.T)   # (p0.T[k] is column k: the same products, per row)
    planes[valid, :3] = nrm[valid]
    planes[valid, 3] = d[valid]
    return planes, valid, tri


def signed_distance(xyz64, plane):
    """e(p) = ((n_x x + n_y y) + n_z z) + d"""
    with np.errstate(all="ignore"):
        return ((plane[0] * xyz64[:, 0] + plane[1] * xyz64[:, 1]) + plane[2] * xyz64[:, 2]) + plane[3]


def inliers(xyz, plane, distance, below=False):
    P = np.asarray(xyz, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    e = signed_distance(P, np.asarray(plane, dtype=np.float64))
    with np.errstate(all="ignore"):
        return (e <= distance) if below else (np.abs(e) <= distance)


def counts(xyz, planes, valid, distance):
    P = np.asarray(xyz, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    block = max(1, min(128, (1 << 23) // max(len(P), 1)))      # hypotheses at a time: the temporaries stay within 64 MB each
    out = np.zeros(len(planes), dtype=np.uint32)
    hs = np.nonzero(valid)[0]
    with np.errstate(all="ignore"):
        for at in range(0, len(hs), block):
            h = hs[at:at + block]
            pl = planes[h]
            e = ((pl[:, 0:1] * P[:, 0][None, :] + pl[:, 1:2] * P[:, 1][None, :]) + pl[:, 2:3] * P[:, 2][None, :]) + pl[:, 3:4]
            out[h] = (np.abs(e) <= distance).sum(axis=1)
    return out


def best(counts_, valid):
    """(found, h): the largest count among the valid, the smallest h on a tie"""
    hs = np.nonzero(valid)[0]
    if len(hs) == 0:
        return False, 0
    return True, int(hs[np.argmax(counts_[hs])])   # (argmax returns the first of equals)


# ---------------------------------------------------------------------------
# the refit
# ---------------------------------------------------------------------------
def refit_sums(xyz, plane, distance, anchor):
    """cnt, S1[3], S2[6] as Python integers"""
    P = np.asarray(xyz, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    inl = inliers(xyz, plane, distance)
    s = FIX / distance
    with np.errstate(all="ignore"):
        q = np.rint((P[inl] - np.asarray(anchor, dtype=np.float64)[None, :]) * s)
        part = (np.abs(q) <= MAX_OFFSET).all(axis=1)
    o = q[part].astype(np.int64)
    out = [int(len(o))] + [int(o[:, a].sum()) for a in range(3)]
    for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
        out.append(int((o[:, a] * o[:, b]).sum()))
    return out


def refit_matrix(sums):
    """M_ab = cnt * S2_ab - S1_a * S1_b in Python integers, each rounded to float once: xx xy xz yy yz zz"""
    cnt, s1, s2 = sums[0], sums[1:4], sums[4:10]
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    exact = [cnt * s2[i] - s1[a] * s1[b] for i, (a, b) in enumerate(pairs)]
    return [float(v) for v in exact], exact


def smallest_eigvec(M6):
    """csrc/smallest_eigvec.hpp, line by line, in Python floats: the same IEEE operations in the same order"""
    a = [[M6[0], M6[1], M6[2]], [M6[1], M6[3], M6[4]], [M6[2], M6[4], M6[5]]]
    v = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(12):
        off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2]
        whole = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2] + 2.0 * off
        if not (off > 1e-32 * whole):
            break
        for r in range(3):
            p, q = (1 if r == 2 else 0), (1 if r == 0 else 2)
            apq = a[p][q]
            if apq == 0.0:
                continue
            theta = (a[q][q] - a[p][p]) / (2.0 * apq)
            t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            for k in range(3):
                akp, akq = a[k][p], a[k][q]
                a[k][p] = c * akp - s * akq
                a[k][q] = s * akp + c * akq
            for k in range(3):
                apk, aqk = a[p][k], a[q][k]
                a[p][k] = c * apk - s * aqk
                a[q][k] = s * apk + c * aqk
            for k in range(3):
                vkp, vkq = v[k][p], v[k][q]
                v[k][p] = c * vkp - s * vkq
                v[k][q] = s * vkp + c * vkq
    m = 0
    if a[1][1] < a[m][m]:
        m = 1
    if a[2][2] < a[m][m]:
        m = 2
    ln = math.sqrt(v[0][m] * v[0][m] + v[1][m] * v[1][m] + v[2][m] * v[2][m])
    return [v[k][m] / ln for k in range(3)]


def eigh_normal(exact6):
    """The same eigenvector from numpy.linalg.eigh of the exact matrix (scaled by a power of two so that it fits a double well)"""
    M = np.array([[exact6[0], exact6[1], exact6[2]], [exact6[1], exact6[3], exact6[4]], [exact6[2], exact6[4], exact6[5]]], dtype=object)
    top = max(1, max(abs(int(v)) for v in exact6))
    scale = 1 << max(0, top.bit_length() - 60)
    A = np.array([[float(int(v) / scale) for v in row] for row in M], dtype=np.float64)
    w, vec = np.linalg.eigh(A)
    return vec[:, 0], w


def fdot(n, a):
    return (n[0] * a[0] + n[1] * a[1]) + n[2] * a[2]


def refit_plane(sums, anchor, hyp, distance, axis=(0.0, 0.0, 0.0), min_abs_cos=0.0):
    """(ok, plane', M6): the refit of RULE S from the sums; ok False where n' is not finite or misses the constraint"""
    M6, _ = refit_matrix(sums)
    n = smallest_eigvec(M6)
    if not all(math.isfinite(x) for x in n):
        return False, [0.0] * 4, M6
    if not (fdot(n, hyp) >= 0.0):
        n = [-x for x in n]
    if constrained(axis, min_abs_cos) and not (abs(fdot(n, [float(a) for a in axis])) >= min_abs_cos):
        return False, [0.0] * 4, M6
    s = FIX / distance
    cnt = float(sums[0])
    c = [float(anchor[a]) + (float(sums[1 + a]) / cnt) / s for a in range(3)]
    return True, [n[0], n[1], n[2], -fdot(n, c)], M6


def orient(plane, axis=(0.0, 0.0, 0.0), min_abs_cos=0.0):
    a = [float(x) for x in axis] if constrained(axis, min_abs_cos) else [0.0, 1.0, 0.0]
    return [-x for x in plane] if fdot(plane, a) < 0.0 else list(plane)


class Found:
    def __init__(self):
        self.plane = [0.0] * 4
        self.hypothesis = [0.0] * 4
        self.sums = [0] * 10
        self.M = [0.0] * 6
        self.best = 0
        self.triple = [0, 0, 0]
        self.count = self.recount = self.valid = 0
        self.found = self.refined = 0
        self.planes = self.counts = self.valid_rows = self.triples = None

    def tobytes(self):
        return struct.pack(RESULT_FORMAT, *self.plane, *self.hypothesis, *self.sums, *self.M, self.best, *self.triple, self.count, self.recount,
                           self.valid, self.found, self.refined, 0)


def find(xyz, distance, H, seed=0, axis=(0.0, 0.0, 0.0), min_abs_cos=0.0, refine=True):
    """cwipc_hip_plane_find on the CPU.  xyz: (n, 3) float32."""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    f = Found()
    f.planes, f.valid_rows, f.triples = table(xyz, H, seed, axis, min_abs_cos)
    f.counts = counts(xyz, f.planes, f.valid_rows, distance)
    f.valid = int(f.valid_rows.sum())
    ok, h = best(f.counts, f.valid_rows)
    if not ok:
        return f
    f.found, f.best, f.count = 1, h, int(f.counts[h])
    f.hypothesis = [float(v) for v in f.planes[h]]
    f.triple = [int(v) for v in f.triples[h]]
    chosen = f.hypothesis
    if refine:
        anchor = xyz[f.triple[0]].astype(np.float64)
        f.sums = refit_sums(xyz, f.hypothesis, distance, anchor)
        if 3 <= f.sums[0] <= MAX_CNT:
            ok, plane, f.M = refit_plane(f.sums, anchor, f.hypothesis, distance, axis, min_abs_cos)
            if ok:
                f.recount = int(inliers(xyz, plane, distance).sum())
                if f.recount >= f.count:
                    f.refined, chosen = 1, plane
    f.plane = orient(chosen, axis, min_abs_cos)
    return f


def partition(xyz, plane, distance, flags):
    """(indices of the result in input order, n_first): the stable two-class partition"""
    inl = inliers(xyz, plane, distance, below=bool(flags & BELOW_IS_INLIER))
    a = np.nonzero(inl)[0] if flags & KEEP_INLIERS else np.zeros(0, dtype=np.int64)
    b = np.nonzero(~inl)[0] if flags & KEEP_REST else np.zeros(0, dtype=np.int64)
    return np.concatenate([a, b]), len(a)


def angle_deg(a, b):
    a, b = np.asarray(a[:3], dtype=np.float64), np.asarray(b[:3], dtype=np.float64)
    c = abs(float(a @ b)) / (np.linalg.norm(a) * np.linalg.norm(b))
    s = np.linalg.norm(np.cross(a, b)) / (np.linalg.norm(a) * np.linalg.norm(b))
    return math.degrees(math.atan2(s, c))


# ---------------------------------------------------------------------------
# the same rule in pure Python, for small clouds
# ---------------------------------------------------------------------------
def brute_force(xyz, distance, H, seed=0, axis=(0.0, 0.0, 0.0), min_abs_cos=0.0, refine=True):
    """Loops and Python numbers only (a Python float is an IEEE double, math.sqrt is correctly rounded).  Returns a Found whose
    planes / counts / valid_rows / triples are lists."""
    pts = [[float(np.float32(v)) for v in p] for p in np.asarray(xyz, dtype=np.float32).reshape(-1, 3)]
    n = len(pts)
    base = splitmix64_int((seed + TAG_PLANE) & MASK)
    con = constrained(axis, min_abs_cos)
    ax = [float(a) for a in axis]
    f = Found()
    f.planes, f.counts, f.valid_rows, f.triples = [], [], [], []

    def e_of(pl, p):
        return ((pl[0] * p[0] + pl[1] * p[1]) + pl[2] * p[2]) + pl[3]

    def count_of(pl):
        return sum(1 for p in pts if abs(e_of(pl, p)) <= distance)

    for h in range(H):
        idx = []
        for k in range(3):
            x = splitmix64_int((base + (3 * h + k + 1) * GOLDEN) & MASK)
            idx.append(((x >> 32) * n) >> 32)
        plane, ok = [0.0] * 4, len(set(idx)) == 3
        if ok:
            p0, p1, p2 = pts[idx[0]], pts[idx[1]], pts[idx[2]]
            ok = all(math.isfinite(v) for v in p0 + p1 + p2)
        if ok:
            u = [p1[a] - p0[a] for a in range(3)]
            v = [p2[a] - p0[a] for a in range(3)]
            try:
                c = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
                l2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
            except OverflowError:   # (Python raises where IEEE gives an infinity: invalid either way)
                l2 = math.inf
            ok = math.isfinite(l2) and l2 > 0.0
        if ok:
            ln = math.sqrt(l2)
            nrm = [c[0] / ln, c[1] / ln, c[2] / ln]
            ok = not con or abs(fdot(nrm, ax)) >= min_abs_cos
        if ok:
            plane = nrm + [-fdot(nrm, p0)]
        cnt = count_of(plane) if ok else 0
        f.planes.append(plane); f.counts.append(cnt); f.valid_rows.append(ok); f.triples.append(idx)
        if ok:
            f.valid += 1
            if not f.found or cnt > f.count:
                f.found, f.best, f.count, f.hypothesis, f.triple = 1, h, cnt, plane, idx
    if not f.found:
        return f
    chosen = f.hypothesis
    if refine:
        anchor = pts[f.triple[0]]
        s = FIX / distance
        sums = [0] * 10
        for p in pts:
            if not abs(e_of(f.hypothesis, p)) <= distance:
                continue
            q = [(p[a] - anchor[a]) * s for a in range(3)]
            if not all(math.isfinite(v) for v in q):
                continue
            o = [round(v) for v in q]   # (round half to even, as rint)
            if any(abs(v) > 262144 for v in o):
                continue
            sums[0] += 1
            for a in range(3):
                sums[1 + a] += o[a]
            for i, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                sums[4 + i] += o[a] * o[b]
        f.sums = sums
        if 3 <= sums[0] <= MAX_CNT:
            ok, plane, f.M = refit_plane(sums, anchor, f.hypothesis, distance, axis, min_abs_cos)
            if ok:
                f.recount = count_of(plane)
                if f.recount >= f.count:
                    f.refined, chosen = 1, plane
    f.plane = orient(chosen, axis, min_abs_cos)
    return f


# ---------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------
def rotation_about(axis, degrees):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    t = math.radians(degrees)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)


def scene(n=20000, floor_share=0.30, tilt_deg=7.0, noise=0.004, seed=11):
    """A noisy tilted floor, a body blob and a wall.  Returns (xyz float32 (n, 3), the floor's true unit normal (towards +Y), its d)."""
    rng = np.random.default_rng(seed)
    nf = int(round(n * floor_share))
    nw = int(round(n * 0.25))
    nb = n - nf - nw
    floor = np.stack([rng.uniform(-2, 2, nf), rng.normal(0, noise, nf), rng.uniform(-2, 2, nf)], axis=1)
    body = rng.normal((0.0, 0.9, 0.0), (0.2, 0.45, 0.15), (nb, 3))
    wall = np.stack([rng.uniform(-2, 2, nw), rng.uniform(0, 2.0, nw), 2.0 + rng.normal(0, noise, nw)], axis=1)
    R = rotation_about((1.0, 0.0, 0.5), tilt_deg)
    shift = np.array([0.1, -0.3, 0.2])
    pts = np.concatenate([floor, body, wall]) @ R.T + shift
    pts = pts[rng.permutation(n)]
    normal = R @ np.array([0.0, 1.0, 0.0])
    return pts.astype(np.float32), normal, -float(normal @ shift)


def to_points(xyz, seed=5):
    """A structured cwipc_point array with colours and tiles that tell the points apart"""
    from cwipc_util_amd.util import cwipc_point_numpy_dtype
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    pts = np.zeros(len(xyz), dtype=cwipc_point_numpy_dtype)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["r"] = rng.integers(0, 256, len(xyz)); pts["g"] = rng.integers(0, 256, len(xyz)); pts["b"] = np.arange(len(xyz)) & 255
    pts["tile"] = 1 << rng.integers(0, 4, len(xyz))
    return pts
