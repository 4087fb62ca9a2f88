"""numpy float64 restatement of the direction filter (reference python/cwipc/registration/util.py:114-143), for the tests.

The reference estimates normals with open3d (KDTreeSearchParamHybrid(radius, max_nn), EstimateNormals,
orient_normals_towards_camera_location(centroid), then negates them).  open3d is not needed here:
  1. N(p): the points q with |q - p| < radius, the max_nn nearest if there are more; p itself included.
  2. raw normal: (0, 0, 1) if |N| < 3 or the covariance of N (mean-centred, / |N|) is all zero, else the
     unit eigenvector of its smallest eigenvalue (numpy.linalg.eigh).
  3. with c the centroid: negated if n . (c - p) < 0, then negated once more (points away from c).
  4. keep p iff n . d / |d| >= threshold (d unnormalised when |d| = 0).
Neighbours come from a uniform grid of cells of size radius, searched in chunks of query points, so that a
sample of query points can be checked against a whole 10 M-point cloud.  Besides the normals every query
reports what the tests use to leave a point out: the relative eigengap, the orientation margin, a tie at
the cutoff and a neighbour at the radius.
"""
import numpy as np

TIE_REL = 2e-6        # squared distances this close (relative) count as a tie at the cutoff
BOUNDARY_REL = 1e-5   # a point this close (relative) to the radius counts as on the boundary


class _Grid:
    def __init__(self, xyz, h):
        self.xyz = xyz
        self.h = h
        self.lo = xyz.min(axis=0) if len(xyz) else np.zeros(3)
        cell = np.floor((xyz - self.lo) / h).astype(np.int64)
        self.dim = cell.max(axis=0) + 3 if len(xyz) else np.ones(3, np.int64)
        key = self._key(cell)
        self.order = np.argsort(key, kind="stable")
        self.skey = key[self.order]

    def _key(self, cell):
        c = cell + 1   # a margin of one cell on every side: neighbour cells never wrap
        return c[:, 0] + self.dim[0] * (c[:, 1] + self.dim[1] * c[:, 2])

    def candidates(self, q):
        """(query row, point index) for every point in the 27 cells around each query."""
        cell = np.floor((q - self.lo) / self.h).astype(np.int64)
        cell = np.clip(cell, -1, self.dim - 2)
        rows, idx = [], []
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    key = self._key(cell + np.array([dx, dy, dz]))
                    a = np.searchsorted(self.skey, key, side="left")
                    b = np.searchsorted(self.skey, key, side="right")
                    cnt = b - a
                    tot = int(cnt.sum())
                    if tot == 0:
                        continue
                    r = np.repeat(np.arange(len(q)), cnt)
                    starts = np.repeat(a - np.cumsum(cnt) + cnt, cnt)
                    pos = starts + np.arange(tot)
                    rows.append(r)
                    idx.append(self.order[pos])
        if not rows:
            return np.zeros(0, np.int64), np.zeros(0, np.int64)
        return np.concatenate(rows), np.concatenate(idx)


def centroid(xyz):
    return xyz.astype(np.float64).mean(axis=0) if len(xyz) else np.full(3, np.nan)


def estimate(xyz, radius=0.02, max_nn=30, query=None, chunk=20000):
    """Normals of the points `query` (indices, default all) of the cloud xyz (n, 3) float32, and the facts per query:
    normals (m, 3) f64 final orientation, nn (m,) neighbourhood size, gap (relative eigengap (l1 - l0) / l2, inf where the
    (0, 0, 1) rule decides), orient (|n . (c - p)| / |c - p|), tie (a tie at the cutoff), boundary (a point within
    BOUNDARY_REL of the radius), neighbours (list of index arrays, sorted by distance then index), centroid."""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    pts = xyz.astype(np.float64)
    n = len(pts)
    query = np.arange(n) if query is None else np.asarray(query, dtype=np.int64)
    m = len(query)
    cen = centroid(xyz)
    out = dict(index=query, centroid=cen, normals=np.zeros((m, 3)), nn=np.zeros(m, np.int64), gap=np.full(m, np.inf),
               orient=np.zeros(m), tie=np.zeros(m, bool), boundary=np.zeros(m, bool), neighbours=[None] * m)
    if m == 0:
        return out
    grid = _Grid(pts, radius)
    r2 = radius * radius
    for c0 in range(0, m, chunk):
        qi = query[c0:c0 + chunk]
        q = pts[qi]
        rows, idx = grid.candidates(q)
        d2 = ((pts[idx] - q[rows]) ** 2).sum(axis=1)
        d = np.sqrt(d2)
        near_r = np.abs(d - radius) <= BOUNDARY_REL * radius
        inside = d2 < r2
        np.logical_or.at(out["boundary"][c0:c0 + chunk], rows[near_r], True)
        rows, idx, d2 = rows[inside], idx[inside], d2[inside]
        o = np.lexsort((idx, d2, rows))
        rows, idx, d2 = rows[o], idx[o], d2[o]
        counts = np.bincount(rows, minlength=len(qi))
        first = np.cumsum(counts) - counts
        rank = np.arange(len(rows)) - first[rows]
        for j in range(len(qi)):
            k = counts[j]
            a = first[j]
            kk = min(k, max_nn)
            nb = idx[a:a + kk]
            if k > max_nn:
                dk, dn = d2[a + max_nn - 1], d2[a + max_nn]
                out["tie"][c0 + j] = dn - dk <= TIE_REL * max(dk, 1e-300)
            out["neighbours"][c0 + j] = nb
            out["nn"][c0 + j] = kk
            p = q[j]
            nrm = np.array([0.0, 0.0, 1.0])
            if kk >= 3:
                P = pts[nb]
                C = np.cov(P.T, bias=True)
                if np.any(C != 0):
                    w, v = np.linalg.eigh(C)
                    nrm = v[:, 0] / np.linalg.norm(v[:, 0])
                    out["gap"][c0 + j] = (w[1] - w[0]) / w[2] if w[2] > 0 else 0.0
            tc = float(nrm @ (cen - p))
            if tc < 0:
                nrm = -nrm
            nrm = -nrm
            dist = float(np.linalg.norm(cen - p))
            out["orient"][c0 + j] = abs(tc) / dist if dist > 0 else 0.0
            out["normals"][c0 + j] = nrm
        del rank
    return out


def direction_mask(est, direction, threshold):
    """(keep, margin) per query of `est`: keep iff n . d_hat >= threshold, margin = |n . d_hat - threshold|."""
    d = np.asarray(direction, dtype=np.float64).reshape(3)
    nrm = np.linalg.norm(d)
    if nrm != 0:
        d = d / nrm
    dot = est["normals"] @ d
    return dot >= threshold, np.abs(dot - threshold)


def reliable(est, gap_min=1e-2, orient_min=1e-6):
    """Queries whose normal is well defined: no tie at the cutoff, no point at the radius, an eigengap of at least gap_min
    (or the (0, 0, 1) rule) and an orientation that is not a coin toss."""
    return ~est["tie"] & ~est["boundary"] & (est["gap"] >= gap_min) & (est["orient"] >= orient_min)
