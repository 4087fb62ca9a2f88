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

estimate() is the model of the reference's open3d call: its distances are f64, so it cannot say what the kernel does at a tie at
the cutoff or at a point near the radius, and flags those queries.  estimate_exact() restates the KERNEL's definition of the
neighbourhood instead (FLANN's float32 distance, the float32 radius^2, every tied point in): it predicts nn for every query, and
gives the normal of the kernel's own fixed-point matrix next to the f64 covariance's.  Vectorised over the candidate pairs.
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


DIR_FIX = 1048576.0   # the kernel's fixed-point units per cutoff distance (2^20)
PAIR_BUDGET = 6_000_000   # candidate pairs expanded at a time


def flann_d2(q32, p32):
    """FLANN L2_Simple<float>: (dx*dx + dy*dy) + dz*dz, every operation rounded to float32 on its own."""
    d = q32 - p32
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def r2_of(radius):
    r = np.float32(radius)
    return np.float32(r * r)


def _candidate_pairs(grid, q, budget=PAIR_BUDGET):
    """Yields (j0, j1, rows, idx): the candidates (27 cells) of the queries q[j0:j1], rows relative to j0, at most about `budget`
    pairs at a time."""
    cell = np.floor((q - grid.lo) / grid.h).astype(np.int64)
    cell = np.clip(cell, -1, grid.dim - 2)
    offs = [np.array([dx, dy, dz]) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    lo = np.empty((27, len(q)), np.int64)
    cnt = np.empty((27, len(q)), np.int64)
    for o, off in enumerate(offs):
        key = grid._key(cell + off)
        lo[o] = np.searchsorted(grid.skey, key, side="left")
        cnt[o] = np.searchsorted(grid.skey, key, side="right") - lo[o]
    per = cnt.sum(axis=0)
    cum = np.cumsum(per)
    j0 = 0
    while j0 < len(q):
        base = cum[j0 - 1] if j0 else 0
        j1 = max(int(np.searchsorted(cum, base + budget, side="right")), j0 + 1)
        a, c = lo[:, j0:j1].ravel(), cnt[:, j0:j1].ravel()
        tot = int(c.sum())
        rows = np.repeat(np.tile(np.arange(j1 - j0), 27), c)
        pos = np.repeat(a - np.cumsum(c) + c, c) + np.arange(tot)
        yield j0, j1, rows, grid.order[pos]
        j0 = j1


def exact_neighbourhoods(xyz, radius=0.02, max_nn=30, query=None):
    """The kernel's DEFINITION of the neighbourhood, for every query, no exclusions: with d2 FLANN's float32 distance, r2 the
    float32 product radius * radius and cutoff the max_nn-th smallest d2 under r2 (r2 if there are fewer),
    N(p) = {q : d2 <= cutoff and d2 < r2} -- every point tied at the cutoff is in, so |N| may exceed max_nn.
    Returns (rows, idx, d2, cutoff): pairs sorted by query row then d2 then index, and the float32 cutoff per query.
    Candidates come from the f64 bucket grid (cells a little wider than the radius, 27 cells around the query)."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    n = len(xyz)
    query = np.arange(n) if query is None else np.asarray(query, dtype=np.int64)
    r2 = r2_of(radius)
    pts = xyz.astype(np.float64)
    # float32 rounding can put a point whose true distance is a few 1e-7 beyond the radius under r2: cells wider by 1e-5
    grid = _Grid(pts, float(np.float32(radius)) * (1.0 + 1e-5))
    out_rows, out_idx, out_d2 = [], [], []
    cutoff = np.full(len(query), r2, np.float32)
    for j0, j1, rows, idx in _candidate_pairs(grid, pts[query]):
        d2 = flann_d2(xyz[query[j0:j1]][rows], xyz[idx])
        inside = d2 < r2
        rows, idx, d2 = rows[inside], idx[inside], d2[inside]
        # one sort of (row, d2) as one integer key finds the cutoffs (a non-negative float32 orders as its bits do); only the
        # few pairs at or under them are then put in order
        key = np.sort((rows.astype(np.uint64) << np.uint64(32)) | d2.view(np.uint32).astype(np.uint64))
        counts = np.bincount(rows, minlength=j1 - j0)
        first = np.cumsum(counts) - counts
        full = counts >= max_nn
        cut = np.full(j1 - j0, r2, np.float32)
        cut[full] = (key[first[full] + max_nn - 1] & np.uint64(0xffffffff)).astype(np.uint32).view(np.float32)
        cutoff[j0:j1] = cut
        keep = d2 <= cut[rows]
        rows, idx, d2 = rows[keep], idx[keep], d2[keep]
        o = np.lexsort((idx, d2, rows))
        rows, idx, d2 = rows[o], idx[o], d2[o]
        out_rows.append(rows + j0)
        out_idx.append(idx)
        out_d2.append(d2)
    if not out_rows:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32), cutoff
    return np.concatenate(out_rows), np.concatenate(out_idx), np.concatenate(out_d2), cutoff


def _sum_rows(values, first, counts):
    """Per-row sums of values (pairs sorted by row; first / counts per row), exact for integers; empty rows give 0."""
    out = np.zeros((len(first),) + values.shape[1:], values.dtype)
    has = counts > 0
    if has.any():
        out[has] = np.add.reduceat(values, first[has], axis=0)
    return out


def _smallest_eigvec_eigh(A, ok):
    """Unit eigenvector of the smallest eigenvalue (numpy.linalg.eigh) of the matrices A[ok], (0, 0, 1) elsewhere; also the
    relative eigengap (w1 - w0) / w2 (inf where not ok, 0 where w2 <= 0) and w1 - w0 itself."""
    m = len(A)
    nrm = np.tile([0.0, 0.0, 1.0], (m, 1))
    gap = np.full(m, np.inf)
    split = np.full(m, np.inf)
    if ok.any():
        w, v = np.linalg.eigh(A[ok])
        v0 = v[:, :, 0]
        nrm[ok] = v0 / np.linalg.norm(v0, axis=1, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            gap[ok] = np.where(w[:, 2] > 0, (w[:, 1] - w[:, 0]) / w[:, 2], 0.0)
        split[ok] = w[:, 1] - w[:, 0]
    return nrm, gap, split


def _orient(nrm, p, cen):
    """The final orientation (towards the centroid, then negated) and the margin |n . (c - p)| / |c - p|."""
    tc = (nrm * (cen - p)).sum(axis=1)
    out = np.where((tc < 0)[:, None], nrm, -nrm)
    dist = np.linalg.norm(cen - p, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = np.where(dist > 0, np.abs(tc) / dist, 0.0)
    return out, margin


def quantised_matrix(d, cutoff, first, counts):
    """The kernel's matrix cnt * S2 - S1 S1^T from offsets d (pairs, f64: neighbour - query) in fixed point, 2^-20 of the cutoff
    distance: integer sums (exact, as the kernel's int64), then the kernel's f64 operations.  (m, 3, 3) float64."""
    rows = np.repeat(np.arange(len(first)), counts)
    c64 = cutoff.astype(np.float64)
    with np.errstate(divide="ignore"):
        scale = np.where(c64 > 0, DIR_FIX / np.sqrt(c64), 0.0)
    u = np.rint(d * scale[rows][:, None]).astype(np.int64)
    s1 = _sum_rows(u, first, counts).astype(np.float64)
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    s2 = _sum_rows(np.stack([u[:, a] * u[:, b] for a, b in pairs], axis=1), first, counts).astype(np.float64)
    m = counts.astype(np.float64)
    A = np.empty((len(first), 3, 3))
    for k, (a, b) in enumerate(pairs):
        A[:, a, b] = A[:, b, a] = m * s2[:, k] - s1[:, a] * s1[:, b]
    return A


def estimate_exact(xyz, radius=0.02, max_nn=30, query=None, cen=None):
    """As estimate(), on the kernel's exactly defined neighbourhood (exact_neighbourhoods): nn is what the kernel must give for
    EVERY query.  Two normals per query, both in their final orientation:
      normals_q  from the kernel's own matrix (quantised_matrix) through numpy.linalg.eigh: only the kernel's eigen-solver and
                 its float32 store separate the kernel's normal from this one
      normals    from the f64 covariance of N(p) (mean-centred, / |N|), as estimate()
    gap and orient as estimate() (of the unquantised normal), gap_q the quantised matrix's, split the covariance's w1 - w0.  nb_rows / nb_index / nb_first: the
    neighbourhoods as sorted pairs.  cen: the centroid to orient against (default: the cloud's f64 mean)."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    pts = xyz.astype(np.float64)
    n = len(pts)
    query = np.arange(n) if query is None else np.asarray(query, dtype=np.int64)
    m = len(query)
    cen = centroid(xyz) if cen is None else np.asarray(cen, dtype=np.float64)
    rows, idx, d2, cutoff = exact_neighbourhoods(xyz, radius, max_nn, query)
    counts = np.bincount(rows, minlength=m)
    first = np.cumsum(counts) - counts
    p = pts[query]
    d = pts[idx] - p[rows]
    enough = counts >= 3
    # quantised: the kernel's matrix
    Aq = quantised_matrix(d, cutoff, first, counts)
    nq, gap_q, _ = _smallest_eigvec_eigh(Aq, enough & np.any(Aq != 0, axis=(1, 2)))
    # unquantised: the f64 covariance
    k = np.maximum(counts, 1).astype(np.float64)
    centred = d - (_sum_rows(d, first, counts) / k[:, None])[rows]
    C = _sum_rows(centred[:, :, None] * centred[:, None, :], first, counts) / k[:, None, None]
    nu, gap, split = _smallest_eigvec_eigh(C, enough & np.any(C != 0, axis=(1, 2)))
    normals_q, orient_q = _orient(nq, p, cen)
    normals, orient = _orient(nu, p, cen)
    return dict(index=query, centroid=cen, normals=normals, normals_q=normals_q, raw=nu, raw_q=nq, nn=counts, gap=gap, gap_q=gap_q, split=split,
                orient=np.minimum(orient, orient_q), cutoff=cutoff, nb_rows=rows, nb_index=idx, nb_first=first, nb_d2=d2)


def neighbours_of(est, j):
    a = est["nb_first"][j]
    return est["nb_index"][a:a + est["nn"][j]]


def direction_mask(est, direction, threshold, normals="normals"):
    """(keep, margin) per query of `est`: keep iff n . d_hat >= threshold, margin = |n . d_hat - threshold|."""
    d = np.asarray(direction, dtype=np.float64).reshape(3)
    nrm = np.linalg.norm(d)
    if nrm != 0:
        d = d / nrm
    dot = est[normals] @ d
    return dot >= threshold, np.abs(dot - threshold)


def reliable(est, gap_min=1e-2, orient_min=1e-6):
    """Queries whose normal is well defined: an eigengap of at least gap_min (or the (0, 0, 1) rule) and an orientation that is
    not a coin toss -- and, for the f64 estimate() only, which cannot say what happens there: no tie at the cutoff, no point at the
    radius."""
    good = (est["gap"] >= gap_min) & (est["orient"] >= orient_min)
    if "tie" in est:
        good &= ~est["tie"] & ~est["boundary"]
    return good
