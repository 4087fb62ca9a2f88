"""numpy oracle of the registration analyzer's arithmetic (test infrastructure; needs neither a GPU nor the library).

  * nn_distance2 / nn_distance: brute force, in blocks -- per source point the (nth + 1)-th smallest
        d2 = (dx*dx + dy*dy) + dz*dz,   dx = float64(qx) - float64(px), ...     (every operation rounded on its own)
    among the reference points with d2 < max_distance * max_distance, inf when there are fewer; the distance is numpy.sqrt of it.
    tests/test_analyze_oracle.py pins this to scipy.spatial.KDTree.query(..., k=[nth + 1], distance_upper_bound=...) bit for bit.
  * nn_distance2_grid: the same values for clouds too big for brute force -- the reference points bucketed into coarse cells, a
    query's candidates taken from the 27 cells around it, the answer accepted only if it is closer than the nearest face of that
    block of cells (then nothing outside can undercut it, and the (nth + 1)-th smallest of the same d2 values is the same number);
    otherwise the block is doubled, until it is the whole grid.  tests/test_analyze_oracle.py holds it to the brute force, bit for bit.
  * gaussian_kde: density[j] = sum_i exp(-0.5 ((at[j] - s[i]) / h)^2) / (n h sqrt(2 pi)), h = std(s, ddof=1) * factor, summed by
    numpy (pairwise) over blocks of samples.
  * analyze: the analyzer's reductions over a distance array, with the density estimate of this file.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np


def nn_distance2(source_xyz, reference_xyz, nth=0, max_distance=np.inf, block=512):
    q = np.asarray(source_xyz, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    p = np.asarray(reference_xyz, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    out = np.full(len(q), np.inf)
    if len(p) <= nth or len(q) == 0:
        return out
    max2 = np.float64(max_distance) * np.float64(max_distance)
    block = max(1, min(block, (1 << 22) // len(p)))
    px, py, pz = p[:, 0][None, :], p[:, 1][None, :], p[:, 2][None, :]
    for lo in range(0, len(q), block):
        b = q[lo:lo + block]
        dx, dy, dz = b[:, 0][:, None] - px, b[:, 1][:, None] - py, b[:, 2][:, None] - pz
        d2 = (dx * dx + dy * dy) + dz * dz
        kth = np.partition(d2, nth, axis=1)[:, nth]
        out[lo:lo + block] = np.where(kth < max2, kth, np.inf)
    return out


def nn_distance(source_xyz, reference_xyz, nth=0, max_distance=np.inf, block=512):
    return np.sqrt(nn_distance2(source_xyz, reference_xyz, nth, max_distance, block))


def nn_distance2_grid_many(source_xyz, reference_xyz, nths=(0,), bounds=(np.inf,), per_cell=96):
    """{(nth, bound): squared distances} for every combination, the candidates of a query gathered once per block size."""
    q = np.asarray(source_xyz, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    p = np.asarray(reference_xyz, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    nths = sorted(set(int(n) for n in nths))
    raw = {n: np.full(len(q), np.inf) for n in nths}          # without a bound
    if len(q) and len(p):
        lo, hi = p.min(axis=0), p.max(axis=0)
        ext = max(float((hi - lo).max()), 1e-9)
        # surface-like data: points per occupied cell grow with the square of the cell size
        c = ext / max(1.0, np.sqrt(len(p) / float(per_cell)))
        dim = np.floor((hi - lo) / c).astype(np.int64) + 1
        cell = np.minimum(np.floor((p - lo) / c).astype(np.int64), dim - 1)
        key = cell[:, 0] + dim[0] * (cell[:, 1] + dim[1] * cell[:, 2])
        order = np.argsort(key, kind="stable")
        ps, keys = p[order], key[order]
        qc = np.clip(np.floor((q - lo) / c).astype(np.int64), 0, dim - 1)      # a query outside the box starts from the nearest cell
        d0, d1, d2_ = int(dim[0]), int(dim[1]), int(dim[2])
        for i in range(len(q)):
            cx, cy, cz = int(qc[i, 0]), int(qc[i, 1]), int(qc[i, 2])
            todo = list(nths)
            radius = 1
            while todo:
                # the block of cells `radius` around the query's: how far it reaches along every axis before cells that were left
                # out begin (a little less is claimed: rounding); a side where the block has reached the grid's edge leaves nothing out
                reach = np.inf
                for a, (cc, dd) in enumerate(((cx, d0), (cy, d1), (cz, d2_))):
                    if cc - radius > 0:
                        reach = min(reach, q[i, a] - (lo[a] + (cc - radius) * c))
                    if cc + radius < dd - 1:
                        reach = min(reach, lo[a] + (cc + radius + 1) * c - q[i, a])
                reach2 = reach * reach * (1 - 1e-9) if np.isfinite(reach) else np.inf
                x0, x1 = max(cx - radius, 0), min(cx + radius, d0 - 1)
                zz, yy = np.meshgrid(np.arange(max(cz - radius, 0), min(cz + radius, d2_ - 1) + 1),
                                     np.arange(max(cy - radius, 0), min(cy + radius, d1 - 1) + 1), indexing="ij")
                rows = (d0 * (yy + d1 * zz)).reshape(-1)
                first, last = np.searchsorted(keys, rows + x0), np.searchsorted(keys, rows + (x1 + 1))
                take = last > first
                if take.any():
                    cand = np.concatenate([ps[a:b] for a, b in zip(first[take], last[take])])
                    dx, dy, dz = q[i, 0] - cand[:, 0], q[i, 1] - cand[:, 1], q[i, 2] - cand[:, 2]
                    d2 = (dx * dx + dy * dy) + dz * dz
                    have = [n for n in todo if n < len(d2)]
                    part = np.partition(d2, have) if have else d2
                    for n in list(todo):
                        if n < len(d2) and (part[n] < reach2 or reach2 == np.inf):
                            raw[n][i] = part[n]
                            todo.remove(n)
                if reach2 == np.inf:
                    break          # the block was the whole grid: what is still to do has no answer
                radius *= 2
    out = {}
    for n in nths:
        for bound in bounds:
            max2 = np.float64(bound) * np.float64(bound)
            out[(n, bound)] = np.where(raw[n] < max2, raw[n], np.inf)
    return out


def nn_distance2_grid(source_xyz, reference_xyz, nth=0, max_distance=np.inf, per_cell=96):
    return nn_distance2_grid_many(source_xyz, reference_xyz, (nth,), (max_distance,), per_cell)[(int(nth), max_distance)]


def bandwidth(samples, bw_method=None):
    s = np.asarray(samples, dtype=np.float64).reshape(-1)
    n = s.size
    if bw_method is None or bw_method == "scott":
        factor = float(n) ** -0.2
    elif bw_method == "silverman":
        factor = (float(n) * 3.0 / 4.0) ** -0.2
    else:
        factor = float(bw_method)
    return float(np.std(s, ddof=1)) * factor


def gaussian_kde_h(samples, h, at):
    s = np.asarray(samples, dtype=np.float64).reshape(-1)
    x = np.asarray(at, dtype=np.float64).reshape(-1)
    # blocks of samples (about 4 M terms each), summed by numpy and added up in their order; the threads only share the work
    block = max(256, (1 << 22) // max(len(x), 1))

    def part(lo):
        z = (x[:, None] - s[None, lo:lo + block]) / h
        return np.exp(-0.5 * z * z).sum(axis=1)

    total = np.zeros(len(x))
    with ThreadPoolExecutor(max_workers=max(1, min(16, os.cpu_count() or 1))) as pool:
        for piece in pool.map(part, range(0, len(s), block)):
            total += piece
    return total / (len(s) * h * np.sqrt(2 * np.pi))


def gaussian_kde(samples, at, bw_method=None):
    return gaussian_kde_h(samples, bandwidth(samples, bw_method), at)


def trim_mean(a, proportiontocut):
    a = np.asarray(a)
    lowercut = int(proportiontocut * a.shape[0])
    uppercut = a.shape[0] - lowercut
    part = np.partition(a, (lowercut, uppercut - 1))
    return np.mean(part[lowercut:uppercut])


def analyze(raw_distances, source_count, reference_count, measure="mean", others=(), use_kde=True, bincount=400, binsize=0.0,
            symmetric=False):
    """The analyzer's result fields, as a dict, from the distances of one run (inf where there was no correspondence)."""
    d = np.asarray(raw_distances, dtype=np.float64).reshape(-1)
    d = d[np.isfinite(d)]
    r = dict(minCorrespondence=0, minCorrespondenceCount=0, mean=None, stddev=None, tmean=None, mode=None, median=None,
             sourcePointCount=source_count, referencePointCount=reference_count, histogram=None, histogramEdges=None, ok=False)
    if d.min() == d.max():
        r.update(minCorrespondence=d[0], minCorrespondenceCount=len(d), histogram=np.array([d[0]]), histogramEdges=np.array([d[0], d[0]]))
        return r
    if binsize > 0:
        bincount = int((d.max() - 0) / binsize)
    if use_kde:
        edges = np.linspace(0, d.max(), bincount + 1)
        hist = gaussian_kde(d, edges[1:])
    else:
        hist, edges = np.histogram(d, bins=bincount)
    r["histogram"], r["histogramEdges"] = hist, edges
    wanted = list(others)
    if measure not in wanted:
        wanted.append(measure)
    if "median" in wanted:
        r["median"] = float(np.median(d))
    if "mean" in wanted:
        r["mean"], r["stddev"] = float(np.mean(d)), float(np.std(d))
    if "tmean" in wanted:
        r["tmean"] = float(trim_mean(d, 0.1))
    if "mode" in wanted or "2mode" in wanted:
        r["mode"] = edges[np.argmax(hist) + 1]
    if measure in ("mean", "tmean", "median", "mode"):
        value = r[measure]
    elif measure == "2mode":
        value = 2 * r["mode"]
    else:
        assert measure.startswith("q=")
        value = float(np.percentile(d, int(measure[2:])))
    r["minCorrespondence"] = value
    r["minCorrespondenceCount"] = int(np.count_nonzero(d <= value))
    if symmetric:
        r["sourcePointCount"] = r["referencePointCount"] = source_count + reference_count
    r["ok"] = True
    return r
