"""The exact grid walk (csrc/exact_walk.hpp: cell_of, GridRows<SPARSE>::range, walk_exact) compiled for the host as a stand-alone
program (tests/abi/exact_walk_host.cpp, its own main) with -ffp-contract=off -fsanitize=address,undefined, on grids that the TEST
decides -- the GPU tests cannot put reference points on cell faces, the grid's h is decided on the device.  The program builds the
dense or the sparse cell arrays itself, runs walk_exact per query with icp_correspond_kernel's candidate rule (`nearest`) or
nn_distance2_kernel's sorted list (`kth`), and writes the answer and every scan(first, last) call with limit() at its entry.  CPU
only; the host C++ compiler is required (a missing one fails the tests).

Held against brute force in f64 (icp_model.correspondences, analyze_oracle.nn_distance2: the squared value that nn_distance takes the
root of), bit for bit:
  * value and index: idx and d2 equal the model's; the kth distance equals the model's for want in 1, 2, 4, 32;
  * completeness: every reference point with d2 <= min(answer, max2) was scanned, when that minimum is finite -- a tie in another
    cell is always seen (walk_exact's "every bound is short");
  * no point is scanned twice (how often each sorted element was scanned is what the scan records say: the ranges are the counts);
  * necessity: every scanned element lies in a row of cells whose y-z distance from the query is under the limit() recorded at that
    scan's entry.  Per axis the row distance is max(gap - 2e-6 h, 0) from the cell's faces in f64: the walk states its bounds short
    by 1e-6 of a cell plus 1e-9 of themselves, which on grids of a few dozen cells is far less than another 1e-6 of a cell, so twice
    1e-6 h is derived from the walk's statement, not measured;
  * the dense and the sparse layout walk the same elements: the two outputs are the same bytes.

A third mode, `within`, is cluster_link_kernel's use of the walk (kernels_cluster.hip): a constant limit() = max2 and every candidate
with d2 < max2 taken.  Per query the count, the sum and the xor of the indices taken equal brute force's (check_within, on every case
above): a missed candidate that is not the nearest passes `nearest` and `kth`, and changes all three here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import analyze_oracle as ao
import icp_model as im

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANTS = (1, 2, 4, 32)
ANSWER = np.dtype([("idx", "<u4"), ("scans", "<u4"), ("d2", "<f8")])
SCAN = np.dtype([("first", "<u4"), ("last", "<u4"), ("limit", "<f8")])
WITHIN = np.dtype([("count", "<u4"), ("scans", "<u4"), ("sum", "<u4"), ("xor", "<u4")])     # the `within` mode's use of an answer's 16 bytes


class Grid:
    def __init__(self, mn, dim, h):
        self.mn = np.asarray(mn, dtype=np.float32)
        self.dim = np.asarray(dim, dtype=np.int64)
        self.h = float(h)
        self.inv_h = 1.0 / self.h      # as the library's grid_dims

    def face(self, axis, k):
        """the k-th face along axis, in f64: what the walk measures from"""
        return np.float64(self.mn[axis]) + np.asarray(k, dtype=np.float64) * self.h

    def coord(self, v, axis):
        """floor((v - mn) * inv_h) in f64, clamped: the cell of a coordinate"""
        c = np.floor((np.asarray(v, dtype=np.float64) - np.float64(self.mn[axis])) * self.inv_h)
        return np.clip(c, 0, self.dim[axis] - 1).astype(np.int64)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: exact_walk.hpp cannot be checked"
    d = tmp_path_factory.mktemp("exact_walk")
    exe = str(d / "exact_walk_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cwipc_util_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "exact_walk_host.cpp"), "-o", exe], check=True)

    def run(grid, ref, queries, max2, mode, kind, want=1, seed=0):
        """One run of the program.  The points go in shuffled, each with its model index: neither the file's order nor the sorted
        order is the index.  -> (raw bytes, ids of the sorted points, answers, scans)"""
        ref = np.asarray(ref, dtype=np.float32).reshape(-1, 3)
        queries = np.asarray(queries, dtype=np.float32).reshape(-1, 3)
        max2 = np.broadcast_to(np.asarray(max2, dtype=np.float64), (len(queries),))
        inp, out = str(d / "case.bin"), str(d / "out.bin")
        shuffle = np.random.default_rng(seed).permutation(len(ref))
        pts = np.zeros(len(ref), dtype=[("xyz", "<f4", 3), ("id", "<u4")])
        pts["xyz"], pts["id"] = ref[shuffle], shuffle
        with open(inp, "wb") as f:
            f.write(np.array([0x4B4C5758, len(ref), len(queries), *grid.dim, 0, 0], dtype="<i4").tobytes())
            f.write(np.array([*grid.mn, 0], dtype="<f4").tobytes())
            f.write(np.array([grid.h, grid.inv_h], dtype="<f8").tobytes())
            f.write(pts.tobytes())
            f.write(queries.astype("<f8").tobytes())
            f.write(max2.astype("<f8").tobytes())
        subprocess.run([exe, inp, out, mode, kind, str(want)], check=True, timeout=300)
        raw = open(out, "rb").read()
        n, nq = len(ref), len(queries)
        ids = np.frombuffer(raw, dtype="<u4", count=n)
        answers = np.frombuffer(raw, dtype=ANSWER, count=nq, offset=4 * n)
        scans = np.frombuffer(raw, dtype=SCAN, offset=4 * n + 16 * nq)
        assert len(raw) == 4 * n + 16 * nq + 16 * int(answers["scans"].sum(dtype=np.int64))
        return raw, ids, answers, scans
    return run


def check_trace(grid, ref, queries, max2, ids, answers, scans, near, near_reach):
    """Completeness (near, near_reach: near_pairs and the reach it was made for), no point twice, necessity -- from the scan records of one run.  -> the number of scanned candidates"""
    ref = np.asarray(ref, dtype=np.float32).reshape(-1, 3)
    q = np.asarray(queries, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    max2 = np.broadcast_to(np.asarray(max2, dtype=np.float64), (len(q),))
    n, nq = len(ref), len(q)
    # the sorted points are the reference points, each once, in the order of their cells (x fastest)
    assert np.array_equal(np.sort(ids), np.arange(n, dtype=np.uint32))
    p = ref[ids].astype(np.float64)
    cell = [grid.coord(p[:, a], a) for a in range(3)]
    flat = cell[0] + grid.dim[0] * (cell[1] + grid.dim[1] * cell[2])
    assert np.all(np.diff(flat) >= 0)
    # every scanned (query, element), with the limit at its scan's entry
    first, last = scans["first"].astype(np.int64), scans["last"].astype(np.int64)
    assert np.all(first <= last) and np.all(last <= n)
    length = last - first
    scan_q = np.repeat(np.arange(nq), answers["scans"].astype(np.int64))
    which = np.repeat(np.arange(len(scans)), length)
    elem = first[which] + (np.arange(int(length.sum())) - np.repeat(np.cumsum(length) - length, length))
    qid, limit = scan_q[which], scans["limit"][which]
    keys = np.sort(qid * n + elem)
    assert np.all(np.diff(keys) > 0), "a point was scanned twice"
    # necessity: the element's row of cells, from its faces in f64, each axis short by 2e-6 h
    row2 = np.zeros(len(elem))
    for a in (1, 2):
        c = cell[a][elem]
        gap = np.maximum(np.maximum(grid.face(a, c) - q[qid, a], q[qid, a] - grid.face(a, c + 1)), 0.0)
        t = np.maximum(gap - 2e-6 * grid.h, 0.0)
        row2 += t * t
    needless = ~(row2 < limit)
    assert not needless.any(), "%d of %d scanned candidates lie in rows beyond limit()" % (int(needless.sum()), len(elem))
    # completeness: all of brute force's points up to the answer were scanned
    reach = np.minimum(answers["d2"], max2)
    pq, pj, pd = near
    assert np.all(reach[np.isfinite(reach)] <= near_reach[np.isfinite(reach)])     # (the shared pairs reach as far as this run's answers)
    must = pd <= reach[pq]                 # (an infinite reach asks nothing: the pairs only go as far as a finite one)
    must &= np.isfinite(reach[pq])
    pos = np.empty(n, dtype=np.int64)
    pos[ids] = np.arange(n)
    need = pq[must] * n + pos[pj[must]]
    at = np.minimum(np.searchsorted(keys, need), max(len(keys) - 1, 0))
    seen = keys[at] == need if len(keys) else np.zeros(len(need), dtype=bool)
    assert seen.all(), "%d points at or under the answer were never scanned" % int((~seen).sum())
    return len(elem)


def unbounded_model(queries, ref, wants=WANTS):
    """(idx, d2, {want: kth d2}) of the two brute-force models without a bound"""
    widx, wd2 = im.correspondences(queries, ref, None, np.inf)
    return widx, wd2, {w: ao.nn_distance2(queries, ref, w - 1, np.inf) for w in wants}


def bounded_model(base, queries, ref, max2, every):
    """The models' answers under max2, from their unbounded answers: both compare a candidate with max2 strictly and change nothing
    else (icp_model: dd[~(dd < max2)] = inf before the argmin; analyze_oracle: where(kth < max2, kth, inf)), so the bound decides
    only whether the unbounded answer stands.  The models called WITH the bound say the same on every `every`-th query (all of
    them for every = 1); max_distance is the root of max2, which squares back to the very double."""
    widx, wd2, kth = base
    gone = ~(wd2 < max2)
    idx, d2 = np.where(gone, np.uint32(im.NONE), widx), np.where(gone, np.inf, wd2)
    kk = {w: np.where(v < max2, v, np.inf) for w, v in kth.items()}
    for m2 in np.unique(max2):
        sel = np.flatnonzero(max2 == m2)[::every]
        maxd = np.sqrt(m2)
        assert maxd * maxd == m2
        i, d = im.correspondences(queries[sel], ref, None, maxd)
        assert np.array_equal(i, idx[sel]) and d.tobytes() == d2[sel].tobytes()
        for w in kk:
            assert ao.nn_distance2(queries[sel], ref, w - 1, maxd).tobytes() == kk[w][sel].tobytes()
    return idx, d2, kk


def near_pairs(queries, ref, reach):
    """(query, reference point, d2) of every pair with d2 <= reach[query], by brute force in f64: what a run must have scanned is a
    subset of these, whichever of the runs it is"""
    q, r = queries.astype(np.float64), ref.astype(np.float64)
    out = []
    for lo in range(0, len(q), 4096):
        b = q[lo:lo + 4096]
        dx, dy, dz = b[:, None, 0] - r[None, :, 0], b[:, None, 1] - r[None, :, 1], b[:, None, 2] - r[None, :, 2]
        dd = (dx * dx + dy * dy) + dz * dz
        qq, jj = np.nonzero(dd <= reach[lo:lo + 4096, None])
        out.append((qq + lo, jj, dd[qq, jj]))
    return tuple(np.concatenate(v) for v in zip(*out))


def check_within(host, grid, ref, queries, max2, seed=0):
    """The `within` mode -- the clusters' link kernel's use of the walk: a constant limit, EVERY candidate with d2 < max2 taken --
    against brute force in f64: per query the count, the sum and the xor of the original indices taken.  A missed candidate that is
    not the nearest, which `nearest` and `kth` both let pass, changes all three; a range scanned twice changes the count.  Dense and
    sparse: the same bytes.  -> the number of candidates taken"""
    ref = np.asarray(ref, dtype=np.float32).reshape(-1, 3)
    queries = np.asarray(queries, dtype=np.float32).reshape(-1, 3)
    max2 = np.ascontiguousarray(np.broadcast_to(np.asarray(max2, dtype=np.float64), (len(queries),)))
    q, r = queries.astype(np.float64), ref.astype(np.float64)
    idx = np.arange(len(ref), dtype=np.int64)
    count, total, xor = (np.zeros(len(q), dtype=np.int64) for _ in range(3))
    for lo in range(0, len(q), 4096):
        b = q[lo:lo + 4096]
        dx, dy, dz = b[:, None, 0] - r[None, :, 0], b[:, None, 1] - r[None, :, 1], b[:, None, 2] - r[None, :, 2]
        take = ((dx * dx + dy * dy) + dz * dz) < max2[lo:lo + 4096, None]
        count[lo:lo + 4096] = take.sum(axis=1)
        total[lo:lo + 4096] = (take * idx[None, :]).sum(axis=1)
        xor[lo:lo + 4096] = np.bitwise_xor.reduce(np.where(take, idx[None, :], 0), axis=1) if len(ref) else 0
    raw, ids, answers, scans = host(grid, ref, queries, max2, "dense", "within", seed=seed)
    got = answers.view(WITHIN)
    assert np.array_equal(np.sort(ids), np.arange(len(ref), dtype=np.uint32))
    assert np.array_equal(got["count"], count), (int(np.sum(got["count"] != count)), int((got["count"].astype(np.int64) - count).max()))
    assert np.array_equal(got["sum"], total & 0xFFFFFFFF) and np.array_equal(got["xor"], xor)
    assert scans["limit"].tobytes() == np.repeat(max2, got["scans"].astype(np.int64)).tobytes()      # the limit never moves
    assert host(grid, ref, queries, max2, "sparse", "within", seed=seed)[0] == raw
    return int(count.sum())


def check_case(host, grid, ref, queries, max2, wants=WANTS, trace_wants=WANTS, seed=0, base=None, every=1):
    """All of the module's assertions for one grid, reference, queries and bounds.  -> scanned candidates of the traced runs"""
    ref = np.asarray(ref, dtype=np.float32).reshape(-1, 3)
    queries = np.asarray(queries, dtype=np.float32).reshape(-1, 3)
    max2 = np.ascontiguousarray(np.broadcast_to(np.asarray(max2, dtype=np.float64), (len(queries),)))
    widx, wd2, kth = bounded_model(base or unbounded_model(queries, ref, wants), queries, ref, max2, every)
    # the furthest that any run's answer reaches, where it is finite
    reaches = np.stack([np.minimum(v, max2) for v in [wd2] + [kth[w] for w in wants]])
    near_reach = np.where(np.isfinite(reaches), reaches, -np.inf).max(axis=0)
    near = near_pairs(queries, ref, near_reach)
    scanned = 0
    raw, ids, answers, scans = host(grid, ref, queries, max2, "dense", "nearest", seed=seed)
    assert np.array_equal(answers["idx"], widx), int(np.sum(answers["idx"] != widx))
    assert answers["d2"].tobytes() == wd2.tobytes()
    scanned += check_trace(grid, ref, queries, max2, ids, answers, scans, near, near_reach)
    assert host(grid, ref, queries, max2, "sparse", "nearest", seed=seed)[0] == raw
    for w in wants:
        raw, ids, answers, scans = host(grid, ref, queries, max2, "dense", "kth", w, seed=seed)
        assert answers["d2"].tobytes() == kth[w].tobytes(), (w, int(np.sum(answers["d2"] != kth[w])))
        if w == 1:
            assert answers["d2"].tobytes() == wd2.tobytes()
        if w in trace_wants:
            scanned += check_trace(grid, ref, queries, max2, ids, answers, scans, near, near_reach)
        assert host(grid, ref, queries, max2, "sparse", "kth", w, seed=seed)[0] == raw
    check_within(host, grid, ref, queries, max2, seed=seed)
    return scanned


# ---------------------------------------------------------------------------
# the dyadic lattice: every second reference point on a face, ties of 2, 4 and 8 across faces
# ---------------------------------------------------------------------------
LATTICE_MN, LATTICE_H = (1.0, 0.5, -1.0), 1.0 / 8


def axis_values(lo, cells, step, outside):
    """lo - outside cells ... lo + (cells + outside) cells, in steps of `step` (all dyadic: exact in float32)"""
    k = np.arange(int(round((cells + 2 * outside) * LATTICE_H / step)) + 1)
    return lo - outside * LATTICE_H + k * step


def product(xs, ys, zs):
    return np.stack(np.meshgrid(xs, ys, zs, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)


_LATTICE = {}


def lattice_case(dim, duplicated):
    """(reference, queries, the models' unbounded answers) of one lattice, made once for its three bounds"""
    if (dim, duplicated) not in _LATTICE:
        lat = product(*[axis_values(LATTICE_MN[a], dim[a], 1 / 16, 0) for a in range(3)])
        queries = product(*[axis_values(LATTICE_MN[a], dim[a], 1 / 32, 2) for a in range(3)])
        assert len(lat) == np.prod(2 * np.array(dim) + 1) and len(queries) == np.prod(4 * (np.array(dim) + 4) + 1)
        rng = np.random.default_rng(sum(dim) + 7 * duplicated)
        ref = np.concatenate([lat, lat]) if duplicated else lat
        ref = np.ascontiguousarray(ref[rng.permutation(len(ref))])
        _LATTICE[(dim, duplicated)] = (ref, queries, unbounded_model(queries, ref))
    return _LATTICE[(dim, duplicated)]


@pytest.mark.parametrize("max2", [np.inf, (1 / 32) ** 2, (1 / 16) ** 2], ids=["inf", "1/32", "1/16"])
@pytest.mark.parametrize("duplicated", [False, True], ids=["plain", "duplicated"])
@pytest.mark.parametrize("dim", [(4, 4, 4), (4, 1, 4), (4, 1, 1), (1, 4, 4)], ids=lambda d: "x".join(map(str, d)))
def test_dyadic_lattice(host, dim, duplicated, max2):
    """Grid mn = (1, 0.5, -1), h = 1/8.  Reference: the lattice of spacing 1/16 over the grid's box (every second point on a face),
    plain or twice, its indices permuted.  Queries: the lattice of spacing 1/32 from two cells outside the box to two cells outside
    on the other side -- on points, on faces, between 2, 4 and 8 equally distant points, outside along one, two and three axes.
    max2 of (1/32)^2 and (1/16)^2 are lattice distances: candidates AT them are excluded, strictly."""
    grid = Grid(LATTICE_MN, dim, LATTICE_H)
    ref, queries, base = lattice_case(dim, duplicated)
    # with a bound the walks are short and every list width is traced; without one a trace is the whole grid per query: the
    # widths at the two ends
    scanned = check_case(host, grid, ref, queries, max2, trace_wants=WANTS if np.isfinite(max2) else (1, 32), base=base, every=16)
    print("lattice %s, %d points, %d queries: %d scanned candidates checked" % (dim, len(ref), len(queries), scanned))
    if np.isfinite(max2):
        # every candidate under a constant limit: at the tie distance itself (check_case above) the equally distant ones are all left
        # out, one step above it they are all taken -- 2, 4 or 8 more per query that sits between lattice points
        at, above = check_within(host, grid, ref, queries, max2), check_within(host, grid, ref, queries, np.nextafter(max2, 1))
        assert above >= at + 2 * len(ref)
    # the construction: the model's answers hold ties of 2, 4 and 8 (twice that with duplicates), across faces
    if np.isinf(max2):
        r, q = ref.astype(np.float64), queries[::7].astype(np.float64)
        dd = ((q[:, None, :] - r[None]) ** 2).sum(axis=2)
        ties = (dd == dd.min(axis=1, keepdims=True)).sum(axis=1) // (2 if duplicated else 1)
        assert {1, 2}.issubset(set(ties.tolist())) and (dim[1] == 1 or {4, 8}.issubset(set(ties.tolist())))


# ---------------------------------------------------------------------------
# random grids
# ---------------------------------------------------------------------------
def test_random_grids(host):
    """Dims 1 to 9 per axis (one axis forced to 1 in a fifth of the grids), 1 to 40 points with a third of the coordinates snapped to
    faces, queries from half a box outside to half a box beyond, finite and infinite max2 mixed, want beyond the number of points."""
    rng = np.random.default_rng(20240)
    scanned = flat = fewer = 0
    for trial in range(40):
        dim = rng.integers(1, 10, size=3)
        if trial % 5 == 0:
            dim[rng.integers(0, 3)] = 1
            flat += 1
        h = float(rng.choice([1 / 8, 1 / 4, 0.1, float(np.float32(0.07)), rng.uniform(0.05, 0.5)]))
        grid = Grid(rng.uniform(-2, 2, size=3).astype(np.float32), dim, h)
        n = int(rng.integers(1, 41))
        fewer += n < 32
        ext = dim * h
        ref = np.float64(grid.mn) + rng.uniform(0, 1, size=(n, 3)) * ext
        snap = rng.uniform(size=(n, 3)) < 1 / 3
        faces = np.stack([grid.face(a, rng.integers(0, dim[a] + 1, size=n)) for a in range(3)], axis=1)
        ref = np.where(snap, faces, ref).astype(np.float32)
        # float32 rounding may put a point on the box's face a hair outside the box: the library's grid always holds its points
        ref = np.clip(ref, grid.mn, np.nextafter((np.float64(grid.mn) + ext).astype(np.float32), np.float32(-np.inf)))
        if trial % 3 == 0 and n > 1:
            ref[n // 2:] = ref[:n - n // 2]            # duplicates: the index rule
        nq = 300
        queries = (np.float64(grid.mn) + rng.uniform(-0.5, 1.5, size=(nq, 3)) * ext).astype(np.float32)
        queries[:n] = ref[rng.permutation(n)][:nq]     # ... and queries on points
        bound = rng.uniform(0.3, 3.0, size=nq) * h
        max2 = np.where(rng.uniform(size=nq) < 0.5, np.inf, bound * bound)
        scanned += check_case(host, grid, ref, queries, max2, seed=trial)
    assert flat >= 8 and fewer > 15
    print("random grids: %d scanned candidates checked" % scanned)


# ---------------------------------------------------------------------------
# rows of segments: what the sparse layout adds
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dim0", [1, 16, 17, 33])
def test_dense_and_sparse_walk_the_same_elements(host, dim0):
    """dim[0] of 1, 16, 17 and 33 (one segment, a full one, a second with one cell, a third with one cell); points only in some
    stretches of x, so rows have segments missing at the front, in the middle and at the end, and the grid's last segment is empty."""
    rng = np.random.default_rng(dim0)
    dim = np.array([dim0, 3, 2])
    grid = Grid((0.3, -0.7, 1.1), dim, 1 / 16)
    n = 120
    cx = rng.choice(np.array([0, 1, 15, 16, 20, 31, 32])[np.array([0, 1, 15, 16, 20, 31, 32]) < dim0], size=n)
    cy, cz = rng.integers(0, 3, size=n), rng.integers(0, 2, size=n)
    if dim0 > 1:
        keep = ~((cy == 2) & (cz == 1))                # the last row holds nothing: its segments, the grid's last one, are empty
        keep &= ~((cy == 0) & (cx < 16)) | (dim0 <= 16)  # rows that begin with a missing segment
        keep &= ~((cy == 1) & (cx >= 16) & (cx < 32))  # ... and rows with one missing in the middle
        cx, cy, cz = cx[keep], cy[keep], cz[keep]
    cells = np.stack([cx, cy, cz], axis=1)
    ref = (np.float64(grid.mn) + (cells + rng.uniform(0.05, 0.95, size=cells.shape)) * grid.h).astype(np.float32)
    for a in range(3):
        assert np.array_equal(grid.coord(ref[:, a], a), cells[:, a])
    queries = (np.float64(grid.mn) + rng.uniform(-0.2, 1.2, size=(400, 3)) * dim * grid.h).astype(np.float32)
    bound = rng.uniform(1.0, 6.0, size=400) * grid.h
    max2 = np.where(rng.uniform(size=400) < 0.4, np.inf, bound * bound)
    check_case(host, grid, ref, queries, max2, seed=dim0)   # (dense == sparse, byte for byte, is asserted for every run in there)


# ---------------------------------------------------------------------------
# h and mn that are no dyadic numbers: a point may sit a rounding error beyond its cell's face
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mn,h", [((0.3, -0.7, 1.1), float(np.float32(0.1))), ((0.3, -0.7, 1.1), 0.1), ((0.3, -0.7, 1.1), float(np.float32(0.07))),
                                  ((0.0, 0.0, 0.0), 0.4572502374649048)], ids=["0.1f", "0.1", "0.07f", "h * (1 / h) < 1"])
def test_points_a_rounding_error_from_their_faces(host, mn, h):
    """Points (float)(mn + k h) and their float neighbours on both sides, with h and mn that are no dyadic numbers: the case that
    exact_walk.hpp's 1e-6 of a cell is there for.  The last h is a float32 value with h * (1 / h) < 1 in f64 and mn = 0: the points
    k h for k = 1, 2, 4 are floats, lie exactly ON face k, and floor((v - mn) * inv_h) puts them into cell k - 1, on the other side
    of the face from where the exact quotient would -- asserted below, so that the case is known to be met."""
    rng = np.random.default_rng(3)
    dim = np.array([5, 4, 3])
    grid = Grid(np.float32(mn), dim, h)
    per_axis = []
    misplaced = on_face = 0
    for a in range(3):
        on = grid.face(a, np.arange(dim[a] + 1)).astype(np.float32)
        vals = np.concatenate([on, np.nextafter(on, np.float32(-np.inf)), np.nextafter(on, np.float32(np.inf))])
        vals = vals[(vals >= grid.mn[a]) & (vals.astype(np.float64) <= grid.face(a, dim[a]))]
        c = grid.coord(vals, a)
        k = np.rint((vals.astype(np.float64) - np.float64(grid.mn[a])) / h).astype(np.int64)   # the face that the value was made from
        on_face += int(np.sum(vals.astype(np.float64) == grid.face(a, k)))
        misplaced += int(np.sum((vals.astype(np.float64) >= grid.face(a, k)) & (c < np.minimum(k, dim[a] - 1))))
        mid = (grid.face(a, np.arange(dim[a])) + 0.5 * h).astype(np.float32)
        per_axis.append((vals, np.concatenate([vals, mid, np.float32([grid.mn[a] - 1.5 * h, grid.face(a, dim[a]) + 2.25 * h])])))
    print("h = %r: %d coordinates exactly on a face, %d at or above a face and in the cell below it" % (h, on_face, misplaced))
    assert on_face >= 3 and (mn != (0.0, 0.0, 0.0) or misplaced >= 6)
    ref = np.stack([rng.choice(per_axis[a][0], size=600) for a in range(3)], axis=1)
    queries = np.stack([rng.choice(per_axis[a][1], size=2500) for a in range(3)], axis=1)
    queries[:600] = ref
    max2 = np.where(np.arange(2500) % 3 == 0, np.inf, np.where(np.arange(2500) % 3 == 1, h * h, 4 * h * h))
    check_case(host, grid, ref, queries, max2)


# ---------------------------------------------------------------------------
# a query far from every point, no limit
# ---------------------------------------------------------------------------
def test_far_query_scans_the_whole_grid_once(host):
    """Queries 40 boxes away from a grid of 20 points.  The nearest point and the 1st to 4th distances are brute force's; the 32nd
    does not exist, so nothing ever bounds that walk: it scans the whole grid, every point exactly once, and answers inf."""
    rng = np.random.default_rng(9)
    dim = np.array([6, 5, 4])
    grid = Grid((0.25, -1.0, 2.0), dim, 1 / 8)
    ref = (np.float64(grid.mn) + rng.uniform(0, 1, size=(20, 3)) * dim * grid.h).astype(np.float32)
    dirs = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 1], [-1, 1, -1], [1, -1, 0], [0, 1, -1]])
    centre = np.float64(grid.mn) + 0.5 * dim * grid.h
    queries = (centre + dirs * 40.0 * dim * grid.h).astype(np.float32)
    check_case(host, grid, ref, queries, np.inf)
    for mode in ("dense", "sparse"):
        _, ids, answers, scans = host(grid, ref, queries, np.inf, mode, "kth", 32)
        assert np.all(np.isposinf(answers["d2"])) and np.all(np.isposinf(scans["limit"]))
        for s in np.split(np.arange(len(scans)), np.cumsum(answers["scans"].astype(np.int64))[:-1]):
            seen = np.zeros(len(ref), dtype=np.int64)
            for k in s:
                seen[scans["first"][k]:scans["last"][k]] += 1
            assert np.all(seen == 1)


# ---------------------------------------------------------------------------
# every point in one cell
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [(1, 1, 1), (7, 5, 3)], ids=["a grid of one cell", "one cell of many"])
def test_all_points_in_a_single_cell(host, dim):
    """What outliers do to a cloud's grid: 500 points, duplicates among them, all in ONE cell -- the grid's only cell, or cell
    (3, 2, 1) of 7 x 5 x 3 -- queries on the points, elsewhere in the grid and outside it.  Bounds from a fraction of the cluster
    of points to beyond the grid, the distances between chosen pairs exactly and one step above, and none."""
    rng = np.random.default_rng(500)
    dim = np.array(dim)
    grid = Grid((-0.4, 0.2, 1.0), dim, 0.25)
    cell = np.array([3, 2, 1]) if dim[0] > 1 else np.zeros(3)
    ref = (np.float64(grid.mn) + (cell + rng.uniform(0.02, 0.98, size=(500, 3))) * grid.h).astype(np.float32)
    ref[400:] = ref[:100]
    for a in range(3):
        assert np.all(grid.coord(ref[:, a], a) == cell[a])
    queries = (np.float64(grid.mn) + rng.uniform(-0.3, 1.3, size=(900, 3)) * dim * grid.h).astype(np.float32)
    queries[:500] = ref
    pair = ref[rng.integers(0, 500, size=900)].astype(np.float64) - queries.astype(np.float64)
    tie = (pair[:, 0] * pair[:, 0] + pair[:, 1] * pair[:, 1]) + pair[:, 2] * pair[:, 2]
    bound = rng.uniform(0.05, 8.0, size=900) * grid.h
    k = np.arange(900) % 4
    max2 = np.where(k == 0, np.inf, np.where(k == 1, bound * bound, np.where(k == 2, tie, np.nextafter(tie, np.inf))))
    check_case(host, grid, ref, queries, np.where(k % 2 == 0, np.inf, bound * bound), seed=int(dim[0]))   # (the models take the root of a bound)
    taken = check_within(host, grid, ref, queries, max2, seed=int(dim[0]))
    assert taken > 225 * 500       # (the unbounded queries alone take every point)
