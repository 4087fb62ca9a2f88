"""Tiled frames for the multi-camera tests, cut from a cloud of points: N cameras looking at the scene from around the y axis, each
seeing an angular sector, neighbouring sectors overlapping (a point in an overlap goes to ONE of the cameras that see it, so the
cameras hold independent samples of the same surface); a floor band under the scene; a few dozen points duplicated into another
tile, so that a distance of exactly 0 between two tiles occurs.  Test infrastructure: numpy only."""
import numpy as np


def xyz_of(p):
    return np.column_stack([p["x"], p["y"], p["z"]]).astype(np.float32)


def sector_tiles(x, z, centre, ntiles, rng, overlap=1.5):
    """Per point the tile bit (1 << k) of one of the cameras whose sector holds its angle around `centre`; a sector is `overlap` times
    as wide as a ntiles-th of the circle."""
    ang = np.arctan2(z - centre[1], x - centre[0])
    half = np.pi / ntiles * overlap
    seen = np.zeros((len(x), ntiles), dtype=bool)
    for k in range(ntiles):
        mid = -np.pi + (k + 0.5) * 2 * np.pi / ntiles
        seen[:, k] = np.abs((ang - mid + np.pi) % (2 * np.pi) - np.pi) <= half
    pick = rng.random((len(x), ntiles)) * seen
    return (1 << np.argmax(pick, axis=1)).astype(np.uint8)


def make_frame(pts, ntiles=4, seed=0, floor_fraction=0.12, duplicates=48, shuffle=True):
    """pts (cwipc point records, any tiles) -> a frame of ntiles cameras (tiles 1, 2, 4, ...) with a floor band at 0 <= y < 0.08."""
    rng = np.random.default_rng(seed)
    body = pts.copy()
    centre = (float(np.mean(body["x"])), float(np.mean(body["z"])))
    radius = float(np.max(np.hypot(body["x"] - centre[0], body["z"] - centre[1])))
    nfloor = int(len(body) * floor_fraction)
    floor = np.zeros(nfloor, dtype=body.dtype)
    r, theta = radius * 1.2 * np.sqrt(rng.random(nfloor)), rng.random(nfloor) * 2 * np.pi
    floor["x"] = (centre[0] + r * np.cos(theta)).astype(np.float32)
    floor["z"] = (centre[1] + r * np.sin(theta)).astype(np.float32)
    floor["y"] = (rng.random(nfloor) * 0.08).astype(np.float32)
    floor["r"] = floor["g"] = floor["b"] = 128
    frame = np.concatenate([body, floor])
    frame["tile"] = sector_tiles(frame["x"], frame["z"], centre, ntiles, rng)
    if duplicates:
        dup = frame[rng.choice(len(frame), duplicates, replace=False)].copy()
        k = np.log2(dup["tile"]).astype(int)
        dup["tile"] = (1 << ((k + 1) % ntiles)).astype(np.uint8)
        frame = np.concatenate([frame, dup])
    if shuffle:
        frame = frame[rng.permutation(len(frame))]
    return np.ascontiguousarray(frame)


def takes_part(pts, mask, y_limits):
    """numpy's reading of a job's predicate on one side: (tile & mask) != 0 (mask 0: every point) and lo < (double)y < hi."""
    ok = np.ones(len(pts), dtype=bool) if mask == 0 else (pts["tile"] & np.uint8(mask)) != 0
    y = pts["y"].astype(np.float64)
    return ok & (y_limits[0] < y) & (y < y_limits[1])


def rigid(rx_deg=0.0, ry_deg=0.0, rz_deg=0.0, t=(0.0, 0.0, 0.0), pivot=(0.0, 0.0, 0.0)):
    """4x4 of a rotation about `pivot` (x, then y, then z axis, degrees) followed by the translation t."""
    ax, ay, az = np.radians([rx_deg, ry_deg, rz_deg])
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    rot = rz @ ry @ rx
    m = np.identity(4)
    m[:3, :3] = rot
    m[:3, 3] = np.asarray(t, dtype=float) + np.asarray(pivot, dtype=float) - rot @ np.asarray(pivot, dtype=float)
    return m
