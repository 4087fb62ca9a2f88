"""numpy model of cwipc_hip_render's contract (include/cwipc_util_amd/hip_ext.h, csrc/kernels_render.hip): the projection vectorised
in float64, every operation rounded on its own and in the contract's order, then a lexicographic sort on (pixel, float32 depth, point
index) whose first entry per pixel is the winner.  Test infrastructure: the GPU tests compare bytes with it, and test_render_model.py
compares it with a plain loop over points and splat pixels (`render_loops`).

A view is anything with width, height, fx, fy, cx, cy, near, far and a 4x4 extrinsic (registration.render.PinholeView)."""
import math

import numpy as np


def project(pts, view, point_size, tilemask):
    """(idx, col, row, depth): the points that take part and can touch the image, their pixel and their float32 depth."""
    h = (point_size - 1) // 2
    E = np.asarray(view.extrinsic, dtype=np.float64)
    x, y, z = (pts[f].astype(np.float64) for f in ('x', 'y', 'z'))
    tile = pts['tile'].astype(np.int64)
    with np.errstate(all='ignore'):
        take = np.isfinite(pts['x']) & np.isfinite(pts['y']) & np.isfinite(pts['z'])
        if tilemask != 0:
            take &= (tile & tilemask) != 0
        xc = ((E[0, 0] * x + E[0, 1] * y) + E[0, 2] * z) + E[0, 3]
        yc = ((E[1, 0] * x + E[1, 1] * y) + E[1, 2] * z) + E[1, 3]
        zc = ((E[2, 0] * x + E[2, 1] * y) + E[2, 2] * z) + E[2, 3]
        take &= (view.near < zc) & (zc < view.far)
        fu = np.floor(view.fx * (xc / zc) + view.cx)
        fv = np.floor(view.fy * (yc / zc) + view.cy)
        take &= (-(h + 1) < fu) & (fu < view.width + h) & (-(h + 1) < fv) & (fv < view.height + h)   # (False for NaN and the infinities)
        idx = np.nonzero(take)[0]
        return idx, fu[idx].astype(np.int64), fv[idx].astype(np.int64), zc[idx].astype(np.float32)


def render_model(pts, view, point_size=5, tilemask=0, background=(255, 255, 255)):
    """(rgb uint8[H, W, 3], depth float32[H, W], index int32[H, W], number of covered pixels)."""
    W, H = int(view.width), int(view.height)
    h = (point_size - 1) // 2
    idx, col, row, d = project(pts, view, point_size, tilemask)
    rgb = np.empty((H, W, 3), dtype=np.uint8)
    rgb[:] = np.asarray(background, dtype=np.uint8)
    depth = np.zeros((H, W), dtype=np.float32)
    index = np.full((H, W), -1, dtype=np.int32)
    if len(idx) == 0:
        return rgb, depth, index, 0
    # rank of a point in the order (float32 depth, index): idx ascends, so a stable sort on the depth is that order
    order = np.argsort(d, kind='stable')
    rank = np.empty(len(idx), dtype=np.uint64)
    rank[order] = np.arange(len(idx), dtype=np.uint64)
    entries = []
    for dr in range(-h, h + 1):
        for dc in range(-h, h + 1):
            c, r = col + dc, row + dr
            ok = (c >= 0) & (c < W) & (r >= 0) & (r < H)
            entries.append(((r[ok] * W + c[ok]).astype(np.uint64) << np.uint64(32)) | rank[ok])
    entries = np.sort(np.concatenate(entries))                  # by pixel, then by (depth, index)
    pixel = (entries >> np.uint64(32)).astype(np.int64)
    first = np.ones(len(entries), dtype=bool)
    first[1:] = pixel[1:] != pixel[:-1]
    pixel = pixel[first]
    winner = order[(entries[first] & np.uint64(0xFFFFFFFF)).astype(np.int64)]   # rank -> position in idx
    depth.reshape(-1)[pixel] = d[winner]
    index.reshape(-1)[pixel] = idx[winner]
    for k, f in enumerate(('r', 'g', 'b')):
        rgb.reshape(-1, 3)[pixel, k] = pts[f][idx[winner]]
    return rgb, depth, index, int(len(pixel))


def render_loops(pts, view, point_size=5, tilemask=0, background=(255, 255, 255)):
    """The contract as a loop over the points and over each point's splat pixels, compare and replace; Python floats are float64
    and every operation is rounded on its own.  For small clouds and images."""
    W, H = int(view.width), int(view.height)
    h = (point_size - 1) // 2
    E = [[float(v) for v in r] for r in np.asarray(view.extrinsic, dtype=np.float64)]
    rgb = np.empty((H, W, 3), dtype=np.uint8)
    rgb[:] = np.asarray(background, dtype=np.uint8)
    depth = np.zeros((H, W), dtype=np.float32)
    index = np.full((H, W), -1, dtype=np.int32)
    for i in range(len(pts)):
        if tilemask != 0 and (int(pts['tile'][i]) & tilemask) == 0:
            continue
        x, y, z = float(pts['x'][i]), float(pts['y'][i]), float(pts['z'][i])
        if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
            continue
        xc = ((E[0][0] * x + E[0][1] * y) + E[0][2] * z) + E[0][3]
        yc = ((E[1][0] * x + E[1][1] * y) + E[1][2] * z) + E[1][3]
        zc = ((E[2][0] * x + E[2][1] * y) + E[2][2] * z) + E[2][3]
        if not (view.near < zc and zc < view.far):
            continue
        u = view.fx * (xc / zc) + view.cx
        v = view.fy * (yc / zc) + view.cy
        if not (math.isfinite(u) and math.isfinite(v)):
            continue
        fu, fv = math.floor(u), math.floor(v)   # (exact integers of any size)
        if not (-(h + 1) < fu < W + h and -(h + 1) < fv < H + h):
            continue
        with np.errstate(over='ignore'):
            d = np.float32(zc)
        for r in range(fv - h, fv + h + 1):
            for c in range(fu - h, fu + h + 1):
                if not (0 <= r < H and 0 <= c < W):
                    continue
                if index[r, c] < 0 or d < depth[r, c] or (d == depth[r, c] and i < index[r, c]):
                    depth[r, c] = d
                    index[r, c] = i
                    rgb[r, c] = (pts['r'][i], pts['g'][i], pts['b'][i])
    return rgb, depth, index, int((index >= 0).sum())
