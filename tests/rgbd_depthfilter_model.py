"""The numpy / plain-Python statement of the raw entry's depth post-processing (test infrastructure): what
cwipc_hip_rgbd_rig_grab_filtered must make of the depth images before rules 1-4 run on them, written from its contract
(include/cwipc_util_amd/hip_ext.h rule 0), not from the code under test.  float64 elementwise operations in the stated
order; depth values in depth units; oma = 1 - alpha once per call; q(x) = (uint16) floor(x + 0.5).

    a pass over a line:   s = d[first];  for each further i in pass order:  c = d[i]
                              d[i] != 0 and s != 0 and |c - s| < delta:   s = (alpha*c) + (oma*s);  d[i] = q(s)      else:  s = c
    spatial, one iteration:  every row forward, every row backward, every column forward, every column backward, each on the last result
    temporal, per pixel:  c != 0:  s != 0 and |c - s| < delta:  s = (alpha*c) + (oma*s);  out = q(s)       else:  s = c;  out = c
                          c == 0:  out = q(s) if s != 0 and persists(mode, h) else 0
                          h = ((h << 1) | (c != 0)) & 0xff

A pass runs over all the lines of an image at once, position by position: the lines do not see each other."""
import numpy as np


def q(x):
    return np.floor(x + np.float64(0.5)).astype(np.uint16)


def line_pass(d, alpha, delta, backward=False):
    """One pass over every row of d (uint16[lines, n]) in place.  For columns hand in the transposed view."""
    alpha, delta = np.float64(alpha), np.float64(delta)
    oma = np.float64(1.0) - alpha
    n = d.shape[1]
    order = list(range(n - 1, -1, -1)) if backward else list(range(n))
    s = d[:, order[0]].astype(np.float64)
    for i in order[1:]:
        here = d[:, i].copy()
        c = here.astype(np.float64)
        blend = (here != 0) & (s != 0) & (np.abs(c - s) < delta)
        mixed = (alpha * c) + (oma * s)
        s = np.where(blend, mixed, c)
        d[:, i] = np.where(blend, q(mixed), here)
    return d


def spatial(depth, magnitude, alpha, delta):
    """Rule 0a: `magnitude` iterations on a copy of depth (uint16[H, W])."""
    out = np.array(depth, dtype=np.uint16, copy=True)
    for _ in range(int(magnitude)):
        line_pass(out, alpha, delta, False)
        line_pass(out, alpha, delta, True)
        line_pass(out.T, alpha, delta, False)
        line_pass(out.T, alpha, delta, True)
    return out


def popcount(h):
    h = np.asarray(h).astype(np.int64)
    return sum((h >> bit) & 1 for bit in range(8))


def persists(mode, h):
    """The persistence table on history bytes (an array or one value)."""
    h = np.asarray(h).astype(np.int64) & 0xff
    if mode == 0:
        return np.zeros(h.shape, dtype=bool)
    if mode == 1:
        return h == 0xff
    if mode == 2:
        return popcount(h & 0x07) >= 2
    if mode == 3:
        return popcount(h & 0x0f) >= 2
    if mode == 4:
        return popcount(h) >= 2
    if mode == 5:
        return (h & 0x03) != 0
    if mode == 6:
        return (h & 0x1f) != 0
    if mode == 7:
        return h != 0
    if mode == 8:
        return np.ones(h.shape, dtype=bool)
    raise ValueError("persistency mode %r" % (mode,))


class History:
    """One camera's temporal state: the running values (float64, 0: none) and the history bytes."""

    def __init__(self, height, width):
        self.value = np.zeros((height, width), dtype=np.float64)
        self.history = np.zeros((height, width), dtype=np.uint8)

    def reset(self):
        self.value[...] = 0.0
        self.history[...] = 0

    def temporal(self, depth, alpha, delta, persistency):
        """Rule 0b on depth (uint16[H, W], after 0a): the output image; the state moves on."""
        alpha, delta = np.float64(alpha), np.float64(delta)
        oma = np.float64(1.0) - alpha
        c = depth.astype(np.float64)
        s = self.value
        has = depth != 0
        blend = has & (s != 0) & (np.abs(c - s) < delta)
        mixed = (alpha * c) + (oma * s)
        keep = ~has & (s != 0) & persists(int(persistency), self.history)
        out = np.where(blend, q(np.where(blend, mixed, 0.0)), np.where(has, depth, np.where(keep, q(np.where(keep, s, 0.0)), 0))).astype(np.uint16)
        self.value = np.where(blend, mixed, np.where(has, c, s))
        self.history = (((self.history.astype(np.int64) << 1) | has) & 0xff).astype(np.uint8)
        return out


def depth_filter(frames, histories, params):
    """One frame -- per camera its (depth, colour) -- through the stages of params that are on (its fields: spatial_magnitude,
    spatial_alpha, spatial_delta, temporal, temporal_alpha, temporal_delta, temporal_persistency; None: none).  histories: one History
    per camera, touched only when the temporal stage is on.  Returns the frame rules 1-4 run on."""
    if params is None:
        return [(depth, colour) for depth, colour in frames]
    out = []
    for (depth, colour), hist in zip(frames, histories):
        d = spatial(depth, params.spatial_magnitude, params.spatial_alpha, params.spatial_delta) if params.spatial_magnitude else depth
        if params.temporal:
            d = hist.temporal(d, params.temporal_alpha, params.temporal_delta, params.temporal_persistency)
        out.append((np.ascontiguousarray(d), colour))
    return out
