"""numpy model of RULE Q (include/cwipc_util_amd/hip_ext.h; csrc/quality_terms.hpp; cwipc_hip_distortion): the distortion sums of a
degraded cloud B against its original A.  The correspondences are icp_model's (brute force, or tree=True for big clouds); the terms
are restated here from the rule's text.  A cloud is a structured array of the library's point dtype (x, y, z float32; r, g, b, tile
uint8); normals are float32 (count(A), 3), or None: no pair has a normal."""
import math

import numpy as np

import icp_model as im

NONE = im.NONE
NSUM = 10
POINT_DTYPE = np.dtype([('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('r', 'u1'), ('g', 'u1'), ('b', 'u1'), ('tile', 'u1')])


def make_cloud(xyz, rgb):
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    pts = np.zeros(len(xyz), dtype=POINT_DTYPE)
    pts['x'], pts['y'], pts['z'] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    rgb = np.asarray(rgb, dtype=np.uint8).reshape(-1, 3)
    pts['r'], pts['g'], pts['b'] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    pts['tile'] = 1
    return pts


def xyz(pts):
    return np.stack([pts['x'], pts['y'], pts['z']], axis=1).astype(np.float32)


def rgb(pts):
    return np.stack([pts['r'], pts['g'], pts['b']], axis=1).astype(np.float64)


def pair_terms(p, q, m, has_normal, src_rgb, ref_rgb, d2):
    """(k, 10) for k pairs: 1 | 1.0 or 0.0 | d2 | r*r | dR*dR, dG*dG, dB*dB | dY*dY, dU*dU, dV*dV; all arguments float64, has_normal bool."""
    p, q, m = (np.asarray(a, dtype=np.float64).reshape(-1, 3) for a in (p, q, m))
    has_normal = np.asarray(has_normal, dtype=bool).reshape(-1)
    k = len(p)
    t = np.zeros((k, NSUM))
    t[:, 0] = 1.0
    t[:, 1] = np.where(has_normal, 1.0, 0.0)
    t[:, 2] = d2
    e = p - q
    with np.errstate(all="ignore"):   # (a pair without a normal may carry anything in m)
        r = (e[:, 0] * m[:, 0] + e[:, 1] * m[:, 1]) + e[:, 2] * m[:, 2]
        t[:, 3] = np.where(has_normal, r * r, 0.0)
    d = np.asarray(src_rgb, dtype=np.float64).reshape(-1, 3) - np.asarray(ref_rgb, dtype=np.float64).reshape(-1, 3)
    dR, dG, dB = d[:, 0], d[:, 1], d[:, 2]
    dY = (0.2126 * dR + 0.7152 * dG) + 0.0722 * dB
    dU = (-0.1146 * dR - 0.3854 * dG) + 0.5 * dB
    dV = (0.5 * dR - 0.4542 * dG) - 0.0458 * dB
    t[:, 4], t[:, 5], t[:, 6] = dR * dR, dG * dG, dB * dB
    t[:, 7], t[:, 8], t[:, 9] = dY * dY, dU * dU, dV * dV
    return t


def one_pass(src, ref, idx, d2, normals, normal_index):
    """A pass's result: dict(n_source, n, n_plane, terms (n, 10), max_d2, idx).  normal_index[j]: the index into `normals` that
    reference point j has (NONE: it has no normal)."""
    matched = idx != NONE
    j = idx[matched].astype(np.int64)
    k = int(matched.sum())
    m = np.zeros((k, 3))
    has = np.zeros(k, dtype=bool)
    if normals is not None and k:
        ni = normal_index[j].astype(np.int64)
        has = ni < len(normals)          # (NONE is beyond every count)
        m[has] = np.asarray(normals, dtype=np.float32)[ni[has]].astype(np.float64)
    t = pair_terms(xyz(src)[matched].astype(np.float64), xyz(ref)[j].astype(np.float64), m, has, rgb(src)[matched], rgb(ref)[j], d2[matched])
    return dict(n_source=len(src), n=k, n_plane=int(has.sum()), terms=t, max_d2=float(d2[matched].max()) if k else 0.0, idx=idx)


def distortion(A, B, max_distance=np.inf, normals=None, tree=False):
    """(forward, backward) of one_pass: backward (source B, reference A) first, its indices hand B's points A's normals."""
    A, B = np.asarray(A, dtype=POINT_DTYPE), np.asarray(B, dtype=POINT_DTYPE)
    idxBA, d2BA = im.correspondences(xyz(B), xyz(A), None, max_distance, tree=tree)
    backward = one_pass(B, A, idxBA, d2BA, normals, np.arange(len(A), dtype=np.uint32))
    idxAB, d2AB = im.correspondences(xyz(A), xyz(B), None, max_distance, tree=tree)
    forward = one_pass(A, B, idxAB, d2AB, normals, idxBA)
    return forward, backward


def sums(one, exact=True):
    """dict(sum_d2, sum_r2, sum_rgb2 (3 ints), sum_yuv2 (3)) of a pass, with math.fsum (or numpy.sum)."""
    t = one["terms"]
    add = (lambda col: math.fsum(col)) if exact else (lambda col: float(np.sum(col)))
    return dict(sum_d2=add(t[:, 2]), sum_r2=add(t[:, 3]), sum_rgb2=[int(add(t[:, 4 + c])) for c in range(3)], sum_yuv2=[add(t[:, 7 + c]) for c in range(3)])


def ratio(total, count):
    return total / count if count else float("nan")


def psnr(peak2, mse):
    if math.isnan(mse):
        return float("nan")
    return math.inf if mse == 0 else 10.0 * math.log10(peak2 / mse)


def results(forward, backward, peak):
    """The model's DistortionResults as a dict of dicts: per direction mse_d1, mse_d2, hausdorff, mse_rgb, mse_yuv; symmetric = the
    larger (NaN propagates); the five PSNRs."""
    out = {}
    for name, one in (("forward", forward), ("backward", backward)):
        s = sums(one)
        out[name] = dict(n_source=one["n_source"], n=one["n"], n_plane=one["n_plane"], mse_d1=ratio(s["sum_d2"], one["n"]),
                         mse_d2=ratio(s["sum_r2"], one["n_plane"]), hausdorff=math.sqrt(one["max_d2"]),
                         mse_rgb=tuple(ratio(v, one["n"]) for v in s["sum_rgb2"]), mse_yuv=tuple(ratio(v, one["n"]) for v in s["sum_yuv2"]))

    def larger(a, b):
        return float("nan") if math.isnan(a) or math.isnan(b) else max(a, b)
    f, b = out["forward"], out["backward"]
    sym = dict(mse_d1=larger(f["mse_d1"], b["mse_d1"]), mse_d2=larger(f["mse_d2"], b["mse_d2"]), hausdorff=larger(f["hausdorff"], b["hausdorff"]),
               mse_rgb=tuple(larger(x, y) for x, y in zip(f["mse_rgb"], b["mse_rgb"])), mse_yuv=tuple(larger(x, y) for x, y in zip(f["mse_yuv"], b["mse_yuv"])))
    out["symmetric"] = sym
    out["psnr_d1"], out["psnr_d2"] = psnr(3 * peak * peak, sym["mse_d1"]), psnr(3 * peak * peak, sym["mse_d2"])
    out["psnr_y"], out["psnr_u"], out["psnr_v"] = (psnr(255.0 * 255.0, v) for v in sym["mse_yuv"])
    return out


def tied_queries(src, ref):
    """How many finite source points have two or more reference points at exactly their smallest d2 (brute force)."""
    p, q = xyz(src).astype(np.float64), xyz(ref).astype(np.float64)
    count = 0
    for lo in range(0, len(p), 256):
        s = p[lo:lo + 256]
        dx, dy, dz = s[:, None, 0] - q[None, :, 0], s[:, None, 1] - q[None, :, 1], s[:, None, 2] - q[None, :, 2]
        dd = (dx * dx + dy * dy) + dz * dz
        count += int(((dd == dd.min(axis=1)[:, None]).sum(axis=1) >= 2).sum())
    return count
