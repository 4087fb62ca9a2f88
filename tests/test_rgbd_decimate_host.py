"""The decimation and hole-filling arithmetic (csrc/rgbd_decimate.hpp: the derived sensor, the value of a block, the fill operator of
mode 1, the pick of modes 2 and 3) compiled for the host as a stand-alone program (tests/abi/rgbd_decimate_host.cpp, its own main)
with -ffp-contract=off -fsanitize=address,undefined, and held to the numpy model (tests/rgbd_decimate_model.py) as RAW BITS: every k
on images of k x k, (2k + 1) x k, (64k + 1) x 3 and 67 x 45 pixels with no, some and only holes and the values 1 and 65535; the
derived sensors; the three fill modes on lines of 1, 2, 64, 65 and 2049 pixels.  The kernels include the same header.  CPU only; the
host C++ compiler is required."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rgbd_decimate_model as cm
from test_rgbd_decimate_model import SENSORS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: rgbd_decimate.hpp cannot be checked"
    d = tmp_path_factory.mktemp("rgbd_decimate")
    exe = str(d / "rgbd_decimate_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cwipc_util_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "rgbd_decimate_host.cpp"), "-o", exe], check=True)

    def run(mode, records, dtype):
        inp, out = str(d / "in.bin"), str(d / "out.bin")
        np.ascontiguousarray(records, dtype=np.float64).tofile(inp)
        subprocess.run([exe, mode, inp, out], check=True, timeout=300)
        return np.fromfile(out, dtype=dtype)

    return run


def holed(rng, w, h, holes):
    """Depths over the whole range, `holes` of the pixels 0, and the two extreme values somewhere."""
    depth = rng.integers(1, 65536, (h, w)).astype(np.uint16)
    depth[rng.random((h, w)) < holes] = 0
    if holes < 1.0:
        flat = depth.reshape(-1)
        flat[rng.integers(0, flat.size)] = 1
        flat[rng.integers(0, flat.size)] = 65535
    return depth


def record(arg, image):
    h, w = image.shape
    return np.concatenate([[arg, w, h], image.reshape(-1).astype(np.float64)])


@pytest.mark.parametrize("k", range(2, 9))
def test_decimated_images_equal_the_model(host, k):
    rng = np.random.default_rng(700 + k)
    # (a 3-row image has no row of blocks for k > 3 and decimates to nothing: (64k + 1) x k stands beside it there)
    images = [holed(rng, w, h, holes) for w, h in ((k, k), (2 * k + 1, k), (64 * k + 1, 3), (64 * k + 1, k), (67, 45)) for holes in (0.0, 0.3, 1.0)]
    images += [np.full((k, k), 65535, dtype=np.uint16), np.full((k, 2 * k), 1, dtype=np.uint16)]
    # blocks with exactly one value, in every position of the block
    single = np.zeros((k, k * k * k), dtype=np.uint16)
    for i in range(k * k):
        single[i // k, i * k + i % k] = 1 + 1000 * i
    images.append(single)
    got = host("decimate", np.concatenate([record(k, image) for image in images]), np.uint16)
    want = np.concatenate([cm.decimate(image, k).reshape(-1) for image in images])
    assert got.tobytes() == want.tobytes()
    assert got[-k * k:].tolist() == [1 + 1000 * i for i in range(k * k)]
    assert (want == 0).any() and (want != 0).any()


def test_derived_sensors_equal_the_model(host):
    rng = np.random.default_rng(720)
    sensors = [s for s, _bits in SENSORS] + [(int(rng.integers(8, 2000)), int(rng.integers(8, 2000)), rng.uniform(100, 2000), rng.uniform(100, 2000),
                                              rng.uniform(-50, 1500), rng.uniform(-50, 1500)) for _ in range(200)]
    records, want = [], []
    for s in sensors:
        for k in range(1, 9):
            records.append((k,) + tuple(s))
            d = cm.derived_sensor(lm_sensor(s), k)
            want.append((d.width, d.height, d.fx, d.fy, d.cx, d.cy))
    got = host("sensor", np.array(records, dtype=np.float64).reshape(-1), np.float64).reshape(-1, 6)
    assert got.view(np.uint64).tobytes() == np.array(want, dtype=np.float64).view(np.uint64).tobytes()
    # k == 1 is the sensor itself, bit for bit
    ones = got[::8]
    assert ones.view(np.uint64).tobytes() == np.array(sensors, dtype=np.float64).view(np.uint64).tobytes()


def lm_sensor(s):
    import rgbd_lens_model as lm
    w, h, fx, fy, cx, cy = s
    return lm.Sensor(w, h, fx, fy, cx, cy, lm.PINHOLE, 0.001, (w, h), 3, (fx, fy, cx, cy), lm.PINHOLE, np.identity(4), np.identity(4), 1)


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_filled_images_equal_the_model(host, mode):
    rng = np.random.default_rng(740 + mode)
    images = []
    for n in (1, 2, 64, 65, 2049):
        for holes in (0.0, 0.5, 0.9, 1.0):
            images.append(holed(rng, n, 1, holes))
            images.append(holed(rng, 1, n, holes) if n < 2049 else holed(rng, n, 3, holes))
        only_first = np.zeros((2, n), dtype=np.uint16)
        only_first[0, 0] = 777
        images.append(only_first)
    got = host("fill", np.concatenate([record(mode, image) for image in images]), np.uint16)
    want = np.concatenate([cm.holefill(image, mode).reshape(-1) for image in images])
    assert got.tobytes() == want.tobytes()
    source = np.concatenate([image.reshape(-1) for image in images])
    assert np.array_equal(got[source != 0], source[source != 0])          # a pixel with depth is never changed
    assert ((source == 0) & (got != 0)).any() and ((source == 0) & (got == 0)).any()
