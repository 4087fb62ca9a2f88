"""The depth post-processing's arithmetic (csrc/rgbd_depthfilter.hpp: the step of a line pass, the temporal pixel update, persists)
compiled for the host as a stand-alone program (tests/abi/rgbd_depthfilter_host.cpp, its own main) with -ffp-contract=off
-fsanitize=address,undefined, and held to the numpy model (tests/rgbd_depthfilter_model.py) as RAW BITS: random lines of the lengths
where a kernel's tile ends, with holes at both ends and in runs and the values 1 and 65535; whole images through the four passes; random
(c, s, h) triples of the temporal update with |c - s| == delta exactly and s == 0 among them; all 9 x 256 persists pairs against the
table written out in tests/test_rgbd_depthfilter_model.py.  The kernels include the same header.  CPU only; the host C++ compiler is
required."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rgbd_depthfilter_model as dm
from test_rgbd_depthfilter_model import HAND_ALPHA, HAND_DELTA, THREE, TWO_BY_TWO, persists_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: rgbd_depthfilter.hpp cannot be checked"
    d = tmp_path_factory.mktemp("rgbd_depthfilter")
    exe = str(d / "rgbd_depthfilter_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cwipc_util_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "rgbd_depthfilter_host.cpp"), "-o", exe], check=True)

    def run(mode, records, dtype):
        inp, out = str(d / "in.bin"), str(d / "out.bin")
        np.ascontiguousarray(records, dtype=np.float64).tofile(inp)
        subprocess.run([exe, mode, inp, out], check=True, timeout=300)
        return np.fromfile(out, dtype=dtype)

    return run


def random_line(rng, n, delta):
    """Depths in a band a few delta wide, with a hole at either end now and then, holes in runs, and the two extreme values."""
    base = int(rng.choice([1, 1000, 30000, 65535 - int(4 * delta)]))
    line = (base + rng.integers(0, int(4 * delta) + 1, n)).clip(1, 65535).astype(np.uint16)
    if rng.random() < 0.3:
        line[rng.integers(0, n)] = 1
    if rng.random() < 0.3:
        line[rng.integers(0, n)] = 65535
    for _ in range(int(rng.integers(0, 1 + n // 16 + 1))):
        start = int(rng.integers(0, n))
        line[start:start + int(rng.integers(1, 6))] = 0
    if rng.random() < 0.4:
        line[0] = 0
    if rng.random() < 0.4:
        line[-1] = 0
    return line


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("alpha,delta", [(0.5, 16.0), (0.4, 20.0), (0.25, 3.5), (1.0, 16.0), (0.6180339887498949, 7.0)])
def test_line_passes_equal_the_model(host, alpha, delta, backward):
    rng = np.random.default_rng(int(alpha * 1000) + int(backward))
    lines = [random_line(rng, n, delta) for n in (1, 2, 3, 64, 65, 640) for _ in range(12)]
    lines += [np.array(v, dtype=np.uint16) for v in ([0], [1], [65535], [0, 0, 0], [1, 65535], [65535, 65535 - 15, 65535], [1, 2, 1, 0, 1],
                                                    THREE[0][0], [1000, 1016], [1016, 1000])]
    record = np.concatenate([[alpha, delta, float(backward)]] + [np.concatenate([[len(l)], l.astype(np.float64)]) for l in lines])
    got = host("lines", record, np.uint16)
    want = np.concatenate([dm.line_pass(l.reshape(1, -1).copy(), alpha, delta, backward)[0] for l in lines])
    assert got.tobytes() == want.tobytes()
    assert np.array_equal(got == 0, np.concatenate(lines) == 0)
    if alpha < 1.0:
        assert (got != np.concatenate(lines)).mean() > 0.2          # both branches: much is blended, and not everything
        assert (got == np.concatenate(lines)).mean() > 0.05
    else:
        assert np.array_equal(got, np.concatenate(lines))


@pytest.mark.parametrize("magnitude", [1, 2, 5])
def test_images_equal_the_model_and_the_hand_worked_cases(host, magnitude):
    rng = np.random.default_rng(50 + magnitude)
    for w, h in ((1, 1), (7, 1), (1, 7), (65, 9), (33, 70)):
        depth = np.stack([random_line(rng, w, 12.0) for _ in range(h)])
        got = host("spatial", np.concatenate([[0.45, 12.0, magnitude, w, h], depth.reshape(-1).astype(np.float64)]), np.uint16).reshape(h, w)
        assert got.tobytes() == dm.spatial(depth, magnitude, 0.45, 12.0).tobytes()
    if magnitude == 1:
        for image, want in (THREE, TWO_BY_TWO, (THREE[0].T, THREE[1].T)):
            h, w = image.shape
            got = host("spatial", np.concatenate([[HAND_ALPHA, HAND_DELTA, 1, w, h], image.reshape(-1).astype(np.float64)]), np.uint16).reshape(h, w)
            assert np.array_equal(got, want)


def test_temporal_updates_equal_the_model(host):
    rng = np.random.default_rng(60)
    alpha, delta = 0.4, 20.0
    records = []
    for _ in range(6000):
        mode, h = int(rng.integers(0, 9)), int(rng.integers(0, 256))
        s = float(rng.choice([0.0, float(rng.integers(1, 65536)), rng.uniform(1.0, 65535.0), 1000.0 + rng.uniform(-30, 30)]))
        if rng.random() < 0.5:      # near the running value: about 40 in 51 of these blend where there is one
            c = min(65535, max(1, int(s) + int(rng.integers(-25, 26))))
        else:
            c = int(rng.choice([0, 0, 1, 65535, int(rng.integers(1, 65536))]))
        records.append((mode, c, s, h))
    # |c - s| == delta exactly, either way, and one ulp inside; no running value; the extreme values
    records += [(3, 1020, 1000.0, 7), (3, 980, 1000.0, 7), (3, 1020, float(np.nextafter(1000.0, np.inf)), 7), (3, 980, float(np.nextafter(1000.0, -np.inf)), 7),
                (8, 0, 0.0, 255), (8, 1, 0.0, 255), (1, 0, 1.0, 255), (1, 0, 65535.0, 255), (1, 0, 65534.5, 255), (1, 0, 1234.4999999999998, 254),
                (7, 65535, 65535.0, 0), (7, 1, 1.0, 0), (7, 1, 20.5, 0)]
    got = host("temporal", np.concatenate([[alpha, delta], np.array(records, dtype=np.float64).reshape(-1)]), np.float64).reshape(-1, 3)
    want = []
    for mode, c, s, h in records:
        hist = dm.History(1, 1)
        hist.value[0, 0], hist.history[0, 0] = s, h
        out = hist.temporal(np.array([[c]], dtype=np.uint16), alpha, delta, mode)
        want.append((float(out[0, 0]), hist.value[0, 0], float(hist.history[0, 0])))
    want = np.array(want, dtype=np.float64)
    assert got.view(np.uint64).tobytes() == want.view(np.uint64).tobytes()
    tail = got[-13:]
    assert tail[0].tolist() == [1020.0, 1020.0, 15.0] and tail[1].tolist() == [980.0, 980.0, 15.0]           # exactly delta: taken over
    assert tail[2, 0] == 1008.0 and tail[3, 0] == 992.0 and tail[2, 1] != 1020.0                            # one ulp inside: blended
    assert tail[4].tolist() == [0.0, 0.0, 254.0] and tail[5].tolist() == [1.0, 1.0, 255.0]
    assert tail[6, 0] == 1.0 and tail[7, 0] == 65535.0 and tail[8, 0] == 65535.0 and tail[9, 0] == 0.0
    blended = np.array([r[1] != 0 and r[2] != 0 and abs(r[1] - r[2]) < delta for r in records])
    assert 0.1 < blended.mean() < 0.9


def test_persists_is_the_literal_table(host):
    got = host("persists", [0.0], np.uint8).reshape(9, 256)
    for mode in range(9):
        assert np.array_equal(got[mode].astype(bool), persists_table(mode))
