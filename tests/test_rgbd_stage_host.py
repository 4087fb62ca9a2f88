"""The RGB-D source's host staging (csrc/rgbd_stage.hpp: the rig's device block with every kind of part, the aligned frame's block, the
temporal state's block and its three views, a frame's upload sizes, the pixel limits, every refusal of a camera, a sensor, a rig and a
frame with its exact text and its precedence, a grab's plan from the four optional structs) compiled for the host as a stand-alone
program (tests/abi/rgbd_stage_host.cpp, its own main) with -fsanitize=address,undefined, on heap blocks of exactly the sizes the header
gives.  A carve that left its block would be an out-of-bounds write on the device; here it ends the program.  CPU only; the host C++
compiler is required."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHECKS = ["rig_block_layout", "frame_block_layout", "state_block_views", "pixel_limits", "camera_refusals", "sensor_refusals", "rig_refusals",
          "grab_plan_refusals", "grab_plans"]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: rgbd_stage.hpp cannot be checked"
    exe = str(tmp_path_factory.mktemp("rgbd_stage") / "rgbd_stage_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cwipc_util_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "abi", "rgbd_stage_host.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("check", CHECKS)
def test_rgbd_stage(host, check):
    done = subprocess.run([host, check], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and done.stdout == "ok\n", (done.stdout, done.stderr)


def test_every_check_of_the_program_is_run(host):
    listed = subprocess.run([host], capture_output=True, text=True, timeout=300)
    assert listed.returncode == 2
    assert [line.strip() for line in listed.stderr.splitlines()[1:]] == CHECKS
