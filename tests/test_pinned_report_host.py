"""The host half of the pinned-word report (csrc/pinned_report.hpp: arming a range of words under the next tag, a packed word or a
range of them landing under that tag only, the plain layout's tag word, the value and raw reads) compiled for the host as a
stand-alone program (tests/abi/pinned_report_host.cpp, its own main) with -fsanitize=address,undefined, on a plain array of exactly
the words it stands for.  Every entry point that waits for a kernel's report reads it through this header.  CPU only; the host C++
compiler is required."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHECKS = ["arming_zeroes_its_range_only", "tags_count_up_and_skip_zero", "packed_word_lands_under_its_tag_only", "range_lands_when_every_word_has",
          "plain_layout_wants_the_tag_word_exactly", "reads_return_the_written_bits"]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: pinned_report.hpp cannot be checked"
    exe = str(tmp_path_factory.mktemp("pinned_report") / "pinned_report_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cwipc_util_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "pinned_report_host.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("check", CHECKS)
def test_pinned_report(host, check):
    done = subprocess.run([host, check], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and done.stdout == "ok\n", (done.stdout, done.stderr)


def test_every_check_of_the_program_is_run(host):
    listed = subprocess.run([host], capture_output=True, text=True, timeout=300)
    assert listed.returncode == 2
    assert [line.strip() for line in listed.stderr.splitlines()[1:]] == CHECKS
