"""The octree codec's host staging (csrc/codec_stage.hpp: the stream table of the entropy stage under the plane-offset rules of RULE E,
T and P with its bound on the stream count, the entropy encoder's work block, RULE T's plane block, the block table of a coded packet,
the decoder's terms, the tile words and the status word's messages) compiled for the host as a stand-alone program
(tests/abi/codec_stage_host.cpp, its own main) with -fsanitize=address,undefined, on heap blocks of exactly the sizes the header
gives.  A carve that left its block would be an out-of-bounds write on the device; here it ends the program.  CPU only; the host C++
compiler is required."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHECKS = ["streams_rule_e", "streams_rule_t", "streams_rule_p", "stream_count_is_bounded", "encode_work_layout", "tree_plane_layout", "block_table",
          "decode_terms_follow_the_layout", "tile_words_give_mode_and_value", "status_words_give_their_messages"]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: codec_stage.hpp cannot be checked"
    exe = str(tmp_path_factory.mktemp("codec_stage") / "codec_stage_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cwipc_util_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "codec_stage_host.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("check", CHECKS)
def test_codec_stage(host, check):
    done = subprocess.run([host, check], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and done.stdout == "ok\n", (done.stdout, done.stderr)


def test_every_check_of_the_program_is_run(host):
    listed = subprocess.run([host], capture_output=True, text=True, timeout=300)
    assert listed.returncode == 2
    assert [line.strip() for line in listed.stderr.splitlines()[1:]] == CHECKS
