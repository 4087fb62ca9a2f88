"""The atomic union-find (csrc/union_find.hpp: uf_find with path halving, uf_union) compiled for the host as a stand-alone program
(tests/abi/union_find_host.cpp, its own main) with -fsanitize=address,undefined and run sequentially.  CPU only; the host C++
compiler is required (a missing one fails the tests).

  * chains of 20 000 points linked i - (i + 1), the unions issued in ascending, descending and shuffled order: every label is 0, and
    the parent words loaded by all finds stay below 20 n.  A Python restatement of halving takes 5 n - 5 steps on the worst of these
    orders and n^2 / 2 = 10 000 n without halving, so the bound tells the two apart with room for another halving variant.
  * random forests against a plain sequential union-find: the same roots (each component's smallest index), parent[x] <= x
    throughout."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 20000


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: union_find.hpp cannot be checked"
    exe = str(tmp_path_factory.mktemp("union_find") / "union_find_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cwipc_util_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "union_find_host.cpp"), "-o", exe], check=True)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], check=True, timeout=120, capture_output=True, text=True).stdout.split()
        return {out[i]: int(out[i + 1]) for i in range(0, len(out), 2)}
    return run


@pytest.mark.parametrize("order,seed", [("ascending", 0), ("descending", 0), ("shuffled", 1), ("shuffled", 2)])
def test_chain_is_one_cluster_in_linear_steps(host, order, seed):
    got = host("chain", N, order, seed)
    print(order, seed, got)
    assert got["labels_zero"] == 1
    assert got["steps"] < 20 * N


@pytest.mark.parametrize("n,m,seed", [(1, 5, 0), (2, 3, 1), (1000, 300, 2), (1000, 1000, 3), (5000, 20000, 4), (20000, 15000, 5)])
def test_random_forests_against_a_plain_union_find(host, n, m, seed):
    got = host("forest", n, m, seed)
    assert got["mismatches"] == 0 and got["invariant"] == 1
