"""include/gnsship_cpp.hpp — the five telemetry decoder families of the C++ mirror against a stub of the C ABI that logs
every call, fails on demand and writes every output to the full extent the C contract allows
(tests/cpp/tlm_mirror_calls_check.cpp has the list of what is checked).  Built with g++ alone, without the library, under
the address and undefined-behaviour sanitizers: no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tmc") / "tlm_mirror_calls_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "tlm_mirror_calls_check.cpp"),
                    "-o", exe, "-lpthread"], check=True)
    return exe


def test_calls_sizes_refusals_and_deletion_through_the_base(checker):
    out = subprocess.run([checker], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("tlm_mirror_calls_check: 0 failures"), out.stdout
