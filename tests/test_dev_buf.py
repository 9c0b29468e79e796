"""gnss_sim_receiver_amd/csrc/host_api.h — the growable device buffer every handle of the C-ABI layer grows its run-sized
buffers through (gnsship::DevBuf, reserve, release), against a fake HIP runtime that counts calls and fails on demand
(tests/cpp/dev_buf_check.cpp has the list of what is checked).  Built with g++ and the HIP headers only, without the HIP
runtime, under the address and undefined-behaviour sanitizers: no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dbc") / "dev_buf_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "gnss_sim_receiver_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "dev_buf_check.cpp"),
                    "-o", exe], check=True)
    return exe


def test_reserve_and_release_contract(checker):
    out = subprocess.run([checker], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("dev_buf_check: 0 failures"), out.stdout
