"""The signal conditioner through the C++ mirror (include/gnsship_cpp.hpp Freq_Xlating_Fir_Filter_Hip):
tests/cpp/cond_mirror_test compiles against the headers (CPU) and, on the GPU, checks the adapter's
lowpass defaults, the accuracy contract against its own float64 model, call-split invariance and the
two-band handle against single-band ones."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "cond_mirror_test")


@pytest.fixture(scope="module")
def cond_bin(built):
    if not os.path.exists(BIN):
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/cond_mirror_test"], check=True)
    return BIN


def test_cond_mirror_test_builds_against_the_headers(cond_bin):
    assert os.access(cond_bin, os.X_OK)


@pytest.mark.gpu
def test_conditioner_through_the_cpp_mirror(cond_bin):
    r = subprocess.run([cond_bin], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cond_mirror_test passed" in r.stdout and "FAIL" not in r.stdout
