"""The conditioner's real-sampled and bit-packed input items through the C++ mirror (include/gnsship_cpp.hpp:
Freq_Xlating_Fir_Filter_Conf::input_item_type and the packed file sources' configurations):
tests/cpp/cond_ingest_mirror_test compiles against the headers and checks the presets' formats (CPU) and, on the
GPU, one real and one packed run against values computed in the test, and a misaligned n_in refused."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "cond_ingest_mirror_test")


@pytest.fixture(scope="module")
def ingest_bin(built):
    if not os.path.exists(BIN):
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/cond_ingest_mirror_test"], check=True)
    return BIN


def test_presets_map_to_their_formats(ingest_bin):
    """The source configurations' defaults and formats, input_item_type and the bits per sample: host only."""
    r = subprocess.run([ingest_bin, "formats"], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cond_ingest_mirror_test formats passed" in r.stdout and "FAIL" not in r.stdout


@pytest.mark.gpu
def test_real_and_packed_items_through_the_cpp_mirror(ingest_bin):
    r = subprocess.run([ingest_bin], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cond_ingest_mirror_test passed" in r.stdout and "FAIL" not in r.stdout
