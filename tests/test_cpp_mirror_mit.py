"""The interference-mitigation classes of the C++ mirror (include/gnsship_cpp.hpp Pulse_Blanking_Filter_Hip,
Notch_Filter_Hip, Notch_Filter_Lite_Hip): tests/cpp/mit_mirror_test prints the *_Conf defaults and the coeff_rate →
n_segments_coeff derivation, compared here with the adapters' values (pulse_blanking_filter.cc:37-49,72-77,
notch_filter.cc:36-46, notch_filter_lite.cc:37-56), and on the GPU runs every class whole against cut into runs."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "mit_mirror_test")


@pytest.fixture(scope="module")
def mit_bin(built):
    if not os.path.exists(BIN):
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/mit_mirror_test"], check=True)
    return BIN


def fields(line):
    t = line.split()
    return t[0], {t[i]: t[i + 1] for i in range(1, len(t) - 1, 2)}


def test_conf_defaults_are_the_adapters(mit_bin):
    r = subprocess.run([mit_bin, "defaults"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [fields(l) for l in r.stdout.strip().splitlines()]
    by = {name: f for name, f in lines if name != "coeff"}
    f32 = lambda v: float(np.float32(float(v)))  # %.9g identifies a float32
    pb = by["pulse_blanking"]
    assert (f32(pb["pfa"]), int(pb["length"]), int(pb["segments_est"]), int(pb["segments_reset"])) == (f32(0.04), 32, 12500, 5000000)
    assert (float(pb["IF"]), float(pb["sampling_frequency"]), float(pb["bw"]), float(pb["tw"])) == (0.0, 4000000.0, 2000000.0, 0.0)
    for name in ("notch", "notch_lite"):
        c = by[name]
        assert (f32(c["pfa"]), f32(c["p_c_factor"]), int(c["length"]), int(c["segments_est"]), int(c["segments_reset"])) == \
            (f32(0.001), f32(0.9), 32, 12500, 5000000)
    # default coeff_rate = sampling_frequency · 0.1: (fs / rate) / 32 = 0.3125 → max(1, 0)
    assert float(by["notch_lite"]["sampling_frequency"]) == 4000000.0 and int(by["notch_lite"]["n_segments_coeff"]) == 1
    coeff = [f for name, f in lines if name == "coeff"]
    assert len(coeff) == 4
    for c in coeff:
        fs, rate, length = np.float32(c["sampling_frequency"]), np.float32(c["coeff_rate"]), int(c["length"])
        want = max(1, int(np.float32(np.float32(fs / rate) / np.float32(length))))  # notch_filter_lite.cc:55-56, float arithmetic
        assert int(c["n_segments_coeff"]) == want, c
    assert [int(c["n_segments_coeff"]) for c in coeff] == [125, 800, 1, 20]


@pytest.mark.gpu
def test_mitigation_through_the_cpp_mirror(mit_bin):
    r = subprocess.run([mit_bin], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mit_mirror_test passed" in r.stdout and "FAIL" not in r.stdout
