"""BeiDou B3I and GPS L2C through the C++ mirror (include/gnsship_cpp.hpp): tests/cpp/b3i_l2c_mirror_test tracks
one channel with Dll_Pll_Veml_Tracking_Hip (system 'C' / signal "B3", system 'G' / signal "2S", the mirror's
code generators) over an IF file and writes its epoch records, which equal the oracle loop's
(test_gpu_trk.compare_exact).  The program leaves vector_length at 0, asks for track_pilot and for
extend_correlation_symbols 0 (B3I) / 4 (L2C): the mirror applies the adapters' vector_length and clamps."""
import os
import subprocess

import numpy as np
import pytest

from gnss_sim_receiver_amd import abi
from oracle import trk as T

import b3i_l2c_scenarios as B
from test_gpu_trk import compare_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "b3i_l2c_mirror_test")


@pytest.fixture(scope="module")
def mirror_bin(built):
    if not os.path.exists(BIN):
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/b3i_l2c_mirror_test"], check=True)
    return BIN


@pytest.mark.gpu
@pytest.mark.parametrize("signal,fs,epochs", [("B3", 12.5e6, 80), ("2S", 1.25e6, 30)])
def test_channel_through_the_cpp_mirror(mirror_bin, tmp_path, signal, fs, epochs):
    sync = B.b3i_sync if signal == "B3" else B.l2c_sync
    sat, k, x, stamp, first, delay, dop = sync(fs, epochs, rotator_avx=1)
    ref = T.track(k, x, sat.code, delay, dop, stamp, first, epochs, buffer_first=first)
    assert len(ref) == epochs and ref["state"][-1] == 4
    if_path, out_path = tmp_path / "if.bin", tmp_path / "rec.bin"
    x.tofile(if_path)
    r = subprocess.run([mirror_bin, signal, str(if_path), repr(fs), str(sat.prn), repr(float(delay)), repr(float(dop)), str(stamp), str(first),
                        str(epochs), str(out_path)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    rec = np.fromfile(out_path, abi.TRK_EPOCH_DTYPE)
    assert len(rec) == epochs
    compare_exact(rec, ref, f"{signal} C++ mirror")
