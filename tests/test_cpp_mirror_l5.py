"""GPS L5 through the C++ mirror (include/gnsship_cpp.hpp): tests/cpp/l5_mirror_test tracks one L5 channel
with Dll_Pll_Veml_Tracking_Hip (system 'G', signal "L5", the mirror's L5 code generators) over an IF file
and writes its epoch records, which equal the oracle loop's (test_gpu_trk.compare_exact)."""
import os
import subprocess

import numpy as np
import pytest

from gnss_sim_receiver_amd import abi
from oracle import trk as T

import l5_scenarios as L5
from test_gpu_trk import compare_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "l5_mirror_test")


@pytest.fixture(scope="module")
def l5_bin(built):
    if not os.path.exists(BIN):
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/l5_mirror_test"], check=True)
    return BIN


@pytest.mark.gpu
def test_l5_channel_through_the_cpp_mirror(l5_bin, tmp_path):
    fs, epochs = 12.5e6, 80
    sat, k, x, stamp, first, delay, dop = L5.sync(fs, epochs, rotator_avx=1)
    ref = T.track(k, x, sat.code, delay, dop, stamp, first, epochs, data_code=sat.code_data, buffer_first=first)
    assert len(ref) == epochs and ref["state"][-1] == 4
    if_path, out_path = tmp_path / "l5_if.bin", tmp_path / "l5_rec.bin"
    x.tofile(if_path)
    r = subprocess.run([l5_bin, str(if_path), repr(fs), str(sat.prn), repr(float(delay)), repr(float(dop)), str(stamp), str(first), str(epochs),
                        str(out_path)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "data-only tracking refused" in r.stdout and "interchange_iq" in r.stdout
    rec = np.fromfile(out_path, abi.TRK_EPOCH_DTYPE)
    assert len(rec) == epochs
    compare_exact(rec, ref, "L5 C++ mirror")
