"""Galileo E5a / E5b through the C++ mirror (include/gnsship_cpp.hpp): tests/cpp/e5_mirror_test writes the codes of
the mirror's generators (compared here with the C ABI's), and tracks one channel with Dll_Pll_Veml_Tracking_Hip
(system 'E', signal "5X" / "7X", the X primary split as the block splits it) over an IF file; its epoch records equal
the oracle loop's with the valid symbols' I and Q exchanged (test_gpu_trk.compare_exact).  The program leaves
vector_length at 0 and asks for extend_correlation_symbols 0 (pilot) / 25 (data-only): the mirror applies the
adapters' vector_length and limits."""
import os
import subprocess

import numpy as np
import pytest

from gnss_sim_receiver_amd import abi, codes

import e5_scenarios as E
from test_gpu_trk import compare_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "e5_mirror_test")


@pytest.fixture(scope="module")
def mirror_bin(built):
    if not os.path.exists(BIN):
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/e5_mirror_test"], check=True)
    return BIN


def test_mirror_generators_equal_the_c_abi(mirror_bin, tmp_path):
    out = tmp_path / "codes.bin"
    r = subprocess.run([mirror_bin, "codes", str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split()
    assert lines[0] == codes.galileo_e5a_q_secondary(11) and lines[1] == codes.galileo_e5b_q_secondary(50)
    assert "out-of-range PRNs refused" in r.stdout
    got = np.fromfile(out, np.float32).view(np.complex64)
    want = np.concatenate([codes.galileo_e5_a_code_gen_complex_primary(11, "5X"), codes.galileo_e5_b_code_gen_complex_primary(50, "7Q"),
                           codes.galileo_e5_a_code_gen_complex_sampled(1, "5I", 12500000, 3),
                           codes.galileo_e5_b_code_gen_complex_sampled(50, "7X", 10000000, 0)])
    assert np.array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("signal,pilot,prn", [("5X", 1, 11), ("7X", 1, 50), ("5X", 0, 11), ("7X", 0, 11)])
def test_channel_through_the_cpp_mirror(mirror_bin, tmp_path, signal, pilot, prn):
    band = "a" if signal == "5X" else "b"
    fs = 12.5e6
    epochs = E.EPOCHS[band] if pilot else 260  # data-only: synchronised by epoch 30, the extension then shows within 260
    sat, k, x, stamp, first, delay, dop = E.sync(band, fs, epochs=epochs, prn=prn, pilot=bool(pilot), rotator_avx=1,
                                                 extend_correlation_symbols=1 if pilot else 25)
    assert k.extend_correlation_symbols == (1 if pilot else len(E.BAND[band][2]))
    ref = E.track(sat, k, x, stamp, first, delay, dop, epochs, pilot=bool(pilot))
    assert len(ref) == epochs and np.any(ref["state"][:230] == 4) and not np.any(ref["flags"] & 2)
    assert np.count_nonzero(ref["flags"] & 1) >= (20 if pilot else 8)
    if_path, out_path = tmp_path / "if.bin", tmp_path / "rec.bin"
    x.tofile(if_path)
    r = subprocess.run([mirror_bin, signal, str(pilot), str(if_path), repr(fs), str(sat.prn), repr(float(delay)), repr(float(dop)), str(stamp),
                        str(first), str(epochs), str(out_path)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    rec = np.fromfile(out_path, abi.TRK_EPOCH_DTYPE)
    assert len(rec) == epochs
    compare_exact(rec, ref, f"{signal} pilot={pilot} C++ mirror")
