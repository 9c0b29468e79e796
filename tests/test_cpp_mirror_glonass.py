"""GLONASS L1 / L2 C/A acquisition through the C++ mirror (include/gnsship_cpp.hpp): tests/cpp/glonass_mirror_test prints
the conf helpers' derived sizes and the bias per PRN (compared here with the reference's values in
tests/golden/glonass_ref.npz) and writes the mirror's codes (compared with the C ABI's); on the GPU it runs the FDMA
sweep and the per-PRN grid of Pcps_Acquisition_Hip over an IF file, compared with the Python binding's results."""
import os
import subprocess

import numpy as np
import pytest

from gnss_sim_receiver_amd import codes, engine, signals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "glonass_mirror_test")
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "glonass_ref.npz"))


@pytest.fixture(scope="module")
def mirror_bin(built):
    if not os.path.exists(BIN):
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/glonass_mirror_test"], check=True)
    return BIN


def test_conf_helpers_derived_sizes_and_bias_per_prn(mirror_bin, tmp_path):
    out = tmp_path / "codes.bin"
    r = subprocess.run([mirror_bin, "conf", str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    # glonass_l1_ca_pcps_acquisition.cc:49-66 at 6.625 Msps, sampled_ms 2: ms_per_code 1, 511 kcps, ceil(6.625e6 / 511e3) = 13
    # samples per chip, 6625 samples per code, no resampler (optimum rate 100e6), the local code two copies of 6625
    for band in (1, 2):
        assert lines[band - 1] == (f"conf {band} ms_per_code 1 chips_per_second 511000 samples_per_chip 13 samples_per_code 6625.0 "
                                   "resampled_fs 6625000 ratio 1.0 code 13250 copies 1")
    f1, d1, f2, d2 = GOLD["constants"][:4]
    table = {int(p): int(k) for p, k in GOLD["prn_table"]}
    for prn in range(25):
        k = table[prn]
        assert lines[2 + prn] == f"prn {prn} k {k} bias1 {int(d1 * k)} bias2 {int(d2 * k)}"
    # glonass_l1_ca_dll_pll_tracking.cc:44-62: pll 50, dll 2, spacing 0.5, vector_length round(fs / 1000); the generic rotator (0)
    for band in (1, 2):
        assert lines[26 + band] == (f"trk {band} system R signal {band}G pll 50.0 dll 2.0 spacing 0.50 vector_length 6625 max_lock_fail 50 "
                                    "pilot 0 rotator 0 if 1000.0")
    assert lines[29] == "PRN 25 refused"
    got = np.fromfile(out, np.float32).view(np.complex64)
    want = np.concatenate([codes.glonass_l1_ca_code_gen_complex(3), codes.glonass_l2_ca_code_gen_complex_sampled(6625000)])
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_fdma_sweep_and_per_prn_grid_through_the_cpp_mirror(ctx, mirror_bin, tmp_path):
    fs, n, chans, prn = 4000000, 4000, [-3, -1, 0, 2], 24  # PRN 24: channel 2
    assert codes.glonass_freq_channel(prn) == 2
    sats = [signals.Satellite(prn=prn, doppler_hz=3000.0, code_delay_chips=450.2, cn0_dbhz=47.0, system="GLO_L1"),
            signals.Satellite(prn=18, doppler_hz=-2000.0, code_delay_chips=100.3, cn0_dbhz=47.0, system="GLO_L1")]  # PRN 18: channel -3
    x = signals.generate_if(fs, n, sats, seed=24)
    path = tmp_path / "if.bin"
    x.tofile(path)
    r = subprocess.run([mirror_bin, "acq", str(path), str(fs), str(prn)] + [str(k) for k in chans], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    acq = engine.glonass_l1_ca_pcps_acquisition(ctx, fs, 5000, 500, freq_channels=chans)
    res, _ = acq.run_fdma(x)
    acq.close()

    def same(text, r, positive):
        dop, delay, stat, pos = text.split()  # %.1f, %.17g, %.9g (a float round-trips), 0 / 1
        return (float(dop), float(delay), np.float32(stat), int(pos)) == (float(r.doppler_hz), r.acq_delay_samples, np.float32(r.test_statistic),
                                                                          positive)

    for g, k in enumerate(chans):
        assert same(lines[g], res[g], 1 if k in (-3, 2) else 0), (k, lines[g], res[g].test_statistic)
    # the block's own grid under PRN 24's bias: the same channel, Doppler reported without the bias
    assert lines[4] == f"bias {codes.glonass_doppler_bias_hz('1G', 2)}"
    assert same(lines[5], res[3], 1), lines[5]
