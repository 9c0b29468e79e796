"""Interference mitigation end to end: the C1 sky (GPS PRN 7, 4 Msps) under a CW jammer through the notch filter and
under pulses through the pulse blanking, each into the PCPS acquisition.

CPU side (no GPU): the scenario means something — on the model, the acquisition statistic of the unmitigated stream
is below half the threshold (pfa 0.01) and that of the mitigated stream above twice the threshold.
GPU side: the device acquisition of the device-mitigated stream equals the oracle acquisition of the model's output
(PRN 7's Doppler bin and delay exactly, the statistic to the acquisition tests' 2e-4), and tools/gnsship_rx
--input-filter notch over the same file reports the control events oracle/receiver.py gives on the model's output.
"""
import os
import subprocess

import numpy as np
import pytest

from gnss_sim_receiver_amd import codes, engine, signals
from oracle import oracle as O
from oracle.receiver import calculate_threshold

import mit_model as M
import mit_scenarios as S

FS, N_MS = 4000000, 4000
N = 16 * N_MS            # 64000 samples
MS = 5                   # the millisecond acquired
DMAX, DSTEP = 5000, 250
N_EST = 1                # one estimation segment: the jammer is there from the first sample
CN0 = {"notch": 52.0, "pulse-blanking": 50.0}
_CACHE = {}


def scenario(kind):
    """(jammed stream, model output, threshold of the filter)."""
    if kind not in _CACHE:
        sig = signals.generate_if(FS, N, signals.c1_sky(CN0[kind]), seed=21)
        if kind == "notch":
            x = (sig + 8.0 * np.exp(2j * np.pi * 0.0431 * np.arange(N))).astype(np.complex64)
            th = S.thres_pfa(0.001, 32)
            m = M.Model(M.NOTCH, th, 32, N_EST, 5000000, p_c=0.9)
        else:
            x = sig.copy()
            carrier = (80.0 * np.exp(2j * np.pi * 0.0431 * np.arange(N))).astype(np.complex64)
            for p in range(700, N, 1000):  # DME-like: a pulsed carrier, 96 of every 1000 samples
                x[p:p + 96] += carrier[p:p + 96]
            th = S.thres_pfa(0.04, 32)
            m = M.Model(M.PULSE_BLANKING, th, 32, 8, 5000000)
        _CACHE[kind] = (x, m.run(x), th)
    return _CACHE[kind]


def oracle_acq(y):
    code = codes.gps_l1_ca_code_gen_complex_sampled(7, FS)
    r, _ = O.pcps_acquisition_core(np.ascontiguousarray(y[MS * N_MS:(MS + 1) * N_MS]), code, FS, DMAX, DSTEP, 0, True)
    return r


@pytest.mark.parametrize("kind", ["notch", "pulse-blanking"])
def test_scenario_needs_the_mitigation(kind):
    if kind == "notch":
        M.require_glibc()
    x, y, _ = scenario(kind)
    T = float(calculate_threshold(0.01, N_MS, 2 * DMAX // DSTEP + 1))
    before, after = oracle_acq(x), oracle_acq(y)
    print(f"{kind}: statistic / threshold {before.test_statistic / T:.3f} unmitigated, {after.test_statistic / T:.3f} mitigated")
    assert before.test_statistic <= T / 2 and after.test_statistic >= 2 * T
    assert after.doppler_hz == 1750 and abs(after.acq_delay_samples - 1234) <= 1


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["notch", "pulse-blanking"])
def test_acquisition_behind_the_mitigation_matches_oracle(ctx, kind):
    if kind == "notch":
        M.require_glibc()
    x, y, th = scenario(kind)
    f = engine.InterferenceMitigation(ctx, kind, N, threshold=th, p_c_factor=0.9, length=32, n_segments_est=N_EST if kind == "notch" else 8,
                                      n_segments_reset=5000000)
    dev, n_out = f.run(x, host=False)
    assert n_out == len(y)
    acq = engine.PcpsAcquisition(ctx, FS, N_MS, DMAX, DSTEP, 0, True)
    acq.set_local_code(codes.gps_l1_ca_code_gen_complex_sampled(7, FS))
    out = np.zeros(N_MS, np.complex64)  # the mitigated millisecond, from the device buffer the filter wrote
    engine.DeviceBuffer.wrap(ctx, dev, 8 * n_out).download(out, 8 * MS * N_MS)
    (r,), _ = acq.run(out)
    acq.close()
    f.close()
    ref = oracle_acq(y)
    assert np.array_equal(out.view(np.uint32), y[MS * N_MS:(MS + 1) * N_MS].view(np.uint32))
    assert (r.doppler_index, r.code_index, r.doppler_hz) == (ref.doppler_index, ref.code_index, ref.doppler_hz)
    assert r.acq_delay_samples == ref.acq_delay_samples
    np.testing.assert_allclose([r.peak, r.input_power, r.test_statistic], [ref.peak, ref.input_power, ref.test_statistic], rtol=2e-4)


@pytest.mark.gpu
def test_gnsship_rx_input_filter_notch_matches_oracle_receiver(built, tmp_path):
    M.require_glibc()
    import test_gpu_receiver as R
    x, y, _ = scenario("notch")
    path = tmp_path / "c1_cw.dat"
    x.tofile(path)
    ev = str(tmp_path / "events.csv")
    assert os.path.exists(R.RX), "tools/gnsship_rx is not built (make tools/gnsship_rx)"
    cmd = [R.RX, "--file", str(path), "--item", "gr_complex", "--fs", str(FS), "--channels", "1", "--in-acquisition", "1", "--rotator", "avx",
           "--block-ms", "100", "--acq-piece", "8192", "--satellite", "0:7", "--events", ev,
           "--input-filter", "notch", "--segments-est", str(N_EST), "--segment-length", "32", "--p-c-factor", "0.9"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    events = np.loadtxt(ev, delimiter=",", skiprows=1, ndmin=2)
    rx = R.oracle_rx(y, channels=1, satellite=[7])
    ref = rx.events
    assert len(ref) >= 1 and events.shape[0] == len(ref)
    np.testing.assert_array_equal(events[:, :4], np.array([e[:4] for e in ref], np.float64))
    pos = [(e, r) for e, r in zip(events, ref) if r[2] == 1]
    assert pos and int(pos[0][1][3]) == 7
    for e, r in pos:
        assert e[4] == r[4] and e[5] == r[5] and abs(e[6] - r[6]) <= 1e-3 * abs(r[6]), (e, r)
