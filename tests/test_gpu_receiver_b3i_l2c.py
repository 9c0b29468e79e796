"""The Channel role on BeiDou B3I and GPS L2C (tools/gnsship_rx --signal B3 / --signal 2S over
include/gnsship_receiver.hpp): the same FSM as the L1 channels, acquisition with the two adapters' parameters
and hand-over to tracking on the same code.  The CPU restatement of the receiver (oracle/receiver.py) knows
GPS L1 only, so the tracking records are compared with the oracle LOOP started from the acquisition outcome
the tool reports (every field equal), and the acquisition outcome with the truth.

The pull-in lasts until the first whole second after the acquisition stamp (dll_pll_veml_tracking.cc:1741), so
the 0.3 s B3I file (12.5 Msps) ends in state 2, as the oracle's; the 1.5 s L2C file (1.25 Msps, 75 epochs of
20 ms) goes on to state 4."""
import os
import subprocess

import numpy as np
import pytest

from gnss_sim_receiver_amd import abi, signals
from oracle import trk as T

import b3i_l2c_scenarios as B
from test_gpu_trk import compare_exact

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RX = os.path.join(ROOT, "tools", "gnsship_rx")
REC = np.dtype([("channel", "<i4"), ("prn", "<i4"), ("e", abi.TRK_EPOCH_DTYPE)])


def run_rx(tmp_path, x, signal, fs, dmax, dstep, extra=()):
    assert os.path.exists(RX), "tools/gnsship_rx is not built (make tools/gnsship_rx)"
    path = tmp_path / "if.dat"
    x.tofile(path)
    ev, rec = str(tmp_path / "events.csv"), str(tmp_path / "records.bin")
    cmd = [RX, "--file", str(path), "--signal", signal, "--fs", str(fs), "--channels", "1", "--in-acquisition", "1", "--satellite", "0:9",
           "--doppler-max", str(dmax), "--doppler-step", str(dstep), "--rotator", "avx", "--pull-in-time-s", "0", "--block-ms", "100",
           "--events", ev, "--records", rec, *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    events = np.loadtxt(ev, delimiter=",", skiprows=1, ndmin=2)  # sample, channel, what, prn, doppler, delay, statistic
    pos = events[events[:, 2] == 1]
    assert len(pos) == 1 and int(pos[0, 3]) == 9
    recs = np.fromfile(rec, REC)
    assert np.all(recs["prn"] == 9)
    return pos[0], recs[recs["channel"] == 0]["e"]


def check_acquisition(pos, sat, fs, window, dstep):
    assert abs(pos[4] - sat.doppler_hz) <= dstep / 2  # the nearest bin
    # Acq_delay_samples: the code start relative to the search window (which ends where the positive decision
    # took effect), modulo the code period, within a sample and a half of the truth
    window_start = int(pos[0]) - window
    truth = (sat.code_delay_chips / sat.code_freq() * fs - window_start) % window
    assert min(abs(pos[5] - truth), window - abs(pos[5] - truth)) <= 1.5


def test_b3i_acquisition_to_tracking(tmp_path):
    fs = 12500000
    sat = B.b3i_satellite(prn=9, dop=1210.0, delay_chips=3100.3, cn0=50.0)
    # the first search window straddles code periods −1 and 0: a bit pattern ending in '0' (and NH20's chips 19 and
    # 0) keeps one sign across it (a sign change there splits the 1 ms coherent sum and moves the Doppler peak)
    sat.bits = "0110"
    x = signals.generate_if(float(fs), int(0.3 * fs), [sat], seed=0x15)
    pos, mine = run_rx(tmp_path, x, "B3", fs, 5000, 250)
    check_acquisition(pos, sat, fs, 12500, 250)
    assert len(mine) > 150
    assert abs(mine["carrier_doppler_hz"][-1] - sat.doppler_hz) < 5.0
    # the oracle loop from the same hand-over: in blocking mode the decision takes effect where the acquisition's
    # sample counter stands (the end of its window) — Acq_samplestamp_samples and the first tracking sample
    first = stamp = int(pos[0])
    k = B.b3i_conf(float(fs), rotator_avx=1, pll_bw_hz=40.0, dll_bw_hz=4.0)  # gnsship_rx's loop bandwidths
    ref = T.track(k, x, sat.code, float(pos[5]), float(pos[4]), stamp, first, len(mine), buffer_first=0)
    compare_exact(mine, ref, "B3I receiver channel")


def test_l2c_acquisition_to_tracking_reaches_state_4(tmp_path):
    fs = 1250000
    sat = B.l2c_satellite(prn=9, dop=1203.0, delay_chips=3100.3, cn0=45.0)
    x = signals.generate_if(float(fs), int(1.5 * fs), [sat], seed=0x15)
    # 25 Hz bins: a 20 ms coherent search resolves 2/(3T) = 33 Hz (gps_l2_m_pcps_acquisition.cc:112-113)
    pos, mine = run_rx(tmp_path, x, "2S", fs, 2000, 25, extra=("--pll-bw", "2", "--dll-bw", "0.25"))
    check_acquisition(pos, sat, fs, 25000, 25)
    assert len(mine) > 60
    assert mine["state"][-1] == 4 and abs(mine["carrier_doppler_hz"][-1] - sat.doppler_hz) < 5.0
    first = stamp = int(pos[0])
    k = B.l2c_conf(float(fs), rotator_avx=1)  # pll 2 Hz, dll 0.25 Hz
    ref = T.track(k, x, sat.code, float(pos[5]), float(pos[4]), stamp, first, len(mine), buffer_first=0)
    assert ref["state"][-1] == 4
    compare_exact(mine, ref, "L2C receiver channel")
