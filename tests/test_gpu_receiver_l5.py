"""The Channel role on GPS L5 (tools/gnsship_rx --signal L5 over include/gnsship_receiver.hpp): the same
FSM as the L1 channels, acquisition on L5I (GpsL5iPcpsAcquisition's parameters), hand-over to tracking
of the L5Q pilot with the L5I data prompt.  The CPU restatement of the receiver (oracle/receiver.py)
knows GPS L1 only, so the tracking records are compared with the oracle LOOP started from the
acquisition outcome the tool reports (every field equal), and the acquisition outcome with the truth."""
import os
import subprocess

import numpy as np
import pytest

from gnss_sim_receiver_amd import abi
from oracle import trk as T

import l5_scenarios as L5
from test_gpu_trk import compare_exact

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RX = os.path.join(ROOT, "tools", "gnsship_rx")
FS = 12500000
REC = np.dtype([("channel", "<i4"), ("prn", "<i4"), ("e", abi.TRK_EPOCH_DTYPE)])


def test_l5_acquisition_to_pilot_tracking(tmp_path):
    from gnss_sim_receiver_amd import signals
    assert os.path.exists(RX), "tools/gnsship_rx is not built (make tools/gnsship_rx)"
    sat = L5.satellite(prn=9, dop=1210.0, delay_chips=3100.3, cn0=50.0)
    x = signals.generate_if(float(FS), int(0.3 * FS), [sat], seed=0x15)
    path = tmp_path / "l5.dat"
    x.tofile(path)
    ev, rec = str(tmp_path / "events.csv"), str(tmp_path / "records.bin")
    cmd = [RX, "--file", str(path), "--signal", "L5", "--fs", str(FS), "--channels", "1", "--in-acquisition", "1", "--satellite", "0:9",
           "--doppler-max", "5000", "--doppler-step", "250", "--rotator", "avx", "--pull-in-time-s", "0", "--block-ms", "100",
           "--events", ev, "--records", rec]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    events = np.loadtxt(ev, delimiter=",", skiprows=1, ndmin=2)  # sample, channel, what, prn, doppler, delay, statistic
    pos = events[events[:, 2] == 1]
    assert len(pos) == 1 and int(pos[0, 3]) == 9
    assert abs(pos[0, 4] - sat.doppler_hz) <= 125.0  # the nearest 250 Hz bin
    # Acq_delay_samples: the code start relative to the 12500-sample search window (which ends where the
    # positive decision took effect), modulo the 1 ms code period, within a sample of the truth
    window_start = int(pos[0, 0]) - 12500
    truth = (sat.code_delay_chips / sat.code_freq() * FS - window_start) % 12500
    assert min(abs(pos[0, 5] - truth), 12500 - abs(pos[0, 5] - truth)) <= 1.5
    recs = np.fromfile(rec, REC)
    mine = recs[recs["channel"] == 0]["e"]
    assert len(mine) > 150 and np.all(recs["prn"] == 9)
    # (a 0.3 s file ends inside the pull-in: counted from the acquisition stamp it lasts until the first
    # whole second, dll_pll_veml_tracking.cc:1746-1752, so the channel is still in state 2 — as the oracle's)
    assert abs(mine["carrier_doppler_hz"][-1] - sat.doppler_hz) < 5.0
    # the oracle loop from the same hand-over: in blocking mode the decision takes effect where the
    # acquisition's sample counter stands (the end of its 12500-sample window) — Acq_samplestamp_samples
    # and the first tracking sample are that position
    first = stamp = int(pos[0, 0])
    k = L5.conf(float(FS), rotator_avx=1, pll_bw_hz=40.0, dll_bw_hz=4.0)  # gnsship_rx's loop bandwidths
    ref = T.track(k, x, sat.code, float(pos[0, 5]), float(pos[0, 4]), stamp, first, len(mine), data_code=sat.code_data, buffer_first=0)
    compare_exact(mine, ref, "L5 receiver channel")
