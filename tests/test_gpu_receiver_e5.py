"""The Channel role on Galileo E5a / E5b (tools/gnsship_rx --signal 5X / --signal 7X over
include/gnsship_receiver.hpp): the same FSM as the other channels, acquisition on the I component with the two
adapters' parameters and hand-over to tracking on the Q pilot with the I component on the data prompt.

oracle/receiver.py restates the receiver for GPS L1 only and cannot be configured for these signals without editing
it, so — as tests/test_gpu_receiver_b3i_l2c.py does — the tool's tracking records are compared with the oracle LOOP
started from the acquisition outcome the tool reports (every field equal), and the acquisition outcome with the truth.

The pull-in lasts until the first whole second after the acquisition stamp (dll_pll_veml_tracking.cc:1741), so the
0.3 s files (12.5 Msps) end in state 2, as the oracle's; the synchronisation on the satellite's own secondary code and
the exchanged symbols are compared through the same C++ classes in tests/test_cpp_mirror_e5.py."""
import os
import subprocess

import numpy as np
import pytest

from gnss_sim_receiver_amd import abi, signals
from oracle import trk as T

import e5_scenarios as E
from test_gpu_trk import compare_exact

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RX = os.path.join(ROOT, "tools", "gnsship_rx")
REC = np.dtype([("channel", "<i4"), ("prn", "<i4"), ("e", abi.TRK_EPOCH_DTYPE)])
PRN = 9


def run_rx(tmp_path, x, signal, fs, dmax, dstep):
    assert os.path.exists(RX), "tools/gnsship_rx is not built (make tools/gnsship_rx)"
    path = tmp_path / "if.dat"
    x.tofile(path)
    ev, rec = str(tmp_path / "events.csv"), str(tmp_path / "records.bin")
    cmd = [RX, "--file", str(path), "--signal", signal, "--fs", str(fs), "--channels", "1", "--in-acquisition", "1", "--satellite", f"0:{PRN}",
           "--doppler-max", str(dmax), "--doppler-step", str(dstep), "--rotator", "avx", "--pull-in-time-s", "0", "--block-ms", "100",
           "--events", ev, "--records", rec]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    events = np.loadtxt(ev, delimiter=",", skiprows=1, ndmin=2)  # sample, channel, what, prn, doppler, delay, statistic
    pos = events[events[:, 2] == 1]
    assert len(pos) == 1 and int(pos[0, 3]) == PRN
    recs = np.fromfile(rec, REC)
    assert np.all(recs["prn"] == PRN)
    return pos[0], recs[recs["channel"] == 0]["e"]


# the first search window straddles code periods −1 and 0: the symbol pattern keeps the I component's sign across
# them (E5a-I's secondary chips 19 and 0 are equal, E5b-I's chips 3 and 0 differ, so its symbol changes there), and
# the sign at which the pilot's cross-correlation adds to the I peak instead of eating into it
@pytest.mark.parametrize("signal,band,bits", [("5X", "a", "0110"), ("7X", "b", "0001")])
def test_acquisition_to_tracking(tmp_path, signal, band, bits):
    fs = 12500000
    sat = E.satellite(band, prn=PRN, dop=1210.0, delay_chips=3100.3, cn0=50.0)
    sat.bits = bits
    x = signals.generate_if(float(fs), int(0.3 * fs), [sat], seed=0x15)
    pos, mine = run_rx(tmp_path, x, signal, fs, 5000, 250)
    assert abs(pos[4] - sat.doppler_hz) <= 125  # the nearest bin
    window_start = int(pos[0]) - 12500
    truth = (sat.code_delay_chips / sat.code_freq() * fs - window_start) % 12500
    assert min(abs(pos[5] - truth), 12500 - abs(pos[5] - truth)) <= 1.5
    assert len(mine) > 150
    assert abs(mine["carrier_doppler_hz"][-1] - sat.doppler_hz) < 5.0
    # the oracle loop from the same hand-over: the decision takes effect where the acquisition's sample counter
    # stands (the end of its window) — Acq_samplestamp_samples and the first tracking sample
    first = stamp = int(pos[0])
    k = E.conf(band, float(fs), PRN, True, rotator_avx=1, pll_bw_hz=40.0, dll_bw_hz=4.0)  # gnsship_rx's loop bandwidths
    code, data = E.replicas(sat, True)
    ref = E.exchanged(T.track(k, x, code, float(pos[5]), float(pos[4]), stamp, first, len(mine), data_code=data, buffer_first=0))
    compare_exact(mine, ref, f"{signal} receiver channel")
