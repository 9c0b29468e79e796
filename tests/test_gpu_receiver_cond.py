"""The receiver core with the signal conditioner ahead of its channels (tools/gnsship_rx --if-hz / --decimation
over Gnss_Receiver_Hip::work_raw, include/gnsship_receiver.hpp): the GPS band of the dual-band ibyte file of
tests/cond_scenarios.py (16 Msps, GPS L1 C/A at +4 MHz, BeiDou B1I at −4 MHz) is translated to baseband and
decimated to 4 Msps on the device; acquisition and tracking run on the conditioned stream with the
channels' own IF at 0, as the reference's channels run behind its Signal_Conditioner
(gnss_flowgraph.cc:1008-1140; conf/gnss-sdr_BDS_B3I_GPS_L1_CA_ibyte.conf:41-96).

Checked: control events and tracking records equal oracle/receiver.py's run on the conditioned 4 Msps
stream (the device conditioner's own output, bit-identical however the stream is cut into calls —
tests/test_gpu_cond.py).  The receiver without the new options is pinned by tests/test_gpu_receiver*.py."""
import os

import numpy as np
import pytest

from gnss_sim_receiver_amd import abi, engine

import cond_scenarios as C
import test_gpu_receiver as R

pytestmark = pytest.mark.gpu


def test_receiver_behind_the_conditioner_matches_oracle(ctx, tmp_path):
    raw, _ = C.raw_stream()
    b = C.BANDS["GPS"]
    fs_out = C.fs_out("GPS")
    assert fs_out == R.FS
    path = tmp_path / "dual_band_ibyte.dat"
    raw.tofile(path)
    assert os.path.exists(R.RX), "tools/gnsship_rx is not built (make tools/gnsship_rx)"
    ev, rec, dump = str(tmp_path / "events.csv"), str(tmp_path / "records.bin"), str(tmp_path / "trk_ch_")
    import subprocess
    cmd = [R.RX, "--file", str(path), "--item", "ibyte", "--fs", str(C.FS), "--if-hz", str(b["if_hz"]), "--decimation", str(b["decim"]),
           "--channels", "3", "--in-acquisition", "1", "--rotator", "avx", "--block-ms", "100", "--acq-piece", "8192",
           "--satellite", "0:7", "--satellite", "1:19", "--satellite", "2:3", "--events", ev, "--records", rec, "--dump", dump]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    events = np.loadtxt(ev, delimiter=",", skiprows=1, ndmin=2)
    recs = np.fromfile(rec, R.REC)

    # the same conditioned stream, from the library's conditioner in one call
    h = engine.cond_lowpass_taps(ctx.lib, float(C.FS), b["decim"])
    cond = engine.SignalConditioner(ctx, C.FS, [(b["if_hz"], b["decim"], h)], C.N_IN)
    (y,) = cond.run(raw)
    cond.close()
    rx = R.oracle_rx(y, satellite=[7, 19, 3])
    assert R.compare(events, recs, rx, dump) == 2
    pos = events[events[:, 2] == 1]
    assert sorted(pos[:, 3].astype(int).tolist()) == [7, 19]
    for prn, dop in ((7, 1730.0), (19, -2270.0)):
        assert abs(pos[pos[:, 3] == prn][0][4] - dop) <= 250.0  # within a Doppler bin of the truth, the IF removed


def test_conditioner_options_are_checked(tmp_path):
    """A bad conditioner option is a usage error (exit status 2, the reason on stderr), found before the device is used."""
    import subprocess
    path = tmp_path / "empty.dat"
    np.zeros(64, np.int8).tofile(path)
    for extra, why in ((["--decimation", "3"], "--decimation must divide --fs"),
                       (["--if-hz", "4000000.5"], "whole numbers of Hz"),
                       (["--decimation", "4", "--filter-bw", "9000000"], "--filter-bw must lie in"),
                       (["--decimation", "4", "--filter-tw", "-1"], "--filter-tw be positive"),
                       (["--decimation", "4", "--filter-tw", "10"], "more than 4096 taps")):
        out = subprocess.run([R.RX, "--file", str(path), "--item", "ibyte", "--fs", "16000000", *extra], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and why in out.stderr, (extra, out.returncode, out.stderr)
