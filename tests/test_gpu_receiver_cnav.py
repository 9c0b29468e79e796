"""tools/gnsship_rx --cnav (include/gnsship_receiver.hpp Receiver_Conf::cnav): the opt-in GPS CNAV telemetry decoder behind
the 2S and L5 channels.

A whole message through the receiver needs 300 bits and the decoder's tail behind it: about 7 s of L5 signal (10 ms
symbols) or 14 s of L2C signal (20 ms symbols), after the tracker's pull-in.  That is deliberately not a GPU test: files
of that length take minutes to make and to track, and the decoder itself is held against the model on whole messages in
tests/test_gpu_cnav.py.  Here, on a short L2C file (1.5 s: the channel reaches state 4 and hands over symbols) and a short
L5 file (0.3 s: the channel is still in its pull-in, no symbol yet), the check is what the option must leave alone —
events, records and the summary stay byte for byte what they are without it, and no message line is printed — and that
the decoder's per-channel state after the run is the model's after the symbols of the tool's own records."""
import json
import os
import subprocess

import numpy as np
import pytest

import cnav_model as M
from gnss_sim_receiver_amd import abi, signals
from test_cpp_mirror_cnav import state_line

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RX = os.path.join(ROOT, "tools", "gnsship_rx")
REC = np.dtype([("channel", "<i4"), ("prn", "<i4"), ("e", abi.TRK_EPOCH_DTYPE)])


def run_rx(tmp_path, tag, path, signal, fs, dmax, dstep, extra):
    ev, rec = str(tmp_path / f"events_{tag}.csv"), str(tmp_path / f"records_{tag}.bin")
    cmd = [RX, "--file", str(path), "--signal", signal, "--fs", str(fs), "--channels", "1", "--in-acquisition", "1", "--satellite", "0:9",
           "--doppler-max", str(dmax), "--doppler-step", str(dstep), "--rotator", "avx", "--pull-in-time-s", "0", "--block-ms", "100",
           "--events", ev, "--records", rec] + list(extra)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    return out, ev, rec


def check_option(tmp_path, path, signal, fs, dmax, dstep, extra, mode, prompt):
    off, ev0, rec0 = run_rx(tmp_path, "off", path, signal, fs, dmax, dstep, extra)
    assert off.returncode == 0, off.stdout + off.stderr
    on, ev1, rec1 = run_rx(tmp_path, "on", path, signal, fs, dmax, dstep, list(extra) + ["--cnav"])
    assert on.returncode == 0, on.stdout + on.stderr
    assert open(ev0, "rb").read() == open(ev1, "rb").read()
    assert open(rec0, "rb").read() == open(rec1, "rb").read() and os.path.getsize(rec0) > 60 * 104
    assert not [l for l in on.stdout.splitlines() if l.startswith("message ")]
    assert not [l for l in off.stdout.splitlines() if l.startswith("cnav-state ")]
    a, b = json.loads(off.stdout.strip().splitlines()[-1]), json.loads(on.stdout.strip().splitlines()[-1])
    for k in ("samples", "acq_positive", "acq_negative", "losses", "channels"):
        assert a[k] == b[k], k
    assert b["losses"] == 0 and b["acq_positive"] == 1
    # the decoder's state: a new object when the channel was given its satellite, then every symbol of the records
    e = np.fromfile(rec1, REC)
    e = e[e["channel"] == 0]["e"]
    sel = (e["flags"] & 1) != 0
    blk = M.CnavBlock(mode)
    recs, fault, _, _ = blk.run(e[prompt][sel], sample_counters=e["sample_counter"][sel])
    assert not recs and not fault
    got = [l.split() for l in on.stdout.splitlines() if l.startswith("cnav-state ")]
    want = state_line(0, blk.state())
    want[0] = "cnav-state"
    assert len(got) == 1 and float(got[0][4]) == float(want[4]) and got[0][:4] + got[0][5:] == want[:4] + want[5:], (got, want)
    return int(sel.sum())


def test_cnav_option_on_l2c(tmp_path):
    import b3i_l2c_scenarios as B
    assert os.path.exists(RX), "tools/gnsship_rx is not built (make tools/gnsship_rx)"
    fs = 1250000
    sat = B.l2c_satellite(prn=9, dop=1203.0, delay_chips=3100.3, cn0=45.0)
    path = tmp_path / "l2c.dat"
    signals.generate_if(float(fs), int(1.5 * fs), [sat], seed=0x15).tofile(path)
    n_sym = check_option(tmp_path, path, "2S", fs, 2000, 25, ["--pll-bw", "2", "--dll-bw", "0.25"], M.L2C, "prompt_i")
    assert n_sym >= 5  # the channel reached state 4: symbols went through the decoder
    for signal in ("1C", "7X"):
        bad, _, _ = run_rx(tmp_path, "bad" + signal, path, signal, fs, 2000, 25, ["--cnav"])
        assert bad.returncode != 0 and "cnav" in bad.stderr
    bad, _, _ = run_rx(tmp_path, "bad_lnav", path, "2S", fs, 2000, 25, ["--lnav"])  # --lnav and --telemetry keep their meaning
    assert bad.returncode != 0 and "lnav" in bad.stderr
    bad, _, _ = run_rx(tmp_path, "bad_tlm", path, "2S", fs, 2000, 25, ["--telemetry"])
    assert bad.returncode != 0 and "telemetry" in bad.stderr


def test_cnav_option_on_l5(tmp_path):
    import l5_scenarios as L5
    assert os.path.exists(RX), "tools/gnsship_rx is not built (make tools/gnsship_rx)"
    fs = 12500000
    sat = L5.satellite(prn=9, dop=1210.0, delay_chips=3100.3, cn0=50.0)
    path = tmp_path / "l5.dat"
    signals.generate_if(float(fs), int(0.3 * fs), [sat], seed=0x15).tofile(path)
    check_option(tmp_path, path, "L5", fs, 5000, 250, [], M.L5, "prompt_q")
