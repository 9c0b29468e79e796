"""tools/gnsship_rx --lnav (include/gnsship_receiver.hpp Receiver_Conf::lnav): the opt-in GPS L1 C/A telemetry decoder
behind the 1C channels.  A subframe cannot appear before six seconds of signal have passed, so on a 0.3 s file the check
is what the option must leave alone: events, records and the summary stay byte for byte what they are without it and no
subframe line is printed.  The second test feeds the tool 14.4 s carrying built subframes and requires the printed lines
to be what tests/lnav_model.py gives on the tool's own records."""
import json
import os
import subprocess

import numpy as np
import pytest

import lnav_model as M
from gnss_sim_receiver_amd import abi, signals

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RX = os.path.join(ROOT, "tools", "gnsship_rx")
FS = 4000000  # the rate of the 1C receiver tests (tests/test_gpu_receiver.py)
REC = np.dtype([("channel", "<i4"), ("prn", "<i4"), ("e", abi.TRK_EPOCH_DTYPE)])


def run_rx(tmp_path, tag, path, signal, extra, channels=2):
    ev, rec = str(tmp_path / f"events_{tag}.csv"), str(tmp_path / f"records_{tag}.bin")
    cmd = [RX, "--file", str(path), "--signal", signal, "--fs", str(FS), "--channels", str(channels), "--in-acquisition", "1", "--satellite", "0:7",
           "--doppler-max", "5000", "--doppler-step", "250", "--rotator", "avx", "--pull-in-time-s", "0", "--block-ms", "100",
           "--events", ev, "--records", rec] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    return out, ev, rec


def test_lnav_option_leaves_the_receiver_outputs_alone(tmp_path):
    assert os.path.exists(RX), "tools/gnsship_rx is not built (make tools/gnsship_rx)"
    path = tmp_path / "if.dat"
    signals.generate_if(float(FS), int(0.3 * FS), signals.c1_sky(cn0=50.0), seed=0x17).tofile(path)
    off, ev0, rec0 = run_rx(tmp_path, "off", path, "1C", [])
    assert off.returncode == 0, off.stdout + off.stderr
    on, ev1, rec1 = run_rx(tmp_path, "on", path, "1C", ["--lnav"])
    assert on.returncode == 0, on.stdout + on.stderr
    assert open(ev0, "rb").read() == open(ev1, "rb").read()
    assert open(rec0, "rb").read() == open(rec1, "rb").read() and os.path.getsize(rec0) > 150 * 104
    assert not [l for l in on.stdout.splitlines() if l.startswith("subframe ")]
    a, b = json.loads(off.stdout.strip().splitlines()[-1]), json.loads(on.stdout.strip().splitlines()[-1])
    for k in ("samples", "acq_positive", "acq_negative", "losses", "channels"):
        assert a[k] == b[k], k
    bad, _, _ = run_rx(tmp_path, "bad", path, "7X", ["--lnav"])
    assert bad.returncode != 0 and "lnav" in bad.stderr
    bad, _, _ = run_rx(tmp_path, "bad2", path, "1C", ["--telemetry"])  # --telemetry stays the Galileo option
    assert bad.returncode != 0 and "telemetry" in bad.stderr


def test_subframes_from_the_receiver(tmp_path):
    """14.4 s of GPS PRN 7 at 4 Msps, 50 dB-Hz (8-bit samples, generated on the device piece by piece): two seconds of idle
    bits, then built subframes 1..5 with the TOW rising, two of them whole.  The tracker takes the first preamble pattern it
    meets once it looks for one as the bit synchronisation; in this receiver that is somewhat over a second after the
    start (with 0.2 s and with 1 s of idle bits it passed the first preamble by and aligned on a look-alike in the first
    subframe's data, 18 and 62 bits in), so the idle lead keeps everything but the true preamble away from it.
    Satellite.bits sends a '0' as +1, so the channel may lock inverted: either polarity is right.  The printed lines are
    the model's subframes over the tool's own records."""
    bits, words = M.five_subframes(31, tow0=2000)
    pattern = np.concatenate([np.zeros(100, np.uint8)] + bits)
    sat = signals.c1_sky(cn0=50.0)[0]
    sat.bits = "".join(str(int(b)) for b in pattern)
    n, step = int(14.4 * FS), int(0.9 * FS)
    path = tmp_path / "gps_lnav.dat"
    try:
        with open(path, "wb") as f:
            for a in range(0, n, step):  # one generator call per piece: each piece has its own noise seed, the signal is continuous
                x = signals.generate_if_device(float(FS), min(step, n - a), [sat], seed=0x19 + a // step, start=a, device="cuda")
                signals.to_ibyte(x.cpu().numpy()).tofile(f)
        out, _, rec_path = run_rx(tmp_path, "subframes", path, "1C", ["--item", "ibyte", "--lnav"], channels=1)
    finally:
        if os.path.exists(path):
            os.remove(path)
    assert out.returncode == 0, out.stdout + out.stderr
    assert json.loads(out.stdout.strip().splitlines()[-1])["losses"] == 0
    lines = [l for l in out.stdout.splitlines() if l.startswith("subframe ")]
    # the model over the tool's records: every epoch with flags & 1 is a symbol, flags & 4 its 180° flag
    rec = np.fromfile(rec_path, REC)
    e = rec[rec["channel"] == 0]["e"]
    sel = (e["flags"] & 1) != 0
    recs, fault, _, _ = M.LnavDecoder().run(e["prompt_i"][sel].astype(np.float32), e["sample_counter"][sel], (e["flags"][sel] & 4) != 0)
    want = ["subframe channel 0 prn 7 symbol %d id %d tow %d %s %s" % (r["symbol_counter"], r["subframe_id"], r["tow_s"],
                                                                       "ok" if r["flags"] & M.F_OK else "fail",
                                                                       " ".join("%08x" % w for w in r["words"])) for r in recs]
    assert lines == want and not fault, out.stdout
    ok = [l.split() for l in lines if l.split()[11] == "ok"]
    assert len(ok) >= 2, out.stdout
    built = {tuple("%08x" % w for w in ws): k for k, ws in enumerate(words)}
    which = [built.get(tuple(t[12:22])) for t in ok]
    assert None not in which, out.stdout
    for a, b, ka, kb in zip(ok, ok[1:], which, which[1:]):
        assert int(b[6]) - int(a[6]) == 300 and int(b[10]) - int(a[10]) == 6 and kb == ka + 1
        assert int(a[8]) == ka + 1 and int(a[10]) == 6 * (2000 + ka)
