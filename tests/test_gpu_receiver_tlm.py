"""tools/gnsship_rx --telemetry (include/gnsship_receiver.hpp Receiver_Conf::telemetry): the opt-in telemetry framing
behind the Galileo E5b channels.  A page part cannot appear before required + 1 + 2·period symbols (over four seconds of
signal) have passed, so on the 0.3 s file of tests/test_gpu_receiver_e5.py the check is what the option must leave
alone: every tracking block's device records go through the decoder, and events, records and the summary stay byte for
byte what they are without it; no page line is printed; the option is refused where there is no Galileo telemetry.
The second test feeds the tool 7.6 s carrying built I/NAV parts and reads them back from its page lines."""
import json
import os
import subprocess

import pytest

from gnss_sim_receiver_amd import signals

import e5_scenarios as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RX = os.path.join(ROOT, "tools", "gnsship_rx")


def run_rx(tmp_path, tag, path, signal, fs, extra, channels=2):
    ev, rec = str(tmp_path / f"events_{tag}.csv"), str(tmp_path / f"records_{tag}.bin")
    cmd = [RX, "--file", str(path), "--signal", signal, "--fs", str(fs), "--channels", str(channels), "--in-acquisition", "1", "--satellite", "0:9",
           "--doppler-max", "5000", "--doppler-step", "250", "--rotator", "avx", "--pull-in-time-s", "0", "--block-ms", "100",
           "--events", ev, "--records", rec] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    return out, ev, rec


def test_telemetry_option_leaves_the_receiver_outputs_alone(tmp_path):
    assert os.path.exists(RX), "tools/gnsship_rx is not built (make tools/gnsship_rx)"
    fs = 12500000
    sat = E.satellite("b", prn=9, dop=1210.0, delay_chips=3100.3, cn0=50.0)
    sat.bits = "0001"
    path = tmp_path / "if.dat"
    signals.generate_if(float(fs), int(0.3 * fs), [sat], seed=0x15).tofile(path)
    off, ev0, rec0 = run_rx(tmp_path, "off", path, "7X", fs, [])
    assert off.returncode == 0, off.stdout + off.stderr
    for mode in ("reference", "full"):
        on, ev1, rec1 = run_rx(tmp_path, mode, path, "7X", fs, ["--telemetry", "--telemetry-mode", mode])
        assert on.returncode == 0, on.stdout + on.stderr
        assert open(ev0, "rb").read() == open(ev1, "rb").read()
        assert open(rec0, "rb").read() == open(rec1, "rb").read() and os.path.getsize(rec0) > 150 * 104
        assert not [l for l in on.stdout.splitlines() if l.startswith("page ")]
        a, b = json.loads(off.stdout.strip().splitlines()[-1]), json.loads(on.stdout.strip().splitlines()[-1])
        for k in ("samples", "acq_positive", "acq_negative", "losses", "channels"):
            assert a[k] == b[k], k
    bad, _, _ = run_rx(tmp_path, "bad", path, "1C", fs, ["--telemetry"])
    assert bad.returncode != 0 and "telemetry" in bad.stderr
    bad, _, _ = run_rx(tmp_path, "bad2", path, "7X", fs, ["--telemetry-mode", "fast"])
    assert bad.returncode != 0


def test_page_parts_from_the_receiver(tmp_path):
    """7.6 s of one E5b satellite at 12.5 Msps (8-bit samples, generated on the device piece by piece) with four built
    I/NAV parts cycling on E5b-I: acquisition, hand-over, tracking and the telemetry framing in the tool; every printed part
    is one of those built, even and odd alternate, and an odd part joined to its even part passes the CRC."""
    import numpy as np

    import tlm_model as M
    fs = 12500000
    parts = M.four_parts(M.INAV, 21)
    symbols = np.concatenate([M.build_part(M.INAV, b) for b in parts])
    sat = E.satellite("b", prn=9, dop=1210.0, delay_chips=3100.3, cn0=50.0)
    sat.bits = "".join("0" if s > 0 else "1" for s in symbols)
    n, step = int(7.6 * fs), int(0.8 * fs)
    path = tmp_path / "e5b_inav.dat"
    try:
        with open(path, "wb") as f:
            for a in range(0, n, step):  # one generator call per piece: each piece has its own noise seed, the signal is continuous
                x = signals.generate_if_device(float(fs), min(step, n - a), [sat], seed=0x15 + a // step, start=a, device="cuda")
                signals.to_ibyte(x.cpu().numpy()).tofile(f)
        out, _, _ = run_rx(tmp_path, "pages", path, "7X", fs, ["--item", "ibyte", "--telemetry"], channels=1)
    finally:
        if os.path.exists(path):
            os.remove(path)
    assert out.returncode == 0, out.stdout + out.stderr
    pages = [l.split() for l in out.stdout.splitlines() if l.startswith("page ")]
    # page channel C prn P symbol N even|odd crc ok|fail HEX
    assert len(pages) >= 2 and all(p[2] == "0" and p[4] == "9" for p in pages), out.stdout
    nibbles = lambda b: "".join("0123456789abcdef"[int("".join(str(int(v)) for v in list(b[i:i + 4]) + [0] * (4 - len(b[i:i + 4]))), 2)]
                                for i in range(0, len(b), 4))
    built = {nibbles(b): ("odd" if b[0] else "even") for b in parts}
    for p in pages:
        assert built.get(p[10]) == p[7], p
    counters = [int(p[6]) for p in pages]
    assert all(b - a == 250 for a, b in zip(counters, counters[1:]))
    odd = [p for p in pages[1:] if p[7] == "odd"]
    assert odd and all(p[9] == "ok" for p in odd)
    assert json.loads(out.stdout.strip().splitlines()[-1])["losses"] == 0
