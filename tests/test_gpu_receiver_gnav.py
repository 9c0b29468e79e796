"""tools/gnsship_rx --gnav (include/gnsship_receiver.hpp Receiver_Conf::gnav): the opt-in GLONASS GNAV telemetry decoder
behind the system 'R' channels.  On a 0.3 s file no string can be decoded, so the first check is what the option must leave
alone: events, records and the summary stay byte for byte what they are without it.  The second test feeds the tool one
GLONASS L1 satellite carrying built strings, long enough for one decode, and requires the printed lines to be what
tests/gnav_model.py gives on the tool's own records."""
import json
import os
import subprocess

import numpy as np
import pytest

import gnav_model as M
from gnss_sim_receiver_amd import abi, signals

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RX = os.path.join(ROOT, "tools", "gnsship_rx")
FS = 4000000
REC = np.dtype([("channel", "<i4"), ("prn", "<i4"), ("e", abi.TRK_EPOCH_DTYPE)])
# The length of the long file.  The data start 300 ms before a time mark, so that the tracker (whose first symbol comes some
# tens of ms in) sees that mark whole.  The decoder takes a mark as a hit when it is the oldest 300 symbols of a full
# history — 1.7 s after the mark has ended — needs a second hit 2 s later and decodes 2 s after that: the first string is
# due 300 + 300 + 1700 + 4000 = 6300 ms into the file, whatever the tracker's start.  6.5 s hold it with 200 ms to spare.
SECONDS, LEAD_MS = 6.5, 300


def satellite(bits):
    return signals.Satellite(prn=24, doppler_hz=2000.0, code_delay_chips=207.3, carrier_phase_rad=0.9, cn0_dbhz=50.0, system="GLO_L1", bits=bits,
                             symbols_per_bit=10)


def run_rx(tmp_path, tag, path, extra):
    ev, rec = str(tmp_path / f"events_{tag}.csv"), str(tmp_path / f"records_{tag}.bin")
    cmd = [RX, "--file", str(path), "--signal", "1G", "--fs", str(FS), "--channels", "1", "--in-acquisition", "1", "--satellite", "0:24",
           "--doppler-max", "5000", "--doppler-step", "500", "--pll-bw", "50", "--dll-bw", "2", "--block-ms", "100", "--events", ev, "--records", rec] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    return out, ev, rec


def test_gnav_option_leaves_the_receiver_outputs_alone(tmp_path):
    assert os.path.exists(RX), "tools/gnsship_rx is not built (make tools/gnsship_rx)"
    path = tmp_path / "if.dat"
    signals.generate_if(float(FS), int(0.3 * FS), [satellite("0100111010110001")], seed=0x16).tofile(path)
    off, ev0, rec0 = run_rx(tmp_path, "off", path, [])
    assert off.returncode == 0, off.stdout + off.stderr
    on, ev1, rec1 = run_rx(tmp_path, "on", path, ["--gnav"])
    assert on.returncode == 0, on.stdout + on.stderr
    assert open(ev0, "rb").read() == open(ev1, "rb").read()
    assert open(rec0, "rb").read() == open(rec1, "rb").read() and os.path.getsize(rec0) > 250 * 104
    assert not [l for l in on.stdout.splitlines() if l.startswith("gnav-string ")]
    a, b = json.loads(off.stdout.strip().splitlines()[-1]), json.loads(on.stdout.strip().splitlines()[-1])
    for k in ("samples", "acq_positive", "acq_negative", "losses", "channels"):
        assert a[k] == b[k], k
    bad = subprocess.run([RX, "--file", str(path), "--signal", "1C", "--fs", str(FS), "--channels", "1", "--gnav"], capture_output=True, text=True,
                         timeout=60)
    assert bad.returncode != 0 and "gnav" in bad.stderr


def built_frame():
    """Two strings, cyclic on the air, as half-bits ('0' is sent as +1): the last LEAD_MS of the second string's data, then
    time mark, data, time mark, data.  The 400 half-bits hold the time mark, in either polarity, at its two places only."""
    mark = "".join(str(b) for b in M.MARK)
    for seed in range(200):
        rng = np.random.default_rng(seed)
        strings = [M.build_string(1, [((10, 12), 777)], rng.integers(0, 2, 72)), M.build_string(2, [(M.F_TB, 41)], rng.integers(0, 2, 72))]
        half = []
        for s in strings:  # string_symbols: ten symbols per half-bit, +1 for a '1'
            sym = M.string_symbols(s)[::10]
            half.append("".join("1" if v > 0 else "0" for v in sym))
        air = half[0] + half[1]  # data 0, mark, data 1, mark
        cyc = air + air[:29]
        inv = mark.translate(str.maketrans("01", "10"))
        if [i for i in range(400) if cyc[i:i + 30] in (mark, inv)] == [170, 370]:
            k = 170 - LEAD_MS // 10
            rotated = air[k:] + air[:k]
            return strings, rotated.translate(str.maketrans("01", "10"))  # Satellite.bits sends '0' as +1
    raise AssertionError("no seed gives a pattern free of look-alikes")


def test_a_string_from_the_receiver(tmp_path):
    """SECONDS of GLONASS L1 PRN 24 (frequency channel 2) at 4 Msps, 50 dB-Hz, 8-bit samples generated on the device piece by
    piece.  The channel may lock half a cycle off: either polarity is right.  The printed lines are the model's strings over
    the tool's own records, and each carries a string that was built, accepted without correction."""
    strings, bits = built_frame()
    sat = satellite(bits)
    path = tmp_path / "glo.dat"
    n, step = int(SECONDS * FS), int(0.5 * FS)
    try:
        with open(path, "wb") as f:
            for a in range(0, n, step):  # one generator call per piece: each piece has its own noise seed, the signal is continuous
                x = signals.generate_if_device(float(FS), min(step, n - a), [sat], seed=0x31 + a // step, start=a, device="cuda")
                signals.to_ibyte(x.cpu().numpy()).tofile(f)
        out, _, rec_path = run_rx(tmp_path, "long", path, ["--item", "ibyte", "--gnav"])
    finally:
        if os.path.exists(path):
            os.remove(path)
    assert out.returncode == 0, out.stdout + out.stderr
    assert json.loads(out.stdout.strip().splitlines()[-1])["losses"] == 0
    lines = [l for l in out.stdout.splitlines() if l.startswith("gnav-string ")]
    rec = np.fromfile(rec_path, REC)
    e = rec[rec["channel"] == 0]["e"]
    sel = (e["flags"] & 1) != 0
    recs, _, _ = M.run([M.Decoder(24, 0)], e["prompt_i"][:, None], sel[:, None], e["sample_counter"][:, None])
    want = ["gnav-string channel 0 prn 24 slot %d symbol %d sample %d string %d flipped %d tow_ms %d tow %.17g flags %02x bits %08x %08x %08x" % (
        r["prn"], r["symbol_counter"], r["sample_counter"], r["string_id"], r["flipped_bit"], r["tow_at_current_symbol_ms"], r["tow"], r["flags"],
        *r["bits"]) for r in recs[0]]
    print("first symbol at record", int(np.argmax(sel)), "sample", int(e["sample_counter"][np.argmax(sel)]), "symbols", int(sel.sum()),
          "strings at", [r["symbol_counter"] for r in recs[0]])
    assert lines == want and len(lines) >= 1, out.stdout
    built = {tuple(M.pack_bits([s[84 - i] for i in range(85)])): s for s in strings}
    for r in recs[0]:
        assert tuple(r["bits"]) in built and r["flags"] & M.CRC_OK and not r["flags"] & M.CORRECTED and r["flipped_bit"] == -1, out.stdout
        assert r["string_id"] == built[tuple(r["bits"])][4] + 2 * built[tuple(r["bits"])][3] and r["prn"] == 24
