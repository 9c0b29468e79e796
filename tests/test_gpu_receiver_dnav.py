"""tools/gnsship_rx --dnav (include/gnsship_receiver.hpp Receiver_Conf::dnav): the opt-in BeiDou D1/D2 telemetry decoder
behind the B3 channels.  On the 0.3 s B3I file of tests/test_gpu_receiver_b3i_l2c.py the tracker ends in pull-in and no
symbol reaches the decoder, so the check is what the option must leave alone: events, records and the summary stay byte
for byte what they are without it.  The second test feeds the tool a B3I GEO satellite carrying built D2 subframes, long
enough for a decode, and requires the printed lines to be what tests/dnav_model.py gives on the tool's own records.  A D1
subframe through the receiver needs over 12 s at 12.5 Msps and is deliberately not a GPU test."""
import json
import os
import subprocess

import numpy as np
import pytest

import b3i_l2c_scenarios as B
import dnav_model as M
from gnss_sim_receiver_amd import abi, signals

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RX = os.path.join(ROOT, "tools", "gnsship_rx")
FS = 12500000
REC = np.dtype([("channel", "<i4"), ("prn", "<i4"), ("e", abi.TRK_EPOCH_DTYPE)])
# The length of the GEO file.  The decoder's first record falls on its 611th symbol at the earliest (two preambles, the
# second one the oldest 11 of a full history).  Measured on the records of a 4.2 s file of this very signal: the tracker's
# first valid symbol is record 1220 at sample 15 291 273 (1.22 s: the pull-in lasts to the first whole second after the
# acquisition stamp, then the tracker synchronises on a preamble) and it is the symbol behind that preamble, so the next
# preamble is the oldest 11 of the history at the decoder's symbol 600 and the first record falls on symbol 900, 3.02 s
# into the file (records at 900 and 1200 in 4.2 s).  3.2 s hold 988 symbols: one record.
GEO_SECONDS = 3.2


def run_rx(tmp_path, tag, path, prn, extra):
    ev, rec = str(tmp_path / f"events_{tag}.csv"), str(tmp_path / f"records_{tag}.bin")
    cmd = [RX, "--file", str(path), "--signal", "B3", "--fs", str(FS), "--channels", "1", "--in-acquisition", "1", "--satellite", f"0:{prn}",
           "--doppler-max", "5000", "--doppler-step", "250", "--rotator", "avx", "--pull-in-time-s", "0", "--block-ms", "100",
           "--events", ev, "--records", rec] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    return out, ev, rec


def test_dnav_option_leaves_the_receiver_outputs_alone(tmp_path):
    assert os.path.exists(RX), "tools/gnsship_rx is not built (make tools/gnsship_rx)"
    sat = B.b3i_satellite(prn=9, dop=1210.0, delay_chips=3100.3, cn0=50.0)
    sat.bits = "0110"
    path = tmp_path / "if.dat"
    signals.generate_if(float(FS), int(0.3 * FS), [sat], seed=0x15).tofile(path)
    off, ev0, rec0 = run_rx(tmp_path, "off", path, 9, [])
    assert off.returncode == 0, off.stdout + off.stderr
    on, ev1, rec1 = run_rx(tmp_path, "on", path, 9, ["--dnav"])
    assert on.returncode == 0, on.stdout + on.stderr
    assert open(ev0, "rb").read() == open(ev1, "rb").read()
    assert open(rec0, "rb").read() == open(rec1, "rb").read() and os.path.getsize(rec0) > 150 * 104
    assert not [l for l in on.stdout.splitlines() if l.startswith("dnav-subframe ")]
    a, b = json.loads(off.stdout.strip().splitlines()[-1]), json.loads(on.stdout.strip().splitlines()[-1])
    for k in ("samples", "acq_positive", "acq_negative", "losses", "channels"):
        assert a[k] == b[k], k
    bad = subprocess.run([RX, "--file", str(path), "--signal", "1C", "--fs", str(FS), "--channels", "1", "--dnav"], capture_output=True, text=True,
                         timeout=60)
    assert bad.returncode != 0 and "dnav" in bad.stderr


def geo_subframes(sow0=123456):
    """Three D2 subframes with FraID 1, pages 1..3 — cyclic on the air — whose 900 bits hold the preamble, in either
    polarity, at the three subframe starts only, so that the tracker's symbol synchronisation and the decoder's state 0
    can meet nothing but a true preamble."""
    pre = "".join("1" if p > 0 else "0" for p in M.PREAMBLE)
    inv = pre.translate(str.maketrans("01", "10"))
    for seed in range(200):
        rng = np.random.default_rng(seed)
        specs = [(1, 1 + k, sow0 + k) for k in range(3)]
        subs = [M.build_subframe(True, f, p, s, rng.integers(0, 2, 182)) for f, p, s in specs]
        text = "".join("".join(str(b) for b in air) for _, air in subs)
        cyc = text + text[:10]
        hits = [i for i in range(900) if cyc[i:i + 11] in (pre, inv)]
        if hits == [0, 300, 600]:
            return specs, subs, text
    raise AssertionError("no seed gives a pattern free of look-alikes")


def generate_geo_file(path, seconds, text):
    sat = B.b3i_satellite(prn=3, dop=1210.0, delay_chips=3100.3, cn0=50.0)
    sat.bits = text
    n, step = int(seconds * FS), int(0.5 * FS)
    with open(path, "wb") as f:
        for a in range(0, n, step):  # one generator call per piece: each piece has its own noise seed, the signal is continuous
            x = signals.generate_if_device(float(FS), min(step, n - a), [sat], seed=0x23 + a // step, start=a, device="cuda")
            signals.to_ibyte(x.cpu().numpy()).tofile(f)


def model_lines(rec_path):
    """The model over the tool's records: every epoch with flags & 1 is a symbol."""
    rec = np.fromfile(rec_path, REC)
    e = rec[rec["channel"] == 0]["e"]
    sel = (e["flags"] & 1) != 0
    recs, _, _ = M.run([M.Decoder(M.B3I, 3, 0)], e["prompt_i"].astype(np.float32)[:, None], sel[:, None], None, e["sample_counter"][:, None])
    lines = ["dnav-subframe channel 0 prn 3 symbol %d fraid %d pnum %d sow %d tow_ms %d corrected %05x flags %02x %s" % (
        r["symbol_counter"], r["fra_id"], r["pnum"], r["sow"], r["tow_at_current_symbol_ms"], r["corrected_mask"], r["flags"],
        " ".join("%08x" % w for w in r["words"])) for r in recs[0]]
    return e, sel, recs[0], lines


def test_d2_subframes_from_the_receiver(tmp_path):
    """GEO_SECONDS of BeiDou B3I PRN 3 (GEO: 2 ms symbols, no NH code) at 12.5 Msps, 50 dB-Hz (8-bit samples, generated on
    the device piece by piece).  Satellite.bits sends a '0' as +1, so the channel sees the stream inverted unless the PLL
    locks half a cycle off: either polarity is right.  The printed lines are the model's subframes over the tool's own
    records, and they carry the built FraID, Pnum and SOW."""
    specs, subs, text = geo_subframes()
    path = tmp_path / "bds_geo.dat"
    try:
        generate_geo_file(path, GEO_SECONDS, text)
        out, _, rec_path = run_rx(tmp_path, "geo", path, 3, ["--item", "ibyte", "--dnav"])
    finally:
        if os.path.exists(path):
            os.remove(path)
    assert out.returncode == 0, out.stdout + out.stderr
    assert json.loads(out.stdout.strip().splitlines()[-1])["losses"] == 0
    lines = [l for l in out.stdout.splitlines() if l.startswith("dnav-subframe ")]
    e, sel, recs, want = model_lines(rec_path)
    print("first symbol at record", int(np.argmax(sel)), "sample", int(e["sample_counter"][np.argmax(sel)]), "symbols", int(sel.sum()),
          "records", [r["symbol_counter"] for r in recs])
    assert lines == want, out.stdout
    assert [r["symbol_counter"] for r in recs] == [900] and 900 <= int(sel.sum()) < 1200, out.stdout
    built = {tuple(M.read_unsigned(plain, [(30 * w + 1, 30)]) for w in range(10)): spec for spec, (plain, _) in zip(specs, subs)}
    for r in recs:
        assert tuple(r["words"]) in built and r["corrected_mask"] == 0, out.stdout
        assert (r["fra_id"], r["pnum"], r["sow"]) == built[tuple(r["words"])]
        assert r["flags"] & M.F_D2_DECODER and r["flags"] & M.F_D2_TIMING and r["flags"] & M.F_NEW_SOW
    assert recs[0]["tow_at_current_symbol_ms"] == (recs[0]["sow"] + 14) * 1000 + 311 * 2
