"""The receiver core on a bit-packed real-IF file (tools/gnsship_rx --item 2bit --sample-type real over
Gnss_Receiver_Hip::work_raw, include/gnsship_receiver.hpp): the 2-bit 16 Msps file of
tests/cond_ingest_scenarios.py goes to the device as it is (a quarter byte per sample), is translated from +4 MHz
to baseband and decimated to 4 Msps there; acquisition and tracking run on the conditioned stream, as the
reference's channels run behind Two_Bit_Packed_File_Signal_Source and its Freq_Xlating_Fir_Filter
(conf/gnss-sdr_GPS_L1_nsr_twobit_packed.conf:35-91).

Checked: control events and tracking records equal oracle/receiver.py's run on the conditioned 4 Msps stream
(the library conditioner's own output on the same packed bytes, bit-identical however the stream is cut into
calls — tests/test_gpu_cond_ingest.py); packed complex items with the conditioner off, unpacked by the tool, give
the output of the ibyte file of the same values; the option checks of the new item types."""
import os
import subprocess

import numpy as np
import pytest

from gnss_sim_receiver_amd import abi, engine, signals as S

import cond_ingest_model as I
import cond_ingest_scenarios as P
import test_gpu_receiver as R

pytestmark = pytest.mark.gpu


def test_receiver_on_a_two_bit_packed_real_file_matches_oracle(ctx, tmp_path):
    raw, _ = P.packed_stream()
    assert P.FS // P.DECIM == R.FS
    path = tmp_path / "two_bit_real.dat"
    raw.tofile(path)
    assert os.path.getsize(path) == P.N_IN // 4
    assert os.path.exists(R.RX), "tools/gnsship_rx is not built (make tools/gnsship_rx)"
    ev, rec, dump = str(tmp_path / "events.csv"), str(tmp_path / "records.bin"), str(tmp_path / "trk_ch_")
    cmd = [R.RX, "--file", str(path), "--item", "2bit", "--sample-type", "real", "--fs", str(P.FS), "--if-hz", str(P.IF_HZ),
           "--decimation", str(P.DECIM), "--channels", "3", "--in-acquisition", "1", "--rotator", "avx", "--block-ms", "100",
           "--acq-piece", "8192", "--satellite", "0:7", "--satellite", "1:19", "--satellite", "2:3", "--events", ev, "--records", rec,
           "--dump", dump]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert f'"samples": {P.N_IN},' in out.stdout
    events = np.loadtxt(ev, delimiter=",", skiprows=1, ndmin=2)
    recs = np.fromfile(rec, R.REC)

    # the same conditioned stream, from the library's conditioner in one call on the packed bytes
    h = engine.cond_lowpass_taps(ctx.lib, float(P.FS), P.DECIM)
    cond = engine.SignalConditioner(ctx, P.FS, [(P.IF_HZ, P.DECIM, h)], P.N_IN)
    (y,) = cond.run(raw, fmt=P.FMT)
    cond.close()
    rx = R.oracle_rx(y, satellite=[7, 19, 3])
    assert R.compare(events, recs, rx, dump) == 2
    pos = events[events[:, 2] == 1]
    assert sorted(pos[:, 3].astype(int).tolist()) == [7, 19]
    for prn, dop in ((7, 1730.0), (19, -2270.0)):
        assert abs(pos[pos[:, 3] == prn][0][4] - dop) <= 250.0  # within a Doppler bin of the truth, the IF removed


@pytest.mark.parametrize("item,extra,preset", [("4bit-cpx", ["--sample-type", "qi"], "four_bit_cpx_qi"), ("2bit-cpx", [], "two_bit_cpx")])
def test_packed_complex_items_without_the_conditioner_are_unpacked_by_the_tool(tmp_path, item, extra, preset):
    """A packed complex baseband file with the conditioner off: the tool unpacks it to gr_complex on the host, as
    it converts ishort / ibyte — the same events and records, byte for byte, as the ibyte file of the unpacked values."""
    fmt = I.PRESETS[preset][0]
    bits = abi.fmt_packed_fields(fmt)[0]
    x = S.generate_if(R.FS, int(0.2 * R.FS), S.c1_sky(extra=((3, -2400.0, 3001.0),)), seed=0x6E550021)
    top = (1 << (bits - 1)) - 1
    s = np.clip(np.floor(np.stack([x.real, x.imag], -1) * (2.0 if bits == 4 else 0.7)), -top - 1, top)     # value 2s + 1
    raw = I.pack_samples((2 * s[:, 0] + 1) + 1j * (2 * s[:, 1] + 1), fmt)
    ibyte = I.unpack_int8(raw, fmt)
    assert len(ibyte) == 2 * len(x) and np.array_equal(ibyte.astype(np.float64), (2 * s + 1).reshape(-1))
    out = {}
    for name, data, it, ex in (("packed", raw, item, extra), ("ibyte", ibyte, "ibyte", [])):
        d = tmp_path / name
        d.mkdir()
        data.tofile(d / "in.dat")
        R.run_rx(d / "in.dat", d, "--satellite", "0:7", "--satellite", "1:3", "--satellite", "2:9", *ex, item=it)
        out[name] = (open(d / "events.csv", "rb").read(), open(d / "records.bin", "rb").read())
    assert out["packed"] == out["ibyte"]
    assert len(out["packed"][1]) > 0 and out["packed"][0].count(b"\n") >= 3


def test_item_options_are_checked(tmp_path):
    """A bad item option is a usage error (exit status 2, the reason on stderr), found before the device is used."""
    path = tmp_path / "empty.dat"
    np.zeros(64, np.int8).tofile(path)
    for extra, why in ((["--item", "2bit"], "real-sampled items need the conditioner"),
                       (["--item", "nsr"], "real-sampled items need the conditioner"),
                       (["--item", "byte"], "real-sampled items need the conditioner"),
                       (["--item", "float"], "real-sampled items need the conditioner"),
                       (["--item", "2bit", "--sample-type", "complex", "--decimation", "4"], "--sample-type must be real, iq or qi"),
                       (["--item", "4bit-cpx", "--sample-type", "real"], "--sample-type must be iq or qi"),
                       (["--item", "4bit-cpx", "--big-endian-bytes"], "--big-endian-bytes with --item 2bit"),
                       (["--item", "ibyte", "--sample-type", "iq"], "--sample-type goes with"),
                       (["--item", "3bit"], "--item must be")):
        out = subprocess.run([R.RX, "--file", str(path), "--fs", "16000000", *extra], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and why in out.stderr, (extra, out.returncode, out.stderr)
