"""The BeiDou D1/D2 telemetry classes of the C++ mirror (include/gnsship_cpp.hpp Beidou_B1i_Telemetry_Decoder_Hip,
Beidou_B3i_Telemetry_Decoder_Hip, beidou_b1i_tlm_conf, beidou_b3i_tlm_conf): tests/cpp/dnav_mirror_test prints the
configurations, and on the GPU takes built streams of three channels (D1, D2, PRN 60) through work_symbols in runs of 500
symbols, with reset() and set_satellite() between runs, and through work_records — every line equal to what
tests/dnav_model.py gives."""
import os
import subprocess

import numpy as np
import pytest

import dnav_model as M
import test_dnav_model as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "dnav_mirror_test")
STATE = ("symbol_counter", "preamble_index", "last_valid_preamble", "tow_at_preamble_ms", "tow_at_current_symbol_ms", "sow",
         "symbol_duration_ms", "stat", "crc_error_counter", "history_size", "prn", "sow_set", "frame_sync", "valid_word", "new_sow_available",
         "sent_tlm_failed", "d2_decoder", "d2_timing")


@pytest.fixture(scope="module")
def dnav_bin(built):
    if not os.path.exists(BIN):
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/dnav_mirror_test"], check=True)
    return BIN


def test_dnav_confs(dnav_bin):
    r = subprocess.run([dnav_bin, "confs"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    for line in r.stdout.strip().splitlines():
        t = line.split()
        got[t[0]] = {t[i]: int(t[i + 1]) for i in range(1, len(t) - 1, 2)}
    assert got == dict(b1i=dict(max_rounds=601, signal=M.B1I, reserved=0, subframes_per_run=3, size=88, state=64),
                       b3i=dict(max_rounds=1300, signal=M.B3I, reserved=0, subframes_per_run=5, size=88, state=64))


def sub_line(tag, c, r, with_sample=False):
    t = [tag, str(c), str(r["symbol_counter"]), str(r["fra_id"]), str(r["pnum"]), str(r["sow"]), str(r["corrected_mask"]),
         str(r["tow_at_current_symbol_ms"]), str(r["flags"])] + ["%08x" % w for w in r["words"]]
    return t + [str(r["sample_counter"])] if with_sample else t


@pytest.mark.gpu
@pytest.mark.parametrize("signal", ["b1i", "b3i"])
def test_work_through_the_cpp_mirror(dnav_bin, tmp_path, signal):
    mode = M.B3I if signal == "b3i" else M.B1I
    n, cut, prns = 1300, 500, [20, 3, 60]
    cols = []
    for c, prn in enumerate(prns):
        f = C.d2_stream if M.is_d2_decoder(mode, prn) else C.d1_stream
        cols.append(f(7 * c, 5, 4000 + c, inverted=c == 1, seed=11 + c)[:n] * np.float32(1.0 + 0.5 * c))
    x = np.stack(cols, axis=1).astype(np.float32)
    path = tmp_path / "dnav_streams.f32"
    np.ascontiguousarray(x).tofile(path)
    r = subprocess.run([dnav_bin, "run", str(path), str(n), "3", str(cut), signal] + [str(p) for p in prns], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "dnav_mirror_test done" in r.stdout, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.strip().splitlines()]
    mods = [M.Decoder(mode, prn, c) for c, prn in enumerate(prns)]
    want_subs, want_streams = [], []
    for run, k in enumerate(range(0, n, cut)):
        if run == 1:
            mods[0].set_satellite(3)
        recs, tow, sf = M.run(mods, x[k:k + cut])
        for c in range(3):
            want_subs += [sub_line("sub", c, rec) for rec in recs[c]]
            want_streams.append(["stream", str(run), str(c), str(int(tow[:, c].astype(np.uint64).sum() & 0xFFFFFFFF)), str(int(sf[:, c].sum()))])
        if run == 0:
            mods[2].reset()
        if run == 1:
            mods[0].set_satellite(prns[0])
    assert sorted(t for t in lines if t[0] == "sub") == sorted(want_subs) and len(want_subs) >= 8
    assert sorted(t for t in lines if t[0] == "stream") == sorted(want_streams)
    for c, m in enumerate(mods):
        got = [t for t in lines if t[:2] == ["state", str(c)]][0]
        st = m.state()
        assert got == ["state", str(c)] + [str(st[f]) for f in STATE], (c, got)
    for what in ("too_many", "bad_channel", "bad_prn", "wrong_signal"):
        assert [what, "refused"] in lines
    # work_records: the symbol rounds alone count, the completing record's sample counter
    want_r = []
    for c, prn in enumerate(prns):
        recs, _, _ = M.run([M.Decoder(mode, prn, c)], x[:, c:c + 1], None, None, (1000000 + 16000 * np.arange(n) + c)[:, None])
        want_r += [sub_line("rsub", c, rec, True) for rec in recs[0]]
    assert [t for t in lines if t[0] == "rsub"] == want_r and len(want_r) >= 8
