"""The GPS L1 C/A telemetry class of the C++ mirror (include/gnsship_cpp.hpp Gps_L1_Ca_Telemetry_Decoder_Hip,
gps_l1_ca_tlm_conf): tests/cpp/lnav_mirror_test prints the configuration, and on the GPU takes built LNAV streams of three
channels through work_symbols in runs of 600 symbols, with set_satellite() and reset() after the first run, and through
work_records — every line equal to what tests/lnav_model.py gives."""
import os
import subprocess

import numpy as np
import pytest

import lnav_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "lnav_mirror_test")
STATE = ("symbol_counter", "preamble_index", "last_valid_preamble", "subframes_tried", "prev_word", "tow_at_preamble_ms",
         "tow_at_current_symbol_ms", "nav_tow_s", "stat", "crc_error_counter", "history_size", "pll_180", "frame_sync", "tow_set", "sent_tlm_failed")


@pytest.fixture(scope="module")
def lnav_bin(built):
    if not os.path.exists(BIN):
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/lnav_mirror_test"], check=True)
    return BIN


def test_lnav_conf(lnav_bin):
    r = subprocess.run([lnav_bin, "confs"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    t = r.stdout.split()
    assert t[0] == "lnav" and {t[i]: int(t[i + 1]) for i in range(1, len(t) - 1, 2)} == dict(max_rounds=600, reserved=0, subframes_per_run=4, size=80)


def sub_line(tag, c, r, with_sample=False):
    t = [tag, str(c), str(r["symbol_counter"]), str(r["subframe_id"]), str(r["tow_s"]), str(r["crc_error_counter"]), str(r["parity_fail_mask"]),
         str(r["flags"])] + ["%08x" % w for w in r["words"]]
    return t + [str(r["sample_counter"])] if with_sample else t


@pytest.mark.gpu
def test_work_through_the_cpp_mirror(lnav_bin, tmp_path):
    n, C, cut = 1800, 3, 600
    leads = [13, 150, 77]
    x = np.stack([M.build_stream(M.five_subframes(5 + c)[0], n, leads[c], 40 + c) * np.float32(1.0 if c != 1 else -1.5) for c in range(C)],
                 axis=1).astype(np.float32)
    path = tmp_path / "lnav_streams.f32"
    np.ascontiguousarray(x).tofile(path)
    r = subprocess.run([lnav_bin, "run", str(path), str(n), str(C), str(cut)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "lnav_mirror_test done" in r.stdout, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.strip().splitlines()]
    # work_symbols in runs, with the channel control after the first
    mods = [M.LnavDecoder() for _ in range(C)]
    want_subs, want_faults, want_streams = [], [], []
    for run, k in enumerate(range(0, n, cut)):
        for c, m in enumerate(mods):
            recs, fault, tow, sf = m.run(x[k:k + cut, c])
            want_subs += [sub_line("sub", c, rec) for rec in recs]
            if fault:
                want_faults.append(["fault", str(run), str(c)])
            want_streams.append(["stream", str(run), str(c), str(int(tow.astype(np.uint64).sum() & 0xFFFFFFFF)), str(int(sf.sum()))])
        if run == 0:
            mods[1].set_satellite()
            mods[C - 1].reset()
    got_subs = [t for t in lines if t[0] == "sub"]
    assert sorted(got_subs) == sorted(want_subs) and len(want_subs) >= 6
    assert [t for t in lines if t[0] == "fault"] == want_faults
    assert sorted(t for t in lines if t[0] == "stream") == sorted(want_streams)
    for c, m in enumerate(mods):
        s = m.state()
        want = ["state", str(c)] + [str(s[f]) for f in STATE]
        assert want in lines, (c, want)
    assert ["too_many", "refused"] in lines and ["bad_channel", "refused"] in lines
    # work_records: the symbol rounds alone count, channel 1 seeds inverted, the record carries the completing sample counter
    want_r = []
    for c in range(C):
        recs, _, _, _ = M.LnavDecoder().run(x[:, c], 1000000 + 16000 * np.arange(n) + c, np.full(n, c == 1))
        want_r += [sub_line("rsub", c, rec, True) for rec in recs]
    assert [t for t in lines if t[0] == "rsub"] == want_r and len(want_r) >= 6
