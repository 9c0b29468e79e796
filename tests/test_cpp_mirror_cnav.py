"""The GPS CNAV telemetry classes of the C++ mirror (include/gnsship_cpp.hpp Gps_L2c_Telemetry_Decoder_Hip,
Gps_L5_Telemetry_Decoder_Hip, gps_l2c_tlm_conf, gps_l5_tlm_conf): tests/cpp/cnav_mirror_test prints the configurations, and
on the GPU takes built CNAV streams of three channels through work_symbols in runs of 600 symbols, with reset() after the
first run, and through work_records — every line equal to what tests/cnav_model.py gives."""
import os
import subprocess

import numpy as np
import pytest

import cnav_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "cnav_mirror_test")
BLOCK = ("symbol_counter", "last_valid_preamble", "tow_s", "tow_ms", "tow_at_preamble", "pll_180", "valid_word", "sent_tlm_failed")
PART = ("n_symbols", "n_decoded", "n_crc_fail", "decisions_index", "old_is_metrics2", "preamble_seen", "invert", "message_lock", "crc_ok", "init")


@pytest.fixture(scope="module")
def cnav_bin(built):
    if not os.path.exists(BIN):
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/cnav_mirror_test"], check=True)
    return BIN


def test_cnav_confs(cnav_bin):
    r = subprocess.run([cnav_bin, "confs"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    for line in r.stdout.strip().splitlines():
        t = line.split()
        got[t[0]] = {t[i]: int(t[i + 1]) for i in range(1, len(t) - 1, 2)}
    assert got == dict(l2c=dict(max_rounds=600, signal=M.L2C, reserved=0, messages_per_run=M.messages_per_run(600), size=72, state=2520),
                       l5=dict(max_rounds=1200, signal=M.L5, reserved=0, messages_per_run=M.messages_per_run(1200), size=72, state=2520))


def msg_line(tag, c, r, with_sample=False):
    t = [tag, str(c), str(r["symbol_counter"]), str(r["prn"]), str(r["msg_id"]), str(r["tow"]), str(r["alert"]), str(r["delay"]), str(r["part"]),
         str(r["flags"]), r["raw"][:38].hex()]
    return t + [str(r["sample_counter"])] if with_sample else t


def state_line(c, st):
    t = ["state", str(c)] + [repr(float(st[f])) if f == "tow_s" else str(st[f]) for f in BLOCK]
    w64 = np.arange(1, 65, dtype=np.uint64)
    for k in range(2):
        p = st[f"part{k}"]
        metrics = int((p["metrics"][0].astype(np.uint64) * w64).sum() + (p["metrics"][1].astype(np.uint64) * (w64 + np.uint64(64))).sum())
        d = p["decisions"].astype(np.uint64)
        decisions = int((d[:, 0] * (2 * w64 - np.uint64(1))).sum() + (d[:, 1] * (2 * w64)).sum())
        symbols = int((p["symbols"].astype(np.uint64) * np.arange(1, 129, dtype=np.uint64)).sum())
        decoded = int((p["decoded"].astype(np.uint64) * w64).sum())
        t += [str(int(p[f])) for f in PART] + [str(metrics), str(decisions), str(symbols), str(decoded)]
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("signal", ["l2c", "l5"])
def test_work_through_the_cpp_mirror(cnav_bin, tmp_path, signal):
    mode = M.L5 if signal == "l5" else M.L2C
    n, C, cut = 1800, 3, 600
    g = M.golden_streams()
    x = np.stack([M.to_float(g[name][0][:n]) * np.float32(1.0 + 0.5 * c) for c, name in enumerate(("lead0_neg", "lead1_pos", "flips"))],
                 axis=1).astype(np.float32)
    path = tmp_path / "cnav_streams.f32"
    np.ascontiguousarray(x).tofile(path)
    r = subprocess.run([cnav_bin, "run", str(path), str(n), str(C), str(cut), signal], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "cnav_mirror_test done" in r.stdout, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.strip().splitlines()]
    mods = [M.CnavBlock(mode) for _ in range(C)]
    want_msgs, want_faults, want_streams = [], [], []
    for run, k in enumerate(range(0, n, cut)):
        for c, m in enumerate(mods):
            recs, fault, tow, sf = m.run(x[k:k + cut, c], channel=c)
            want_msgs += [msg_line("msg", c, rec) for rec in recs]
            if fault:
                want_faults.append(["fault", str(run), str(c)])
            want_streams.append(["stream", str(run), str(c), str(int(tow.astype(np.uint64).sum() & 0xFFFFFFFF)), str(int(sf.sum()))])
        if run == 0:
            mods[C - 1].reset()
    assert sorted(t for t in lines if t[0] == "msg") == sorted(want_msgs) and len(want_msgs) >= 6
    assert [t for t in lines if t[0] == "fault"] == want_faults
    assert sorted(t for t in lines if t[0] == "stream") == sorted(want_streams)
    for c, m in enumerate(mods):
        got = [t for t in lines if t[:2] == ["state", str(c)]][0]
        want = state_line(c, m.state())
        assert float(got[4]) == float(want[4]) and got[:4] + got[5:] == want[:4] + want[5:], (c, got, want)
    assert ["too_many", "refused"] in lines and ["bad_channel", "refused"] in lines and ["wrong_signal", "refused"] in lines
    # work_records: the symbol rounds alone count, the prompt this signal reads, the completing record's sample counter
    want_r = []
    for c in range(C):
        recs, _, _, _ = M.CnavBlock(mode).run(x[:, c], sample_counters=1000000 + 16000 * np.arange(n) + c, channel=c)
        want_r += [msg_line("rmsg", c, rec, True) for rec in recs]
    assert [t for t in lines if t[0] == "rmsg"] == want_r and len(want_r) >= 6
