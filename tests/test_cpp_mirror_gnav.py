"""The GLONASS GNAV telemetry classes of the C++ mirror (include/gnsship_cpp.hpp Glonass_L1_Ca_Telemetry_Decoder_Hip,
Glonass_L2_Ca_Telemetry_Decoder_Hip, glonass_l1_ca_tlm_conf, glonass_l2_ca_tlm_conf): tests/cpp/gnav_mirror_test prints the
configurations, and on the GPU takes built streams of three channels through work_symbols in runs of 3000 symbols, with
set_satellite() between runs and a state copied from one channel to another, and through work_records — every line equal
to what tests/gnav_model.py gives."""
import os
import subprocess

import numpy as np
import pytest

import gnav_model as M
from test_gnav_model import bits_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "gnav_mirror_test")
DOUBLES = ("tow_at_current_symbol", "tow", "tau_c", "tau_gps", "chip_acc")
INTS = ("stat", "crc_error_counter", "history_size", "prn", "wn", "t_k", "t_b", "previous_tb", "n_t", "n", "n_4", "frame_sync")


@pytest.fixture(scope="module")
def gnav_bin(built):
    if not os.path.exists(BIN):
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/gnav_mirror_test"], check=True)
    return BIN


def test_gnav_confs(gnav_bin):
    r = subprocess.run([gnav_bin, "confs"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    for line in r.stdout.strip().splitlines():
        t = line.split()
        got[t[0]] = {t[i]: int(t[i + 1]) for i in range(1, len(t) - 1, 2)}
    assert got == dict(l1=dict(max_rounds=2001, signal=M.L1CA, reserved=0, strings_per_run=2, size=64, state=416),
                       l2=dict(max_rounds=9999, signal=M.L2CA, reserved=0, strings_per_run=5, size=64, state=416))


def str_line(tag, c, r, with_sample=False):
    t = [tag, str(c), str(r["symbol_counter"]), str(r["prn"]), str(r["string_id"]), str(r["flipped_bit"]), str(r["tow_at_current_symbol_ms"]),
         str(r["flags"]), "%016x" % bits_of(r["tow"])] + ["%08x" % w for w in r["bits"]]
    return t + [str(r["sample_counter"])] if with_sample else t


def state_line(tag, c, st):
    return ([tag, str(c), str(st["symbol_counter"]), str(st["preamble_index"])] + ["%016x" % bits_of(st[f]) for f in DOUBLES] + [str(st[f]) for f in INTS]
            + [str(f) for f in st["ephemeris_str"]] + [str(st["utc_model_str_5"]), str(st["tow_set"]), str(st["tow_new"])]
            + [str(sum(st[f])) for f in ("half_pos", "half_neg", "history")])


@pytest.mark.gpu
@pytest.mark.parametrize("signal", ["l1", "l2"])
def test_work_through_the_cpp_mirror(gnav_bin, tmp_path, signal):
    n, cut, prns = 10300, 3000, [1, 2, 0]
    rng = np.random.default_rng(21)
    cols = []
    for c in range(3):
        strings = M.frame_strings(t_k_raw=300 + c, t_b_raw=9, n_t=700 + c, n=5 + c, n_4=7, tau_c=-99 * c, tau_gps=c, rng=rng, ids=(1, 2, 3, 4, 5, 1))
        cols.append(M.stream(strings, lead=9 + 40 * c, inverted=c == 1)[:n] * np.float32(1.0 + 0.5 * c))
    x = np.stack(cols, axis=1).astype(np.float32)
    path = tmp_path / "gnav_streams.f32"
    np.ascontiguousarray(x).tofile(path)
    r = subprocess.run([gnav_bin, "run", str(path), str(n), "3", str(cut), signal] + [str(p) for p in prns], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "gnav_mirror_test done" in r.stdout, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.strip().splitlines()]
    mods = [M.Decoder(prn, c) for c, prn in enumerate(prns)]
    want_strs, want_streams = [], []
    for run, k in enumerate(range(0, n, cut)):
        if run == 1:
            mods[0].set_satellite(9)
        recs, tow, sf = M.run(mods, x[k:k + cut])
        for c in range(3):
            want_strs += [str_line("str", c, rec) for rec in recs[c]]
            want_streams.append(["stream", str(run), str(c), str(int(tow[:, c].astype(np.uint64).sum() & 0xFFFFFFFF)), str(int(sf[:, c].sum()))])
    assert sorted(t for t in lines if t[0] == "str") == sorted(want_strs) and len(want_strs) == 9  # strings 3, 4, 5 of each channel
    assert sorted(t for t in lines if t[0] == "stream") == sorted(want_streams)
    for c, m in enumerate(mods):
        assert [t for t in lines if t[:2] == ["state", str(c)]][0] == state_line("state", c, m.state()), c
    assert [t for t in lines if t[0] == "copy"][0] == state_line("copy", 0, mods[1].state())
    for what in ("too_many", "bad_channel", "bad_prn", "bad_state", "wrong_signal"):
        assert [what, "refused"] in lines
    # work_records: the symbol rounds alone count, the completing record's sample counter
    want_r = []
    for c, prn in enumerate(prns):
        recs, _, _ = M.run([M.Decoder(prn, c)], x[:, c:c + 1], None, (1000000 + 4000 * np.arange(n) + c)[:, None])
        want_r += [str_line("rstr", c, rec, True) for rec in recs[0]]
    assert [t for t in lines if t[0] == "rstr"] == want_r and len(want_r) == 9
