"""The telemetry class of the C++ mirror (include/gnsship_cpp.hpp Galileo_Telemetry_Decoder_Hip,
galileo_inav/fnav/cnav_tlm_conf): tests/cpp/tlm_mirror_test prints the configurations, and on the GPU takes built I/NAV
streams of three channels through work_symbols in runs of 600 symbols, with set_satellite() and reset() after the first
run, and through work_records — every line equal to what tests/tlm_model.py gives."""
import os
import subprocess

import numpy as np
import pytest

import tlm_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "tlm_mirror_test")


@pytest.fixture(scope="module")
def tlm_bin(built):
    if not os.path.exists(BIN):
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/tlm_mirror_test"], check=True)
    return BIN


def test_tlm_confs(tlm_bin):
    r = subprocess.run([tlm_bin, "confs"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    by = {}
    for line in r.stdout.strip().splitlines():
        t = line.split()
        by[t[0]] = {t[i]: int(t[i + 1]) for i in range(1, len(t) - 1, 2)}
    assert by == {"inav": dict(frame_type=1, vit_mode=0, max_rounds=600, reserved=0),
                  "fnav": dict(frame_type=2, vit_mode=0, max_rounds=1200, reserved=0),
                  "cnav": dict(frame_type=3, vit_mode=1, max_rounds=2500, reserved=0)}


@pytest.mark.gpu
def test_work_through_the_cpp_mirror(tlm_bin, tmp_path):
    n, C, cut = 1800, 3, 600
    leads = [13, 150, 77]
    x = np.stack([M.build_stream(M.INAV, M.four_parts(M.INAV, 5 + c), n, leads[c], 40 + c) * np.float32(1.0 if c != 1 else -1.5)
                  for c in range(C)], axis=1).astype(np.float32)
    path = tmp_path / "inav_streams.f32"
    np.ascontiguousarray(x).tofile(path)
    r = subprocess.run([tlm_bin, "run", str(path), str(n), str(C), str(cut)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "tlm_mirror_test done" in r.stdout, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.strip().splitlines()]
    as_string = lambda b: "".join("01"[int(v)] for v in b)
    # work_symbols in runs, with the channel control after the first
    mods = [M.TlmDecoder(M.INAV) for _ in range(C)]
    want_pages, want_faults = [], []
    for run, k in enumerate(range(0, n, cut)):
        for c, m in enumerate(mods):
            pages, fault = m.run(x[k:k + cut, c])
            want_pages += [["page", str(c), str(p["symbol_counter"]), str(p["flags"]), str(p["crc_error_counter"]), as_string(p["bits"])]
                           for p in pages]
            if fault:
                want_faults.append(["fault", str(run), str(c)])
        if run == 0:
            mods[1].set_satellite()
            mods[C - 1].reset()
    got_pages = [t for t in lines if t[0] == "page"]
    assert sorted(got_pages) == sorted(want_pages) and len(want_pages) >= 4
    assert [t for t in lines if t[0] == "fault"] == want_faults
    for c, m in enumerate(mods):
        s = m.state()
        want = ["state", str(c)] + [str(s[f]) for f in ("symbol_counter", "preamble_index", "last_valid_preamble", "stat", "crc_error_counter",
                                                        "history_size", "pll_180", "frame_sync", "even_word_arrived", "flag_crc_test",
                                                        "sent_tlm_failed")]
        assert want in lines, (c, want)
    assert ["too_many", "refused"] in lines and ["bad_channel", "refused"] in lines
    # work_records: the symbol rounds alone count, the page carries the completing record's sample counter
    want_r = []
    for c in range(C):
        pages, _ = M.TlmDecoder(M.INAV).run(x[:, c], 1000000 + 16000 * np.arange(n) + c)
        want_r += [["rpage", str(c), str(p["symbol_counter"]), str(p["flags"]), str(p["crc_error_counter"]), as_string(p["bits"]),
                    str(p["sample_counter"])] for p in pages]
    assert [t for t in lines if t[0] == "rpage"] == want_r and len(want_r) >= 4
