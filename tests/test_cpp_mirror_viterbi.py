"""The Viterbi classes of the C++ mirror (include/gnsship_cpp.hpp Viterbi_Decoder_Hip, Galileo_Page_Decoder_Hip,
galileo_inav/fnav/cnav_vit_conf): tests/cpp/viterbi_mirror_test prints the page configurations, compared here with
the page sizes (I/NAV 8 × 30 → 114 bits, F/NAV 8 × 61 → 238, C/NAV 8 × 123 → 486), and on the GPU decodes the
fixture's I/NAV frames through Viterbi_Decoder_Hip::decode (equal to the compiled reference's recorded bits and
carried metrics) and through Galileo_Page_Decoder_Hip::decode_frames (equal to the model on the prepared symbols)."""
import os
import subprocess

import numpy as np
import pytest

import viterbi_model as V
from viterbi_cases import FRAMES, case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "viterbi_mirror_test")


@pytest.fixture(scope="module")
def vit_bin(built):
    if not os.path.exists(BIN):
        subprocess.run(["make", "-s", "-C", ROOT, "tests/cpp/viterbi_mirror_test"], check=True)
    return BIN


def test_page_confs(vit_bin):
    r = subprocess.run([vit_bin, "confs"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    by = {}
    for line in r.stdout.strip().splitlines():
        t = line.split()
        by[t[0]] = {t[i]: int(t[i + 1]) for i in range(1, len(t) - 1, 2)}
    assert set(by) == {"inav", "fnav", "cnav"}
    for name, (rows, cols, LL) in (("inav", (8, 30, 114)), ("fnav", (8, 61, 238)), ("cnav", (8, 123, 486))):
        c = by[name]
        assert (c["constraint_length"], c["rate_n"], c["g0"], c["g1"]) == (7, 2, 0o171, 0o133)
        assert (c["interleaver_rows"], c["interleaver_cols"], c["data_length"], c["invert_g2"]) == (rows, cols, LL, 1)
        assert rows * cols == 2 * (LL + 6) <= 1024
    assert (by["inav"]["mode"], by["fnav"]["mode"], by["cnav"]["mode"]) == (0, 0, 1)  # the default and the argument


@pytest.mark.gpu
def test_decode_through_the_cpp_mirror(vit_bin, tmp_path):
    sym, bits, sec, _ = case(114, 1)
    path = tmp_path / "inav_frames.f32"
    np.ascontiguousarray(sym).tofile(path)
    r = subprocess.run([vit_bin, "run", str(path), str(FRAMES)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "viterbi_mirror_test done" in r.stdout, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.strip().splitlines()]
    decode = {int(t[1]): t[2] for t in lines if t[0] == "decode"}
    section = {int(t[1]): np.array([int(w, 16) for w in t[2:]], np.uint32) for t in lines if t[0] == "section"}
    frames = {int(t[1]): t[2] for t in lines if t[0] == "frames"}
    as_string = lambda b: "".join("01"[int(v)] for v in b)
    for f in range(FRAMES):
        assert decode[f] == as_string(bits[f]), f
        assert np.array_equal(section[f], sec[f].view(np.uint32)), f
    # the same frames taken as received pages: channels 3 .. 0, the odd frames negated, new objects
    prepared = np.stack([V.prepare(sym[f], 8, 30, True, bool(f & 1)) for f in range(FRAMES)])
    want, _ = V.decode_batch(prepared, V.new_section(FRAMES))
    for f in range(FRAMES):
        assert frames[f] == as_string(want[f]), f
    assert ["duplicate", "refused"] in lines
