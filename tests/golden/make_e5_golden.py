"""Generate tests/golden/galileo_e5_codes_ref.npz from the REFERENCE's own Galileo E5a / E5b generators.

    python tests/golden/make_e5_golden.py REFERENCE_TREE SCRATCH_DIRECTORY

Run in the build container only (it needs the reference tree).  The script compiles
tests/golden/e5_ref_shim.cc — extern "C" wrappers that pull in the reference's
galileo_e5_signal_replica.cc and gnss_signal_replica.cc by name from the include path — into a shared
object in the scratch directory, outside the repository, and stores what it produces as data:

  e5a_i_bits, e5a_q_bits, e5b_i_bits, e5b_q_bits
                       uint8[50, 1279]: np.packbits of the chip bits (1 ↔ chip −1.0) of PRN 1..50,
                       10230 chips each, from the "5I" / "5Q" / "7I" / "7Q" primaries
  x_matches            1: the "5X" / "7X" primaries of every PRN carry the I chips in the real part and
                       the Q chips in the imaginary part (checked here)
  sampled_<sig>_<fs>_<prn>_<shift>_re / _im
                       np.packbits of the sampled code's sign bits per part; a part the signal does not
                       carry ("5I": imaginary, "5Q": also imaginary — the reference puts both single
                       components in the real part) is all zero, checked here and not stored
  sampled_signals, sampled_rates, sampled_prns, sampled_shifts
  e5a_i_secondary, e5b_i_secondary      the fixed secondary codes as '0' / '1' strings
  e5a_q_secondary, e5b_q_secondary      str[50]: the pilot secondary code of PRN 1..50, 100 chips (the
                       reference's E5a-Q table ends at PRN 47: the entries of PRN 48..50 are empty)
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SIGNALS = ("5I", "5Q", "5X", "7X")
RATES = (12500000, 10230000, 10000000, 8184000)
PRNS = (1, 50)
SHIFTS = (0, 3)
f32p = ctypes.POINTER(ctypes.c_float)

# complex_exp_gen's NCO: named by gnss_signal_replica.cc, called by nothing the shim uses
NCO_STAND_IN = """#pragma once
#include <complex>
#include <cstddef>
namespace gr {
class fxpt_nco {
public:
    void set_freq(float) {}
    void sincos(std::complex<float>*, std::size_t, int) {}
};
}
"""


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    ref, scratch = sys.argv[1], sys.argv[2]
    inc = os.path.join(scratch, "e5_stand_in")
    os.makedirs(os.path.join(inc, "gnuradio"), exist_ok=True)
    for name in ("fxpt_nco.h", "gr_complex.h"):
        with open(os.path.join(inc, "gnuradio", name), "w") as f:
            f.write(NCO_STAND_IN if name == "fxpt_nco.h" else "#pragma once\n#include <complex>\nusing gr_complex = std::complex<float>;\n")
    so = os.path.join(scratch, "libe5ref.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-std=c++20", "-DHAS_STD_SPAN=1", "-I" + inc,
                    "-I" + os.path.join(ref, "src/algorithms/libs"), "-I" + os.path.join(ref, "src/core/system_parameters"),
                    os.path.join(HERE, "e5_ref_shim.cc"), "-o", so], check=True)
    R = ctypes.CDLL(so)
    R.ref_e5_primary.argtypes = [f32p, ctypes.c_int32, ctypes.c_char_p]
    R.ref_e5_primary.restype = None
    R.ref_e5_sampled.argtypes = [f32p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_int32, ctypes.c_uint32]
    R.ref_e5_sampled.restype = ctypes.c_int
    for name in ("ref_e5a_i_secondary", "ref_e5b_i_secondary"):
        getattr(R, name).restype = ctypes.c_char_p
    for name in ("ref_e5a_q_secondary", "ref_e5b_q_secondary"):
        getattr(R, name).argtypes = [ctypes.c_int32]
        getattr(R, name).restype = ctypes.c_char_p

    def primary(prn, sig):
        buf = np.zeros(2 * 10230, np.float32)
        R.ref_e5_primary(buf.ctypes.data_as(f32p), prn, sig.encode())
        return buf[0::2].copy(), buf[1::2].copy()

    out = {}
    chips = {}
    for band, b in (("5", "e5a"), ("7", "e5b")):
        for comp in "IQ":
            c = np.zeros((50, 10230), np.float32)
            for k in range(50):
                re, im = primary(k + 1, band + comp)
                assert not np.any(im)  # both single components lie in the real part
                c[k] = re
            assert np.all(np.abs(c) == 1.0)
            chips[band + comp] = c
            out[f"{b}_{comp.lower()}_bits"] = np.packbits(c < 0, axis=1)
        for k in range(50):
            re, im = primary(k + 1, band + "X")
            assert np.array_equal(re, chips[band + "I"][k]) and np.array_equal(im, chips[band + "Q"][k])
    out["x_matches"] = np.int64(1)
    for sig in SIGNALS:
        for fs in RATES:
            n = int(fs / 1000)
            for prn in PRNS:
                for shift in SHIFTS:
                    buf = np.zeros(2 * n, np.float32)
                    assert R.ref_e5_sampled(buf.ctypes.data_as(f32p), prn, sig.encode(), fs, shift) == n
                    re, im = buf[0::2], buf[1::2]
                    assert np.all(np.abs(re) == 1.0)
                    out[f"sampled_{sig}_{fs}_{prn}_{shift}_re"] = np.packbits(re < 0)
                    if sig[1] == "X":
                        assert np.all(np.abs(im) == 1.0)
                        out[f"sampled_{sig}_{fs}_{prn}_{shift}_im"] = np.packbits(im < 0)
                    else:
                        assert not np.any(im)
    out["sampled_signals"] = np.array(SIGNALS)
    out["sampled_rates"] = np.array(RATES, np.int64)
    out["sampled_prns"] = np.array(PRNS, np.int64)
    out["sampled_shifts"] = np.array(SHIFTS, np.int64)
    out["e5a_i_secondary"] = np.array(R.ref_e5a_i_secondary().decode())
    out["e5b_i_secondary"] = np.array(R.ref_e5b_i_secondary().decode())
    out["e5a_q_secondary"] = np.array([R.ref_e5a_q_secondary(p).decode() for p in range(1, 51)])
    out["e5b_q_secondary"] = np.array([R.ref_e5b_q_secondary(p).decode() for p in range(1, 51)])
    # the reference's E5a-Q table holds 47 strings: its rows of PRN 48..50 are empty, and stay empty here
    assert all(len(s) == 100 for s in out["e5a_q_secondary"][:47]) and all(len(s) == 0 for s in out["e5a_q_secondary"][47:])
    assert all(len(s) == 100 for s in out["e5b_q_secondary"])
    path = os.path.join(HERE, "galileo_e5_codes_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
