"""Generate tests/golden/gps_l5_codes_ref.npz from the REFERENCE's own GPS L5 generators.

    python tests/golden/make_l5_golden.py REFERENCE_TREE SCRATCH_DIRECTORY

Run in the build container only (it needs the reference tree).  The script compiles
tests/golden/l5_ref_shim.cc — extern "C" wrappers that pull in the reference's
gps_l5_signal_replica.cc by name from the include path — into a shared object in the scratch
directory, outside the repository, and stores what it produces as data:

  l5i_bits, l5q_bits   uint8[32, 1279]: np.packbits of the chip bits (1 ↔ chip −1.0) of PRN 1..32,
                       10230 chips each
  sampled_<c>_<fs>_<prn>  np.packbits of the sampled code's sign bits, c = 'i' (the code lies in the
                       real part, the imaginary part is zero) or 'q' (imaginary part, real zero)
  sampled_rates, sampled_prns

The sample rates are ones at which the reference's index before the forced last sample,
ceil(ts·(i + 1)/tc) − 1 in float, stays below 10230 for every i (checked here): the reference reads
its chip array at that index without a bound check.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RATES = (12500000, 25000000)
PRNS = (3, 29)
f32p = ctypes.POINTER(ctypes.c_float)


def max_index(fs: int) -> int:
    """The largest chip index the reference forms before its forced last sample (float arithmetic)."""
    n = int(float(fs) / (10.23e6 / 10230.0))
    ts = np.float32(1.0) / np.float32(fs)
    m = 0
    for tc in (np.float32(1.0 / float(np.float32(10.23e6))), np.float32(1.0) / np.float32(10.23e6)):  # L5I's and L5Q's tc
        i = np.arange(n - 1, dtype=np.float32)
        idx = np.ceil((ts * (i + np.float32(1.0))) / tc).astype(np.int64) - 1
        assert idx.min() >= 0
        m = max(m, int(idx.max()))
    return m


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    ref, scratch = sys.argv[1], sys.argv[2]
    so = os.path.join(scratch, "libl5ref.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-std=c++20", "-DHAS_STD_SPAN=1",
                    "-I" + os.path.join(ref, "src/algorithms/libs"), "-I" + os.path.join(ref, "src/core/system_parameters"),
                    os.path.join(HERE, "l5_ref_shim.cc"), "-o", so], check=True)
    R = ctypes.CDLL(so)
    for name in ("ref_gps_l5i_code_gen_float", "ref_gps_l5q_code_gen_float"):
        getattr(R, name).argtypes = [f32p, ctypes.c_uint32]
    for name in ("ref_gps_l5i_code_gen_complex_sampled", "ref_gps_l5q_code_gen_complex_sampled"):
        getattr(R, name).argtypes = [f32p, ctypes.c_uint32, ctypes.c_int32]
        getattr(R, name).restype = ctypes.c_int
    out = {}
    for comp, fn in (("i", R.ref_gps_l5i_code_gen_float), ("q", R.ref_gps_l5q_code_gen_float)):
        chips = np.zeros((32, 10230), np.float32)
        for k in range(32):
            fn(chips[k].ctypes.data_as(f32p), k + 1)
        assert np.all(np.abs(chips) == 1.0)
        out[f"l5{comp}_bits"] = np.packbits(chips < 0, axis=1)
    for fs in RATES:
        assert max_index(fs) < 10230, (fs, max_index(fs))
        for prn in PRNS:
            n = int(fs / 1000)
            for comp, fn in (("i", R.ref_gps_l5i_code_gen_complex_sampled), ("q", R.ref_gps_l5q_code_gen_complex_sampled)):
                buf = np.zeros(2 * n, np.float32)
                assert fn(buf.ctypes.data_as(f32p), prn, fs) == n
                code, other = (buf[0::2], buf[1::2]) if comp == "i" else (buf[1::2], buf[0::2])
                assert np.all(np.abs(code) == 1.0) and not np.any(other)
                out[f"sampled_{comp}_{fs}_{prn}"] = np.packbits(code < 0)
    out["sampled_rates"] = np.array(RATES, np.int64)
    out["sampled_prns"] = np.array(PRNS, np.int64)
    path = os.path.join(HERE, "gps_l5_codes_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
