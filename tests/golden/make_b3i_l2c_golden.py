"""Generate tests/golden/b3i_l2c_codes_ref.npz from the REFERENCE's own BeiDou B3I and GPS L2C generators.

    python tests/golden/make_b3i_l2c_golden.py REFERENCE_TREE SCRATCH_DIRECTORY

Run in the build container only (it needs the reference tree).  The script compiles
tests/golden/b3i_l2c_ref_shim.cc — extern "C" wrappers that pull in the reference's
beidou_b3i_signal_replica.cc and gps_l2c_signal_replica.cc by name from the include path — into a shared
object in the scratch directory, outside the repository, and stores what it produces as data:

  b3i_bits   uint8[63, 1279]: np.packbits of (chip < 0) of B3I PRN 1..63, 10230 chips each
  l2c_bits   uint8[50, 1279]: the same of the L2 CM code of PRN 1..50
  sampled_b3i_<fs>_<prn>_<chip_shift>   np.packbits of (code < 0) of the sampled B3I code (real part; the
             imaginary part is zero)
  sampled_l2c_<fs>_<prn>                the same of the sampled L2 CM code (imaginary part; real zero)
  b3i_rates, l2c_rates, sampled_prns, b3i_shifts (the chip shifts stored at b3i_rates[0]; other rates: 0)

The sample rates are ones at which the reference's chip index before the forced last sample stays below
10230 for every sample (checked here): the reference reads its chip array at that index unchecked.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
B3I_RATES = (12500000, 25000000)
L2C_RATES = (1250000, 2000000)
PRNS = (9, 30)
B3I_SHIFTS = (0, 37)
L = 10230
f32p = ctypes.POINTER(ctypes.c_float)


def max_index(fs: int, chip_rate: float, rule: str) -> int:
    """The largest chip index the reference forms before its forced last sample (float arithmetic)."""
    n = int(float(fs) / (chip_rate / L))
    ts = np.float32(1.0) / np.float32(fs)
    # B3I forms tc as 1.0 / float (a double division), L2C as 1.0F / float
    tc = np.float32(1.0 / float(np.float32(chip_rate))) if rule == "trunc" else np.float32(1.0) / np.float32(chip_rate)
    i = np.arange(n - 1, dtype=np.float32)
    aux = (ts * (i + np.float32(1.0))) / tc
    idx = ((aux + np.float32(1.0)).astype(np.int64) if rule == "trunc" else np.ceil(aux).astype(np.int64)) - 1
    assert idx.min() >= 0
    return int(idx.max())


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    ref, scratch = sys.argv[1], sys.argv[2]
    so = os.path.join(scratch, "libb3il2cref.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-std=c++20", "-DHAS_STD_SPAN=1",
                    "-I" + os.path.join(ref, "src/algorithms/libs"), "-I" + os.path.join(ref, "src/core/system_parameters"),
                    os.path.join(HERE, "b3i_l2c_ref_shim.cc"), "-o", so], check=True)
    R = ctypes.CDLL(so)
    R.ref_beidou_b3i_code_gen_float.argtypes = [f32p, ctypes.c_int32, ctypes.c_uint32]
    R.ref_gps_l2c_m_code_gen_float.argtypes = [f32p, ctypes.c_uint32]
    R.ref_beidou_b3i_code_gen_complex_sampled.argtypes = [f32p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint32]
    R.ref_gps_l2c_m_code_gen_complex_sampled.argtypes = [f32p, ctypes.c_uint32, ctypes.c_int32]
    out = {}
    chips = np.zeros((63, L), np.float32)
    for k in range(63):
        R.ref_beidou_b3i_code_gen_float(chips[k].ctypes.data_as(f32p), k + 1, 0)
    assert np.all(np.abs(chips) == 1.0)
    out["b3i_bits"] = np.packbits(chips < 0, axis=1)
    chips = np.zeros((50, L), np.float32)
    for k in range(50):
        R.ref_gps_l2c_m_code_gen_float(chips[k].ctypes.data_as(f32p), k + 1)
    assert np.all(np.abs(chips) == 1.0)
    out["l2c_bits"] = np.packbits(chips < 0, axis=1)
    for fs in B3I_RATES:
        assert max_index(fs, 10.23e6, "trunc") < L, (fs, max_index(fs, 10.23e6, "trunc"))
        n = int(fs / 1000)
        for prn in PRNS:
            for shift in (B3I_SHIFTS if fs == B3I_RATES[0] else (0,)):
                buf = np.zeros(2 * n, np.float32)
                assert R.ref_beidou_b3i_code_gen_complex_sampled(buf.ctypes.data_as(f32p), prn, fs, shift) == n
                assert np.all(np.abs(buf[0::2]) == 1.0) and not np.any(buf[1::2])
                out[f"sampled_b3i_{fs}_{prn}_{shift}"] = np.packbits(buf[0::2] < 0)
    for fs in L2C_RATES:
        assert max_index(fs, 0.5115e6, "ceil") < L, (fs, max_index(fs, 0.5115e6, "ceil"))
        n = int(fs / 50)
        for prn in PRNS:
            buf = np.zeros(2 * n, np.float32)
            assert R.ref_gps_l2c_m_code_gen_complex_sampled(buf.ctypes.data_as(f32p), prn, fs) == n
            assert np.all(np.abs(buf[1::2]) == 1.0) and not np.any(buf[0::2])
            out[f"sampled_l2c_{fs}_{prn}"] = np.packbits(buf[1::2] < 0)
    out["b3i_rates"] = np.array(B3I_RATES, np.int64)
    out["l2c_rates"] = np.array(L2C_RATES, np.int64)
    out["sampled_prns"] = np.array(PRNS, np.int64)
    out["b3i_shifts"] = np.array(B3I_SHIFTS, np.int64)
    path = os.path.join(HERE, "b3i_l2c_codes_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
