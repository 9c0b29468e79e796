"""Generate tests/golden/glonass_ref.npz from the REFERENCE's own GLONASS code generator, tables and loop filters.

    python tests/golden/make_glonass_golden.py REFERENCE_TREE SCRATCH_DIRECTORY

It needs the reference tree.  The script compiles
tests/golden/glonass_ref_shim.cc — extern "C" wrappers that pull in the reference's
glonass_l1_signal_replica.cc, tracking_2nd_DLL_filter.cc, tracking_2nd_PLL_filter.cc and GLONASS_L1_L2_CA.h by
name from the include path — into a shared object in the scratch directory, outside the repository, and
stores what it produces as data:

  chips_<shift>        int8[511]: glonass_l1_ca_code_gen_complex's real part (±1; the imaginary part is
                       zero, checked here) for chip shifts 0, 3 and 510
  sampled_<fs>_<shift> uint8: np.packbits of the sign bits (1 ↔ −1.0) of glonass_l1_ca_code_gen_complex_sampled's
                       real part, floor(fs / 1000) samples, at 4, 6.625 and 10 Msps and shifts 0 and 3 (the
                       imaginary part is zero, checked here)
  chip_shifts, sampled_rates, sampled_shifts
  prn_table            int32[25, 2]: (PRN, frequency channel) of every GLONASS_PRN entry, PRN 0 (the
                       reference's test entry) first
  constants            float64[8]: FREQ1_GLO, DFRQ1_GLO, FREQ2_GLO, DFRQ2_GLO, the L1 code rate and code
                       length, the L2 code rate and code length
  filter_in            float32[64]: a fixed input sequence for the two loop filters
  dll_out, pll_out     float32[64]: Tracking_2nd_DLL_filter (2 Hz) and Tracking_2nd_PLL_filter (50 Hz) over
                       filter_in, pdi 1 ms, after initialize()
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CHIP_SHIFTS = (0, 3, 510)
RATES = (4000000, 6625000, 10000000)
SAMPLED_SHIFTS = (0, 3)
f32p = ctypes.POINTER(ctypes.c_float)


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    ref, scratch = sys.argv[1], sys.argv[2]
    os.makedirs(scratch, exist_ok=True)
    so = os.path.join(scratch, "libgloref.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-std=c++20", "-DHAS_STD_SPAN=1",
                    "-I" + os.path.join(ref, "src/algorithms/libs"), "-I" + os.path.join(ref, "src/algorithms/tracking/libs"),
                    "-I" + os.path.join(ref, "src/core/system_parameters"), os.path.join(HERE, "glonass_ref_shim.cc"), "-o", so], check=True)
    R = ctypes.CDLL(so)
    R.ref_glo_chips.argtypes = [f32p, ctypes.c_uint32]
    R.ref_glo_chips.restype = None
    R.ref_glo_sampled.argtypes = [f32p, ctypes.c_int32, ctypes.c_uint32]
    R.ref_glo_sampled.restype = ctypes.c_int
    R.ref_glo_freq_channel.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_int32)]
    R.ref_glo_freq_channel.restype = ctypes.c_int
    R.ref_glo_constants.argtypes = [ctypes.POINTER(ctypes.c_double)]
    R.ref_glo_constants.restype = None
    for name in ("ref_glo_dll_filter", "ref_glo_pll_filter"):
        getattr(R, name).argtypes = [ctypes.c_float, f32p, f32p, ctypes.c_int]
        getattr(R, name).restype = None

    out = {}
    for shift in CHIP_SHIFTS:
        buf = np.zeros(2 * 511, np.float32)
        R.ref_glo_chips(buf.ctypes.data_as(f32p), shift)
        assert np.all(np.abs(buf[0::2]) == 1.0) and not np.any(buf[1::2])
        out[f"chips_{shift}"] = buf[0::2].astype(np.int8)
    for fs in RATES:
        n = int(fs / 1000)
        for shift in SAMPLED_SHIFTS:
            buf = np.zeros(2 * n, np.float32)
            assert R.ref_glo_sampled(buf.ctypes.data_as(f32p), fs, shift) == n
            assert np.all(np.abs(buf[0::2]) == 1.0) and not np.any(buf[1::2])
            out[f"sampled_{fs}_{shift}"] = np.packbits(buf[0::2] < 0)
    out["chip_shifts"] = np.array(CHIP_SHIFTS, np.int64)
    out["sampled_rates"] = np.array(RATES, np.int64)
    out["sampled_shifts"] = np.array(SAMPLED_SHIFTS, np.int64)
    table = []
    for prn in range(0, 64):
        k = ctypes.c_int32(0)
        if R.ref_glo_freq_channel(prn, ctypes.byref(k)):
            table.append((prn, k.value))
    out["prn_table"] = np.array(table, np.int32)
    assert out["prn_table"].shape == (25, 2)
    consts = np.zeros(8, np.float64)
    R.ref_glo_constants(consts.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    out["constants"] = consts
    # a discriminator-like sequence: a decaying oscillation plus noise, |x| < 0.5
    rng = np.random.default_rng(20171)
    t = np.arange(64)
    x = (0.3 * np.exp(-t / 25.0) * np.cos(0.4 * t) + 0.05 * rng.standard_normal(64)).astype(np.float32)
    out["filter_in"] = x
    for name, bw in (("dll", 2.0), ("pll", 50.0)):
        y = np.zeros(64, np.float32)
        getattr(R, f"ref_glo_{name}_filter")(bw, x.ctypes.data_as(f32p), y.ctypes.data_as(f32p), 64)
        out[f"{name}_out"] = y
    path = os.path.join(HERE, "glonass_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
