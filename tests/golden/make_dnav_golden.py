"""Generate tests/golden/dnav_ref.npz from the REFERENCE's own Beidou_Dnav_Navigation_Message.

    python tests/golden/make_dnav_golden.py REFERENCE_TREE SCRATCH_DIRECTORY

It needs the reference tree.  The script compiles tests/golden/dnav_ref_shim.cc — extern "C" wrappers that pull in the
reference's beidou_dnav_navigation_message.cc, beidou_dnav_ephemeris.cc and gnss_satellite.cc by name from the include
path — into a shared object in the scratch directory, outside the repository.  glog and Boost are not needed for what is
called: the script writes stand-in <glog/logging.h> and <boost/serialization/nvp.hpp> into the scratch directory, as
make_lnav_golden.py does.

Two Beidou_Dnav_Navigation_Message objects, one per decoder, are each given 64 subframes in turn: 300 bits as the
telemetry block hands them over, built by tests/dnav_model.build_subframe with random payloads, FraID 0..7, Pnum 0..15
(D2) or 0..127 (D1) and SOW values that include 0 and 2^20 - 1.  The new-SOW flag is cleared after every call, as the block
does.  Stored, as data, per decoder (axis 0: D1, D2):
  bits     uint8[2, 64, 38]  the 300 bits, packed MSB first
  ids      int32[2, 64]      what the decoder returned
  sows     float64[2, 64]    get_SOW() after the call
  crc      uint8[2, 64]      get_flag_CRC_test() after the call
  new_sow  uint8[2, 64]      get_flag_new_SOW_available() after the call
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dnav_model as M  # noqa: E402  (the transmitter that makes the inputs)
from make_lnav_golden import GLOG_HEADER, NVP_HEADER  # noqa: E402

N = 64


def build(ref, scratch):
    for sub, name, text in (("glog", "logging.h", GLOG_HEADER), ("boost/serialization", "nvp.hpp", NVP_HEADER)):
        os.makedirs(os.path.join(scratch, sub), exist_ok=True)
        with open(os.path.join(scratch, sub, name), "w") as f:
            f.write(text)
    so = os.path.join(scratch, "libdnavref.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-I" + scratch, "-I" + os.path.join(ref, "src/core/system_parameters"),
                    "-I" + os.path.join(ref, "src/algorithms/libs"), os.path.join(HERE, "dnav_ref_shim.cc"), "-o", so], check=True)
    R = ctypes.CDLL(so)
    R.ref_dnav_new.restype = ctypes.c_void_p
    R.ref_dnav_decode.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double),
                                  ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
    R.ref_dnav_decode.restype = ctypes.c_int32
    R.ref_dnav_delete.argtypes = [ctypes.c_void_p]
    R.ref_dnav_delete.restype = None
    return R


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    R = build(sys.argv[1], sys.argv[2])
    rng = np.random.default_rng(20260)
    bits = np.zeros((2, N, 38), np.uint8)
    ids, sows = np.zeros((2, N), np.int32), np.zeros((2, N), np.float64)
    crc, new_sow = np.zeros((2, N), np.uint8), np.zeros((2, N), np.uint8)
    for d2 in (0, 1):
        fra = np.concatenate([[0, 1, 6, 2, 7, 3, 4, 5], rng.integers(0, 8, N - 8)])
        pn = np.concatenate([np.arange(16), rng.integers(0, 16, N - 16)]) if d2 else rng.integers(0, 128, N)
        if d2:
            fra[8:40] = 1  # most Pnum values under FraID 1, where they matter
            pn[8:24] = np.arange(16)
        sow = rng.integers(1, 1 << 20, N)
        sow[[1, 9, 30]] = 0
        sow[[3, 10, 31]] = (1 << 20) - 1
        h = R.ref_dnav_new()
        for k in range(N):
            plain, _ = M.build_subframe(bool(d2), int(fra[k]), int(pn[k]), int(sow[k]), rng.integers(0, 2, 182))
            bits[d2, k] = np.packbits(np.array(plain + [0] * 4, np.uint8))
            text = "".join("1" if b else "0" for b in plain).encode()
            s, c, f = ctypes.c_double(), ctypes.c_int32(), ctypes.c_int32()
            ids[d2, k] = R.ref_dnav_decode(h, d2, text, ctypes.byref(s), ctypes.byref(c), ctypes.byref(f))
            sows[d2, k], crc[d2, k], new_sow[d2, k] = s.value, c.value, f.value
        R.ref_dnav_delete(h)
    path = os.path.join(HERE, "dnav_ref.npz")
    np.savez_compressed(path, bits=bits, ids=ids, sows=sows, crc=crc, new_sow=new_sow)
    print(path, os.path.getsize(path), ids[:, :10].tolist(), sows[:, :6].tolist(), new_sow[:, :10].tolist())


if __name__ == "__main__":
    main()
