"""Generate tests/golden/cnav_ref.npz from the REFERENCE's own libswiftcnav.

    python tests/golden/make_cnav_golden.py REFERENCE_TREE SCRATCH_DIRECTORY

It needs the reference tree.  The script compiles tests/golden/cnav_ref_shim.c together with the library's cnav_msg.c,
viterbi27.c, bits.c and edc.c, named on the compile line from the reference tree as separate translation units, into a
shared object in the scratch directory, outside the repository.  Only the recorded data is committed.

The inputs are tests/cnav_model.golden_streams(): hard symbols from the model's transmitter.  Stored per stream NAME:
  NAME_sym      uint8[]        the input symbols, one bit each (1 -> 0xFF, 0 -> 0x00), packed
  NAME_n        int32          how many
  NAME_bias     uint32         what ref_cnav_add_metrics put on every metric before the first symbol
  NAME_ev       int32[k, 6]    every symbol (index) at which cnav_msg_decoder_add_symbol returned true, with delay, tow,
                               msg_id, prn, alert
  NAME_raw      uint8[k, 64]   the raw message of each
  NAME_snap     int32[m, 21]   after every 64th symbol and after the last: the symbols so far, then all scalar members of
                               both parts (cnav_ref_shim.c, ref_cnav_scalars)
  NAME_metrics  uint32[2, 2, 64], NAME_decisions uint32[2, 64, 2], NAME_symbols uint8[2, 128], NAME_decoded uint8[2, 64]
                               the struct contents after the last symbol, per part
The archive is written with fixed time stamps, so regenerating reproduces the committed file byte for byte.
"""
from __future__ import annotations

import ctypes
import io
import os
import subprocess
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cnav_model as M  # noqa: E402  (the transmitter that makes the inputs)

LIB = "src/algorithms/telemetry_decoder/libs/libswiftcnav"


def build(ref, scratch):
    os.makedirs(scratch, exist_ok=True)
    so = os.path.join(scratch, "libcnavref.so")
    lib = os.path.join(ref, LIB)
    subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-std=gnu11", "-I" + lib, os.path.join(HERE, "cnav_ref_shim.c")] +
                   [os.path.join(lib, f) for f in ("cnav_msg.c", "viterbi27.c", "bits.c", "edc.c")] + ["-o", so], check=True)
    R = ctypes.CDLL(so)
    R.ref_cnav_new.restype = ctypes.c_void_p
    R.ref_cnav_delete.argtypes = [ctypes.c_void_p]
    R.ref_cnav_delete.restype = None
    R.ref_cnav_add_metrics.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    R.ref_cnav_add_metrics.restype = None
    R.ref_cnav_add_symbol.argtypes = [ctypes.c_void_p, ctypes.c_uint8, ctypes.c_void_p, ctypes.c_void_p]
    R.ref_cnav_add_symbol.restype = ctypes.c_int32
    R.ref_cnav_scalars.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    R.ref_cnav_scalars.restype = None
    R.ref_cnav_arrays.argtypes = [ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_void_p] * 5
    R.ref_cnav_arrays.restype = None
    return R


def record(R, name, bits, bias, out):
    h = R.ref_cnav_new()
    if bias:
        R.ref_cnav_add_metrics(h, bias)
    ev, raws, snaps = [], [], []
    out5, raw, sc = np.zeros(5, np.uint32), np.zeros(64, np.uint8), np.zeros(20, np.int32)
    n = len(bits)
    for k in range(n):
        if R.ref_cnav_add_symbol(h, 255 if bits[k] else 0, out5.ctypes.data, raw.ctypes.data):
            ev.append([k] + out5.tolist())
            raws.append(raw.copy())
        if (k + 1) % 64 == 0 or k + 1 == n:
            R.ref_cnav_scalars(h, sc.ctypes.data)
            snaps.append([k + 1] + sc.tolist())
    metrics, dec = np.zeros((2, 2, 64), np.uint32), np.zeros((2, 64, 2), np.uint32)
    symbols, decoded = np.zeros((2, 128), np.uint8), np.zeros((2, 64), np.uint8)
    for p in range(2):
        R.ref_cnav_arrays(h, p, metrics[p, 0].ctypes.data, metrics[p, 1].ctypes.data, dec[p].ctypes.data, symbols[p].ctypes.data, decoded[p].ctypes.data)
    R.ref_cnav_delete(h)
    out[name + "_sym"] = np.packbits(np.asarray(bits, np.uint8))
    out[name + "_n"] = np.int32(n)
    out[name + "_bias"] = np.uint32(bias)
    out[name + "_ev"] = np.array(ev, np.int32).reshape(-1, 6)
    out[name + "_raw"] = np.array(raws, np.uint8).reshape(-1, 64)
    out[name + "_snap"] = np.array(snaps, np.int32)
    out[name + "_metrics"], out[name + "_decisions"], out[name + "_symbols"], out[name + "_decoded"] = metrics, dec, symbols, decoded
    return ev


def save(path, arrays):
    """An .npz with fixed member time stamps."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    R = build(sys.argv[1], sys.argv[2])
    out = {}
    for name, (bits, bias) in M.golden_streams().items():
        ev = record(R, name, bits, bias, out)
        print(name, len(bits), [e[0] for e in ev][:8])
    path = os.path.join(HERE, "cnav_ref.npz")
    save(path, out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
