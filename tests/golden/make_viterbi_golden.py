"""Generate tests/golden/viterbi_ref.npz from the REFERENCE's own Viterbi_Decoder.

    python tests/golden/make_viterbi_golden.py REFERENCE_TREE SCRATCH_DIRECTORY

It needs the reference tree.  The script compiles tests/golden/viterbi_ref_shim.cc — extern "C" wrappers that pull
in the reference's viterbi_decoder.cc by name from the include path — into a shared object in the scratch
directory, outside the repository.  The decoder's one outside call is volk_gnsssdr_32f_index_max_32u; the script
writes into the scratch directory a <volk_gnsssdr/volk_gnsssdr.h> that holds that one declaration and a C file that
defines it from the reference's _generic kernel header (LV_HAVE_GENERIC, include paths as in oracle/Makefile).

For LL in 114, 238, 486 (I/NAV, F/NAV, C/NAV) and each kind of input, ONE decoder object decodes four consecutive
frames (reset() is called ahead of the third: it leaves the metrics alone).  Kinds:
  0  encoded random bits, ±1 symbols plus Gaussian noise of sigma 0.3
  1  the same at sigma 0.6
  2  the sigma 0.6 symbols of kind 1 rounded to multiples of 0.5 (frequent ties)
  3  alternating all-zero and pure-noise (sigma 1) frames
Stored per (LL, kind), as data:
  sym_<LL>_<kind>    float32[4, 2·(LL + 6)]  what decode() was given
  bits_<LL>_<kind>   uint8: np.packbits of the int32[4, LL] decode() returned (all 0 / 1, checked here), per frame
  sec_<LL>_<kind>    float32[4, 64]          d_prev_section after each call
  truth_<LL>_<kind>  uint8: np.packbits of the encoded bits (kinds 0-2)
  lengths, kinds, g
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import viterbi_model as V  # noqa: E402  (the encoder that makes the inputs)

LENGTHS = (114, 238, 486)
KINDS = (0, 1, 2, 3)
FRAMES = 4
G = (121, 91)
f32p = ctypes.POINTER(ctypes.c_float)
i32p = ctypes.POINTER(ctypes.c_int32)

VOLK_HEADER = """#include <stdint.h>
#ifdef __cplusplus
extern "C"
#endif
void volk_gnsssdr_32f_index_max_32u(uint32_t* target, const float* src0, uint32_t num_points);
"""
VOLK_SOURCE = """#define LV_HAVE_GENERIC 1
#include <volk_gnsssdr_32f_index_max_32u.h>
void volk_gnsssdr_32f_index_max_32u(uint32_t* target, const float* src0, uint32_t num_points)
{
    volk_gnsssdr_32f_index_max_32u_generic(target, src0, num_points);
}
"""


def build(ref, scratch):
    os.makedirs(os.path.join(scratch, "volk_gnsssdr"), exist_ok=True)
    with open(os.path.join(scratch, "volk_gnsssdr", "volk_gnsssdr.h"), "w") as f:
        f.write(VOLK_HEADER)
    src = os.path.join(scratch, "vit_index_max.c")
    with open(src, "w") as f:
        f.write(VOLK_SOURCE)
    volk = os.path.join(ref, "src/algorithms/libs/volk_gnsssdr_module/volk_gnsssdr")
    obj = os.path.join(scratch, "vit_index_max.o")
    subprocess.run(["gcc", "-O2", "-fPIC", "-ffp-contract=off", "-std=gnu11", "-I" + os.path.join(volk, "include"),
                    "-I" + os.path.join(volk, "kernels/volk_gnsssdr"), "-c", src, "-o", obj], check=True)
    so = os.path.join(scratch, "libvitref.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-std=c++17", "-I" + scratch,
                    "-I" + os.path.join(ref, "src/algorithms/telemetry_decoder/libs"), os.path.join(HERE, "viterbi_ref_shim.cc"), obj,
                    "-o", so], check=True)
    R = ctypes.CDLL(so)
    R.ref_vit_new.argtypes = [ctypes.c_int32] * 5
    R.ref_vit_new.restype = ctypes.c_void_p
    R.ref_vit_decode.argtypes = [ctypes.c_void_p, f32p, ctypes.c_int32, i32p, ctypes.c_int32, f32p]
    R.ref_vit_decode.restype = None
    R.ref_vit_reset.argtypes = [ctypes.c_void_p]
    R.ref_vit_reset.restype = None
    R.ref_vit_delete.argtypes = [ctypes.c_void_p]
    R.ref_vit_delete.restype = None
    return R


def inputs(LL, rng):
    """{kind: (symbols float32[4, frame], truth uint8[4, LL] or None)}."""
    frame = 2 * (LL + 6)
    out = {}
    for kind, sigma in ((0, 0.3), (1, 0.6)):
        truth = rng.integers(0, 2, (FRAMES, LL)).astype(np.uint8)
        clean = np.stack([V.encode(b, G) for b in truth])
        out[kind] = ((clean + sigma * rng.standard_normal((FRAMES, frame))).astype(np.float32), truth)
    out[2] = ((np.round(out[1][0] * 2.0) / 2.0).astype(np.float32), out[1][1])
    sym = np.zeros((FRAMES, frame), np.float32)
    sym[1::2] = rng.standard_normal((FRAMES // 2, frame)).astype(np.float32)
    out[3] = (sym, None)
    return out


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    R = build(sys.argv[1], sys.argv[2])
    rng = np.random.default_rng(20211)
    out = {"lengths": np.array(LENGTHS, np.int64), "kinds": np.array(KINDS, np.int64), "g": np.array(G, np.int64)}
    for LL in LENGTHS:
        for kind, (sym, truth) in inputs(LL, rng).items():
            h = R.ref_vit_new(7, 2, LL, G[0], G[1])
            bits = np.zeros((FRAMES, LL), np.int32)
            sec = np.zeros((FRAMES, 64), np.float32)
            for f in range(FRAMES):
                if f == 2:
                    R.ref_vit_reset(h)
                x = np.ascontiguousarray(sym[f])
                R.ref_vit_decode(h, x.ctypes.data_as(f32p), x.size, bits[f].ctypes.data_as(i32p), LL, sec[f].ctypes.data_as(f32p))
            R.ref_vit_delete(h)
            assert np.all((bits == 0) | (bits == 1))
            out[f"sym_{LL}_{kind}"] = sym
            out[f"bits_{LL}_{kind}"] = np.packbits(bits.astype(np.uint8), axis=1)
            out[f"sec_{LL}_{kind}"] = sec
            if truth is not None:
                out[f"truth_{LL}_{kind}"] = np.packbits(truth, axis=1)
    path = os.path.join(HERE, "viterbi_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
