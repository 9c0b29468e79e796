"""Generate tests/golden/lnav_ref.npz from the REFERENCE's own Gps_Navigation_Message.

    python tests/golden/make_lnav_golden.py REFERENCE_TREE SCRATCH_DIRECTORY

It needs the reference tree.  The script compiles tests/golden/lnav_ref_shim.cc — extern "C" wrappers that pull in the
reference's gps_navigation_message.cc, gps_ephemeris.cc and gnss_satellite.cc by name from the include path — into a
shared object in the scratch directory, outside the repository.  glog and Boost are not needed for what is called: the
script writes stand-in <glog/logging.h> (LOG / DLOG into a sink) and <boost/serialization/nvp.hpp> (the one macro; the
serialisation templates are never instantiated) into the scratch directory.

One Gps_Navigation_Message object is given 64 subframes in turn, each 40 bytes: the ten words as the telemetry block
stores them, built by tests/lnav_model.build_subframe with random payloads, IDs 0..7 and TOW counts that include 0.
Stored, as data:
  subframes  uint8[64, 40]   what subframe_decoder() was given
  ids        int32[64]       what it returned
  tows       int32[64]       get_TOW() after the call (an ID outside 1..5 leaves it alone)
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lnav_model as M  # noqa: E402  (the transmitter that makes the inputs)

N = 64

GLOG_HEADER = """#pragma once
#include <ostream>
struct lnav_golden_sink
{
    template <class T>
    lnav_golden_sink& operator<<(const T&) { return *this; }
    lnav_golden_sink& operator<<(std::ostream& (*)(std::ostream&)) { return *this; }
};
#define LOG(severity) lnav_golden_sink()
#define DLOG(severity) lnav_golden_sink()
#define VLOG(level) lnav_golden_sink()
"""
NVP_HEADER = """#pragma once
#define BOOST_SERIALIZATION_NVP(x) x
namespace boost
{
namespace serialization
{
template <class T>
T& make_nvp(const char*, T& t) { return t; }
}  // namespace serialization
}  // namespace boost
"""


def build(ref, scratch):
    for sub, name, text in (("glog", "logging.h", GLOG_HEADER), ("boost/serialization", "nvp.hpp", NVP_HEADER)):
        os.makedirs(os.path.join(scratch, sub), exist_ok=True)
        with open(os.path.join(scratch, sub, name), "w") as f:
            f.write(text)
    so = os.path.join(scratch, "liblnavref.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-I" + scratch, "-I" + os.path.join(ref, "src/core/system_parameters"),
                    "-I" + os.path.join(ref, "src/algorithms/libs"), os.path.join(HERE, "lnav_ref_shim.cc"), "-o", so], check=True)
    R = ctypes.CDLL(so)
    R.ref_lnav_new.restype = ctypes.c_void_p
    R.ref_lnav_decode.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int32)]
    R.ref_lnav_decode.restype = ctypes.c_int32
    R.ref_lnav_delete.argtypes = [ctypes.c_void_p]
    R.ref_lnav_delete.restype = None
    return R


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    R = build(sys.argv[1], sys.argv[2])
    rng = np.random.default_rng(20240)
    ids = np.concatenate([[1, 0, 2, 6, 3, 7, 4, 5], rng.integers(0, 8, N - 8)])
    tows = rng.integers(1, 1 << 17, N)
    tows[[2, 11, 12]] = 0
    tows[20] = (1 << 17) - 1
    subframes = np.zeros((N, 40), np.uint8)
    got_ids, got_tows = np.zeros(N, np.int32), np.zeros(N, np.int32)
    h = R.ref_lnav_new()
    for k in range(N):
        _, words = M.build_subframe(int(ids[k]), int(tows[k]), rng.integers(0, 2, 208))
        subframes[k] = np.frombuffer(np.array(words, "<u4").tobytes(), np.uint8)
        tow = ctypes.c_int32()
        got_ids[k] = R.ref_lnav_decode(h, subframes[k].tobytes(), ctypes.byref(tow))
        got_tows[k] = tow.value
    R.ref_lnav_delete(h)
    path = os.path.join(HERE, "lnav_ref.npz")
    np.savez_compressed(path, subframes=subframes, ids=got_ids, tows=got_tows)
    print(path, os.path.getsize(path), got_ids[:12].tolist(), got_tows[:12].tolist())


if __name__ == "__main__":
    main()
