"""Generate tests/golden/gnav_ref.npz from the REFERENCE's own Glonass_Gnav_Navigation_Message and Glonass_Gnav_Ephemeris.

    python tests/golden/make_gnav_golden.py REFERENCE_TREE SCRATCH_DIRECTORY

It needs the reference tree.  The script compiles tests/golden/gnav_ref_shim.cc — extern "C" wrappers that pull in the
reference's glonass_gnav_navigation_message.cc, glonass_gnav_ephemeris.cc, glonass_gnav_utc_model.cc and gnss_satellite.cc
by name from the include path — into a shared object in the scratch directory, outside the repository.  glog and
<boost/serialization/nvp.hpp> are stood in for as make_lnav_golden.py does.

glonass_gnav_ephemeris.cc also needs boost::gregorian and boost::posix_time, and Boost is not assumed to be installed: the
script writes stand-in date-time headers into the scratch directory that cover what that file uses and no more — date(y, m,
d), days, date +- days, date - date, ptime(date, time_duration), .date(), .time_of_day().total_seconds(), ptime +
time_duration, >=, a default ptime, and time_duration(h, m, s) of integers with Boost's rule for a negative part.  THE TIME
OF WEEK IN THIS GOLDEN THEREFORE RESTS ON A STAND-IN CALENDAR, NOT ON BOOST ITSELF.  To pin that down the script asks the
compiled stand-in for every date and second of day it used (ref_gnav_calendar) and compares each with Python's datetime,
and it checks the five (week, tow) cases of the reference's glonass_gnav_ephemeris_test.cc in the one-sided form that test
asserts them (two of the five are calendar facts and come out exactly; the expected values of the other three are not what
the reference computes, see main()), and every direct call against plain day counting in Python.  Everything else in the file (CRC_test, string_decoder, the flags) uses no Boost at all.

Stored, as data:
  chars   uint8[N, 85]  the strings fed, character 0 first, one row per string_decoder call
  seq     int32[N]      the sequence the call belongs to: each sequence starts on a new navigation object
  ret     int32[N]      what string_decoder returned
  bits    uint8[N, 85]  the bitset after CRC_test, bits[0] first
  flags   uint8[N, 6]   flag_CRC_test, flag_TOW_set, flag_TOW_new, have_new_ephemeris(), have_new_utc_model(),
                        flag_update_slot_number, after the call (the last four are then cleared as the block clears them)
  tow, wn, n            d_TOW float64[N], d_WN int32[N], d_n float64[N] after the call
  glot    float64[K, 7] direct glot_to_gpst calls: d_yr, d_N_T, tod_offset, tau_c, tau_gps, then the week and tow returned
"""
from __future__ import annotations

import ctypes
import datetime
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gnav_model as M  # noqa: E402  (the transmitter that makes the inputs)
from make_lnav_golden import GLOG_HEADER, NVP_HEADER  # noqa: E402

DATE_TIME_HEADER = """#pragma once
// Stand-in for the parts of Boost.Date_Time that glonass_gnav_ephemeris.cc uses (tests/golden/make_gnav_golden.py).
#include <cstdint>
namespace boost
{
namespace gregorian
{
struct date_duration
{
    long v;
    date_duration(long d) : v(d) {}
    long days() const { return v; }
};
typedef date_duration days;
struct date
{
    long n;  // days since 1970-01-01, proleptic Gregorian
    date() : n(0) {}
    date(long y, int m, int d)
    {
        y -= m <= 2;
        const long era = (y >= 0 ? y : y - 399) / 400;
        const long yoe = y - era * 400;
        const long doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1;
        const long doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
        n = era * 146097 + doe - 719468;
    }
};
inline date operator+(const date& a, const date_duration& b)
{
    date r;
    r.n = a.n + b.v;
    return r;
}
inline date operator-(const date& a, const date_duration& b)
{
    date r;
    r.n = a.n - b.v;
    return r;
}
inline date_duration operator-(const date& a, const date& b) { return date_duration(a.n - b.n); }
}  // namespace gregorian
namespace posix_time
{
struct time_duration
{
    int64_t s;
    time_duration() : s(0) {}
    time_duration(int64_t h, int64_t m, int64_t sec)
    {
        if (h < 0 || m < 0 || sec < 0)
            {
                h = h < 0 ? -h : h;
                m = m < 0 ? -m : m;
                sec = sec < 0 ? -sec : sec;
                s = -(h * 3600 + m * 60 + sec);
            }
        else
            {
                s = h * 3600 + m * 60 + sec;
            }
    }
    int64_t total_seconds() const { return s; }
};
struct ptime
{
    int64_t t;   // seconds since 1970-01-01
    bool valid;  // a default ptime is not a date-time
    ptime() : t(0), valid(false) {}
    ptime(const gregorian::date& d, const time_duration& td) : t(d.n * 86400 + td.s), valid(true) {}
    gregorian::date date() const
    {
        gregorian::date r;
        r.n = t >= 0 ? t / 86400 : -((-t + 86399) / 86400);
        return r;
    }
    time_duration time_of_day() const
    {
        time_duration r;
        r.s = t - date().n * 86400;
        return r;
    }
    bool operator>=(const ptime& o) const { return t >= o.t; }
};
inline ptime operator+(const ptime& a, const time_duration& b)
{
    ptime r = a;
    r.t += b.s;
    return r;
}
}  // namespace posix_time
}  // namespace boost
"""

CALENDAR_USED = []  # (base year, days added, seconds) of every instant a sequence or a direct call touches


def build(ref, scratch):
    headers = [("glog", "logging.h", GLOG_HEADER), ("boost/serialization", "nvp.hpp", NVP_HEADER)]
    headers += [("boost/date_time/posix_time", name, DATE_TIME_HEADER) for name in ("ptime.hpp", "posix_time.hpp", "time_formatters.hpp")]
    for sub, name, text in headers:
        os.makedirs(os.path.join(scratch, sub), exist_ok=True)
        with open(os.path.join(scratch, sub, name), "w") as f:
            f.write(text)
    so = os.path.join(scratch, "libgnavref.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-I" + scratch, "-I" + os.path.join(ref, "src/core/system_parameters"),
                    "-I" + os.path.join(ref, "src/algorithms/libs"), os.path.join(HERE, "gnav_ref_shim.cc"), "-o", so], check=True)
    R = ctypes.CDLL(so)
    R.ref_gnav_new.restype = ctypes.c_void_p
    R.ref_gnav_decode.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double),
                                  ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)]
    R.ref_gnav_decode.restype = ctypes.c_int32
    R.ref_gnav_delete.argtypes = [ctypes.c_void_p]
    R.ref_gnav_delete.restype = None
    R.ref_gnav_glot_to_gpst.argtypes = [ctypes.c_double] * 5 + [ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)]
    R.ref_gnav_glot_to_gpst.restype = None
    R.ref_gnav_calendar.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    R.ref_gnav_calendar.restype = None
    return R


def frame(rng, t_k_raw, t_b_raw, n_t, n, n_4, tau_c, tau_gps, ids=(1, 2, 3, 4, 5)):
    t_k = (t_k_raw >> 7) * 3600 + ((t_k_raw >> 1) & 63) * 60 + (t_k_raw & 1) * 30
    CALENDAR_USED.append((1992 + 4 * n_4, n_t - 1, t_k + 10 - 10800))
    return M.frame_strings(t_k_raw, t_b_raw, n_t, n, n_4, tau_c, tau_gps, rng, ids)


def almanac(rng, sid):
    """An almanac string with a random payload: its slot number (characters 9..13) is sometimes outside 1..24."""
    return M.build_string(sid, (), rng.integers(0, 2, 72))


def sequences(rng):
    seqs = []
    rnd = lambda: dict(t_k_raw=int(rng.integers(0, 4096)), t_b_raw=int(rng.integers(1, 96)), n_t=int(rng.integers(1, 1462)), n=int(rng.integers(1, 25)),
                       n_4=int(rng.integers(1, 12)), tau_c=int(rng.integers(-2 ** 31 + 1, 2 ** 31)), tau_gps=int(rng.integers(-2 ** 21 + 1, 2 ** 21)))
    # full frames in order, almanac strings included
    s = []
    for _ in range(2):
        s += frame(rng, **rnd()) + [almanac(rng, sid) for sid in range(6, 16)]
    s += [almanac(rng, sid) for sid in (6, 8, 10, 12, 14, 0)] * 3
    seqs.append(s)
    # a string missing from the chain, then the chain complete
    for missing in (1, 2, 3, 4):
        p = rnd()
        seqs.append(frame(rng, ids=tuple(i for i in (1, 2, 3, 4, 5) if i != missing), **p) + frame(rng, **p))
    # t_b == 0 twice; a t_b that changes, and one that does not
    p = dict(rnd(), t_b_raw=0)
    seqs.append(frame(rng, **p) + frame(rng, **p))
    p = rnd()
    seqs.append(frame(rng, **dict(p, t_b_raw=10)) + frame(rng, **dict(p, t_b_raw=11)) + frame(rng, **dict(p, t_b_raw=11)) + frame(rng, **dict(p, t_b_raw=10)))
    # N_T in all four year ranges, at their edges, 0 and beyond; N_4 at 0 and 31; t_k that rolls the date back
    for n_t in (0, 1, 366, 367, 731, 732, 1096, 1097, 1461, 1462, 2047):
        for n_4, t_k_raw in ((0, 0), (31, 4095), (6, 1 << 7), (7, 23 << 7 | 59 << 1 | 1)):
            seqs.append(frame(rng, **dict(rnd(), n_t=n_t, n_4=n_4, t_k_raw=t_k_raw)))
    # every single-bit error of a string with even parity over its information bits, and of one with odd; double-bit errors
    found = {}
    while len(found) < 2:
        ch = M.build_string(1, [((10, 12), 1234)], rng.integers(0, 2, 72))
        found.setdefault(sum(ch[:77]) % 2, ch)
    for ch in (found[0], found[1]):
        s = [ch]
        for i in range(85):
            e = list(ch)
            e[i] ^= 1
            s.append(e)
        for _ in range(150):
            e = list(ch)
            i, j = rng.choice(85, 2, replace=False)
            e[i] ^= 1
            e[j] ^= 1
            s.append(e)
        seqs.append(s)
    return seqs


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    R = build(sys.argv[1], sys.argv[2])
    rng = np.random.default_rng(20261)
    rows = []
    for k, seq in enumerate(sequences(rng)):
        h = R.ref_gnav_new()
        for ch in seq:
            text = "".join("1" if b else "0" for b in ch).encode()
            out = ctypes.create_string_buffer(85)
            flags, tow, wn, n = (ctypes.c_int32 * 6)(), ctypes.c_double(), ctypes.c_int32(), ctypes.c_double()
            ret = R.ref_gnav_decode(h, text, out, flags, ctypes.byref(tow), ctypes.byref(wn), ctypes.byref(n))
            rows.append((list(ch), k, ret, [int(c == ord("1")) for c in out.raw], list(flags), tow.value, wn.value, n.value))
        R.ref_gnav_delete(h)
    # direct calls: the five cases of glonass_gnav_ephemeris_test.cc, negative and large offsets, a leap addition across midnight
    direct = [(2004, 394, 48600 + 10800, 0, 0), (2016, 268, 7560 + 10800, 0, 0), (2016, 62, 7560 + 10800, 0, 0), (2019, 1366, 7560 + 10800, 0, 0),
              (2020, 62, 7560 + 10800, 0, 0), (2016, 1, 10, 0.25, -0.125), (2017, 366, 10800 + 86390, 0, 0), (2012, 182, 10800 + 86399, 0, 0),
              (2012, 183, 10800 - 1, 0, 0), (1992, 0, 0, 0, 0), (2100, 60, 50000, 0, 0), (2116, 1461, 100000, 0, 0)]
    facts = [(1307, 480600 + 13), (1915, 518400 + 17 + 7560), (1886, 259200 + 17 + 7560), (2072, 447120 + 18 + 7560), (2095, 259200 + 18 + 7560)]
    glot = []
    for yr, n_t, tod, tc, tg in direct:
        j = 1 if 1 <= n_t <= 366 else 2 if n_t <= 731 and n_t >= 367 else 3 if 732 <= n_t <= 1096 else 4 if 1097 <= n_t <= 1461 else 0
        CALENDAR_USED.append((yr - j + 1, n_t - 1, tod - 10800))
        wn, tow = ctypes.c_int32(), ctypes.c_double()
        R.ref_gnav_glot_to_gpst(yr, n_t, tod, tc, tg, ctypes.byref(wn), ctypes.byref(tow))
        glot.append((yr, n_t, tod, tc, tg, wn.value, tow.value))
    # The reference's test asserts `week - true_week < FLT_EPSILON` and `tow - true_tow < FLT_EPSILON`: one-sided.  Cases 2 and
    # 3 are calendar facts and come out exactly.  The expected values of cases 1, 4 and 5 are not what the reference computes
    # (case 1 expects a date a year later than d_yr - J + 1 and N_T give, 4 and 5 the weekday of case 3) and pass there only
    # because the assertions are one-sided: here they must hold in that form, and all five must equal plain day counting.
    assert [(g[5], g[6]) for g in glot[1:3]] == [(w, float(t)) for w, t in facts[1:3]], glot[:5]
    assert all(g[5] - w < 1e-7 and g[6] - t < 1e-7 for g, (w, t) in zip(glot, facts)), glot[:5]
    for (yr, n_t, tod, _, _), g in zip(direct, glot):
        j = 1 if 1 <= n_t <= 366 else 2 if 367 <= n_t <= 731 else 3 if 732 <= n_t <= 1096 else 4 if 1097 <= n_t <= 1461 else 0
        utc = datetime.datetime(yr - j + 1, 1, 1) + datetime.timedelta(days=n_t - 1, seconds=tod - 10800)
        leap = next(sec for when, sec in M.LEAP if utc >= when)
        gps = utc + datetime.timedelta(seconds=leap)
        total = (utc.date() - datetime.date(1980, 1, 6)).days * 86400 + gps.hour * 3600 + gps.minute * 60 + gps.second
        assert (g[5], g[6] - g[3] - g[4]) == (total // 604800, float(total % 604800)), (g, total)
    # the stand-in calendar against Python's, on every instant used and on the leap-second dates
    epoch = datetime.datetime(1980, 1, 6)
    for when, _ in M.LEAP:
        CALENDAR_USED.append((when.year, (when - datetime.datetime(when.year, 1, 1)).days, 0))
    for y, add, sec in CALENDAR_USED:
        day, second = ctypes.c_int64(), ctypes.c_int64()
        R.ref_gnav_calendar(y, add, sec, ctypes.byref(day), ctypes.byref(second))
        t = datetime.datetime(y, 1, 1) + datetime.timedelta(days=add, seconds=sec)
        assert (day.value, second.value) == ((t - epoch).days, t.hour * 3600 + t.minute * 60 + t.second), (y, add, sec, day.value, second.value)
    path = os.path.join(HERE, "gnav_ref.npz")
    np.savez_compressed(path, chars=np.array([r[0] for r in rows], np.uint8), seq=np.array([r[1] for r in rows], np.int32),
                        ret=np.array([r[2] for r in rows], np.int32), bits=np.array([r[3] for r in rows], np.uint8),
                        flags=np.array([r[4] for r in rows], np.uint8), tow=np.array([r[5] for r in rows], np.float64),
                        wn=np.array([r[6] for r in rows], np.int32), n=np.array([r[7] for r in rows], np.float64), glot=np.array(glot, np.float64))
    print(path, os.path.getsize(path), len(rows), "calls,", len(CALENDAR_USED), "calendar checks")


if __name__ == "__main__":
    main()
