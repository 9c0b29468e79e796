"""GPS L2C tracking (GNSSHIP_SYS_GPS_L2C: 3 taps on the 10230-chip L2 CM replica, one 20 ms code period per
epoch and per telemetry symbol, no secondary code) on the device vs the oracle loop configured with the L2C
constants (tests/b3i_l2c_scenarios.py), at the reference's L2C loop bandwidths (pll 2 Hz, dll 0.25 Hz).

Every comparison is test_gpu_trk.compare_exact's rule — every epoch-record field equal, NaN equal to NaN —
and every test asserts the engine that ran.  N = 25000 (1.25 Msps) is a 196-task epoch of 49 product groups,
N = 40000 (2 Msps) a 313-task one of 79: trk_fast's latency form holds the whole epoch's phasor slots and a
product ring of 9 and 8 groups.
"""
import functools

import numpy as np
import pytest

from gnss_sim_receiver_amd import abi, engine, signals
from oracle import trk as T

import b3i_l2c_scenarios as B
import trk_scenarios as S
from test_gpu_trk import SHARED, compare_exact, dev_conf

pytestmark = pytest.mark.gpu
FS_A, FS_B, EPOCHS = 1.25e6, 2e6, 60
DERIVED = ("slope", "spc", "y_intercept")  # left at the library defaults: the engine sets them for L2C


def l2c_dev_conf(k, **forced):
    c = engine.gps_l2c_trk_conf(k.fs_in)
    assert c.vector_length == k.vector_length and c.system == abi.SYS_GPS_L2C
    assert c.extend_correlation_symbols == 1 and c.track_pilot == 0
    for f in SHARED:
        if f not in DERIVED:
            setattr(c, f, getattr(k, f))
    c.rotator = abi.ROTATOR_AVX if k.rotator_avx else abi.ROTATOR_GENERIC
    for f, v in forced.items():
        setattr(c, f, v)
    return c


@functools.lru_cache(maxsize=None)
def scenario(fs, avx=1):
    """(sat, k, x, stamp, first, delay, dop, oracle records): computed once, shared, never modified."""
    sat, k, x, stamp, first, delay, dop = B.l2c_sync(fs, EPOCHS, rotator_avx=avx)
    ref = T.track(k, x, sat.code, delay, dop, stamp, first, EPOCHS, buffer_first=first)
    assert len(ref) == EPOCHS and np.all(ref["state"][1:] == 4)
    x.setflags(write=False)
    ref.setflags(write=False)
    return sat, k, x, stamp, first, delay, dop, ref


def run_one(ctx, sc, sig=None, n_ch=2, ch=1, dump=False, **forced):
    sat, k, x, stamp, first, delay, dop, _ = sc
    trk = engine.DllPllVemlTracking(ctx, l2c_dev_conf(k, **forced), n_ch)
    ctx.set_code(80, sat.code)
    trk.start(ch, 80, delay, dop, stamp, first, prn=sat.prn)
    out = trk.run(x if sig is None else sig, first, len(sc[7]), dump=dump)
    eng = trk.last_engine()
    trk.close()
    return out, eng


@pytest.mark.parametrize("fs", [FS_A, FS_B])
def test_default_dispatch(ctx, fs):
    """trk_fast's long-epoch form on the sign-bit replica, channel 0 left idle; N = 25000 and N = 40000."""
    sc = scenario(fs)
    assert sc[1].vector_length == int(fs) // 50
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_FAST_LATENCY, abi.TRK_ENGINE_NAMES[eng]
    assert rounds == EPOCHS
    compare_exact(rec[:, 1], sc[7], f"L2C {fs / 1e6} Msps trk_fast")
    assert not np.any(rec[:, 0]["flags"])


@pytest.mark.parametrize("fs", [FS_A, FS_B])
def test_lanes(ctx, monkeypatch, fs):
    monkeypatch.setenv("GNSSHIP_TRK_LANE", "1")
    sc = scenario(fs)
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_LANES, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], sc[7], f"L2C {fs / 1e6} Msps trk_lane")
    assert not np.any(rec[:, 0]["flags"])


def test_persist_avx(ctx, monkeypatch):
    """GNSSHIP_TRK_FAST=0: trk_persist.hip's sixteen-chain AVX form (chains_avx)."""
    monkeypatch.setenv("GNSSHIP_TRK_FAST", "0")
    sc = scenario(FS_A)
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_PERSIST, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], sc[7], "L2C trk_persist avx")


def test_persist_generic_rotator(ctx):
    sc = scenario(FS_A, avx=0)
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_PERSIST, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], sc[7], "L2C trk_persist generic")


def test_extension_and_pilot_settings_are_forced(ctx):
    """extend_correlation_symbols = 4 and track_pilot = 1 in the device configuration give the records of 1 / 0:
    the block forces track_pilot off for 2S and the adapter forces one symbol."""
    sc = scenario(FS_A)
    (rec, rounds), eng = run_one(ctx, sc, n_ch=1, ch=0, extend_correlation_symbols=4, track_pilot=1)
    assert eng == abi.TRK_ENGINE_FAST_LATENCY, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 0], sc[7], "L2C forced settings")


def test_ci8_input(ctx):
    sat, k, x, stamp, first, delay, dop, _ = scenario(FS_A)
    raw = signals.to_ibyte(x)
    xq = raw.astype(np.float32).view(np.complex64)
    ref = T.track(k, xq, sat.code, delay, dop, stamp, first, EPOCHS, buffer_first=first)
    assert ref["state"][-1] == 4
    (rec, rounds), eng = run_one(ctx, (sat, k, x, stamp, first, delay, dop, ref), sig=raw)
    assert eng == abi.TRK_ENGINE_FAST_LATENCY, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], ref, "L2C ci8")


def test_dump_records_equal_the_oracle(ctx):
    sat, k, x, stamp, first, delay, dop, _ = scenario(FS_A)
    ref, rdump = T.track(k, x, sat.code, delay, dop, stamp, first, EPOCHS, buffer_first=first, dump=True, prn=sat.prn)
    (rec, rounds, dump), eng = run_one(ctx, (sat, k, x, stamp, first, delay, dop, ref), n_ch=1, ch=0, dump=True)
    assert eng == abi.TRK_ENGINE_FAST_LATENCY, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 0], ref, "L2C dump run")
    ran = (rec[:, 0]["flags"] & 8) != 0
    d_rec, d_dump = rec[ran, 0], dump[ran, 0]
    assert np.array_equal(d_rec["flags"] & 16, ref["flags"] & 16)
    w = (ref["flags"] & 16) != 0
    a, b = d_dump[w], rdump[w]
    assert len(a) > 20
    for f in abi.TRK_DUMP_DTYPE.names:
        same = (a[f] == b[f]) | (np.isnan(a[f]) & np.isnan(b[f])) if a[f].dtype.kind == "f" else a[f] == b[f]
        assert np.all(same), (f, int(np.count_nonzero(~same)), a[f][~same][:3], b[f][~same][:3])


def test_l1_and_l2c_trackers_on_one_context(ctx):
    """A GPS L1 tracker and an L2C tracker on one context over their own buffers, run alternately: L2C's kernels
    and LDS plans (the sign-bit single-replica form of L1's tap layout) leave L1 alone."""
    l2 = scenario(FS_A)
    sat1, k1, x1, stamp1, first1, delay1, dop1 = S.sync("GPS", 4e6, 60, rotator_avx=1)
    ref1 = T.track(k1, x1, sat1.code, delay1, dop1, stamp1, first1, 60, buffer_first=first1)
    t1 = engine.DllPllVemlTracking(ctx, dev_conf(k1, "GPS"), 1)
    t2 = engine.DllPllVemlTracking(ctx, l2c_dev_conf(l2[1]), 1)
    ctx.set_code(60, sat1.code)
    ctx.set_code(80, l2[0].code)
    t2.start(0, 80, l2[5], l2[6], l2[3], l2[4], prn=l2[0].prn)
    t1.start(0, 60, delay1, dop1, stamp1, first1)
    half = EPOCHS // 2
    rec2a, _ = t2.run(l2[2], l2[4], half)
    rec1, _ = t1.run(x1, first1, 60)
    rec2b, _ = t2.run(l2[2], l2[4], EPOCHS - half)
    assert t1.last_engine() == abi.TRK_ENGINE_FAST_LATENCY and t2.last_engine() == abi.TRK_ENGINE_FAST_LATENCY
    t1.close()
    t2.close()
    compare_exact(rec1[:, 0], ref1, "GPS L1 beside L2C")
    compare_exact(np.concatenate([rec2a[:, 0], rec2b[:, 0]]), l2[7], "L2C beside GPS L1")
