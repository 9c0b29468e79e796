"""BeiDou B3I tracking (GNSSHIP_SYS_BDS_B3I: 3 taps on one 10230-chip replica, NH20 — a GEO satellite: the D2
preamble) on the device vs the oracle loop configured with the B3I constants (tests/b3i_l2c_scenarios.py).

Every comparison is test_gpu_trk.compare_exact's rule — every epoch-record field equal, NaN equal to NaN —
and every test asserts the engine that ran (gnsship_trk_last_engine):
  trk_fast.hip     the default for few channels; with ±1 codes the replica is held as sign bits
                   (code_bits.h) — the form that gives the throughput variant a plan at N = 12500 — and as
                   floats otherwise or with GNSSHIP_TRK_FAST_PACKED=0
  trk_lane.hip     GNSSHIP_TRK_LANE=1 (the default above one channel per compute unit)
  trk_persist.hip  GNSSHIP_TRK_FAST=0 with the AVX rotator (u_avx's chains on sixteen lanes for this system),
                   a non-±1 code in the throughput form, and the generic rotator's serial pipeline
The device configuration carries the library's default slope / spc / y_intercept: the engine derives the
values the block sets for B3I (1, early_late_space_chips, 1), which the oracle is given.
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
FS_A, EPOCHS_A = 12.5e6, 120
DERIVED = ("slope", "spc", "y_intercept")  # left at the library defaults: the engine sets them for B3I


def b3i_dev_conf(k):
    c = engine.beidou_b3i_trk_conf(k.fs_in)
    assert c.vector_length == k.vector_length and c.system == abi.SYS_BDS_B3I
    for f in SHARED:
        if f not in DERIVED:
            setattr(c, f, getattr(k, f))
    c.rotator = abi.ROTATOR_AVX if k.rotator_avx else abi.ROTATOR_GENERIC
    return c


@functools.lru_cache(maxsize=None)
def scenario(fs, epochs, avx=1, ext=1, prn=9):
    """(sat, k, x, stamp, first, delay, dop, oracle records): computed once, shared, never modified."""
    sat, k, x, stamp, first, delay, dop = B.b3i_sync(fs, epochs, prn=prn, rotator_avx=avx, extend_correlation_symbols=ext)
    ref = T.track(k, x, sat.code, delay, dop, stamp, first, epochs, buffer_first=first)
    x.setflags(write=False)
    ref.setflags(write=False)
    return sat, k, x, stamp, first, delay, dop, ref


def run_one(ctx, sc, sig=None, n_ch=2, ch=1, dump=False, code=None):
    sat, k, x, stamp, first, delay, dop, _ = sc
    trk = engine.DllPllVemlTracking(ctx, b3i_dev_conf(k), n_ch)
    ctx.set_code(80, sat.code if code is None else code)
    trk.start(ch, 80, delay, dop, stamp, first, prn=sat.prn)
    out = trk.run(x if sig is None else sig, first, len(sc[7]), dump=dump)
    eng = trk.last_engine()
    trk.close()
    return out, eng


def test_default_dispatch_fast_long_epoch_form(ctx):
    """12.5 Msps, N = 12500 ≥ the long-epoch threshold: trk_fast on the sign-bit replica, channel 0 left idle."""
    sc = scenario(FS_A, EPOCHS_A)
    assert sc[7]["state"][-1] == 4
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_FAST_LATENCY, abi.TRK_ENGINE_NAMES[eng]
    assert rounds == EPOCHS_A
    compare_exact(rec[:, 1], sc[7], "B3I 12.5 Msps trk_fast")
    assert not np.any(rec[:, 0]["flags"])


def test_fast_latency_wave_count(ctx):
    """8.184 Msps, N = 8184 < 10000: trk_fast with the latency form's wave count."""
    sc = scenario(8.184e6, EPOCHS_A)
    assert sc[1].vector_length == 8184 and sc[7]["state"][-1] == 4
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_FAST_LATENCY, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], sc[7], "B3I 8.184 Msps trk_fast")


def test_fast_throughput_form(ctx, monkeypatch):
    """GNSSHIP_TRK_THRU=1 without trk_lane: trk_fast's throughput form (72 KiB of LDS), which has a plan at
    N = 12500 only because the replica is held as sign bits (a float replica leaves it one product group)."""
    monkeypatch.setenv("GNSSHIP_TRK_THRU", "1")
    monkeypatch.setenv("GNSSHIP_TRK_LANE", "0")
    sc = scenario(FS_A, EPOCHS_A)
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_FAST_THROUGHPUT, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], sc[7], "B3I trk_fast throughput")
    assert not np.any(rec[:, 0]["flags"])


def test_fast_float_replica(ctx, monkeypatch):
    """GNSSHIP_TRK_FAST_PACKED=0: trk_fast on the float replica (the A/B knob of the two new systems)."""
    monkeypatch.setenv("GNSSHIP_TRK_FAST_PACKED", "0")
    sc = scenario(FS_A, EPOCHS_A)
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_FAST_LATENCY, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], sc[7], "B3I trk_fast float replica")


def test_lanes(ctx, monkeypatch):
    """trk_lane (one 16-lane row per channel, sign-bit replicas), two channels, one left idle."""
    monkeypatch.setenv("GNSSHIP_TRK_LANE", "1")
    sc = scenario(FS_A, EPOCHS_A)
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_LANES, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], sc[7], "B3I trk_lane")
    assert not np.any(rec[:, 0]["flags"])


def test_persist_avx(ctx, monkeypatch):
    """GNSSHIP_TRK_FAST=0: trk_persist.hip with the AVX rotator, which for B3I runs u_avx's sixteen chains on
    sixteen lanes with serial sums (chains_avx), as every AVX layout of trk_persist now does."""
    monkeypatch.setenv("GNSSHIP_TRK_FAST", "0")
    sc = scenario(FS_A, EPOCHS_A)
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_PERSIST, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], sc[7], "B3I trk_persist avx")


def test_persist_generic_rotator(ctx):
    """The generic rotator: trk_persist.hip's serial pipeline (serial_rotator.h)."""
    sc = scenario(FS_A, EPOCHS_A, avx=0)
    assert sc[7]["state"][-1] == 4
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_PERSIST, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], sc[7], "B3I trk_persist generic")


@pytest.mark.parametrize("thru", [0, 1])
def test_code_that_is_not_binary(ctx, monkeypatch, thru):
    """A code with one chip set to 0.5 cannot be held as sign bits: the latency form runs trk_fast on the float
    replica; the throughput form has no plan with it (and trk_lane needs ±1 codes), so the run falls to
    trk_persist.  Both equal the oracle given the same code."""
    if thru:
        monkeypatch.setenv("GNSSHIP_TRK_THRU", "1")
    sat, k, x, stamp, first, delay, dop, _ = scenario(FS_A, EPOCHS_A)
    code = sat.code.copy()
    code[4321] = 0.5
    ref = T.track(k, x, code, delay, dop, stamp, first, EPOCHS_A, buffer_first=first)
    assert ref["state"][-1] == 4
    (rec, rounds), eng = run_one(ctx, (sat, k, x, stamp, first, delay, dop, ref), code=code)
    want = abi.TRK_ENGINE_PERSIST if thru else abi.TRK_ENGINE_FAST_LATENCY
    assert eng == want, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], ref, f"B3I non-binary code thru={thru}")


@pytest.mark.parametrize("quant", ["ci16", "ci8"])
def test_quantised_input_formats(ctx, quant):
    """Shape A with CI16 / CI8 input: the oracle gets the same quantised samples as floats."""
    sat, k, x, stamp, first, delay, dop, _ = scenario(FS_A, EPOCHS_A)
    raw = signals.to_ishort(x) if quant == "ci16" else signals.to_ibyte(x)
    xq = raw.astype(np.float32).view(np.complex64)
    ref = T.track(k, xq, sat.code, delay, dop, stamp, first, EPOCHS_A, buffer_first=first)
    assert ref["state"][-1] == 4
    (rec, rounds), eng = run_one(ctx, (sat, k, x, stamp, first, delay, dop, ref), sig=raw)
    assert eng == abi.TRK_ENGINE_FAST_LATENCY, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], ref, f"B3I {quant}")


def test_extended_integration(ctx):
    """extend_correlation_symbols = 5 on shape A: state-3 coherent epochs between narrow updates."""
    sc = scenario(FS_A, 160, ext=5)
    st = sc[7]["state"]
    assert np.sum(st == 3) >= 3 * 4 and np.sum(st == 4) >= 3
    (rec, rounds), eng = run_one(ctx, sc, n_ch=1, ch=0)
    assert eng == abi.TRK_ENGINE_FAST_LATENCY, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 0], sc[7], "B3I x5")


def test_dump_records_equal_the_oracle(ctx):
    """log_data's records for shape A: written on the same epochs, every field equal."""
    sat, k, x, stamp, first, delay, dop, _ = scenario(FS_A, EPOCHS_A)
    ref, rdump = T.track(k, x, sat.code, delay, dop, stamp, first, EPOCHS_A, buffer_first=first, dump=True, prn=sat.prn)
    (rec, rounds, dump), eng = run_one(ctx, (sat, k, x, stamp, first, delay, dop, ref), n_ch=1, ch=0, dump=True)
    assert eng == abi.TRK_ENGINE_FAST_LATENCY, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 0], ref, "B3I dump run")
    ran = (rec[:, 0]["flags"] & 8) != 0
    d_rec, d_dump = rec[ran, 0], dump[ran, 0]
    assert np.array_equal(d_rec["flags"] & 16, ref["flags"] & 16)
    w = (ref["flags"] & 16) != 0
    a, b = d_dump[w], rdump[w]
    assert len(a) > 20
    for f in abi.TRK_DUMP_DTYPE.names:
        same = (a[f] == b[f]) | (np.isnan(a[f]) & np.isnan(b[f])) if a[f].dtype.kind == "f" else a[f] == b[f]
        assert np.all(same), (f, int(np.count_nonzero(~same)), a[f][~same][:3], b[f][~same][:3])


@pytest.mark.parametrize("ext", [1, 5])
def test_geo_beside_meo(ctx, ext):
    """GEO PRN 3 (start's prn: the D2 preamble at 2 symbols per bit, no NH, extend capped at 2) next to a MEO
    channel (PRN 9) of the same engine, which keeps the NH20 profile and the configured extend."""
    fs, epochs = FS_A, 160
    geo, kg, xg, stamp, first, delay_g, dop_g = B.b3i_sync(fs, epochs, prn=3, rotator_avx=1, extend_correlation_symbols=ext)
    meo, km, xm, _, _, delay_m, dop_m = B.b3i_sync(fs, epochs, prn=9, dop=-830.0, delay_chips=1500.6, seed=6, rotator_avx=1,
                                                   extend_correlation_symbols=ext)
    assert kg.extend_correlation_symbols == min(ext, 2) and km.extend_correlation_symbols == ext
    trk = engine.DllPllVemlTracking(ctx, b3i_dev_conf(km), 2)  # the MEO configuration: GEO settings come from the PRN
    ctx.set_code(60, geo.code)
    ctx.set_code(61, meo.code)
    both = (xg + xm).astype(np.complex64)
    trk.start(0, 60, delay_g, dop_g, stamp, first, prn=3)
    trk.start(1, 61, delay_m, dop_m, stamp, first, prn=9)
    rec, rounds = trk.run(both, first, epochs)
    assert trk.last_engine() == abi.TRK_ENGINE_FAST_LATENCY
    trk.close()
    ref_g = T.track(kg, both, geo.code, delay_g, dop_g, stamp, first, epochs, buffer_first=first)
    ref_m = T.track(km, both, meo.code, delay_m, dop_m, stamp, first, epochs, buffer_first=first)
    assert ref_g["state"][-1] in (3, 4) and ref_m["state"][-1] in (3, 4)
    assert np.any(ref_g["state"] == 4) and np.any(ref_m["state"] == 4)
    compare_exact(rec[:, 0], ref_g, f"B3I geo x{ext}")
    compare_exact(rec[:, 1], ref_m, f"B3I meo x{ext}")


def test_four_channels_in_one_buffer(ctx):
    """Mixed load: four B3I satellites of different PRN, Doppler and delay in one buffer, started together."""
    fs, epochs = FS_A, 60
    k = B.b3i_conf(fs, rotator_avx=1)
    sats = [B.b3i_satellite(prn=p, dop=d, delay_chips=c, cn0=48.0, phase=ph)
            for p, d, c, ph in ((12, -2310.0, 9911.7, 0.3), (24, 640.5, 17.2, 2.1), (37, 3875.0, 5120.4, 4.0), (51, -95.0, 7000.9, 5.5))]
    first = int(fs)
    x = signals.generate_if(fs, k.vector_length * (epochs + 5), sats, seed=21, start=first)
    trk = engine.DllPllVemlTracking(ctx, b3i_dev_conf(k), len(sats))
    starts = []
    for ch, s in enumerate(sats):
        ctx.set_code(90 + ch, s.code)
        starts.append((ch, 90 + ch, B.acq_delay_for(s, fs, 0, first, B.B3I_PERIOD_S) + 0.3 - 0.2 * ch, s.doppler_hz - 20.0 + 10.0 * ch, 0, first,
                       -1, s.prn))
    trk.start_many(starts)
    rec, rounds = trk.run(x, first, epochs)
    assert trk.last_engine() == abi.TRK_ENGINE_FAST_LATENCY
    trk.close()
    for ch, s in enumerate(sats):
        ref = T.track(k, x, s.code, starts[ch][2], starts[ch][3], 0, first, epochs, buffer_first=first)
        assert len(ref) >= epochs - 2
        compare_exact(rec[:, ch], ref, f"B3I ch{ch} PRN {s.prn}")


def test_b1i_and_b3i_trackers_on_one_context(ctx):
    """A B1I tracker and a B3I tracker on one context, run alternately: B3I's LDS plans and kernels (the sign-bit
    single-replica form beside B1I's float one of the same tap layout) leave B1I alone."""
    b3 = scenario(FS_A, EPOCHS_A)
    sat1, k1, x1, stamp1, first1, delay1, dop1 = S.sync("BDS", 4.092e6, 80, rotator_avx=1)
    ref1 = T.track(k1, x1, sat1.code, delay1, dop1, stamp1, first1, 80, buffer_first=first1)
    t1 = engine.DllPllVemlTracking(ctx, dev_conf(k1, "BDS"), 1)
    t3 = engine.DllPllVemlTracking(ctx, b3i_dev_conf(b3[1]), 1)
    ctx.set_code(60, sat1.code)
    ctx.set_code(80, b3[0].code)
    t3.start(0, 80, b3[5], b3[6], b3[3], b3[4], prn=b3[0].prn)
    t1.start(0, 60, delay1, dop1, stamp1, first1, prn=sat1.prn)
    half = EPOCHS_A // 2
    rec3a, _ = t3.run(b3[2], b3[4], half)
    rec1a, _ = t1.run(x1, first1, 40)
    rec3b, _ = t3.run(b3[2], b3[4], EPOCHS_A - half)
    rec1b, _ = t1.run(x1, first1, 40)
    assert t1.last_engine() == abi.TRK_ENGINE_FAST_LATENCY and t3.last_engine() == abi.TRK_ENGINE_FAST_LATENCY
    t1.close()
    t3.close()
    compare_exact(np.concatenate([rec1a[:, 0], rec1b[:, 0]]), ref1, "B1I beside B3I")
    compare_exact(np.concatenate([rec3a[:, 0], rec3b[:, 0]]), b3[7], "B3I beside B1I")
