"""GPS L5 pilot tracking (GNSSHIP_SYS_GPS_L5: 3 taps on L5Q + the L5I data prompt) on the device vs the
oracle loop configured with the L5 signal constants (tests/l5_scenarios.py).

Every comparison is test_gpu_trk.compare_exact's rule — every epoch-record field equal, NaN equal to
NaN — and every test asserts the engine that ran (gnsship_trk_last_engine):
  trk_fast.hip   the default for few channels; the two 10230-chip replicas are held as sign bits
                 (code_bits.h), N = 12500 runs its long-epoch form, N = 8184 the latency wave count
  trk_lane.hip   GNSSHIP_TRK_LANE=1 (the default above one channel per compute unit)
  trk_persist.hip  GNSSHIP_TRK_FAST=0 with the AVX rotator (u_avx's chains on sixteen lanes for this layout), and the
                 generic rotator's serial pipeline
The device configuration carries the library's default slope / spc / y_intercept: the engine derives
the values the block sets for L5 (1, early_late_space_chips, 1), which the oracle is given.
"""
import functools

import numpy as np
import pytest

from gnss_sim_receiver_amd import abi, engine, signals
from oracle import trk as T

import l5_scenarios as L5
import trk_scenarios as S
from test_gpu_trk import SHARED, compare_exact, dev_conf

pytestmark = pytest.mark.gpu
FS_A, EPOCHS_A = 12.5e6, 120
DERIVED = ("slope", "spc", "y_intercept")  # left at the library defaults: the engine sets them for L5


def l5_dev_conf(k):
    c = engine.gps_l5_trk_conf(k.fs_in)
    assert c.vector_length == k.vector_length and c.system == abi.SYS_GPS_L5
    for f in SHARED:
        if f not in DERIVED:
            setattr(c, f, getattr(k, f))
    c.rotator = abi.ROTATOR_AVX if k.rotator_avx else abi.ROTATOR_GENERIC
    return c


@functools.lru_cache(maxsize=None)
def scenario(fs, epochs, avx=1, ext=1):
    """(sat, k, x, stamp, first, delay, dop, oracle records): computed once, shared, never modified."""
    sat, k, x, stamp, first, delay, dop = L5.sync(fs, epochs, rotator_avx=avx, extend_correlation_symbols=ext)
    ref = T.track(k, x, sat.code, delay, dop, stamp, first, epochs, data_code=sat.code_data, buffer_first=first)
    x.setflags(write=False)
    ref.setflags(write=False)
    return sat, k, x, stamp, first, delay, dop, ref


def run_one(ctx, sc, sig=None, n_ch=2, ch=1, dump=False):
    sat, k, x, stamp, first, delay, dop, _ = sc
    trk = engine.DllPllVemlTracking(ctx, l5_dev_conf(k), n_ch)
    ctx.set_code(80, sat.code)
    ctx.set_code(81, sat.code_data)
    trk.start(ch, 80, delay, dop, stamp, first, data_code_id=81, prn=sat.prn)
    out = trk.run(x if sig is None else sig, first, len(sc[7]), dump=dump)
    eng = trk.last_engine()
    trk.close()
    return out, eng


def test_sync_to_state_4_fast_long_epoch_form(ctx):
    """(a) 12.5 Msps, N = 12500 ≥ the long-epoch threshold: trk_fast, channel 0 left idle."""
    sc = scenario(FS_A, EPOCHS_A)
    assert sc[7]["state"][-1] == 4
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_FAST_LATENCY, abi.TRK_ENGINE_NAMES[eng]
    assert rounds == EPOCHS_A
    compare_exact(rec[:, 1], sc[7], "L5 12.5 Msps trk_fast")
    assert not np.any(rec[:, 0]["flags"])


def test_sync_to_state_4_fast_latency_wave_count(ctx):
    """(b) 8.184 Msps, N = 8184 < 10000: trk_fast with the latency form's wave count (the oracle reaches
    state 4 at this rate: tests/test_oracle_trk_l5.py)."""
    sc = scenario(8.184e6, EPOCHS_A)
    assert sc[1].vector_length == 8184 and sc[7]["state"][-1] == 4
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_FAST_LATENCY, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], sc[7], "L5 8.184 Msps trk_fast")


def test_sync_to_state_4_lanes(ctx, monkeypatch):
    """(c) trk_lane (one 16-lane row per channel, sign-bit replicas), two channels, one left idle."""
    monkeypatch.setenv("GNSSHIP_TRK_LANE", "1")
    sc = scenario(FS_A, EPOCHS_A)
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_LANES, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], sc[7], "L5 trk_lane")
    assert not np.any(rec[:, 0]["flags"])


def test_sync_to_state_4_persist_avx(ctx, monkeypatch):
    """(d) GNSSHIP_TRK_FAST=0: trk_persist.hip with the AVX rotator.  For this tap layout its AVX form runs
    u_avx's sixteen chains on sixteen lanes with serial sums (chains_avx), not the task tree it once ran
    (which differed from the oracle by one ulp of the prompt in 42 of these 120 epochs; the tree is gone
    for every layout since)."""
    monkeypatch.setenv("GNSSHIP_TRK_FAST", "0")
    sc = scenario(FS_A, EPOCHS_A)
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_PERSIST, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], sc[7], "L5 trk_persist avx")


def test_sync_to_state_4_persist_generic_rotator(ctx):
    """(e) the generic rotator: trk_persist.hip's serial pipeline (serial_rotator.h)."""
    sc = scenario(FS_A, EPOCHS_A, avx=0)
    assert sc[7]["state"][-1] == 4
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_PERSIST, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], sc[7], "L5 trk_persist generic")


@pytest.mark.parametrize("quant", ["ci16", "ci8"])
def test_quantised_input_formats(ctx, quant):
    """Shape (a) with CI16 / CI8 input: the oracle gets the same quantised samples as floats."""
    sat, k, x, stamp, first, delay, dop, _ = scenario(FS_A, EPOCHS_A)
    raw = signals.to_ishort(x) if quant == "ci16" else signals.to_ibyte(x)
    xq = raw.astype(np.float32).view(np.complex64)
    ref = T.track(k, xq, sat.code, delay, dop, stamp, first, EPOCHS_A, data_code=sat.code_data, buffer_first=first)
    assert ref["state"][-1] == 4
    (rec, rounds), eng = run_one(ctx, (sat, k, x, stamp, first, delay, dop, ref), sig=raw)
    assert eng == abi.TRK_ENGINE_FAST_LATENCY, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], ref, f"L5 {quant}")


def test_extended_integration(ctx):
    """extend_correlation_symbols = 5 on shape (a): state-3 coherent epochs between narrow updates."""
    sc = scenario(FS_A, 160, ext=5)
    st = sc[7]["state"]
    assert np.sum(st == 3) >= 3 * 4 and np.sum(st == 4) >= 3
    (rec, rounds), eng = run_one(ctx, sc, n_ch=1, ch=0)
    assert eng == abi.TRK_ENGINE_FAST_LATENCY, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 0], sc[7], "L5 x5")


def test_dump_records_equal_the_oracle(ctx):
    """log_data's records for shape (a): written on the same epochs, every field equal."""
    sat, k, x, stamp, first, delay, dop, _ = scenario(FS_A, EPOCHS_A)
    ref, rdump = T.track(k, x, sat.code, delay, dop, stamp, first, EPOCHS_A, data_code=sat.code_data, buffer_first=first, dump=True,
                         prn=sat.prn)
    (rec, rounds, dump), eng = run_one(ctx, (sat, k, x, stamp, first, delay, dop, ref), n_ch=1, ch=0, dump=True)
    assert eng == abi.TRK_ENGINE_FAST_LATENCY, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 0], ref, "L5 dump run")
    ran = (rec[:, 0]["flags"] & 8) != 0
    d_rec, d_dump = rec[ran, 0], dump[ran, 0]
    assert np.array_equal(d_rec["flags"] & 16, ref["flags"] & 16)
    w = (ref["flags"] & 16) != 0
    a, b = d_dump[w], rdump[w]
    assert len(a) > 20
    for f in abi.TRK_DUMP_DTYPE.names:
        same = (a[f] == b[f]) | (np.isnan(a[f]) & np.isnan(b[f])) if a[f].dtype.kind == "f" else a[f] == b[f]
        assert np.all(same), (f, int(np.count_nonzero(~same)), a[f][~same][:3], b[f][~same][:3])


def test_four_channels_in_one_buffer(ctx):
    """Mixed load: four L5 satellites of different PRN, Doppler and delay in one buffer, one tracker."""
    fs, epochs = FS_A, 60
    k = L5.conf(fs, rotator_avx=1)
    sats = [L5.satellite(prn=p, dop=d, delay_chips=c, cn0=48.0, phase=ph)
            for p, d, c, ph in ((2, -2310.0, 9911.7, 0.3), (14, 640.5, 17.2, 2.1), (25, 3875.0, 5120.4, 4.0), (31, -95.0, 7000.9, 5.5))]
    first = int(fs)
    x = signals.generate_if(fs, k.vector_length * (epochs + 5), sats, seed=21, start=first)
    trk = engine.DllPllVemlTracking(ctx, l5_dev_conf(k), len(sats))
    starts = []
    for ch, s in enumerate(sats):
        ctx.set_code(90 + 2 * ch, s.code)
        ctx.set_code(91 + 2 * ch, s.code_data)
        starts.append((ch, 90 + 2 * ch, L5.acq_delay_for(s, fs, 0, first) + 0.3 - 0.2 * ch, s.doppler_hz - 20.0 + 10.0 * ch, 0, first,
                       91 + 2 * ch, s.prn))
    trk.start_many(starts)
    rec, rounds = trk.run(x, first, epochs)
    assert trk.last_engine() == abi.TRK_ENGINE_FAST_LATENCY
    trk.close()
    for ch, s in enumerate(sats):
        ref = T.track(k, x, s.code, starts[ch][2], starts[ch][3], 0, first, epochs, data_code=s.code_data, buffer_first=first)
        assert len(ref) >= epochs - 2
        compare_exact(rec[:, ch], ref, f"L5 ch{ch} PRN {s.prn}")


def test_data_only_tracking_is_rejected(ctx):
    """track_pilot = 0 on L5 is the reference's interchange_iq path, which the engine does not restate."""
    c = engine.gps_l5_trk_conf(FS_A, track_pilot=0)
    with pytest.raises(abi.GnssHipError) as e:
        engine.DllPllVemlTracking(ctx, c, 1)
    assert e.value.code == abi.E_INVAL
    assert "track_pilot = 0" in str(e.value) and "interchange_iq" in str(e.value)


def test_l1_and_l5_trackers_on_one_context(ctx):
    """A GPS L1 tracker and an L5 tracker on one context, run alternately: the L5 LDS plans (sign-bit
    replicas, a larger dynamic LDS size on the shared kernels' attributes) leave the L1 ones alone."""
    l5 = scenario(FS_A, EPOCHS_A)
    sat1, k1, x1, stamp1, first1, delay1, dop1 = S.sync("GPS", 4e6, 60, rotator_avx=1)
    ref1 = T.track(k1, x1, sat1.code, delay1, dop1, stamp1, first1, 60, buffer_first=first1)
    t1 = engine.DllPllVemlTracking(ctx, dev_conf(k1, "GPS"), 1)
    t5 = engine.DllPllVemlTracking(ctx, l5_dev_conf(l5[1]), 1)
    ctx.set_code(60, sat1.code)
    ctx.set_code(80, l5[0].code)
    ctx.set_code(81, l5[0].code_data)
    t5.start(0, 80, l5[5], l5[6], l5[3], l5[4], data_code_id=81)
    t1.start(0, 60, delay1, dop1, stamp1, first1)
    half = EPOCHS_A // 2
    rec5a, _ = t5.run(l5[2], l5[4], half)
    rec1, _ = t1.run(x1, first1, 60)
    rec5b, _ = t5.run(l5[2], l5[4], EPOCHS_A - half)
    assert t1.last_engine() == abi.TRK_ENGINE_FAST_LATENCY and t5.last_engine() == abi.TRK_ENGINE_FAST_LATENCY
    t1.close()
    t5.close()
    compare_exact(rec1[:, 0], ref1, "GPS L1 beside L5")
    compare_exact(np.concatenate([rec5a[:, 0], rec5b[:, 0]]), l5[7], "L5 beside GPS L1")
