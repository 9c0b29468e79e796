"""trk_fast.hip's steady regime against the oracle loop, bit for bit.

In state 4 with both discriminators taken from the accumulator waves (no secondary code, no extended
integration, the run's tap spacing), the pull-in over and no FLL, the control wave seeds the next epoch
before it runs epoch_pre, and the lock wave forms the prompt from the stored taps itself.  The flag is
decided per epoch when it is seeded, so these runs cross every edge of the regime: entering it from
state 2, a lost lock inside it (the cancelled epoch, the lock wave's skip) and a restart of the same
channel, launches that begin and end inside it, configurations that never enter it (FLL, a secondary
code), and the dump records written after the deferred epoch_pre.

One or two channels of GPS L1 C/A at 4 Msps (N = 4000), AVX rotator: the smallest shape that reaches
state 4 and runs on trk_fast's latency form.  Every record field is compared for equality
(test_gpu_trk.compare_exact), traced taps too (test_gpu_c5_closed_loop.trace_exact).

The records do not say which order an epoch took.  That the GPS runs here take the steady one rests on
the kernel's conditions and the scenarios: trk_scenarios.sync sets pull_in_time_s = 0 (the pull-in ends in
the first epoch), GPS L1 C/A has no secondary code and runs with extend 1, so every state-4 epoch the
oracle counts (asserted below) is seeded steady unless the FLL is on.
"""
import functools

import numpy as np
import pytest

from gnss_sim_receiver_amd import abi, engine, signals
from oracle import trk as T

import trk_scenarios as S
from test_gpu_c5_closed_loop import trace_exact
from test_gpu_trk import compare_exact, dev_conf

pytestmark = pytest.mark.gpu
FS = 4e6
EPOCHS = 700


@functools.lru_cache(maxsize=None)
def gps_700():
    """The 700-epoch synchronisation scenario and the oracle's single run of it (shared, read only)."""
    sat, k, x, stamp, first, delay, dop = S.sync("GPS", FS, EPOCHS, rotator_avx=1)
    ref = T.track(k, x, sat.code, delay, dop, stamp, first, EPOCHS, buffer_first=first)
    x.setflags(write=False)
    ref.setflags(write=False)
    return sat, k, x, stamp, first, delay, dop, ref


def test_entering_the_regime(ctx):
    """States 2 → 4 inside the run: the first steady epoch follows the last hand-off epoch."""
    sat, k, x, stamp, first, delay, dop, ref = gps_700()
    assert np.sum(ref["state"] == 4) >= 300 and ref["state"][0] == 2
    trk = engine.DllPllVemlTracking(ctx, dev_conf(k, "GPS"), 2)
    ctx.set_code(20, sat.code)
    trk.start(1, 20, delay, dop, stamp, first)  # channel 0 left idle
    trk.set_trace(True)
    rec, rounds = trk.run(x, first, EPOCHS)
    tr = trk.trace(EPOCHS)[:, 1]
    assert trk.last_engine() == abi.TRK_ENGINE_FAST_LATENCY
    trk.close()
    assert rounds == EPOCHS
    compare_exact(rec[:, 1], ref, "entering")
    assert trace_exact(tr, x, first, sat.code, None, "entering") == EPOCHS
    assert not np.any(rec[:, 0]["flags"])


def test_loss_of_lock_inside_the_regime_and_restart(ctx):
    """Signal for 0.3 s, then noise (test_gpu_trk.test_loss_of_lock_matches_oracle's scenario) on the AVX
    engine: the lock is lost in state 4, after the next epoch was seeded — that epoch is cancelled and
    the lock detectors must not see it.  The same channel, started again, then tracks a second segment
    in a second launch exactly as a fresh oracle run does."""
    kw = dict(cn0=45.0, cn0_smoother_alpha=0.02, cn0_min=35, rotator_avx=1)
    sat, k, x, stamp, first, delay, dop = S.sync("GPS", FS, 1200, **kw)
    cut = int(0.3 * FS)
    noise = signals.generate_if(FS, len(x) - cut, [], seed=99, start=first + cut)
    x = np.concatenate([x[:cut], noise])
    ctx.set_code(5, sat.code)
    trk = engine.DllPllVemlTracking(ctx, dev_conf(k, "GPS"), 1)
    trk.start(0, 5, delay, dop, stamp, first)
    rec, rounds = trk.run(x, first, 1200)
    assert trk.last_engine() == abi.TRK_ENGINE_FAST_LATENCY
    ref = T.track(k, x, sat.code, delay, dop, stamp, first, 1200, buffer_first=first)
    assert ref["flags"][-1] & 2 and len(ref) < 1200 and ref["state"][-1] == 4
    compare_exact(rec[:, 0], ref, "loss")
    assert rounds == len(ref)
    assert trk.channel_state(0)[0] == 0
    # the second segment: another satellite geometry, the same loop configuration
    sat2, k2, x2, stamp2, first2, delay2, dop2 = S.sync("GPS", FS, 600, dop=-2310.0, delay_chips=611.7, seed=8, **kw)
    trk.start(0, 5, delay2, dop2, stamp2, first2)
    rec2, rounds2 = trk.run(x2, first2, 600)
    ref2 = T.track(k2, x2, sat2.code, delay2, dop2, stamp2, first2, 600, buffer_first=first2)
    assert len(ref2) == 600 and np.sum(ref2["state"] == 4) >= 200
    compare_exact(rec2[:, 0], ref2, "restart")
    assert rounds2 == 600
    trk.close()


def test_launch_boundaries_inside_the_regime(ctx):
    """One scenario in three launches, both boundaries in state 4: max_rounds ends the first launch, the
    buffer's end the second.  A launch that starts in the regime seeds its first epoch steady."""
    sat, k, x, stamp, first, delay, dop, ref = gps_700()
    n1 = 350
    trk = engine.DllPllVemlTracking(ctx, dev_conf(k, "GPS"), 1)
    ctx.set_code(3, sat.code)
    trk.start(0, 3, delay, dop, stamp, first)
    a, ra = trk.run(x, first, n1)
    st, nx = trk.channel_state(0)
    assert ra == n1 and st == 4
    o = int(nx - first)
    b, rb = trk.run(x[o:o + 150 * 4000 + 1234], nx, EPOCHS)
    st, nx2 = trk.channel_state(0)
    assert 140 <= rb <= 151 and st == 4
    assert ref["state"][n1 - 1] == 4 and ref["state"][n1 + rb - 1] == 4
    c, rc = trk.run(x[int(nx2 - first):], nx2, EPOCHS - n1 - rb)
    trk.close()
    assert rc == EPOCHS - n1 - rb
    got = np.concatenate([a[:ra, 0], b[:rb, 0], c[:rc, 0]])
    compare_exact(got, ref, "three launches")


def test_regime_off_fll(ctx):
    """enable_fll_steady_state: state 4 is reached, the regime never is (run_dll_pll's FLL branch reads
    the prompts epoch_pre accumulates)."""
    sat, k, x, stamp, first, delay, dop = S.sync("GPS", FS, 300, rotator_avx=1, enable_fll_steady_state=1)
    trk = engine.DllPllVemlTracking(ctx, dev_conf(k, "GPS"), 1)
    ctx.set_code(40, sat.code)
    trk.start(0, 40, delay, dop, stamp, first)
    rec, rounds = trk.run(x, first, 300)
    assert trk.last_engine() == abi.TRK_ENGINE_FAST_LATENCY
    trk.close()
    ref = T.track(k, x, sat.code, delay, dop, stamp, first, 300, buffer_first=first)
    assert len(ref) == 300 and np.sum(ref["state"] == 4) >= 50
    compare_exact(rec[:, 0], ref, "fll")


def test_regime_off_secondary_code(ctx):
    """Galileo E1 (pilot secondary code, data prompt): no discriminators from the accumulator waves, so
    every epoch keeps the hand-off; the job layout is shared."""
    fs = 25e6 / 4
    sat, k, x, stamp, first, delay, dop = S.sync("GAL", fs, 90, rotator_avx=1)
    trk = engine.DllPllVemlTracking(ctx, dev_conf(k, "GAL"), 1)
    ctx.set_code(30, sat.code)
    ctx.set_code(31, sat.code_data)
    trk.start(0, 30, delay, dop, stamp, first, data_code_id=31)
    rec, rounds = trk.run(x, first, 90)
    assert trk.last_engine() == abi.TRK_ENGINE_FAST_LATENCY
    trk.close()
    ref = T.track(k, x, sat.code, delay, dop, stamp, first, 90, data_code=sat.code_data, buffer_first=first)
    assert ref["state"][-1] == 4
    compare_exact(rec[:, 0], ref, "E1")


def test_dump_records_in_the_regime(ctx):
    """log_data's records (written by epoch_post, after the deferred epoch_pre) against the oracle's, as
    test_gpu_trk.test_dump_records_match_oracle compares them."""
    epochs = 600
    sat, k, x, stamp, first, delay, dop = S.sync("GPS", FS, epochs, rotator_avx=1)
    trk = engine.DllPllVemlTracking(ctx, dev_conf(k, "GPS"), 1)
    ctx.set_code(70, sat.code)
    trk.start(0, 70, delay, dop, stamp, first, prn=sat.prn)
    rec, rounds, dump = trk.run(x, first, epochs, dump=True)
    assert trk.last_engine() == abi.TRK_ENGINE_FAST_LATENCY
    trk.close()
    ref, rdump = T.track(k, x, sat.code, delay, dop, stamp, first, epochs, buffer_first=first, dump=True, prn=sat.prn)
    assert np.sum(ref["state"] == 4) >= 300
    compare_exact(rec[:, 0], ref, "dump")
    ran = (rec[:, 0]["flags"] & 8) != 0
    d_rec, d_dump = rec[ran, 0], dump[ran, 0]
    assert np.array_equal(d_rec["flags"] & 16, ref["flags"] & 16)
    w = (ref["flags"] & 16) != 0
    a, b = d_dump[w], rdump[w]
    assert len(a) > 20 and np.sum(ref["state"][w] == 4) >= 10
    for f in ("PRN_start_sample_count", "aux2", "PRN"):
        assert np.array_equal(a[f], b[f]), f
    for f in ("abs_VE", "abs_E", "abs_P", "abs_L", "abs_VL", "prompt_I", "prompt_Q"):
        np.testing.assert_allclose(a[f], b[f], rtol=1e-4, atol=1e-3, err_msg=f)
    for f, at in [("acc_carrier_phase_rad", 1e-2), ("carrier_doppler_hz", 2e-3), ("code_freq_chips", 2e-3), ("carr_error_hz", 1e-3),
                  ("carr_error_filt_hz", 2e-3), ("code_error_chips", 1e-4), ("code_error_filt_chips", 1e-4), ("CN0_SNV_dB_Hz", 5e-3),
                  ("carrier_lock_test", 1e-4), ("aux1", 1e-4), ("carrier_doppler_rate_hz", 0.5), ("code_freq_rate_chips", 0.5)]:
        np.testing.assert_allclose(a[f], b[f], rtol=1e-5, atol=at, err_msg=f)
