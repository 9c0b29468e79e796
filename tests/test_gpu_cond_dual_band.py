"""Dual-band end to end on the GPU: a 16 Msps ibyte stream with GPS L1 C/A at +4 MHz and BeiDou B1I at
−4 MHz (tests/cond_scenarios.py) goes through one two-band signal conditioner in blocks, each band
assembled contiguously in the caller's device buffers; acquisition and tracking then consume the
conditioned bands in place (device pointers), as the reference's channels consume its Signal_Conditioner's
output (gnss_flowgraph.cc:1008-1140).

Contract: acquisition's peak bin and code index equal the oracle acquisition's on the same conditioned
samples pulled to the host, and sit within one Doppler bin and ±1 decimated sample of the synthetic truth
(group delay (T − 1)/(2D) included); every tracking record field equals the oracle loop's fed the same
conditioned samples (test_gpu_trk.compare_exact), on the default engine dispatch."""
import numpy as np
import pytest

from gnss_sim_receiver_amd import abi, engine

import cond_model as M
import cond_scenarios as C
from test_gpu_trk import compare_exact, dev_conf

pytestmark = pytest.mark.gpu

SYSTEMS = ("GPS", "BDS")


@pytest.fixture(scope="module")
def conditioned(ctx):
    """The two bands conditioned on the device in three blocks into contiguous per-band device buffers:
    {system: (DeviceBuffer, host copy, taps)}."""
    raw, _ = C.raw_stream()
    hs = {s: C.taps(lambda fs, d: engine.cond_lowpass_taps(ctx.lib, fs, d), s) for s in SYSTEMS}
    n_out = {s: C.N_IN // C.BANDS[s]["decim"] for s in SYSTEMS}
    bufs = {s: engine.DeviceBuffer(ctx, 8 * n_out[s]) for s in SYSTEMS}
    src = ctx.upload(raw)
    block = 1_600_000
    cond = engine.SignalConditioner(ctx, C.FS, [(C.BANDS[s]["if_hz"], C.BANDS[s]["decim"], hs[s]) for s in SYSTEMS], block)
    for b0 in range(0, C.N_IN, block):
        dst = [bufs[s].ptr + 8 * (b0 // C.BANDS[s]["decim"]) for s in SYSTEMS]
        got = cond.run(src.ptr + 2 * b0, fmt=abi.FMT_CI8, on_device=True, n_in=block, dev_dst=dst)
        assert got == [(dst[i], block // C.BANDS[s]["decim"]) for i, s in enumerate(SYSTEMS)]
    assert cond.samples_in() == C.N_IN
    ctx.sync()
    out = {s: (bufs[s], bufs[s].download(np.empty(n_out[s], np.complex64)), hs[s]) for s in SYSTEMS}
    cond.close()
    src.free()
    yield out
    for s in SYSTEMS:
        bufs[s].free()


@pytest.mark.parametrize("system", SYSTEMS)
def test_conditioned_band_meets_the_accuracy_contract(conditioned, system):
    """The first 40 000 outputs of the long run against the float64 model (the whole stream's phase origin)."""
    _, y, h = conditioned[system]
    b = C.BANDS[system]
    n = 40_000 * b["decim"]
    x = C.raw_stream()[1][:n]
    assert M.contract_ratio(y[:40_000], *M.model(x, h, b["decim"], b["if_hz"], C.FS), len(h)) <= 1.0


@pytest.mark.parametrize("system", SYSTEMS)
def test_acquisition_and_tracking_on_the_conditioned_band(ctx, conditioned, system):
    buf, y, h = conditioned[system]
    fs = C.fs_out(system)
    a, n = C.dwell(system)
    sats = C.satellites(system)
    acq = engine.PcpsAcquisition(ctx, fs, n, C.DOPPLER_MAX, C.DOPPLER_STEP, 0, True, **C.acq_args(system))
    k = C.trk_conf(system)
    trk = engine.DllPllVemlTracking(ctx, dev_conf(k, system), len(sats))
    results = []
    for ch, sat in enumerate(sats):
        acq.set_local_code(C.local_code(system, sat.prn))
        (res,), _ = acq.run(engine.DeviceBuffer.wrap(ctx, buf.ptr + 8 * a, 8 * n), fmt=abi.FMT_CF32)
        ref = C.oracle_acquisition(system, sat.prn, y)
        assert (res.doppler_index, res.code_index, res.doppler_hz) == (ref.doppler_index, ref.code_index, ref.doppler_hz), (system, sat.prn)
        C.check_acquisition_against_truth(system, sat, res, len(h))
        results.append(res)
        ctx.set_code(100 + ch, sat.code)
        delay, dop, stamp, first = C.trk_start(system, res)
        trk.start(ch, 100 + ch, delay, dop, stamp, first, prn=sat.prn)
    acq.close()
    epochs = C.epochs(system)
    rec, rounds = trk.run(buf, 0, epochs, fmt=abi.FMT_CF32, n_buffer_samples=len(y))
    trk.close()
    assert rounds == epochs
    for ch, sat in enumerate(sats):
        ref = C.oracle_track(system, sat, y, results[ch])
        assert len(ref) == epochs
        compare_exact(rec[:, ch], ref, f"{system} PRN {sat.prn} on the conditioned band")
        assert abs(ref["carrier_doppler_hz"][-1] - sat.doppler_hz) < 10.0
